#!/usr/bin/env python
"""tools/alt_verdict_trace.py KERNEL_TRACE.csv [ANCHOR=ecrecover_rows_pair] [LAST=20] — do consecutive verdict kernels of the
pipelined leg overlap (rocprofv3 --kernel-trace of tools/side_tally_trace.py, IBFT_ALT_VERDICT as set for that run)?  For the
last LAST dispatches of the kernel whose name contains ANCHOR: queue, start and duration, the gap to the previous one's end
(negative: they overlapped), and the tally kernels' queues; then the medians."""
import csv
import sys

import numpy as np

rows = list(csv.DictReader(open(sys.argv[1])))
anchor = sys.argv[2] if len(sys.argv) > 2 else "ecrecover_rows_pair"
last = int(sys.argv[3]) if len(sys.argv) > 3 else 20
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
ver = [r for r in rows if anchor in r["Kernel_Name"]][-last:]
t0 = int(ver[0]["Start_Timestamp"])
tally = [r for r in rows if "tally_kernel" in r["Kernel_Name"] and int(r["Start_Timestamp"]) >= t0]
gaps, durs, steps = [], [], []
for i, r in enumerate(ver):
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    durs.append((e - s) / 1e3)
    line = f"verdict {i:2d} q{r['Queue_Id']} start={(s - t0) / 1e3:9.1f} dur={(e - s) / 1e3:7.1f}"
    if i:
        pe, ps = int(ver[i - 1]["End_Timestamp"]), int(ver[i - 1]["Start_Timestamp"])
        gaps.append((s - pe) / 1e3)
        steps.append((s - ps) / 1e3)
        line += f" gap to previous end={(s - pe) / 1e3:7.1f} start to start={(s - ps) / 1e3:7.1f}"
    print(line)
print(f"# verdict queues {sorted({r['Queue_Id'] for r in ver})}, tally queues {sorted({r['Queue_Id'] for r in tally})}")
print(f"# medians (us): kernel {np.median(durs):.1f}, gap to previous end {np.median(gaps):.1f}, start to start {np.median(steps):.1f}; "
      f"overlapping pairs {sum(g < 0 for g in gaps)} of {len(gaps)}")
