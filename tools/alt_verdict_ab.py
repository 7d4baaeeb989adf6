#!/usr/bin/env python3
"""tools/alt_verdict_ab.py PARENT_LIB [rounds=3] [N …] — the pipelined pass (ibft_seals_submit / _collect, one pass kept in
flight: the bench's headline step) with consecutive verdict launches on two streams (IBFT_ALT_VERDICT=1, round 21) against the
parent commit's library, one lease, separate processes alternating: parent, parent again (the spread of the procedure), this
tree with IBFT_ALT_VERDICT=0, this tree with =1 (every form forced), this tree as it ships (AUTO).  Per size: ms per step over
400 delivered passes (best of three series) behind 150 synchronous ones, the verdict kernel's HIP-event time on every fourth
pass of a further series, the synchronous step, and the passes that took the second stream.  A size written wN is the warm
path (keys known).

    python tools/alt_verdict_ab.py ab/parent/libibftgpu.so 3 > r21_alt_verdict_ab.txt"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import os, sys, time, json
sys.path.insert(0, %r)
import go_ibft_amd.numa as NUMA
NUMA.pin_to_device_node(0)
import numpy as np
import go_ibft_amd.verifier as V, go_ibft_amd.simulate as SIM
out = {}
for key in sys.argv[1:]:
    warm = key.startswith("w")
    n = int(key.lstrip("w"))
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if warm else 0, max_rows=max(n, 1024))
    r = SIM.make_round(bv, n, 600 + n)
    bv.set_validators(1, r.addrs, r.power); bv.seals_stage(r.hash32, r.seal65, r.signer20, None)
    for _ in range(150): v, t = bv.seals_run()
    assert v.all() and t.has_quorum == 1
    if warm: assert bv.cache_stats()[0] == n
    def series(k):
        bv.seals_submit()
        t0 = time.perf_counter()
        for _ in range(k):
            bv.seals_submit()
            v, t = bv.seals_collect()
        dt = time.perf_counter() - t0
        v, t = bv.seals_collect()
        assert v.all() and t.has_quorum == 1 and t.valid_rows == n
        return dt / k * 1e3
    series(50)
    step = min(series(400) for _ in range(3))
    bv.set_kernel_timing(4); bv.last_kernel_ms()
    series(400)
    ms, k = bv.last_kernel_ms()
    bv.set_kernel_timing(0)
    lat = []
    for _ in range(60):
        t0 = time.perf_counter(); bv.seals_run(); lat.append((time.perf_counter() - t0) * 1e3)
    out[key] = {"step_ms": round(step, 5), "kernel_ms": round(ms / max(k, 1), 5), "sync_ms": round(float(np.median(lat)), 5),
                "alt": bv.alt_verdict_passes() if hasattr(bv, "alt_verdict_passes") else 0}
    bv.close()
print(json.dumps(out))
''' % ROOT
parent = os.path.abspath(sys.argv[1])
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
sizes = sys.argv[3:] or ["64", "1024", "2049", "4096", "8192", "w4096", "w16384"]
LEGS = [("parent", {"IBFT_GPU_LIB": parent}), ("parent2", {"IBFT_GPU_LIB": parent}), ("alt0", {"IBFT_ALT_VERDICT": "0"}),
        ("alt1", {"IBFT_ALT_VERDICT": "1"}), ("auto", {})]
acc = {name: {} for name, _ in LEGS}
for rd in range(rounds):
    for name, extra in LEGS:
        env = {k: v for k, v in os.environ.items() if k not in ("IBFT_ALT_VERDICT", "IBFT_GPU_LIB")}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", CHILD] + sizes, env=env, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:   # a child that died: nothing more is started on the device
            print(f"{name}: child exited {p.returncode}", p.stderr[-1500:], flush=True)
            sys.exit(1)
        line = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
        print(f"{name:8s}", line, flush=True)
        for k, v in json.loads(line).items():
            for q, x in v.items():
                acc[name].setdefault(k, {}).setdefault(q, []).append(x)
print("# medians, ms per step: N | parent | parent(2) (spread) | alt0 | alt1 (vs parent median) | auto (vs parent median) || verdict kernel ms "
      "parent / alt1 || synchronous step ms parent / auto || second-stream passes alt1 / auto")
for k in sizes:
    m = {name: {q: float(np.median(acc[name][k][q])) for q in acc[name][k]} for name, _ in LEGS}
    base = (m["parent"]["step_ms"] + m["parent2"]["step_ms"]) / 2
    spread = abs(m["parent"]["step_ms"] - m["parent2"]["step_ms"]) / base
    print(f"# {k:>7s} | {m['parent']['step_ms']:.5f} | {m['parent2']['step_ms']:.5f} ({spread * 100:.2f} %) | {m['alt0']['step_ms']:.5f} | "
          f"{m['alt1']['step_ms']:.5f} ({(m['alt1']['step_ms'] / base - 1) * 100:+.2f} %) | {m['auto']['step_ms']:.5f} "
          f"({(m['auto']['step_ms'] / base - 1) * 100:+.2f} %) || {m['parent']['kernel_ms']:.5f} / {m['alt1']['kernel_ms']:.5f} || "
          f"{m['parent']['sync_ms']:.5f} / {m['auto']['sync_ms']:.5f} || {int(m['alt1']['alt'])} / {int(m['auto']['alt'])}")
