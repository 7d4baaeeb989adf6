#!/usr/bin/env python3
"""tools/qtab_form_ab.py PARENT_LIB [rounds=3] [N …] — the key cache's two table forms against each other and against the
parent commit's library: one lease, separate processes alternating wide / glv / parent (the form is the pool's and is read
when a process creates its first context), `rounds` of each, the order of the three rotating from round to round.  Warm steady state as bench.py's warm sweep drives it
(ibft_seals_submit / _collect, one pass kept in flight) at N = 1 024, 4 096, 16 384, 65 536: ms per step, the warm kernel's
HIP-event time, ibft_cache_memory; ibft_issue_probe on every line.  And at 4 096: the first pass after ibft_set_validators
installs N unknown validators (the cold pass that learns the keys with the table build behind it), wall time.

Read out: glv ÷ wide per N with both legs' min–max, and wide (this build) ÷ parent — which must lie inside the parent's own
min–max spread: the default form is not to move.

    python tools/qtab_form_ab.py ab/parent/libibftgpu.so 3 > profiles/r22_qtab_form_ab.txt"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import os, sys, time, json
sys.path.insert(0, %r)
import go_ibft_amd.numa as NUMA
NUMA.pin_to_device_node(0)
import numpy as np
import go_ibft_amd.verifier as V, go_ibft_amd.simulate as SIM
out = {}
probe = V.BatchVerifier(max_rows=1024)
out["issue_ns"] = round(probe.issue_probe()[0], 4)
probe.close()
for key in sys.argv[1:]:
    n = int(key)
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=max(n, 1024))
    r = SIM.make_round(bv, n, 600 + n)
    rec = {}
    if n == 4096:                                     # N unknown validators: install, learn + build, first warm pass
        t0 = time.perf_counter(); bv.set_validators(1, r.addrs, r.power); rec["install_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
        bv.seals_stage(r.hash32, r.seal65, r.signer20, None)
        t0 = time.perf_counter(); v, t = bv.seals_run(); rec["learn_build_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
        assert v.all()
    else:
        bv.set_validators(1, r.addrs, r.power); bv.seals_stage(r.hash32, r.seal65, r.signer20, None)
    for _ in range(150): v, t = bv.seals_run()
    assert v.all() and t.has_quorum == 1 and bv.cache_stats()[0] == n
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
    rec["step_ms"] = round(min(series(300) for _ in range(3)), 5)
    bv.set_kernel_timing(4); bv.last_kernel_ms()
    series(300)
    ms, k = bv.last_kernel_ms()
    bv.set_kernel_timing(0)
    rec["kernel_ms"] = round(ms / max(k, 1), 5)
    rec["lanes"] = bv.last_dispatch()[1]
    by, used, cap, _ = bv.cache_memory()
    rec["cache_MB"] = round(by / 1e6, 1); rec["slots"] = [used, cap]
    rec["form"] = list(bv.cache_form()) if hasattr(bv._L, "ibft_cache_form") else None
    out[key] = rec
    bv.close()
print(json.dumps(out))
''' % ROOT


def main():
    parent = os.path.abspath(sys.argv[1])
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    sizes = sys.argv[3:] or ["1024", "4096", "16384", "65536"]
    legs = [("wide", {"IBFT_QTAB_FORM": "wide"}), ("glv", {"IBFT_QTAB_FORM": "glv"}), ("parent", {"IBFT_GPU_LIB": parent})]
    acc = {name: {} for name, _ in legs}
    for rd in range(rounds):
        for name, extra in legs[rd % 3:] + legs[:rd % 3]:   # no leg always runs in the same place of a round
            env = {k: v for k, v in os.environ.items() if k not in ("IBFT_QTAB_FORM", "IBFT_GPU_LIB", "IBFT_WARM_LANES")}
            env.update(extra)
            p = subprocess.run([sys.executable, "-c", CHILD] + sizes, env=env, capture_output=True, text=True, timeout=240)
            if p.returncode != 0:   # a child that died: nothing more is started on the device
                print(f"{name}: child exited {p.returncode}", p.stderr[-1500:], flush=True)
                sys.exit(1)
            line = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
            print(f"{name:7s}", line, flush=True)
            for k, v in json.loads(line).items():
                if isinstance(v, dict):
                    for q, x in v.items():
                        if isinstance(x, (int, float)):
                            acc[name].setdefault(k, {}).setdefault(q, []).append(x)

    def mm(name, k, q):
        xs = sorted(acc[name].get(k, {}).get(q, []))
        return (xs[len(xs) // 2], xs[0], xs[-1]) if xs else None

    def fmt(t):
        return "-" if t is None else f"{t[0]:.4f} ({t[1]:.4f} … {t[2]:.4f})"

    for q in ("step_ms", "kernel_ms"):
        print(f"# {q}: median (min … max) | N | wide | glv | parent | glv ÷ wide | wide ÷ parent | inside the parent's spread")
        for k in sizes:
            w, g, p = mm("wide", k, q), mm("glv", k, q), mm("parent", k, q)
            inside = p is not None and w is not None and p[1] <= w[0] <= p[2]
            print(f"# {k:>6s} | {fmt(w)} | {fmt(g)} | {fmt(p)} | {g[0] / w[0]:.3f} | {w[0] / p[0]:.3f} | {'yes' if inside else 'NO'}")
    for q in ("install_ms", "learn_build_ms"):
        print(f"# {q} at 4096: wide {fmt(mm('wide', '4096', q))} | glv {fmt(mm('glv', '4096', q))} | parent {fmt(mm('parent', '4096', q))}")
    for k in sizes:
        print(f"# cache MB at {k}: wide {fmt(mm('wide', k, 'cache_MB'))} | glv {fmt(mm('glv', k, 'cache_MB'))}")


if __name__ == "__main__":
    main()
