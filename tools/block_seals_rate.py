#!/usr/bin/env python3
"""Chain sync rate: blocks/s of ibft_verify_block_seals (every block's committed seals in ONE call) against a loop of
ibft_verify_seals (one call per block) over the same rows on the same context.

    python tools/block_seals_rate.py                       # V ∈ {4, 100, 1024} × blocks per call ∈ {1, 16, 256, max}
    python tools/block_seals_rate.py --v 100 --blocks 655  # one configuration (e.g. under rocprofv3 --kernel-trace --stats)
    python tools/block_seals_rate.py --v 1024 --blocks 1 --repeat 64   # one block of 65 536 rows
    python tools/block_seals_rate.py --stream              # the streamed form (ibft_block_seals_submit / _collect) against the call
    python tools/block_seals_rate.py --recover             # bare seals: ibft_recover_block_seals against the verify call and the host route

Every block carries one seal of every validator (V rows), signed on the device (ibft_sign_seals).  "max" = as many blocks as
fit 65 536 rows.  cold: a context without the key cache (every call recovers); warm: IBFT_FLAG_PUBKEY_CACHE after the
warm-up call built every validator's table.  Both entry points return only after the device finished (they deliver the
verdicts), so host wall time over back-to-back calls after warm-up is device-synchronised time.  The loop calls the C
function directly through ctypes with pointers computed in advance (no numpy slicing inside the timed region).
--stream: three legs over the same batch shape on ONE context, alternated --alternations times (median and min … max of
the rounds are reported): the synchronous call from pageable sources, the synchronous call from ibft_pinned_alloc sources
(pinning alone), and the streamed form from the pinned sources with one batch kept in flight — submit(k + 1), collect(k) —
(pinning + pipelining).  Every leg rotates three distinct pre-signed batches, so no leg re-reads rows a cache still holds.
--recover: headers that carry only signatures.  Three legs over the same batch on one lease, alternated --alternations times
on contexts WITHOUT the key cache: ibft_recover_block_seals (the emitting cold kernels), ibft_verify_block_seals with the
signers given (the same cold kernels comparing), and the host route an embedder has without the recover call — the oracle's
tuned recovery of every row on --threads cores (orc_verify_seals_tuned_mt: it recovers each row's key and address natively on a
thread pool of its own and compares the address, which is the cost of recovering it), then ibft_verify_block_seals.  Kernel times are ibft_last_kernel_ms of the
verdict launch alone.  --parent-lib OLD.so adds a fourth figure: the cold verify launch of ANOTHER build of the library (the
parent commit's) over the same rows, in child processes that alternate with child processes of this build (IBFT_GPU_LIB).
With --stream, --parent-lib OLD.so runs the three legs under BOTH builds instead: per alternation one child process of the
other build, then one of this build, each doing one round of the legs on a context of its own (IBFT_GPU_LIB); median and
min … max over the alternations per build, and whether this build's streamed median lies inside the other build's spread.
The lease's ibft_issue_probe value is printed beside every configuration.
One JSON line per configuration, then a table."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, budget_s=0.25, max_reps=500):
    fn()                                          # warm-up (and a first estimate)
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(3, min(max_reps, int(budget_s / one)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def measure(V_, nb, warm, repeat=1):
    import go_ibft_amd.verifier as V
    from oracle import binding as B, workload as W
    r = W.make_round(V_, 7, raw_len=64)
    per = V_ * repeat                             # rows per block: every validator's seal `repeat` times
    n = nb * per
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if warm else 0, max_rows=65536)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        bh = np.frombuffer(b"".join(B.keccak256(b"blk" + b.to_bytes(4, "little")) for b in range(nb)), np.uint8).reshape(nb, 32)
        off = (np.arange(nb + 1) * per).astype(np.uint32)
        rh = np.repeat(bh, per, axis=0)
        sk = np.tile(np.frombuffer(b"".join(r.sks), np.uint8).reshape(V_, 32), (nb * repeat, 1))
        sig, signer, ok = bv.sign_seals(sk, rh)
        assert ok.all()
        L = bv._L
        mask = np.zeros((n + 63) // 64, np.uint64)
        tal = (V.Tally * nb)()
        args_one = (bv._h, V._p(bh), V._p(off), nb, V._p(sig), V._p(signer), None, V._p(mask), tal)

        def one():
            rc = L.ibft_verify_block_seals(*args_one)
            assert rc == 0, rc

        bmask = np.zeros(nb * ((per + 63) // 64), np.uint64)
        bt = V.Tally()
        addr = lambda a: a.ctypes.data
        per_block = [(bv._h, C.c_void_p(addr(rh) + 32 * b * per), C.c_void_p(addr(sig) + 65 * b * per),
                      C.c_void_p(addr(signer) + 20 * b * per), None, per, C.c_void_p(addr(bmask) + 8 * b * ((per + 63) // 64)),
                      C.byref(bt)) for b in range(nb)]

        def loop():
            for a in per_block:
                rc = L.ibft_verify_seals(*a)
                assert rc == 0, rc

        one()                                     # the key cache learns and builds here (warm); nothing changes cold
        t_one = timed(one)
        t_loop = timed(loop)
        # both forms agree (the tests hold it in full; a spot check that the timed calls did the work)
        got = V.mask_to_bool(mask, n)
        assert got.all() and all(t.has_quorum == 1 for t in tal)
        cold, warm_lanes = bv.last_dispatch()
        tables, warm_passes, cold_passes = bv.cache_stats()
        return {"v": V_, "blocks": nb, "rows": n, "rows_per_block": per, "mode": "warm" if warm else "cold", "one_call_ms": t_one * 1e3,
                "loop_ms": t_loop * 1e3, "blocks_per_s_one": nb / t_one, "blocks_per_s_loop": nb / t_loop,
                "speedup": t_loop / t_one, "cold_lanes": cold, "warm_lanes": warm_lanes, "tables": tables}
    finally:
        bv.close()


def measure_stream(V_, nb, warm, repeat=1, alternations=5, budget_s=0.15):
    import go_ibft_amd.verifier as V
    from oracle import binding as B, workload as W
    r = W.make_round(V_, 7, raw_len=64)
    per = V_ * repeat
    n = nb * per
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if warm else 0, max_rows=65536)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        off = (np.arange(nb + 1) * per).astype(np.uint32)
        sk = np.tile(np.frombuffer(b"".join(r.sks), np.uint8).reshape(V_, 32), (nb * repeat, 1))
        page, pin = [], []
        for k in range(3):                        # three distinct batches: other block hashes, other signatures
            bh = np.frombuffer(b"".join(B.keccak256(b"blk%d" % k + b.to_bytes(4, "little")) for b in range(nb)), np.uint8).reshape(nb, 32)
            sig, signer, ok = bv.sign_seals(sk, np.repeat(bh, per, axis=0))
            assert ok.all()
            page.append((bh.copy(), off.copy(), sig, signer))
            pin.append(tuple(V.pinned_copy(a) for a in page[-1]))
        L = bv._L
        mask = np.zeros((n + 63) // 64, np.uint64)
        tal = (V.Tally * nb)()
        state = {"k": 0}

        def sync_from(batches):
            args = [(bv._h, V._p(bh), V._p(o), nb, V._p(sig), V._p(signer), None, V._p(mask), tal) for bh, o, sig, signer in batches]

            def fn():
                state["k"] = (state["k"] + 1) % 3
                rc = L.ibft_verify_block_seals(*args[state["k"]])
                assert rc == 0, rc
            return fn

        sub = [(bv._h, V._p(bh), V._p(o), nb, V._p(sig), V._p(signer), None) for bh, o, sig, signer in pin]

        def submit():
            state["k"] = (state["k"] + 1) % 3
            rc = L.ibft_block_seals_submit(*sub[state["k"]])
            assert rc == 0, rc

        def collect():
            rc = L.ibft_block_seals_collect(bv._h, V._p(mask), tal)
            assert rc == 0, rc

        def step():                               # one batch kept in flight
            submit()
            collect()

        def check():
            assert V.mask_to_bool(mask, n).all() and all(t.has_quorum == 1 for t in tal)

        legs = {"sync_pageable": sync_from(page), "sync_pinned": sync_from(pin), "stream": step}
        legs["sync_pageable"]()                   # the key cache learns and builds here (warm); nothing changes cold
        check()
        times = {k: [] for k in legs}
        for _ in range(alternations):
            for name, fn in legs.items():
                if name == "stream":
                    submit()                      # prime: the timed steps always find one batch in flight
                times[name].append(timed(fn, budget_s) * 1e3)
                if name == "stream":
                    collect()
                check()
        cold, warm_lanes = bv.last_dispatch()
        res = {"v": V_, "blocks": nb, "rows": n, "rows_per_block": per, "mode": "warm" if warm else "cold", "cold_lanes": cold,
               "warm_lanes": warm_lanes, "alternations": alternations}
        for name, ts in times.items():
            res[name + "_ms"] = float(np.median(ts))
            res[name + "_min_ms"] = min(ts)
            res[name + "_max_ms"] = max(ts)
            res[name + "_all_ms"] = [round(t, 4) for t in ts]
        res["stream_over_sync_pageable"] = res["stream_ms"] / res["sync_pageable_ms"]
        res["stream_over_sync_pinned"] = res["stream_ms"] / res["sync_pinned_ms"]
        return res
    finally:
        bv.close()


def _recover_batch(bv, V_, rows):
    """rows seals, every validator signing every block (blocks of V_ rows), signed on the device"""
    import go_ibft_amd.verifier as V  # noqa: F401
    from oracle import binding as B, workload as W
    r = W.make_round(V_, 7, raw_len=64)
    nb = max(1, rows // V_)
    n = nb * V_
    bv.set_validators(r.height, r.addrs, r.power)
    bh = np.frombuffer(b"".join(B.keccak256(b"rec" + b.to_bytes(4, "little")) for b in range(nb)), np.uint8).reshape(nb, 32).copy()
    off = (np.arange(nb + 1) * V_).astype(np.uint32)
    sk = np.tile(np.frombuffer(b"".join(r.sks), np.uint8).reshape(V_, 32), (nb, 1))
    sig, signer, ok = bv.sign_seals(sk, np.repeat(bh, V_, axis=0))
    assert ok.all()
    return r, nb, n, bh, off, sig, signer


def kernel_leg(V_, rows, leg, reps=30):
    """child process of --recover --parent-lib: kernel ms (median of reps) of ONE leg's verdict launch under the library
    IBFT_GPU_LIB names → one JSON line"""
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(max_rows=65536)
    try:
        r, nb, n, bh, off, sig, signer = _recover_batch(bv, V_, rows)
        fn = (lambda: bv.recover_block_seals(bh, off, sig)) if leg == "recover" else (lambda: bv.verify_block_seals(bh, off, sig, signer))
        for _ in range(3):
            fn()
        bv.set_kernel_timing(1)
        bv.last_kernel_ms()
        ms = []
        for _ in range(reps):
            fn()
            ms.append(bv.last_kernel_ms()[0])
        print(json.dumps({"leg": leg, "v": V_, "rows": n, "kernel_ms": float(np.median(ms)), "kernel_min_ms": min(ms),
                          "cold_lanes": bv.last_dispatch()[0], "lib": os.environ.get("IBFT_GPU_LIB", "")}), flush=True)
    finally:
        bv.close()


def measure_recover(V_, rows, alternations=5, threads=16, budget_s=0.15, parent_lib=None):
    import subprocess
    import go_ibft_amd.verifier as V
    from oracle import binding as B
    bv = V.BatchVerifier(max_rows=65536)
    try:
        probe_ns = bv.issue_probe()[0]
        r, nb, n, bh, off, sig, signer = _recover_batch(bv, V_, rows)
        rh = np.repeat(bh, V_, axis=0)
        L = bv._L
        mask = np.zeros((n + 63) // 64, np.uint64)
        tal = (V.Tally * nb)()
        out_signer = np.zeros((n, 20), np.uint8)
        out_vidx = np.zeros(n, np.int32)
        host_signer = np.zeros((n, 20), np.uint8)
        a_rec = (bv._h, V._p(bh), V._p(off), nb, V._p(sig), None, V._p(out_signer), V._p(out_vidx), V._p(mask), tal)
        a_ver = (bv._h, V._p(bh), V._p(off), nb, V._p(sig), V._p(signer), None, V._p(mask), tal)
        a_host = (bv._h, V._p(bh), V._p(off), nb, V._p(sig), V._p(host_signer), None, V._p(mask), tal)
        vs = B.ValSet(r.addrs, r.power)
        host_signer[:] = signer

        def host_recover_only():
            ok = B.verify_seals_tuned(vs, rh, sig, signer, None, 0, nthreads=threads)
            assert ok.all()

        def recover():
            rc = L.ibft_recover_block_seals(*a_rec)
            assert rc == 0, rc

        def verify():
            rc = L.ibft_verify_block_seals(*a_ver)
            assert rc == 0, rc

        def host_route():
            host_recover_only()
            rc = L.ibft_verify_block_seals(*a_host)
            assert rc == 0, rc

        legs = {"recover": recover, "verify": verify, "host_route": host_route}
        times = {k: [] for k in legs}
        kms = {"recover": [], "verify": []}
        host_only = []
        for _ in range(alternations):
            for name, fn in legs.items():
                if name == "host_route":       # seconds per call at size: a few calls, not a budget of them
                    fn()
                    t0 = time.perf_counter()
                    fn()
                    times[name].append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    host_recover_only()
                    host_only.append((time.perf_counter() - t0) * 1e3)
                else:
                    bv.set_kernel_timing(0)
                    times[name].append(timed(fn, budget_s) * 1e3)
                    bv.set_kernel_timing(1)
                    bv.last_kernel_ms()
                    k = []
                    for _ in range(10):
                        fn()
                        k.append(bv.last_kernel_ms()[0])
                    kms[name].append(float(np.median(k)))
                assert V.mask_to_bool(mask, n).all() and all(t.has_quorum == 1 for t in tal)
            assert (out_signer == signer).all() and (out_vidx == np.tile(np.arange(V_, dtype=np.int32), nb)).all()
        res = {"v": V_, "blocks": nb, "rows": n, "cold_lanes": bv.last_dispatch()[0], "alternations": alternations, "threads": threads,
               "issue_probe_ns": probe_ns}
        for name, ts in times.items():
            res[name + "_ms"] = float(np.median(ts))
            res[name + "_min_ms"] = min(ts)
            res[name + "_max_ms"] = max(ts)
        res["host_recover_only_ms"] = float(np.median(host_only))
        res["host_recover_M_per_s"] = n / res["host_recover_only_ms"] / 1e3
        for name, ks in kms.items():
            res[name + "_kernel_ms"] = float(np.median(ks))
            res[name + "_kernel_all_ms"] = [round(x, 4) for x in ks]
        res["kernel_recover_over_verify"] = res["recover_kernel_ms"] / res["verify_kernel_ms"]
        res["recover_over_host_route"] = res["recover_ms"] / res["host_route_ms"]
    finally:
        bv.close()
    if parent_lib:     # the parent build's cold verify launch against this build's emitting launch: fresh processes, alternating
        got = {"parent_verify": [], "recover": []}
        for _ in range(alternations):
            for key, lib, leg in (("parent_verify", parent_lib, "verify"), ("recover", None, "recover")):
                env = {k: v for k, v in os.environ.items() if k != "IBFT_GPU_LIB"}
                if lib:
                    env.update(IBFT_GPU_LIB=lib, IBFT_MIN_ABI="3")
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-leg", leg, "--v", str(V_), "--rows", str(rows)],
                                   capture_output=True, text=True, timeout=300, env=env)
                if p.returncode != 0:   # (nothing more is started on the device after a child that failed)
                    raise RuntimeError(f"kernel leg {key} failed ({p.returncode}): {p.stdout[-500:]}{p.stderr[-1500:]}")
                got[key].append(json.loads(p.stdout.strip().split("\n")[-1])["kernel_ms"])
        res["parent_verify_kernel_ms"] = float(np.median(got["parent_verify"]))
        res["child_recover_kernel_ms"] = float(np.median(got["recover"]))
        res["parent_verify_kernel_all_ms"] = [round(x, 4) for x in got["parent_verify"]]
        res["child_recover_kernel_all_ms"] = [round(x, 4) for x in got["recover"]]
        res["kernel_recover_over_parent_verify"] = res["child_recover_kernel_ms"] / res["parent_verify_kernel_ms"]
    return res


def main_recover(a):
    vs = a.v if a.v != [4, 100, 1024] else [100, 1024]
    rows = []
    for V_ in vs:
        for n in a.rows:
            res = measure_recover(V_, n, a.alternations, a.threads, parent_lib=a.parent_lib)
            rows.append(res)
            print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for res in rows:
                f.write(json.dumps(res) + "\n")
    print(f"{'V':>5} {'rows':>6} {'lanes':>5} {'probe ns':>8} {'recover ms':>22} {'verify ms':>22} {'host route ms':>24} {'rec/host':>8} "
          f"{'k rec ms':>9} {'k ver ms':>9} {'k rec/ver':>9} {'k parent ver':>12} {'k rec/parent':>12} {'host rec M/s':>12}")
    cell = lambda r, k: f"{r[k + '_ms']:.3f} ({r[k + '_min_ms']:.3f}…{r[k + '_max_ms']:.3f})"
    for r in rows:
        pv = f"{r['parent_verify_kernel_ms']:.4f}" if "parent_verify_kernel_ms" in r else "-"
        pr = f"{r['kernel_recover_over_parent_verify']:.3f}" if "parent_verify_kernel_ms" in r else "-"
        print(f"{r['v']:>5} {r['rows']:>6} {r['cold_lanes']:>5} {r['issue_probe_ns']:>8.3f} {cell(r, 'recover'):>22} {cell(r, 'verify'):>22} "
              f"{cell(r, 'host_route'):>24} {r['recover_over_host_route']:>8.4f} {r['recover_kernel_ms']:>9.4f} {r['verify_kernel_ms']:>9.4f} "
              f"{r['kernel_recover_over_verify']:>9.3f} {pv:>12} {pr:>12} {r['host_recover_M_per_s']:>12.3f}")


STREAM_LEGS = ("sync_pageable", "sync_pinned", "stream")


def stream_child(lib, V_, nb, mode, repeat):
    """one round of the --stream legs in a fresh process under the library `lib` (None: this build) → its JSON line"""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k != "IBFT_GPU_LIB"}
    if lib:
        env["IBFT_GPU_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--stream-child", "--v", str(V_), "--blocks", str(nb), "--modes", mode,
                        "--repeat", str(repeat)], capture_output=True, text=True, timeout=300, env=env)
    if p.returncode != 0:   # (nothing more is started on the device after a child that failed)
        raise RuntimeError(f"stream child under {lib or 'this build'} failed ({p.returncode}): {p.stdout[-500:]}{p.stderr[-1500:]}")
    return json.loads(p.stdout.strip().split("\n")[-1])


def measure_stream_ab(parent_lib, V_, nb, mode, repeat, alternations):
    got = {"parent": {k: [] for k in STREAM_LEGS}, "this": {k: [] for k in STREAM_LEGS}}
    for _ in range(alternations):
        for side, lib in (("parent", parent_lib), ("this", None)):
            r = stream_child(lib, V_, nb, mode, repeat)
            for k in STREAM_LEGS:
                got[side][k].append(r[k + "_ms"])
    res = {"v": V_, "blocks": nb, "rows": r["rows"], "mode": mode, "alternations": alternations, "cold_lanes": r["cold_lanes"],
           "warm_lanes": r["warm_lanes"]}
    for side in got:
        for k, ts in got[side].items():
            res[f"{k}_{side}_ms"] = float(np.median(ts))
            res[f"{k}_{side}_min_ms"] = min(ts)
            res[f"{k}_{side}_max_ms"] = max(ts)
            res[f"{k}_{side}_all_ms"] = [round(t, 4) for t in ts]
    res["stream_this_over_parent"] = res["stream_this_ms"] / res["stream_parent_ms"]
    res["stream_this_inside_parent_spread"] = res["stream_parent_min_ms"] <= res["stream_this_ms"] <= res["stream_parent_max_ms"]
    return res


def main_stream(a):
    shapes = [(4, 16), (4, 16384), (100, 1), (100, 16), (100, 256), (100, 655), (1024, 16), (1024, 64)]
    if a.v != [4, 100, 1024] or a.blocks != ["1", "16", "256", "max"]:
        shapes = [(V_, 65536 // (V_ * a.repeat) if bs == "max" else int(bs)) for V_ in a.v for bs in a.blocks]
    if a.parent_lib:
        rows = []
        for V_, nb in shapes:
            if nb < 1 or nb * V_ * a.repeat > 65536:
                continue
            for mode in a.modes:
                rows.append(measure_stream_ab(a.parent_lib, V_, nb, mode, a.repeat, a.alternations))
                print(json.dumps(rows[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                for res in rows:
                    f.write(json.dumps(res) + "\n")
        cell = lambda r, k: f"{r[k + '_ms']:.3f} ({r[k + '_min_ms']:.3f}…{r[k + '_max_ms']:.3f})"
        print(f"{'V':>5} {'blocks':>6} {'mode':>5} {'sync pinned: parent':>22} {'this':>22} {'streamed: parent':>22} {'this':>22} {'this/parent':>11} {'inside':>6}")
        for r in rows:
            print(f"{r['v']:>5} {r['blocks']:>6} {r['mode']:>5} {cell(r, 'sync_pinned_parent'):>22} {cell(r, 'sync_pinned_this'):>22} "
                  f"{cell(r, 'stream_parent'):>22} {cell(r, 'stream_this'):>22} {r['stream_this_over_parent']:>11.3f} "
                  f"{'yes' if r['stream_this_inside_parent_spread'] else 'NO':>6}")
        return
    rows = []
    for V_, nb in shapes:
        if nb < 1 or nb * V_ * a.repeat > 65536:
            continue
        for mode in a.modes:
            res = measure_stream(V_, nb, mode == "warm", a.repeat, a.alternations)
            rows.append(res)
            print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for res in rows:
                f.write(json.dumps(res) + "\n")
    print(f"{'V':>5} {'blocks':>6} {'rows':>6} {'mode':>5} {'sync pageable ms':>22} {'sync pinned ms':>22} {'streamed ms':>22} {'str/pageable':>12} {'str/pinned':>10}")
    cell = lambda r, k: f"{r[k + '_ms']:.3f} ({r[k + '_min_ms']:.3f}…{r[k + '_max_ms']:.3f})"
    for r in rows:
        print(f"{r['v']:>5} {r['blocks']:>6} {r['rows']:>6} {r['mode']:>5} {cell(r, 'sync_pageable'):>22} {cell(r, 'sync_pinned'):>22} "
              f"{cell(r, 'stream'):>22} {r['stream_over_sync_pageable']:>12.3f} {r['stream_over_sync_pinned']:>10.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--v", type=int, nargs="*", default=[4, 100, 1024])
    ap.add_argument("--blocks", type=str, nargs="*", default=["1", "16", "256", "max"])
    ap.add_argument("--modes", type=str, nargs="*", default=["cold", "warm"])
    ap.add_argument("--repeat", type=int, default=1, help="every validator signs each block this many times (a block of "
                    "V·repeat rows: --v 1024 --blocks 1 --repeat 64 is one block of 65 536 rows)")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON lines here")
    ap.add_argument("--stream", action="store_true", help="the streamed form against the synchronous call (pageable and pinned)")
    ap.add_argument("--alternations", type=int, default=5, help="--stream / --recover: rounds of the legs")
    ap.add_argument("--recover", action="store_true", help="bare seals: ibft_recover_block_seals against ibft_verify_block_seals "
                    "and the host route (CPU recovery, then the verify call)")
    ap.add_argument("--rows", type=int, nargs="*", default=[4096, 16384, 65500], help="--recover: rows per call (rounded down to whole blocks)")
    ap.add_argument("--threads", type=int, default=16, help="--recover: cores of the host route's recovery")
    ap.add_argument("--parent-lib", type=str, default=None, help="--recover: another build of libibftgpu.so whose cold verify "
                    "launch is timed over the same rows in alternating child processes; --stream: the legs under both builds, "
                    "in alternating child processes")
    ap.add_argument("--stream-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kernel-leg", type=str, default=None, choices=["recover", "verify"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernel_leg:
        return kernel_leg(a.v[0], a.rows[0], a.kernel_leg)
    if a.stream_child:
        print(json.dumps(measure_stream(a.v[0], int(a.blocks[0]), a.modes[0] == "warm", a.repeat, 1)), flush=True)
        return
    if a.recover:
        return main_recover(a)
    if a.stream:
        return main_stream(a)
    rows = []
    for V_ in a.v:
        for bs in a.blocks:
            nb = 65536 // (V_ * a.repeat) if bs == "max" else int(bs)
            if nb * V_ * a.repeat > 65536 or nb < 1:
                continue
            for mode in a.modes:
                res = measure(V_, nb, mode == "warm", a.repeat)
                rows.append(res)
                print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for res in rows:
                f.write(json.dumps(res) + "\n")
    print(f"{'V':>5} {'blocks':>6} {'rows':>6} {'mode':>5} {'one call ms':>11} {'loop ms':>9} {'blocks/s one':>13} "
          f"{'blocks/s loop':>13} {'×':>7}")
    for r in rows:
        print(f"{r['v']:>5} {r['blocks']:>6} {r['rows']:>6} {r['mode']:>5} {r['one_call_ms']:>11.3f} {r['loop_ms']:>9.3f} "
              f"{r['blocks_per_s_one']:>13.0f} {r['blocks_per_s_loop']:>13.0f} {r['speedup']:>7.1f}")


if __name__ == "__main__":
    main()
