#!/usr/bin/env python3
"""Chain sync rate: blocks/s of ibft_verify_block_seals (every block's committed seals in ONE call) against a loop of
ibft_verify_seals (one call per block) over the same rows on the same context.

    python tools/block_seals_rate.py                       # V ∈ {4, 100, 1024} × blocks per call ∈ {1, 16, 256, max}
    python tools/block_seals_rate.py --v 100 --blocks 655  # one configuration (e.g. under rocprofv3 --kernel-trace --stats)
    python tools/block_seals_rate.py --v 1024 --blocks 1 --repeat 64   # one block of 65 536 rows
    python tools/block_seals_rate.py --stream              # the streamed form (ibft_block_seals_submit / _collect) against the call

Every block carries one seal of every validator (V rows), signed on the device (ibft_sign_seals).  "max" = as many blocks as
fit 65 536 rows.  cold: a context without the key cache (every call recovers); warm: IBFT_FLAG_PUBKEY_CACHE after the
warm-up call built every validator's table.  Both entry points return only after the device finished (they deliver the
verdicts), so host wall time over back-to-back calls after warm-up is device-synchronised time.  The loop calls the C
function directly through ctypes with pointers computed in advance (no numpy slicing inside the timed region).
--stream: three legs over the same batch shape on ONE context, alternated --alternations times (median and min … max of
the rounds are reported): the synchronous call from pageable sources, the synchronous call from ibft_pinned_alloc sources
(pinning alone), and the streamed form from the pinned sources with one batch kept in flight — submit(k + 1), collect(k) —
(pinning + pipelining).  Every leg rotates three distinct pre-signed batches, so no leg re-reads rows a cache still holds.
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


def main_stream(a):
    shapes = [(4, 16), (4, 16384), (100, 1), (100, 16), (100, 256), (100, 655), (1024, 16), (1024, 64)]
    if a.v != [4, 100, 1024] or a.blocks != ["1", "16", "256", "max"]:
        shapes = [(V_, 65536 // (V_ * a.repeat) if bs == "max" else int(bs)) for V_ in a.v for bs in a.blocks]
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
    ap.add_argument("--alternations", type=int, default=5, help="--stream: rounds of the three legs")
    a = ap.parse_args()
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
