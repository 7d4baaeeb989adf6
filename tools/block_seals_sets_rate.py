#!/usr/bin/env python3
"""Chain sync across validator-set changes: what one ibft_verify_block_seals_sets call over a run of blocks costs against what
a syncer had before it — a cut wherever the set changes — and against the floor, the same rows under one set.

    python tools/block_seals_sets_rate.py                                   # V = 100 × 655 blocks, V = 4 × 16 384 blocks; cold, warm
    python tools/block_seals_sets_rate.py --v 100 --blocks 655 --every 1 --modes cold     # one configuration (e.g. under rocprofv3)

The validator set changes every E blocks (--every: 1, 8, 64, "all" = never), sliding by one validator over a pool of --pool
keys (cyclic: the family holds min(⌈blocks / E⌉, pool) distinct sets).  Every block carries one seal of every validator of ITS
set (V rows), signed on the device.  All columns lie in ibft_pinned_alloc memory.  Three legs on ONE context, alternated
--alternations times (median and min … max of the rounds are reported):
  A  one ibft_verify_block_seals_sets call; the family is installed once, outside the timed region — its install time is
     reported beside it
  B  what there was before: per run of E blocks ibft_set_validators(the run's set) + ibft_verify_block_seals(the run's rows)
     (beyond --b-max-runs runs the leg is timed over that many runs and scaled to all of them: "b_runs_timed")
  C  the floor: ibft_verify_block_seals over all rows under ONE set (the union of the family) — other verdicts, the same work
A / B is the gain, A − C the price of the feature (one dense-table load per row in the tally, one more upload), measured
against leg C of the same run.  cold: no key cache; warm: IBFT_FLAG_PUBKEY_CACHE after the first call built the tables.
The lease's ibft_issue_probe value is on every line.  One JSON line per configuration, then a table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, budget_s=0.2, max_reps=200):
    """seconds per call; a call that alone exceeds the budget is timed once more and that is it"""
    fn()
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    if one >= budget_s:
        return one
    reps = max(3, min(max_reps, int(budget_s / one)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def measure(V_, nb, every, warm, pool, alternations, b_max_runs):
    import go_ibft_amd.verifier as V
    from oracle import binding as B, workload as W
    E = nb if every == "all" else int(every)
    runs = (nb + E - 1) // E
    n_sets = min(runs, pool)
    r = W.make_round(pool, 7, raw_len=64, weighted=True)
    idx = [[(k + j) % pool for j in range(V_)] for k in range(n_sets)]
    power = [np.array([int(r.power[i]) + k for i in ix], np.uint64) for k, ix in enumerate(idx)]
    set_of_block = (np.arange(nb) // E) % n_sets
    n = nb * V_
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if warm else 0, max_rows=65536)
    try:
        L = bv._L
        probe_ns = bv.issue_probe()[0]
        bv.set_validators(1, r.addrs, r.power)
        bh = np.frombuffer(b"".join(B.keccak256(b"set" + b.to_bytes(4, "little")) for b in range(nb)), np.uint8).reshape(nb, 32)
        off = (np.arange(nb + 1) * V_).astype(np.uint32)
        who = np.array([idx[s] for s in set_of_block], np.int64).reshape(-1)
        sk = np.frombuffer(b"".join(r.sks), np.uint8).reshape(pool, 32)[who]
        sig, signer, ok = bv.sign_seals(sk, np.repeat(bh, V_, axis=0))
        assert ok.all()
        bh, off, sig, signer, bset = (V.pinned_copy(np.ascontiguousarray(a)) for a in (bh, off, sig, signer, set_of_block.astype(np.uint32)))
        mask = np.zeros((n + 63) // 64, np.uint64)
        tal = (V.Tally * nb)()
        # the family's columns, flattened once: the install leg times the C call alone
        heights, set_off, fam_addrs, fam_power = V.BatchVerifier._set_columns([(r.addrs[ix], p) for ix, p in zip(idx, power)], False)
        a_install = (bv._h, n_sets, V._p(heights), V._p(set_off), V._p(fam_addrs), V._p(fam_power))
        a_sets = (bv._h, V._p(bh), V._p(off), V._p(bset), nb, V._p(sig), V._p(signer), None, V._p(mask), tal)
        a_floor = (bv._h, V._p(bh), V._p(off), nb, V._p(sig), V._p(signer), None, V._p(mask), tal)
        union_addrs = np.ascontiguousarray(r.addrs)
        union_power = np.ascontiguousarray(r.power, dtype=np.uint64)

        def install():
            rc = L.ibft_set_validator_sets(*a_install)
            assert rc == 0, rc

        def leg_a():
            rc = L.ibft_verify_block_seals_sets(*a_sets)
            assert rc == 0, rc

        def leg_c():
            rc = L.ibft_verify_block_seals(*a_floor)
            assert rc == 0, rc

        # leg B: every run's arguments computed in advance — sub-offsets rebased to 0, pointers into the pinned columns
        timed_runs = min(runs, b_max_runs)
        addr = lambda a: a.ctypes.data
        bmask = np.zeros((n + 63) // 64 + timed_runs + 1, np.uint64)   # (run k's verdict words start at word row0 / 64 + k: no overlap)
        b_args = []
        keep = []
        for k in range(timed_runs):
            b0, b1 = k * E, min(nb, (k + 1) * E)
            s = k % n_sets
            so = np.ascontiguousarray(off[b0:b1 + 1] - off[b0], dtype=np.uint32)
            sa = np.ascontiguousarray(r.addrs[idx[s]])
            keep += [so, sa]
            row0 = int(off[b0])
            b_args.append(((bv._h, 1000 + k, V._p(sa), V._p(power[s]), V_),
                           (bv._h, addr(bh) + 32 * b0, V._p(so), b1 - b0, addr(sig) + 65 * row0, addr(signer) + 20 * row0, None,
                            addr(bmask) + 8 * (row0 // 64 + k), tal)))

        def leg_b():
            for sv, cb in b_args:
                rc = L.ibft_set_validators(*sv)
                assert rc == 0, rc
                rc = L.ibft_verify_block_seals(*cb)
                assert rc == 0, rc

        t_install = timed(install, 0.1) * 1e3
        leg_a()                                   # the key cache learns and builds here (warm); nothing changes cold
        assert V.mask_to_bool(mask, n).all() and all(t.has_quorum == 1 for t in tal)
        times = {"a": [], "b": [], "c": []}
        for _ in range(alternations):
            times["a"].append(timed(leg_a) * 1e3)
            assert V.mask_to_bool(mask, n).all() and all(t.has_quorum == 1 for t in tal)
            times["b"].append(timed(leg_b, 0.5) * 1e3 * runs / timed_runs)
            rc = L.ibft_set_validators(bv._h, 1, V._p(union_addrs), V._p(union_power), pool)   # leg B left the last run's set
            assert rc == 0, rc
            times["c"].append(timed(leg_c) * 1e3)
            assert V.mask_to_bool(mask, n).all()
        cold_lanes, warm_lanes = bv.last_dispatch()
        info = bv.validator_sets_info()
        res = {"v": V_, "blocks": nb, "rows": n, "every": every, "mode": "warm" if warm else "cold", "sets": n_sets, "union": info[1],
               "family_bytes": info[2], "install_ms": t_install, "runs": runs, "b_runs_timed": timed_runs, "cold_lanes": cold_lanes,
               "warm_lanes": warm_lanes, "alternations": alternations, "issue_probe_ns": probe_ns}
        for k, ts in times.items():
            res[k + "_ms"] = float(np.median(ts))
            res[k + "_min_ms"] = min(ts)
            res[k + "_max_ms"] = max(ts)
            res[k + "_all_ms"] = [round(t, 4) for t in ts]
        res["a_over_b"] = res["a_ms"] / res["b_ms"]
        res["a_minus_c_ms"] = res["a_ms"] - res["c_ms"]
        spread = max(res["a_max_ms"] - res["a_min_ms"], res["c_max_ms"] - res["c_min_ms"])
        res["a_minus_c_allowed_ms"] = spread + 0.05 * res["c_ms"]      # beyond this the difference owes a kernel trace
        return res
    finally:
        bv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--v", type=int, nargs="*", default=None)
    ap.add_argument("--blocks", type=int, nargs="*", default=None)
    ap.add_argument("--every", type=str, nargs="*", default=["1", "8", "64", "all"])
    ap.add_argument("--modes", type=str, nargs="*", default=["cold", "warm"])
    ap.add_argument("--pool", type=int, default=256, help="keys the sets slide over (cyclic); the family holds at most this many sets")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--b-max-runs", type=int, default=1024, help="leg B is timed over at most this many runs and scaled")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON lines here")
    a = ap.parse_args()
    shapes = [(100, 655), (4, 16384)] if a.v is None and a.blocks is None else [(v, b) for v in (a.v or [100]) for b in (a.blocks or [655])]
    rows = []
    for V_, nb in shapes:
        if nb * V_ > 65536 or nb < 1 or V_ > a.pool:
            continue
        for mode in a.modes:
            for every in a.every:
                res = measure(V_, nb, every, mode == "warm", a.pool, a.alternations, a.b_max_runs)
                rows.append(res)
                print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for res in rows:
                f.write(json.dumps(res) + "\n")
    cell = lambda r, k: f"{r[k + '_ms']:.3f} ({r[k + '_min_ms']:.3f}…{r[k + '_max_ms']:.3f})"
    print(f"{'V':>4} {'blocks':>6} {'E':>4} {'mode':>5} {'sets':>5} {'probe ns':>8} {'install ms':>10} {'A sets call ms':>22} {'B cut + set ms':>28} "
          f"{'C one set ms':>22} {'A/B':>8} {'A-C ms':>8} {'allowed':>8}")
    for r in rows:
        print(f"{r['v']:>4} {r['blocks']:>6} {r['every']:>4} {r['mode']:>5} {r['sets']:>5} {r['issue_probe_ns']:>8.3f} {r['install_ms']:>10.3f} "
              f"{cell(r, 'a'):>22} {cell(r, 'b'):>28} {cell(r, 'c'):>22} {r['a_over_b']:>8.4f} {r['a_minus_c_ms']:>8.3f} {r['a_minus_c_allowed_ms']:>8.3f}")


if __name__ == "__main__":
    main()
