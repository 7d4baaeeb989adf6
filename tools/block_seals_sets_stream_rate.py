#!/usr/bin/env python3
"""Streamed chain sync across validator-set changes, from the proposals: time per batch of ibft_block_seals_submit_sets_raw
against the two routes a syncer had before it.

    python tools/block_seals_sets_stream_rate.py                         # 65 500 and 16 300 rows at V = 100; cold, warm
    python tools/block_seals_sets_stream_rate.py --blocks 163 --modes cold --out profiles/x.jsonl

Every block carries one seal of every validator of ITS set (V rows, signed on the device) and a proposal of --proposal-bytes
bytes; the set changes every --every blocks, sliding by one validator over a pool of --pool keys.  One lease, one process, one
context; every column — proposal bytes and block_set included — in ibft_pinned_alloc memory; every leg rotates three distinct
batches.  Three legs, alternated --alternations times; the median (min … max) of the rounds is reported, with the lease's
ibft_issue_probe taken beside every round:
  A  ibft_block_seals_submit_sets_raw / ibft_block_seals_collect_ex with one batch kept in flight; the family is installed
     once, outside the timed region
  B  the synchronous route: ibft_proposal_hashes, then ibft_verify_block_seals_sets with those hashes
  C  what a streaming syncer had: the batch cut at every set change — per run of --every blocks ibft_set_validators(the run's
     set) + ibft_block_seals_submit_raw(the run's rows), one run kept in flight, collected with ibft_block_seals_collect_ex
A step is timed by the host clock around calls that end in a wait for the device (a collect, or the synchronous call's
return).  One JSON line per configuration, then a table."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, budget_s=0.3, max_reps=200):
    """seconds per call, over at least three calls behind two untimed ones"""
    fn()
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(3, min(max_reps, int(budget_s / one)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def measure(V_, nb, every, prop_len, warm, pool, alternations):
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    runs = (nb + every - 1) // every
    n_sets = min(runs, pool)
    r = W.make_round(pool, 7, raw_len=64, weighted=True)
    idx = [[(k + j) % pool for j in range(V_)] for k in range(n_sets)]
    power = [np.array([int(r.power[i]) + k for i in ix], np.uint64) for k, ix in enumerate(idx)]
    set_of_block = ((np.arange(nb) // every) % n_sets).astype(np.uint32)
    n = nb * V_
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if warm else 0, max_rows=65536)
    try:
        L, p = bv._L, V._p
        bv.set_validators(1, r.addrs, r.power)     # (sign_seals below; leg C installs its own sets)
        off = (np.arange(nb + 1) * V_).astype(np.uint32)
        who = np.array([idx[s] for s in set_of_block], np.int64).reshape(-1)
        sk = np.frombuffer(b"".join(r.sks), np.uint8).reshape(pool, 32)[who]
        rng = np.random.default_rng(11)
        bt = []
        for k in range(3):   # three distinct batches: (raw, raw_off, round, off, block_set, sig, signer), all pinned
            raw = rng.integers(0, 256, nb * prop_len, dtype=np.uint8)
            roff = (np.arange(nb + 1, dtype=np.uint64) * prop_len).astype(np.uint32)
            rnd = np.arange(nb, dtype=np.uint64) + k
            bh = bv.proposal_hashes((raw, roff), rnd).copy()   # (checked against the oracle by the test suite)
            sig, signer, ok = bv.sign_seals(sk, np.repeat(bh, V_, axis=0))
            assert ok.all()
            bt.append(tuple(V.pinned_copy(np.ascontiguousarray(a)) for a in (raw, roff, rnd, off, set_of_block, sig, signer)))
        bv.set_validator_sets([(r.addrs[ix], pw) for ix, pw in zip(idx, power)])
        mask = np.zeros((n + 63) // 64, np.uint64)
        tal = (V.Tally * nb)()
        hashes = np.zeros((nb, 32), np.uint8)
        state = {"k": 0}

        def nxt():
            state["k"] = (state["k"] + 1) % 3
            return bt[state["k"]]

        def a_submit():
            raw, roff, rnd, o, bset, sig, signer = nxt()
            rc = L.ibft_block_seals_submit_sets_raw(bv._h, p(raw), p(roff), p(rnd), p(o), p(bset), nb, p(sig), p(signer), None)
            assert rc == 0, rc

        def a_collect():
            rc = L.ibft_block_seals_collect_ex(bv._h, p(hashes), None, None, p(mask), tal)
            assert rc == 0, rc

        def a_step():
            a_submit()
            a_collect()

        def leg_b():
            raw, roff, rnd, o, bset, sig, signer = nxt()
            rc = L.ibft_proposal_hashes(bv._h, p(raw), p(roff), p(rnd), nb, p(hashes))
            assert rc == 0, rc
            rc = L.ibft_verify_block_seals_sets(bv._h, p(hashes), p(o), p(bset), nb, p(sig), p(signer), None, p(mask), tal)
            assert rc == 0, rc

        # leg C: every run's arguments computed in advance, for each of the three batches — offsets rebased to 0, pointers into
        # the pinned columns; run j's verdict words and records go to places of their own
        addr = lambda a: a.ctypes.data
        cmask = np.zeros((n + 63) // 64 + runs + 1, np.uint64)
        ctal = (V.Tally * nb)()
        chash = np.zeros((nb, 32), np.uint8)
        keep, c_args = [], []
        for raw, roff, rnd, o, bset, sig, signer in bt:
            per = []
            for j in range(runs):
                b0, b1 = j * every, min(nb, (j + 1) * every)
                s = j % n_sets
                so = V.pinned_copy(np.ascontiguousarray(o[b0:b1 + 1] - o[b0], dtype=np.uint32))
                ro = V.pinned_copy(np.ascontiguousarray(roff[b0:b1 + 1] - roff[b0], dtype=np.uint32))
                sa = np.ascontiguousarray(r.addrs[idx[s]])
                keep += [so, ro, sa]
                row0 = int(o[b0])
                per.append(((bv._h, 1000 + j, p(sa), p(power[s]), V_),
                            (bv._h, addr(raw) + int(roff[b0]), p(ro), addr(rnd) + 8 * b0, p(so), b1 - b0, addr(sig) + 65 * row0,
                             addr(signer) + 20 * row0, None),
                            (bv._h, addr(chash) + 32 * b0, None, None, addr(cmask) + 8 * (row0 // 64 + j),
                             C.cast(C.addressof(ctal) + C.sizeof(V.Tally) * b0, C.c_void_p))))
            c_args.append(per)

        def c_collect(args):
            rc = L.ibft_block_seals_collect_ex(*args)
            assert rc == 0, rc

        def leg_c():
            state["k"] = (state["k"] + 1) % 3
            prev = None
            for sv, sub, col in c_args[state["k"]]:
                rc = L.ibft_set_validators(*sv)     # (waits for the run in flight: the install is synchronous)
                assert rc == 0, rc
                rc = L.ibft_block_seals_submit_raw(*sub)
                assert rc == 0, rc
                if prev is not None:
                    c_collect(prev)
                prev = col
            c_collect(prev)

        def check(m=None):
            assert V.mask_to_bool(mask if m is None else m, n).all() and all(t.has_quorum == 1 for t in tal)

        for _ in range(2):   # warm-up: buffers grow, the key cache learns and builds (warm)
            a_step(); check()
            leg_b(); check()
            leg_c()
            assert all(t.has_quorum == 1 for t in ctal)
        times = {"A": [], "B": [], "C": []}
        probes = []
        for _ in range(alternations):
            probes.append(round(float(bv.issue_probe()[0]), 3))
            a_submit()                     # prime: the timed steps always find one batch in flight
            times["A"].append(timed(a_step) * 1e3)
            a_collect()
            check()
            times["B"].append(timed(leg_b) * 1e3)
            check()
            times["C"].append(timed(leg_c, 0.5) * 1e3)
            assert all(t.has_quorum == 1 for t in ctal)
        res = {"v": V_, "blocks": nb, "rows": n, "every": every, "runs": runs, "sets": n_sets, "proposal_bytes": prop_len,
               "mode": "warm" if warm else "cold", "alternations": alternations, "issue_probe_ns": probes}
        for k, ts in times.items():
            res[k + "_ms"] = float(np.median(ts))
            res[k + "_min_ms"] = min(ts)
            res[k + "_max_ms"] = max(ts)
        res["A_over_B"] = res["A_ms"] / res["B_ms"]
        res["A_over_C"] = res["A_ms"] / res["C_ms"]
        return res
    finally:
        bv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--v", type=int, default=100)
    ap.add_argument("--blocks", type=int, nargs="*", default=[655, 163], help="blocks per batch (× V rows: 65 500 and 16 300)")
    ap.add_argument("--every", type=int, default=64, help="the validator set changes every this many blocks")
    ap.add_argument("--proposal-bytes", type=int, default=1024)
    ap.add_argument("--modes", nargs="*", default=["cold", "warm"])
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON lines and the table here")
    a = ap.parse_args()
    rows, lines = [], []
    for nb in a.blocks:
        for mode in a.modes:
            res = measure(a.v, nb, a.every, a.proposal_bytes, mode == "warm", a.pool, a.alternations)
            rows.append(res)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    cell = lambda r, k: f"{r[k + '_ms']:.3f} ({r[k + '_min_ms']:.3f} … {r[k + '_max_ms']:.3f})"
    lines.append("")
    for r in rows:
        pr = r["issue_probe_ns"]
        lines.append(f"V {r['v']:>4} blocks {r['blocks']:>5} rows {r['rows']:>6} E {r['every']:>3} prop {r['proposal_bytes']:>5} B {r['mode']:>5}  "
                     f"A streamed sets_raw {cell(r, 'A')}  B hashes + sets {cell(r, 'B')}  C cut + submit_raw {cell(r, 'C')}  ms/batch  "
                     f"A/B {r['A_over_B']:.3f}  A/C {r['A_over_C']:.3f}  probe {min(pr)} … {max(pr)} ns")
    print("\n".join(lines[len(rows):]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
