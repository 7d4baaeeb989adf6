#!/usr/bin/env python3
"""The live route across a validator-set change: what one ibft_verify_senders_wire_sets call over a receive-queue batch that
mixes two heights costs against what an integrator had before it — the batch cut by height — and against the floor.

    python tools/wire_sets_rate.py                      # N = 4 096, V = 100; cold, then with known keys
    python tools/wire_sets_rate.py --n 4096 --modes warm

N COMMIT messages signed on the device, half at height h and half at h + 1, INTERLEAVED row by row; the set of h + 1 is the set
of h slid by a tenth of its members over one key pool (V = 100: ten leave, ten join), every validator of a height sending in
turn.  Three legs on ONE context, alternated --alternations times (median and min … max of the rounds are reported); every leg
is the C call itself with preallocated out buffers and no out_rows, ending in the call's own synchronisation:
  A  one ibft_verify_senders_wire_sets call over the whole batch; family and height map are installed once, outside the timed
     region — their install time is reported beside it
  B  what the parent forces: the rows split by height on the host (the split itself is timed apart: "split_ms" — it is host
     work on bytes the integrator has to decode first), then per height ibft_set_validators + ibft_verify_senders_wire
  C  the floor: ONE ibft_verify_senders_wire over the whole batch under the set of h.  Its answers are wrong at the boundary
     ("c_wrong_rows": joiners of h + 1 rejected, leavers accepted); it is what the same rows cost without the feature
A / B is the gain, A / C the price (wire_row_set_kernel, one dense-table load per row and the per-set sums in the tally, two
more columns out).  cold: no key cache; warm: IBFT_FLAG_PUBKEY_CACHE after the first calls built the tables.  The answers of A
are checked against B's before anything is timed.  One JSON line per mode, then a table."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, budget_s=0.25, max_reps=400):
    """seconds per call"""
    fn()
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(5, min(max_reps, int(budget_s / one)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def measure(n, V_, warm, alternations, height=1000):
    import go_ibft_amd.simulate as S
    import go_ibft_amd.verifier as V
    slide = max(1, V_ // 10)
    pool = V_ + slide
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if warm else 0, max_rows=max(n, 1024))
    try:
        L, h, p = bv._L, bv._h, V._p
        sk = S.secret_keys(29, pool)
        H = bv.proposal_hash(b"wire_sets_rate", 0)
        hcol = np.tile(np.frombuffer(H, np.uint8), (pool, 1))
        members = [list(range(0, V_)), list(range(slide, slide + V_))]
        per_height = []
        for k in (0, 1):       # every validator of the height signs once; the batch repeats them in turn
            w, o, frm, ok = S._sign_messages(bv, sk[members[k]], V.MSG_COMMIT, height + k, 0, hcol[:V_])
            assert ok.all()
            per_height.append(([w[int(o[i]):int(o[i + 1])] for i in range(V_)], frm))
        msgs = [per_height[j & 1][0][(j >> 1) % V_] for j in range(n)]
        addrs = [per_height[k][1] for k in (0, 1)]
        power = [np.arange(1, V_ + 1, dtype=np.uint64) + k for k in (0, 1)]

        def pack(rows):
            off = np.zeros(len(rows) + 1, np.uint32)
            off[1:] = np.cumsum([len(x) for x in rows])
            return np.frombuffer(b"".join(rows), np.uint8).copy(), off
        wire, off = pack(msgs)
        t0 = time.perf_counter()
        lens = np.diff(off.astype(np.int64))
        sub = []
        for k in (0, 1):       # the host split: gather the bytes of every second message
            idx = np.arange(k, n, 2)
            o2 = np.zeros(len(idx) + 1, np.uint32)
            o2[1:] = np.cumsum(lens[idx])
            src = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)
            sub.append((wire[src], o2, idx))
        split_s = time.perf_counter() - t0

        mw = (n + 63) // 64
        mask_a, mask_c = np.zeros(mw, np.uint64), np.zeros(mw, np.uint64)
        mask_b = [np.zeros((len(s[2]) + 63) // 64 or 1, np.uint64) for s in sub]
        rset, vidx = np.zeros(n, np.int32), np.zeros(n, np.int32)
        tal2, tal = (V.Tally * 2)(), V.Tally()
        first, rs = np.array([height, height + 1, height + 2], np.uint64), np.array([0, 1], np.uint32)

        def chk(rc):
            if rc:
                raise RuntimeError(f"rc = {rc}: {L.ibft_last_error(h).decode()}")

        t0 = time.perf_counter()
        bv.set_validator_sets([(height + k, addrs[k], power[k]) for k in (0, 1)])
        bv.set_height_sets(first, rs)
        install_s = time.perf_counter() - t0

        def leg_a():
            chk(L.ibft_verify_senders_wire_sets(h, p(wire), p(off), n, p(mask_a), None, p(rset), p(vidx), tal2))

        def leg_b():
            for k in (0, 1):
                chk(L.ibft_set_validators(h, height + k, p(addrs[k]), p(power[k]), V_))
                chk(L.ibft_verify_senders_wire(h, p(sub[k][0]), p(sub[k][1]), len(sub[k][2]), p(mask_b[k]), None, C.byref(tal)))

        def leg_c():
            chk(L.ibft_verify_senders_wire(h, p(wire), p(off), n, p(mask_c), None, C.byref(tal)))

        # the answers first: A against B, row by row; C against A
        for _ in range(3 if warm else 1):
            leg_a()
            leg_b()
        bits_a = V.mask_to_bool(mask_a, n)
        bits_b = np.zeros(n, bool)
        for k in (0, 1):
            bits_b[sub[k][2]] = V.mask_to_bool(mask_b[k], len(sub[k][2]))
        assert (bits_a == bits_b).all() and bits_a.all() and (rset == (np.arange(n) & 1)).all()
        chk(L.ibft_set_validators(h, height, p(addrs[0]), p(power[0]), V_))
        leg_c()
        c_wrong = int((V.mask_to_bool(mask_c, n) != bits_a).sum())

        rounds = {"A": [], "B": [], "C": []}
        for _ in range(alternations):
            rounds["A"].append(timed(leg_a))
            rounds["B"].append(timed(leg_b))
            chk(L.ibft_set_validators(h, height, p(addrs[0]), p(power[0]), V_))      # (outside the timed region)
            rounds["C"].append(timed(leg_c))
        probe = bv.issue_probe() if hasattr(bv, "issue_probe") else None
        ms = {k: 1e3 * statistics.median(v) for k, v in rounds.items()}
        return {"n": n, "validators": V_, "slide": slide, "mode": "warm" if warm else "cold", "alternations": alternations,
                "a_ms": round(ms["A"], 4), "b_ms": round(ms["B"], 4), "c_ms": round(ms["C"], 4),
                "a_range_ms": [round(1e3 * min(rounds["A"]), 4), round(1e3 * max(rounds["A"]), 4)],
                "b_range_ms": [round(1e3 * min(rounds["B"]), 4), round(1e3 * max(rounds["B"]), 4)],
                "c_range_ms": [round(1e3 * min(rounds["C"]), 4), round(1e3 * max(rounds["C"]), 4)],
                "a_over_b": round(ms["A"] / ms["B"], 3), "a_over_c": round(ms["A"] / ms["C"], 3),
                "split_ms": round(1e3 * split_s, 3), "install_ms": round(1e3 * install_s, 3), "c_wrong_rows": c_wrong,
                "issue_probe_ns": probe}
    finally:
        bv.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--v", type=int, default=100)
    ap.add_argument("--modes", default="cold,warm")
    ap.add_argument("--alternations", type=int, default=5)
    a = ap.parse_args()
    out = []
    for mode in a.modes.split(","):
        rec = measure(a.n, a.v, mode == "warm", a.alternations)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    print(f"{'mode':<6}{'A ms':>10}{'B ms':>10}{'C ms':>10}{'A/B':>8}{'A/C':>8}{'split ms':>10}{'install ms':>12}{'C wrong':>9}")
    for r in out:
        print(f"{r['mode']:<6}{r['a_ms']:>10.4f}{r['b_ms']:>10.4f}{r['c_ms']:>10.4f}{r['a_over_b']:>8.3f}{r['a_over_c']:>8.3f}"
              f"{r['split_ms']:>10.3f}{r['install_ms']:>12.3f}{r['c_wrong_rows']:>9}")


if __name__ == "__main__":
    main()
