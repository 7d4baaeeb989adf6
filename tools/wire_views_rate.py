#!/usr/bin/env python3
"""What the quorum records of ibft_verify_senders_wire_views cost on top of the sets call, and against what they replace.

    python tools/wire_views_rate.py                         # N = 4 096, V = 100; both shapes, cold and with known keys
    python tools/wire_views_rate.py --legs b --shapes honest   # the sets call alone (also runs on a library without the views call:
                                                               # IBFT_GPU_LIB=<the parent's libibftgpu.so>, for the A/B of leg b)

N PREPARE and COMMIT messages signed on the device, of two interleaved heights h and h + 1 whose sets differ in a tenth of their
members (tools/wire_sets_rate.py's family: V = 100, ten leave, ten join).  Two shapes:
  honest   every validator of a height sends its PREPARE and its COMMIT of round 0, the batch repeats them in turn, and a
           twentieth of the rows (all of height h + 1) belong to round 1: 6 views
  hostile  the same, except that 2 000 rows are one validator's PREPAREs, each in a round of its own: 2 000 views and more
Three legs on ONE context, alternated --alternations times in one process (median and min … max of the rounds); every leg ends
in a synchronisation of its own:
  a  ibft_verify_senders_wire_views over the batch (views_cap = n; out_rows not asked for)
  b  ibft_verify_senders_wire_sets alone on the same batch — a − b is the price of the feature
  c  the parent's way to the same records: b WITH out_rows, then on the host the rows grouped by view and hash and the last
     message per (view, sender) kept, then per height one ibft_set_validators and per record an ibft_tally over its stored senders.
     ("c_host_ms": the grouping pass alone, numpy + a dictionary walk.)  The PREPARE rule is left out of c (no proposer table is
     installed in this tool): it would add a lookup per record on either side.
The records of a are checked against c's before anything is timed.  One JSON line per (shape, mode), then a table."""
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
HOSTILE_ROWS = 2000


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


def make_batch(bv, S, V, n, V_, shape, height):
    """→ (wire u8, off u32, addrs per height, powers per height)"""
    slide = max(1, V_ // 10)
    pool = V_ + slide
    sk = S.secret_keys(29, pool)
    H = bv.proposal_hash(b"wire_views_rate", 0)
    hcol = np.tile(np.frombuffer(H, np.uint8), (pool, 1))
    members = [list(range(0, V_)), list(range(slide, slide + V_))]
    signed, addrs = {}, []
    for k in (0, 1):
        for typ in (V.MSG_PREPARE, V.MSG_COMMIT):
            for rnd in (0, 1):
                w, o, frm, ok = S._sign_messages(bv, sk[members[k]], typ, height + k, rnd, hcol[:V_])
                assert ok.all()
                signed[(k, typ, rnd)] = [w[int(o[i]):int(o[i + 1])] for i in range(V_)]
        addrs.append(frm)
    msgs = []
    for j in range(n):
        k, i = j & 1, (j >> 1) % V_
        typ = V.MSG_PREPARE if (j >> 1) // V_ % 2 == 0 else V.MSG_COMMIT
        msgs.append(signed[(k, typ, 1 if j % 20 == 19 else 0)][i])
    if shape == "hostile":       # validator 3 of height h: a PREPARE per round, spread over the batch
        one = sk[members[0][3]:members[0][3] + 1]
        at = np.linspace(0, n - 1, HOSTILE_ROWS).astype(int)
        for r, j in enumerate(at):
            w, o, _, ok = S._sign_messages(bv, one, V.MSG_PREPARE, height, 2 + r, hcol[:1])
            assert ok.all()
            msgs[int(j)] = w
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in msgs])
    power = [np.arange(1, V_ + 1, dtype=np.uint64) + k for k in (0, 1)]
    return np.frombuffer(b"".join(msgs), np.uint8).copy(), off, addrs, power


def host_records(rows, bits, rset):
    """the host pass of leg c: group valid rows by (height, round, type, hash), keep the last row per (view, sender) → a list of
    (set, From column of the stored rows) in order of the records' first rows"""
    valid = np.nonzero(bits)[0]
    last = {}
    for j in valid:
        r = rows[j]
        last[(int(r["type"]), int(r["height"]), int(r["round"]), r["from"].tobytes())] = j
    stored = set(last.values())
    groups = {}
    for j in valid:
        r = rows[j]
        g = groups.setdefault((int(r["height"]), int(r["round"]), int(r["type"]), r["proposal_hash"][:int(r["hash_len"])].tobytes()),
                              [int(rset[j]), []])
        if j in stored:
            g[1].append(j)
    return [(s, rows["from"][idx] if idx else np.zeros((0, 20), np.uint8)) for s, idx in groups.values()]


def measure(n, V_, shape, warm, alternations, legs, height=1000):
    import go_ibft_amd.simulate as S
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if warm else 0, max_rows=max(n, 1024))
    try:
        L, h, p = bv._L, bv._h, V._p
        wire, off, addrs, power = make_batch(bv, S, V, n, V_, shape, height)
        mw = (n + 63) // 64
        mask, stored = np.zeros(mw, np.uint64), np.zeros(mw, np.uint64)
        rset, vidx, view = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        rows = np.zeros(n, V.WIRE_ROW)
        tal2, tal = (V.Tally * 2)(), V.Tally()
        nv = C.c_uint32(0)
        first, rs = np.array([height, height + 1, height + 2], np.uint64), np.array([0, 1], np.uint32)
        ones = np.full(mw, 2**64 - 1, np.uint64)
        host_s = []

        def chk(rc):
            if rc:
                raise RuntimeError(f"rc = {rc}: {L.ibft_last_error(h).decode()}")

        bv.set_validator_sets([(height + k, addrs[k], power[k]) for k in (0, 1)])
        bv.set_height_sets(first, rs)
        have_views = hasattr(L, "ibft_verify_senders_wire_views")
        views = np.zeros(n, V.WIRE_VIEW) if have_views else None

        def leg_a():
            chk(L.ibft_verify_senders_wire_views(h, p(wire), p(off), n, n, p(mask), None, p(rset), p(vidx), tal2, p(view), p(stored), p(views),
                                                 C.byref(nv)))

        def leg_b():
            chk(L.ibft_verify_senders_wire_sets(h, p(wire), p(off), n, p(mask), None, p(rset), p(vidx), tal2))

        out_c = []

        def leg_c():
            chk(L.ibft_verify_senders_wire_sets(h, p(wire), p(off), n, p(mask), p(rows), p(rset), p(vidx), tal2))
            t0 = time.perf_counter()
            recs = host_records(rows, V.mask_to_bool(mask, n), rset)
            host_s.append(time.perf_counter() - t0)
            out_c[:] = [None] * len(recs)
            for k in (0, 1):                  # one ibft_set_validators per height, then one ibft_tally per record of that height
                chk(L.ibft_set_validators(h, height + k, p(addrs[k]), p(power[k]), V_))
                for i, (s, frm) in enumerate(recs):
                    if s != k:
                        continue
                    frm = np.ascontiguousarray(frm)
                    chk(L.ibft_tally(h, p(frm), p(ones), len(frm), C.byref(tal)))
                    out_c[i] = (tal.power_lo, tal.power_hi, tal.valid_rows, tal.distinct_senders, tal.has_quorum)

        fns = {"a": leg_a, "b": leg_b, "c": leg_c}
        legs = [x for x in legs if x != "a" or have_views]
        n_views = None
        if "a" in legs and "c" in legs:       # the answers first: a's records against c's
            for _ in range(3 if warm else 1):
                leg_a()
                leg_c()
            n_views = int(nv.value)
            assert n_views == len(out_c), (n_views, len(out_c))
            got = [(int(t["power_lo"]), int(t["power_hi"]), int(t["valid_rows"]), int(t["distinct_senders"]), int(t["has_quorum"]))
                   for t in views["tally"][:n_views]]
            assert got == out_c
            assert V.mask_to_bool(mask, n).all()
        rounds = {k: [] for k in legs}
        for _ in range(alternations):
            for k in legs:
                rounds[k].append(timed(fns[k]))
        probe = bv.issue_probe() if hasattr(bv, "issue_probe") else None
        rec = {"n": n, "validators": V_, "shape": shape, "mode": "warm" if warm else "cold", "alternations": alternations, "views": n_views,
               "library": "IBFT_GPU_LIB" if os.environ.get("IBFT_GPU_LIB") else "tree", "issue_probe_ns": probe}
        for k in legs:
            rec[f"{k}_ms"] = round(1e3 * statistics.median(rounds[k]), 4)
            rec[f"{k}_range_ms"] = [round(1e3 * min(rounds[k]), 4), round(1e3 * max(rounds[k]), 4)]
        if "a" in legs and "b" in legs:
            rec["a_minus_b_ms"] = round(rec["a_ms"] - rec["b_ms"], 4)
        if "a" in legs and "c" in legs:
            rec["a_over_c"] = round(rec["a_ms"] / rec["c_ms"], 3)
            rec["c_host_ms"] = round(1e3 * statistics.median(host_s), 3)
        return rec
    finally:
        bv.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--v", type=int, default=100)
    ap.add_argument("--modes", default="cold,warm")
    ap.add_argument("--shapes", default="honest,hostile")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--alternations", type=int, default=5)
    a = ap.parse_args()
    out = []
    for shape in a.shapes.split(","):
        for mode in a.modes.split(","):
            rec = measure(a.n, a.v, shape, mode == "warm", a.alternations, a.legs.split(","))
            print(json.dumps(rec), flush=True)
            out.append(rec)
    print(f"{'shape':<9}{'mode':<6}{'views':>7}{'a ms':>10}{'b ms':>10}{'c ms':>10}{'a-b ms':>10}{'a/c':>8}{'c host ms':>11}")
    f = lambda r, k, w, d: f"{r[k]:>{w}.{d}f}" if r.get(k) is not None else f"{'-':>{w}}"  # noqa: E731
    for r in out:
        print(f"{r['shape']:<9}{r['mode']:<6}{str(r['views'] if r['views'] is not None else '-'):>7}{f(r, 'a_ms', 10, 4)}{f(r, 'b_ms', 10, 4)}"
              f"{f(r, 'c_ms', 10, 4)}{f(r, 'a_minus_b_ms', 10, 4)}{f(r, 'a_over_c', 8, 3)}{f(r, 'c_host_ms', 11, 3)}")


if __name__ == "__main__":
    main()
