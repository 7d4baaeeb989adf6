#!/usr/bin/env python3
"""What checking the committed seals inside the quorum records (ibft_verify_messages_wire_views) costs on top of the views call,
and against what a caller of the views call has to do for the same answer.

    python tools/wire_view_seals_rate.py                          # N = 4 096, V = 100; both mixes, cold and with known keys
    python tools/wire_view_seals_rate.py --legs b --mixes half    # the views call alone (also runs on a library without the new
                                                                  # call: IBFT_GPU_LIB=<the parent's libibftgpu.so>, for the A/B of leg b)

The batch of tools/wire_views_rate.py: N messages signed on the device, of two interleaved heights h and h + 1 whose sets differ
in a tenth of their members (V = 100, ten leave, ten join), every validator's messages of round 0 repeated in turn, a twentieth
of the rows in round 1; every COMMIT's seal is valid for the hash it names.  Two mixes: `commit` — every message a COMMIT —,
`half` — PREPAREs and COMMITs half and half.  Legs on ONE context, each repetition timed on its own with a synchronising call
at its end, the legs alternated repetition by repetition (median and min … max of --reps repetitions after --warmup):
  a  ibft_verify_messages_wire_views over the batch (views_cap = n; out_rows not asked for)
  b  ibft_verify_senders_wire_views alone on the same batch — a − b is the price of the seals
  c  what a caller does today: b WITH out_rows; on the host the stored COMMIT rows gathered per height into (hash, seal, From)
     columns ("c_host_ms", timed and reported separately, also contained in c_ms; the seals come from a column the tool parsed
     out of the messages beforehand, which a real caller would have to do inside this pass); per height one
     ibft_set_validators and one ibft_verify_seals over those rows; per COMMIT record one ibft_tally
  d  ONE ibft_verify_seals over the seal rows of leg a (all sealable rows, under the union as one set): what the same seal
     checks cost as a launch of their own, to compare a − b with
The seal bits and COMMIT records of a are checked against c's before anything is timed.  One JSON line per (mix, mode), then a
table."""
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
COMMIT = 2


def make_batch(bv, S, V, n, V_, mix, height):
    """→ (wire u8, off u32, addrs per height, powers per height, seal column (n, 65), union addrs)"""
    from oracle import wire_parse as WP
    slide = max(1, V_ // 10)
    pool = V_ + slide
    sk = S.secret_keys(29, pool)
    H = bv.proposal_hash(b"wire_view_seals_rate", 0)
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
        typ = V.MSG_COMMIT if mix == "commit" or (j >> 1) // V_ % 2 else V.MSG_PREPARE
        msgs.append(signed[(k, typ, 1 if j % 20 == 19 else 0)][i])
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in msgs])
    seal = np.zeros((n, 65), np.uint8)
    cache = {}
    for j, m in enumerate(msgs):
        key = bytes(m)
        if key not in cache:
            s = WP.expected(key).committed_seal
            cache[key] = np.frombuffer(s, np.uint8) if len(s) == 65 else np.zeros(65, np.uint8)
        seal[j] = cache[key]
    power = [np.arange(1, V_ + 1, dtype=np.uint64) + k for k in (0, 1)]
    union = np.unique(np.concatenate(addrs), axis=0)
    return np.frombuffer(b"".join(bytes(x) for x in msgs), np.uint8).copy(), off, addrs, power, seal, union


def measure(n, V_, mix, warm, reps, warmup, legs, height=1000):
    import go_ibft_amd.simulate as S
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if warm else 0, max_rows=max(n, 1024))
    try:
        L, h, p = bv._L, bv._h, V._p
        wire, off, addrs, power, seal_col, union = make_batch(bv, S, V, n, V_, mix, height)
        mw = (n + 63) // 64
        mask, stored, seal = np.zeros(mw, np.uint64), np.zeros(mw, np.uint64), np.zeros(mw, np.uint64)
        rset, vidx, view = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        rows = np.zeros(n, V.WIRE_ROW)
        tal2, tal = (V.Tally * 2)(), V.Tally()
        nv = C.c_uint32(0)
        first, rs = np.array([height, height + 1, height + 2], np.uint64), np.array([0, 1], np.uint32)
        host_s = []

        def chk(rc):
            if rc:
                raise RuntimeError(f"rc = {rc}: {L.ibft_last_error(h).decode()}")

        bv.set_validator_sets([(height + k, addrs[k], power[k]) for k in (0, 1)])
        bv.set_height_sets(first, rs)
        have = hasattr(L, "ibft_verify_messages_wire_views")
        views, views_c = np.zeros(n, V.WIRE_VIEW), np.zeros(n, V.WIRE_VIEW)

        def leg_a():
            chk(L.ibft_verify_messages_wire_views(h, p(wire), p(off), n, n, p(mask), None, p(rset), p(vidx), tal2, p(view), p(stored), p(views),
                                                  C.byref(nv), p(seal)))

        def leg_b():
            chk(L.ibft_verify_senders_wire_views(h, p(wire), p(off), n, n, p(mask), None, p(rset), p(vidx), tal2, p(view), p(stored), p(views_c),
                                                 C.byref(nv)))

        out_c = {}
        seal_c = np.zeros(n, bool)

        def leg_c():
            chk(L.ibft_verify_senders_wire_views(h, p(wire), p(off), n, n, p(mask), p(rows), p(rset), p(vidx), tal2, p(view), p(stored), p(views_c),
                                                 C.byref(nv)))
            t0 = time.perf_counter()
            st = V.mask_to_bool(stored, n) & (rows["type"] == COMMIT)
            gathered = []
            for k in (0, 1):
                idx = np.nonzero(st & (rset == k))[0]
                gathered.append((idx, np.ascontiguousarray(rows["proposal_hash"][idx]), np.ascontiguousarray(seal_col[idx]),
                                 np.ascontiguousarray(rows["from"][idx])))
            host_s.append(time.perf_counter() - t0)
            seal_c[:] = False
            out_c.clear()
            nviews = min(int(nv.value), n)
            for k, (idx, hh, sg, fr) in enumerate(gathered):
                chk(L.ibft_set_validators(h, height + k, p(addrs[k]), p(power[k]), V_))
                bits = np.zeros((len(idx) + 63) // 64 or 1, np.uint64)
                chk(L.ibft_verify_seals(h, p(hh), p(sg), p(fr), None, len(idx), p(bits), C.byref(tal)))
                seal_c[idx] = V.mask_to_bool(bits, len(idx))
                for v in range(nviews):
                    r = views_c[v]
                    if int(r["type"]) != COMMIT or int(r["set"]) != k:
                        continue
                    sel = idx[view[idx] == v]
                    frm = np.ascontiguousarray(rows["from"][sel])
                    m = V.bool_to_mask(seal_c[sel]) if len(sel) else np.zeros(1, np.uint64)
                    chk(L.ibft_tally(h, p(frm), p(m), len(sel), C.byref(tal)))
                    out_c[v] = (tal.power_lo, tal.power_hi, tal.valid_rows, tal.distinct_senders, tal.has_quorum)

        d_cols = {}

        def leg_d():
            hh, sg, fr = d_cols["cols"]
            chk(L.ibft_verify_seals(h, p(hh), p(sg), p(fr), None, len(sg), p(d_cols["bits"]), C.byref(tal)))

        fns = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}
        legs = [x for x in legs if have or x in ("b",)]
        n_views = seal_rows = None
        if "a" in legs:       # the answers first: a's seal bits and COMMIT records against c's
            for _ in range(3 if warm else 1):
                leg_c()
                leg_a()
            n_views = int(nv.value)
            seal_rows = bv.wire_seal_stats()[1]
            got = V.mask_to_bool(seal, n)
            st = V.mask_to_bool(stored, n) & (rows["type"] == COMMIT)
            assert (got[st] == seal_c[st]).all() and got[st].all() and V.mask_to_bool(mask, n).all()
            for v, want in out_c.items():
                t = views["tally"][v]
                assert (int(t["power_lo"]), int(t["power_hi"]), int(t["valid_rows"]), int(t["distinct_senders"]), int(t["has_quorum"])) == want, v
            sealable = np.nonzero(rows["type"] == COMMIT)[0]
            assert len(sealable) == seal_rows
            d_cols["cols"] = (np.ascontiguousarray(rows["proposal_hash"][sealable]), np.ascontiguousarray(seal_col[sealable]),
                              np.ascontiguousarray(rows["from"][sealable]))
            d_cols["bits"] = np.zeros((len(sealable) + 63) // 64 or 1, np.uint64)
        if "d" in legs:       # the seal rows under ONE set: the union with unit powers (the verdicts do not depend on the powers)
            chk(L.ibft_set_validators(h, height, p(union), p(np.ones(len(union), np.uint64)), len(union)))
            for _ in range(3 if warm else 1):
                leg_d()
            assert V.mask_to_bool(d_cols["bits"], seal_rows).all()
        times = {k: [] for k in legs}
        for rep in range(warmup + reps):
            for k in legs:
                if k == "d":   # (leg c installs the heights' sets: the union goes back in, outside the timed part)
                    chk(L.ibft_set_validators(h, height, p(union), p(np.ones(len(union), np.uint64)), len(union)))
                t0 = time.perf_counter()
                fns[k]()
                dt = time.perf_counter() - t0
                if rep >= warmup:
                    times[k].append(dt)
        rec = {"n": n, "validators": V_, "mix": mix, "mode": "warm" if warm else "cold", "reps": reps, "warmup": warmup, "views": n_views,
               "seal_rows": seal_rows, "library": "IBFT_GPU_LIB" if os.environ.get("IBFT_GPU_LIB") else "tree"}
        for k in legs:
            rec[f"{k}_ms"] = round(1e3 * statistics.median(times[k]), 4)
            rec[f"{k}_range_ms"] = [round(1e3 * min(times[k]), 4), round(1e3 * max(times[k]), 4)]
        if "a" in legs and "b" in legs:
            rec["a_minus_b_ms"] = round(rec["a_ms"] - rec["b_ms"], 4)
        if "c" in legs:
            rec["c_host_ms"] = round(1e3 * statistics.median(host_s[-reps:]), 4)
            rec["c_less_host_ms"] = round(rec["c_ms"] - rec["c_host_ms"], 4)
            rec["c_stored_commit_rows"] = int((V.mask_to_bool(stored, n) & (rows["type"] == COMMIT)).sum())
        return rec
    finally:
        bv.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--v", type=int, default=100)
    ap.add_argument("--modes", default="cold,warm")
    ap.add_argument("--mixes", default="commit,half")
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    out = []
    for mix in a.mixes.split(","):
        for mode in a.modes.split(","):
            rec = measure(a.n, a.v, mix, mode == "warm", a.reps, a.warmup, a.legs.split(","))
            print(json.dumps(rec), flush=True)
            out.append(rec)
    print(f"{'mix':<8}{'mode':<6}{'seal rows':>10}{'a ms':>10}{'b ms':>10}{'a-b ms':>10}{'d ms':>10}{'c ms':>10}{'c host':>10}{'c-host':>10}")
    f = lambda r, k, w, d: f"{r[k]:>{w}.{d}f}" if r.get(k) is not None else f"{'-':>{w}}"  # noqa: E731
    for r in out:
        print(f"{r['mix']:<8}{r['mode']:<6}{str(r['seal_rows'] if r['seal_rows'] is not None else '-'):>10}{f(r, 'a_ms', 10, 4)}{f(r, 'b_ms', 10, 4)}"
              f"{f(r, 'a_minus_b_ms', 10, 4)}{f(r, 'd_ms', 10, 4)}{f(r, 'c_ms', 10, 4)}{f(r, 'c_host_ms', 10, 4)}{f(r, 'c_less_host_ms', 10, 4)}")


if __name__ == "__main__":
    main()
