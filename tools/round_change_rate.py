#!/usr/bin/env python3
"""What the per-round quorum records of ibft_decide_round_changes_wire cost on top of the decide call, and against what they
replace, on the round change of simulate.make_round_change_round (q = ⌊2N/3⌋ + 1 ROUND_CHANGE messages, every one with the
PreparedCertificate of the prepared round), records only — no per-row output.

    python tools/round_change_rate.py                          # N = 256 and 1 024, cold and with known keys
    python tools/round_change_rate.py --parent-lib PATH         # … and the decide call on another build of the library
    python tools/round_change_rate.py --rehearse                # the batches, the caller's host pass and the checks, no device

Legs, alternated --alternations times in one process on one context (median and min … max of the rounds); every leg ends in a
synchronisation of its own:
  a  ibft_decide_round_changes_wire (rc_cap = n, a query) — one 64-byte answer tells the caller what to do
  b  ibft_decide_certificates_wire on the same batch — a − b is the price of the feature
  c  the caller's route today: b, then on the host the records and decisions grouped by (height, round), the last message per
     (round, sender) kept, those whose round_change is 1 tallied with one ibft_tally per round, the highest round ≥ 1 with a
     quorum picked.  ("c_host_ms": the grouping pass alone.)
  p  (--parent-lib) leg b on that library, in child processes that alternate with child processes on the tree's library: the new
     kernels must not slow the decide call beyond the spread of repeated runs, which is reported ("b_child_range_ms").
The answer of a is checked against c's before anything is timed.  The hostile batch: the honest quorum beside one member's
ROUND_CHANGE in each of 2 000 rounds.  One JSON line per (N, shape, mode), then a table.  Nothing is asserted about the times."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOSTILE_ROUNDS = 2000


def timed(fn, budget_s=0.5, max_reps=100):
    """seconds per call"""
    fn()
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(3, min(max_reps, int(budget_s / one)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def host_pass(certs, dec, n):
    """the host pass of leg c over the level-0 records: → {(height, round): From column of the stored rows whose closure holds},
    in the order of the keys' first rows"""
    last = {}
    for i in range(n):
        c = certs[i]
        if c["cls"] == 0 and c["type"] == 3 and c["from_len"] == 20 and c["bits"] & 1:
            last[(int(c["height"]), int(c["round"]), c["from"].tobytes())] = i
    groups = {}
    for (h, r, _), i in sorted(last.items(), key=lambda kv: kv[1]):
        g = groups.setdefault((h, r), [])
        if dec[i]["round_change"] == 1:
            g.append(i)
    return {k: certs["from"][idx] if idx else np.zeros((0, 20), np.uint8) for k, idx in groups.items()}


def hostile_tail(bv, S, r, n_rounds):
    """one member's bare ROUND_CHANGE in each of n_rounds rounds above the round change's own"""
    sk = S.secret_keys(5, r.n)[:1]
    msgs = []
    for k in range(n_rounds):
        w, o, _, ok = bv.sign_envelopes(sk, 3, r.height, r.new_round + 1 + k, b"", 0, 0)
        assert ok.all()
        msgs.append(bytes(w))
    return msgs


def measure(n, shape, warm, alternations, legs):
    import go_ibft_amd.simulate as S
    import go_ibft_amd.verifier as V
    q = (2 * n) // 3 + 1
    extra = HOSTILE_ROUNDS if shape == "hostile" else 0
    cap = q * (q + 1) + extra + 64
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if warm else 0, max_rows=cap)
    try:
        L, h, p = bv._L, bv._h, V._p
        r = S.make_round_change_round(bv, n, seed=5, distinct=True)
        msgs = [r.wire[int(r.off[i]):int(r.off[i + 1])] for i in range(r.q)] + (hostile_tail(bv, S, r, extra) if extra else [])
        m = len(msgs)
        off = np.zeros(m + 1, np.uint32)
        off[1:] = np.cumsum([len(x) for x in msgs])
        wire = np.frombuffer(b"".join(msgs), np.uint8).copy()
        bv.set_validators(r.height, r.addrs, r.power)
        bv.set_proposers(r.height, 0, [r.addrs[k % n].tobytes() for k in range(8)])
        certs, dec = np.zeros(m, V.CERT_VERDICT), np.zeros(m, V.CERT_DECISION)
        n_rows, n_certs, n_rc = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        have = hasattr(L, "ibft_decide_round_changes_wire")
        recs, ans = (np.zeros(m, V.RC_RECORD), np.zeros(1, V.RC_ANSWER)) if have else (None, None)
        query = V.rc_query(r.height, r.prepared_round) if have else None
        tal = V.Tally()
        ones = np.full((m + 63) // 64, 2**64 - 1, np.uint64)
        host_s, out_c = [], {}

        def chk(rc):
            if rc:
                raise RuntimeError(f"rc = {rc}: {L.ibft_last_error(h).decode()}")

        def leg_a():
            chk(L.ibft_decide_round_changes_wire(h, p(wire), p(off), m, cap, m, C.byref(n_rows), C.byref(n_certs), p(certs), p(dec), None, None, None,
                                                 None, None, None, p(query), None, None, p(recs), m, C.byref(n_rc), p(ans)))

        def leg_b():
            chk(L.ibft_decide_certificates_wire(h, p(wire), p(off), m, cap, m, C.byref(n_rows), C.byref(n_certs), p(certs), p(dec), None, None, None,
                                                None, None, None))

        def leg_c():
            leg_b()
            t0 = time.perf_counter()
            groups = host_pass(certs, dec, m)
            host_s.append(time.perf_counter() - t0)
            best = None
            for (hh, rnd), frm in groups.items():
                frm = np.ascontiguousarray(frm)
                chk(L.ibft_tally(h, p(frm), p(ones), len(frm), C.byref(tal)))
                if hh == r.height and rnd >= 1 and tal.has_quorum and (best is None or rnd > best):
                    best = rnd
            out_c["round"], out_c["keys"] = best, len(groups)

        fns = {"a": leg_a, "b": leg_b, "c": leg_c}
        legs = [x for x in legs if x in fns and (x != "a" or have)]
        if "a" in legs and "c" in legs:       # the answers first
            for _ in range(3 if warm else 1):
                leg_a()
                leg_c()
            a0 = ans[0]
            assert int(n_rc.value) == out_c["keys"] == 1 + extra, (int(n_rc.value), out_c["keys"], extra)
            assert (int(a0["extended"]), int(a0["round"])) == (1, out_c["round"]) and out_c["round"] == r.new_round, (a0, out_c)
        rounds = {k: [] for k in legs}
        for _ in range(alternations):
            for k in legs:
                rounds[k].append(timed(fns[k]))
        rec = {"n": n, "messages": m, "rows": int(n_rows.value), "shape": shape, "mode": "warm" if warm else "cold", "alternations": alternations,
               "keys": int(n_rc.value) if have and "a" in legs else None, "library": os.environ.get("IBFT_GPU_LIB") or "tree"}
        for k in legs:
            rec[f"{k}_ms"] = round(1e3 * statistics.median(rounds[k]), 4)
            rec[f"{k}_range_ms"] = [round(1e3 * min(rounds[k]), 4), round(1e3 * max(rounds[k]), 4)]
        if "a" in legs and "b" in legs:
            rec["a_minus_b_ms"] = round(rec["a_ms"] - rec["b_ms"], 4)
        if "c" in legs:
            rec["c_host_ms"] = round(1e3 * statistics.median(host_s), 3)
        return rec
    finally:
        bv.close()


def child_b(n, warm, lib, alternations):
    """leg b alone in a fresh process, on `lib` (None: the tree's)"""
    env = dict(os.environ)
    env.pop("IBFT_GPU_LIB", None)
    if lib:
        env["IBFT_GPU_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--sizes", str(n), "--modes", "warm" if warm else "cold", "--shapes", "honest",
                          "--legs", "b", "--alternations", str(alternations), "--json-only"], env=env, check=True, capture_output=True, text=True)
    return json.loads(out.stdout.strip().splitlines()[-1])


def rehearse():
    """without a device: the caller's host pass over synthetic records against the model's grouping"""
    import go_ibft_amd.verifier as V
    rng = np.random.default_rng(3)
    m = 4000
    certs, dec = np.zeros(m, V.CERT_VERDICT), np.zeros(m, V.CERT_DECISION)
    certs["type"], certs["from_len"], certs["bits"], certs["height"] = 3, 20, 1, 5
    certs["round"] = rng.integers(1, 40, m)
    certs["from"][:, 0] = rng.integers(0, 50, m)
    dec["round_change"] = rng.integers(-1, 2, m)
    t0 = time.perf_counter()
    groups = host_pass(certs, dec, m)
    dt = time.perf_counter() - t0
    want = {}
    for i in range(m):
        want[(5, int(certs["round"][i]), int(certs["from"][i, 0]))] = i
    per_round = {}
    for (hh, rnd, _), i in want.items():
        per_round.setdefault((hh, rnd), []).append(i)
    assert set(groups) == set(per_round)
    for k, idx in per_round.items():
        assert len(groups[k]) == sum(1 for i in idx if dec["round_change"][i] == 1), k
    print(json.dumps({"rehearsal": "host pass", "records": m, "keys": len(groups), "host_ms": round(1e3 * dt, 3)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--modes", default="cold,warm")
    ap.add_argument("--shapes", default="honest,hostile")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json-only", action="store_true")
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        return rehearse()
    out = []
    for n in (int(x) for x in a.sizes.split(",")):
        for shape in a.shapes.split(","):
            for mode in a.modes.split(","):
                rec = measure(n, shape, mode == "warm", a.alternations, a.legs.split(","))
                if a.parent_lib and shape == "honest":        # processes alternate: tree, parent, tree, parent, …
                    kids = {"tree": [], "parent": []}
                    for _ in range(3):
                        kids["tree"].append(child_b(n, mode == "warm", None, a.alternations)["b_ms"])
                        kids["parent"].append(child_b(n, mode == "warm", os.path.abspath(a.parent_lib), a.alternations)["b_ms"])
                    rec["b_child_ms"], rec["p_child_ms"] = statistics.median(kids["tree"]), statistics.median(kids["parent"])
                    rec["b_child_range_ms"], rec["p_child_range_ms"] = [min(kids["tree"]), max(kids["tree"])], [min(kids["parent"]), max(kids["parent"])]
                print(json.dumps(rec), flush=True)
                out.append(rec)
    if a.json_only:
        return
    print(f"{'N':>6}{'shape':>9}{'mode':>6}{'keys':>7}{'a ms':>11}{'b ms':>11}{'c ms':>11}{'a-b ms':>10}{'c host ms':>11}{'b child':>10}{'parent':>10}")
    f = lambda r, k, w, d: f"{r[k]:>{w}.{d}f}" if r.get(k) is not None else f"{'-':>{w}}"  # noqa: E731
    for r in out:
        print(f"{r['n']:>6}{r['shape']:>9}{r['mode']:>6}{str(r['keys'] if r['keys'] is not None else '-'):>7}{f(r, 'a_ms', 11, 4)}{f(r, 'b_ms', 11, 4)}"
              f"{f(r, 'c_ms', 11, 4)}{f(r, 'a_minus_b_ms', 10, 4)}{f(r, 'c_host_ms', 11, 3)}{f(r, 'b_child_ms', 10, 4)}{f(r, 'p_child_ms', 10, 4)}")


if __name__ == "__main__":
    main()
