"""§8f rank 3 timing (run on the GPU box): sender verification of one round's PREPARE+COMMIT messages from
their wire bytes — stock route (host: proto decode + PayloadNoSig re-marshal + flatten; device: hash +
recover) against the device wire walk (ibft_verify_senders_wire).  Prints one JSON object.

--recode: the price and the gain of IBFT_FLAG_WIRE_RECODE at N = 4 096 COMMIT messages with known keys, the legs alternating in
one process, medians after warm-up: (a) a canonical batch, flag off against flag on, next to the spread of two flag-off legs;
(b) every row in a non-canonical encoding, flag on against the stock route for the same bytes (host decode and re-marshal
through the mirror, then ibft_verify_senders); (c) one row in a hundred in a non-canonical encoding."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import go_ibft_amd.hostlib as H
import go_ibft_amd.verifier as V
import wire_cases as WCASE
from oracle import workload as W



def recode_legs(n=4096, warmup=5, reps=31):
    import random
    import wire_recode_cases as RC
    r = W.make_round(n, 700 + n)
    parts = RC.signed_parts(r, kinds=("commit",))
    rng = random.Random(11)
    canon = [p.canonical for p in parts]
    scr = [RC.spell(p, RC.random_options(rng)) for p in parts]
    one_pct = [s if i % 100 == 50 else c for i, (c, s) in enumerate(zip(canon, scr))]
    batches = {k: RC.pack(v) for k, v in (("canonical", canon), ("scrambled", scr), ("one_pct", one_pct))}
    off_bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=n)
    on_bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE | V.FLAG_WIRE_RECODE, max_rows=n)
    legs = [("a_canonical_flag_off", off_bv, "canonical", False), ("a_canonical_flag_on", on_bv, "canonical", False),
            ("a_canonical_flag_off_again", off_bv, "canonical", False), ("b_scrambled_flag_on", on_bv, "scrambled", False),
            ("b_scrambled_stock_route", off_bv, "scrambled", True), ("c_one_pct_flag_on", on_bv, "one_pct", False),
            ("c_one_pct_flag_off_host_rows", off_bv, "one_pct", False)]
    ts = {name: [] for name, *_ in legs}
    host_rows = {}
    try:
        for bv in (off_bv, on_bv):
            bv.set_validators(1, r.addrs, r.power)
            for _ in range(3):  # the keys become known, the tables are built
                assert bv.is_valid_validator_wire(*batches["canonical"])[0].all()
        for it in range(warmup + reps):
            for name, bv, batch, stock in legs:
                t0 = time.perf_counter()
                v, _, hr = H.verify_senders_wire(bv, *batches[batch], stock=stock)
                dt = (time.perf_counter() - t0) * 1e3
                assert v.all(), name
                host_rows[name] = int(hr)
                if it >= warmup:
                    ts[name].append(dt)
        res = {name: {"ms_p50": float(np.median(t)), "ms_p10": float(np.percentile(t, 10)), "ms_p90": float(np.percentile(t, 90)),
                      "host_rows": host_rows[name]} for name, t in ts.items()}
        res["n"], res["reps"], res["warmup"] = n, reps, warmup
        res["wire_bytes"] = {k: len(b[0]) for k, b in batches.items()}
        p50 = lambda k: res[k]["ms_p50"]
        res["a_price_on_canonical_ms"] = p50("a_canonical_flag_on") - p50("a_canonical_flag_off")
        res["a_spread_of_two_flag_off_legs_ms"] = abs(p50("a_canonical_flag_off_again") - p50("a_canonical_flag_off"))
        res["b_stock_over_recode"] = p50("b_scrambled_stock_route") / p50("b_scrambled_flag_on")
        return res
    finally:
        off_bv.close()
        on_bv.close()


if "--recode" in sys.argv:
    print(json.dumps({"wire_recode_n4096_commit_known_keys": recode_legs()}, indent=1))
    sys.exit(0)

out = {}
for n in (1024, 4096):
    r = W.make_round(n, 700 + n)
    rows = WCASE.canonical_round(r)           # n messages, COMMIT and PREPARE alternating
    wire, off = WCASE.pack(rows)
    for cache in (False, True):
        bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if cache else 0, max_rows=max(n, 1024))
        bv.set_validators(1, r.addrs, r.power)
        res = {}
        for name, stock in (("stock_route", True), ("wire_walk", False)):
            for _ in range(3):
                v, _, _ = H.verify_senders_wire(bv, wire, off, stock=stock)
            assert v.all()
            ts, hs = [], []
            for _ in range(15):
                t0 = time.perf_counter()
                v, host_ms, _ = H.verify_senders_wire(bv, wire, off, stock=stock)
                ts.append((time.perf_counter() - t0) * 1e3)
                hs.append(host_ms)
            res[name] = {"total_ms_p50": float(np.median(ts)), "host_decode_flatten_ms_p50": float(np.median(hs))}
        res["wire_bytes"] = len(wire)
        out[f"n{n}_{'warm' if cache else 'cold'}"] = res
        bv.close()
print(json.dumps(out, indent=1))
