#!/usr/bin/env python
"""tools/sign_rate.py — wall-clock rate of ibft_sign_seals / ibft_sign_seals_ex (f4, simulators) at a few batch sizes, and of
sign → verify on the resident batch.  Prints one JSON object.

  --nonce keccak|rfc6979|both   the nonce rule(s) to time (default keccak: ibft_sign_seals); with `both` every size also
                                carries the ratio of the RFC 6979 rule's time to the Keccak rule's of the same build
  --sizes N[,N…]                batch sizes (default 1024,4096,16384,65536)
  --reps R                      timed calls per size and rule, the best and the spread are reported (default 5)"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import go_ibft_amd.verifier as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nonce", choices=("keccak", "rfc6979", "both"), default="keccak")
ap.add_argument("--sizes", default="1024,4096,16384,65536")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
rules = ("keccak", "rfc6979") if args.nonce == "both" else (args.nonce,)

out = {rule: {} for rule in rules}
ratio = {}
rng = np.random.default_rng(1)
for n in (int(x) for x in args.sizes.split(",")):
    sk = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(-1, 32).copy()
    sk[:, 0] &= 0x7F
    sk[:, 31] |= 1
    hs = np.tile(np.frombuffer(rng.bytes(32), np.uint8), (n, 1))
    bv = V.BatchVerifier(max_rows=n)
    for rule in rules:
        kw = {} if rule == "keccak" else {"nonce": rule}   # (keccak: the plain call, so the tool also runs on an older binding)
        bv.sign_seals(sk, hs, **kw)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sig, signer, ok = bv.sign_seals(sk, hs, **kw)
            times.append(time.perf_counter() - t0)
        best = min(times)
        assert ok.all()
        bv.set_validators(1, signer, np.ones(n, np.uint64))
        t0 = time.perf_counter()
        verdict, t = bv.seals_run()
        tv = time.perf_counter() - t0
        assert verdict.all() and t.has_quorum
        out[rule][str(n)] = {"sign_ms": round(best * 1e3, 3), "sign_ms_all": [round(x * 1e3, 3) for x in times],
                             "seals_per_s": round(n / best), "verify_resident_ms": round(tv * 1e3, 3)}
    if len(rules) == 2:
        ratio[str(n)] = round(out["rfc6979"][str(n)]["sign_ms"] / out["keccak"][str(n)]["sign_ms"], 4)
    bv.close()
res = {"ibft_sign_seals": out["keccak"]} if "keccak" in out else {}
if "rfc6979" in out:
    res["ibft_sign_seals_ex_rfc6979"] = out["rfc6979"]
if ratio:
    res["rfc6979_over_keccak"] = ratio
res["note"] = "host→host wall clock incl. PCIe both ways"
print(json.dumps(res))
