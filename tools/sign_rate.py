#!/usr/bin/env python
"""tools/sign_rate.py — wall-clock rate of ibft_sign_seals / ibft_sign_seals_ex (f4, simulators) at a few batch sizes, and of
sign → verify on the resident batch.  Prints one JSON object.

  --nonce keccak|rfc6979|both   the nonce rule(s) to time (default keccak: ibft_sign_seals); with `both` every size also
                                carries the ratio of the RFC 6979 rule's time to the Keccak rule's of the same build
  --sizes N[,N…]                batch sizes (default 1024,4096,16384,65536)
  --reps R                      timed calls per size and rule, the best and the spread are reported (default 5)
  --messages prepare|commit     the message leg instead: ibft_sign_messages_wire (whole PREPARE / COMMIT messages as wire bytes,
                                height 1, round 0) in messages/s at the same sizes, next to ibft_sign_seals_ex under the same
                                nonce rule and n from the same process, and the ratio of the two times (a COMMIT row is two
                                signatures, one address and two to three Keccak permutations; a bare seal one signature and
                                one address)
  --cpu                         with --messages: also the oracle's rate for the same messages on one core (oracle/wire.py +
                                orc_sign, timed over --cpu-rows rows, default 256)"""
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
ap.add_argument("--messages", choices=("prepare", "commit"))
ap.add_argument("--cpu", action="store_true")
ap.add_argument("--cpu-rows", type=int, default=256)
args = ap.parse_args()
rules = ("keccak", "rfc6979") if args.nonce == "both" else (args.nonce,)


def _best(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        times.append(time.perf_counter() - t0)
    return min(times), times, r


def _oracle_messages_per_s(sk, hs, mtype, rule, rows):
    from oracle import binding as O, wire as W
    sign = O.sign if rule == "keccak" else O.sign_rfc6979
    rows = min(rows, len(sk))
    t0 = time.perf_counter()
    for i in range(rows):
        k, h = sk[i].tobytes(), hs[i].tobytes()
        body = W.commit_body(h, sign(k, h)) if mtype == 2 else W.prepare_body(h)
        m = W.IbftMessage(view=W.View(1, 0), sender=O.address(O.pubkey(k)), type=mtype, payload=body)
        m.signature = sign(k, O.keccak256(m.payload_no_sig()))
        m.encode()
    return rows / (time.perf_counter() - t0)


def messages_leg():
    mtype = {"prepare": 1, "commit": 2}[args.messages]
    res = {"messages": args.messages, "rules": {rule: {} for rule in rules}}
    rng = np.random.default_rng(1)
    for n in (int(x) for x in args.sizes.split(",")):
        sk = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(-1, 32).copy()
        sk[:, 0] &= 0x7F
        sk[:, 31] |= 1
        hs = np.tile(np.frombuffer(rng.bytes(32), np.uint8), (n, 1))
        bv = V.BatchVerifier(max_rows=n)
        for rule in rules:
            tm, tm_all, (wire, off, frm, ok) = _best(lambda: bv.sign_messages(sk, mtype, 1, 0, hs, nonce=rule), args.reps)
            assert ok.all() and len(wire) == int(off[n])
            ts, ts_all, (sig, signer, ok_s) = _best(lambda: bv.sign_seals(sk, hs, nonce=rule), args.reps)
            assert ok_s.all() and (signer == frm).all()
            bv.set_validators(1, frm, np.ones(n, np.uint64))
            verdict, _, _ = bv.is_valid_validator_wire(wire, off)   # what was signed verifies
            assert verdict.all()
            row = {"messages_ms": round(tm * 1e3, 3), "messages_ms_all": [round(x * 1e3, 3) for x in tm_all],
                   "messages_per_s": round(n / tm), "wire_bytes": len(wire),
                   "seals_ms": round(ts * 1e3, 3), "seals_ms_all": [round(x * 1e3, 3) for x in ts_all], "seals_per_s": round(n / ts),
                   "message_over_seal": round(tm / ts, 4)}
            if args.cpu:
                row["oracle_one_core_messages_per_s"] = round(_oracle_messages_per_s(sk, hs, mtype, rule, args.cpu_rows), 1)
            res["rules"][rule][str(n)] = row
        bv.close()
    res["note"] = "host→host wall clock incl. PCIe both ways; messages: ibft_sign_messages_wire, seals: ibft_sign_seals_ex, one process"
    print(json.dumps(res))


if args.messages:
    messages_leg()
    sys.exit(0)

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
