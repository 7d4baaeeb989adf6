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
                                orc_sign, timed over --cpu-rows rows, default 256)
  --envelopes                   the round-change leg instead: simulate.make_round_change_round (PREPAREs from
                                ibft_sign_messages_wire, every PREPREPARE / ROUND_CHANGE envelope from ibft_sign_envelopes_wire) host →
                                host at N = --sizes (default 256,1024) validators, one shared certificate and a certificate per
                                sender, with the device calls' share of it, and ibft_verify_certificates_wire over the result (all
                                bits checked).  With --cpu: the same ROUND_CHANGE messages built by tests/cert_cases.py's oracle
                                route on one core (byte-identical under the keccak rule: asserted), once per N"""
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
ap.add_argument("--envelopes", action="store_true")
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


def envelopes_leg():
    import os
    import types
    import go_ibft_amd.simulate as S
    sizes = [int(x) for x in (args.sizes if args.sizes != ap.get_default("sizes") else "256,1024").split(",")]
    res = {"envelopes": "make_round_change_round", "rules": {rule: {} for rule in rules}, "oracle_one_core": {}}
    for n in sizes:
        bv = V.BatchVerifier(max_rows=max(n, 64))
        q = (2 * n) // 3 + 1
        judge = V.BatchVerifier(max_rows=q * (q + 1) + 64)   # (the whole tree must fit the verifying context)
        calls = {"s": 0.0, "envelopes": []}
        for name in ("sign_envelopes", "sign_messages", "proposal_hash"):   # the device calls' share of the generator's time
            def timed(*a, _f=getattr(bv, name), _name=name, **kw):
                t0 = time.perf_counter()
                try:
                    return _f(*a, **kw)
                finally:
                    calls["s"] += time.perf_counter() - t0
                    if _name == "sign_envelopes":
                        calls["envelopes"].append(time.perf_counter() - t0)
            setattr(bv, name, timed)
        for rule in rules:
            for distinct in (False, True):
                best = None
                for k in range(args.reps + 1):      # (the first call grows the device buffers: not timed)
                    calls["s"], calls["envelopes"] = 0.0, []
                    t0 = time.perf_counter()
                    r = S.make_round_change_round(bv, n, seed=1, distinct=distinct, nonce=rule)
                    t = time.perf_counter() - t0
                    if k and (best is None or t < best[0]):
                        best = (t, calls["s"], list(calls["envelopes"]))
                judge.set_validators(r.height, r.addrs, r.power)
                t0 = time.perf_counter()
                rows_n, _, _, cls, sender, hb, sb = judge.verify_certificates_wire(r.wire, r.off, rows_cap=r.rows + 64, want_rows=False)
                tv = time.perf_counter() - t0
                assert rows_n == r.rows and sender[:rows_n].all() and (cls[:rows_n] == 0).all() and hb[r.q:rows_n].all()
                res["rules"][rule][f"{n}_{'distinct' if distinct else 'shared'}"] = {
                    "round_change_messages": r.q, "tree_rows": r.rows, "messages_signed": (n - 1) + 1 + r.q + 1,
                    "wire_bytes": len(r.wire), "closing_preprepare_bytes": len(r.preprepare),
                    "generate_ms": round(best[0] * 1e3, 3), "device_calls_ms": round(best[1] * 1e3, 3),
                    # the sign_envelopes calls in the generator's order: the certificate's PREPREPARE, the q ROUND_CHANGE messages,
                    # the closing PREPREPARE — ONE message around all of them, one sequential sponge
                    "round_change_batch_ms": round(sum(best[2][1:-1]) * 1e3, 3), "closing_preprepare_ms": round(best[2][-1] * 1e3, 3),
                    "verify_first_call_ms": round(tv * 1e3, 3)}
                if args.cpu and not distinct and rule == "keccak":
                    sys.path.insert(0, os.path.join(__file__.rsplit("/", 2)[0], "tests"))
                    import cert_cases as CC
                    sk = S.secret_keys(1, n)
                    rr = types.SimpleNamespace(n=n, raw=r.raw, sks=[sk[i].tobytes() for i in range(n)], addrs=r.addrs, proposal_hash=None)
                    t0 = time.perf_counter()
                    want = CC.honest_round_change_set(rr, r.height, r.new_round, r.prepared_round, senders=list(range(r.q)))
                    enc = b"".join(m.encode() for m in want)
                    to = time.perf_counter() - t0
                    assert enc == r.wire
                    # (the oracle route signs every nested message again for every sender: q · (q + 1) signatures; it builds the
                    # ROUND_CHANGE batch only, so the device figure next to it is the generator without its closing PREPREPARE)
                    res["oracle_one_core"][str(n)] = {"build_ms": round(to * 1e3, 1), "signatures": r.rows, "signatures_per_s": round(r.rows / to),
                                                      "device_ms_same_bytes": round((best[0] - best[2][-1]) * 1e3, 3),
                                                      "oracle_over_device": round(to / (best[0] - best[2][-1]), 1)}
        bv.close()
        judge.close()
    res["note"] = ("host→host wall clock of simulate.make_round_change_round incl. PCIe both ways and the host's concatenation; "
                   "device_calls_ms: the part spent inside ibft_sign_messages_wire / ibft_sign_envelopes_wire / ibft_proposal_hash; "
                   "oracle_one_core: cert_cases.honest_round_change_set (a certificate signed again for every sender) for the same bytes")
    print(json.dumps(res))


if args.messages:
    messages_leg()
    sys.exit(0)
if args.envelopes:
    envelopes_leg()
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
