#!/usr/bin/env python
"""tools/cert_verdict_rate.py — what the per-carrier records of ibft_judge_certificates_wire cost and save, host bytes →
host-visible results, on the ROUND_CHANGE batch of simulate.make_round_change_round (a certificate of its own per sender):

  (a) ibft_verify_certificates_wire with every output requested (nodes, rows, class, three masks) — what a caller needs today to
      walk the rows itself; the walk is NOT in the figure
  (b) ibft_judge_certificates_wire with the records only — no per-row output

The two legs alternate in one process on one device (--reps of each, default 25, behind --warmup untimed pairs); reported are the
medians, the bytes each leg brings back (into buffers allocated once, through the C ABI), and the time of the two record kernels by
HIP events (ibft_last_kernel_ms after a leg-(b) call: the verdict launches of this path are not timed).  Before timing, the records are checked against the rows: every sender's
pc must be what the generator's bits say.  Prints one JSON object; there is no threshold.

  --sizes N[,N…]     validators (default 256,1024)
  --reps R           timed calls per leg and size (default 25; at least 20 for a median worth quoting)
  --warmup W         untimed pairs first (default 3)
  --cache            contexts with the key cache (warm verdict kernels, two verdict launches) instead of cold ones

--decide: ibft_decide_certificates_wire on the closing PREPREPARE of a round change — the proposal again with the
RoundChangeCertificate of q ROUND_CHANGE messages, the first and the last of which carry the PreparedCertificate of the prepared
round (its PREPREPARE names the hash and carries no Proposal).  Only two, because the device judges a message of at most
IBFT_CERT_DIGEST_MAX_BYTES = 1 MiB: q certificates of q messages are 4 MB at N = 256 and leave the message to the host whatever
its proposal; with two, a proposal of up to about 896 KiB fits at N = 256 —, ONE leg per process,
so that a job script alternates processes (and, through IBFT_GPU_LIB, builds of the library) on one device:

  --leg judge        ibft_judge_certificates_wire, records only (any build that has the call: the parent's too)
  --leg decide       ibft_decide_certificates_wire under the covering table; also the decision stage alone by HIP events — the
                     call's event pairs are the record kernels' and the decision kernels', a judge call on the same bytes gives the
                     first — and the host finish it replaces on one core: the walk over the records for the highest prepared round
                     and one host Keccak (ibft_keccak256) of rawProposal ‖ BE64(round)
  --raw-lens L[,L…]  proposal bytes (default 1024,65536,917504)"""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import go_ibft_amd.simulate as S  # noqa: E402
import go_ibft_amd.verifier as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="256,1024")
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--cache", action="store_true")
ap.add_argument("--decide", action="store_true")
ap.add_argument("--leg", choices=["judge", "decide"], default="decide")
ap.add_argument("--raw-lens", default="1024,65536,917504")
args = ap.parse_args()


def closing_preprepare(bv, n, raw_len, seed=5, height=5, prepared_round=1, new_round=2):
    """→ (message, q, raw, addrs): validator new_round mod n proposes `raw` again over q ROUND_CHANGE messages, the first and the
    last with the certificate of prepared_round (proposer: prepared_round mod n; q − 1 PREPAREs), the others with nothing"""
    q = (2 * n) // 3 + 1
    raw = S._splitmix(seed, (raw_len + 7) // 8).tobytes()[:raw_len]
    h_prepared, h_new = bv.proposal_hash(raw, prepared_round), bv.proposal_hash(raw, new_round)
    sk = S.secret_keys(seed, n)
    proposer, new_proposer = prepared_round % n, new_round % n
    others = [j for j in range(n) if j != proposer]
    pw, poff, paddr, ok = S._sign_messages(bv, sk[others], S.MESSAGE_KINDS["prepare"], height, prepared_round,
                                           np.tile(np.frombuffer(h_prepared, dtype=np.uint8), (len(others), 1)))
    assert ok.all()
    nested = b"".join(S._field(2, pw[int(poff[k]):int(poff[k + 1])]) for k in range(q - 1))
    body = S._field(2, h_prepared)
    pm, _, pm_addr, ok = bv.sign_envelopes(sk[proposer:proposer + 1], 0, height, prepared_round, body, 0, len(body))
    assert ok.all()
    rc_body = S._field(2, S._field(1, pm) + nested)
    lens = np.zeros(q, dtype=np.uint32)
    lens[[0, q - 1]] = len(rc_body)
    wire, off, _, ok = S._sign_envelopes(bv, sk[np.arange(q)], 3, height, new_round, rc_body, np.zeros(q, dtype=np.uint32), lens)
    assert ok.all()
    rcc = b"".join(S._field(1, wire[int(off[i]):int(off[i + 1])]) for i in range(q))
    body = S._field(1, S._proposal(raw, new_round)) + S._field(2, h_new) + S._field(3, rcc)
    closing, _, _, ok = bv.sign_envelopes(sk[new_proposer:new_proposer + 1], 0, height, new_round, body, 0, len(body))
    assert ok.all()
    addrs = np.zeros((n, 20), dtype=np.uint8)
    addrs[others] = paddr
    addrs[proposer] = pm_addr[0]
    return closing, q, raw, addrs


def decide_leg(n, raw_len):
    import ctypes as C
    q = (2 * n) // 3 + 1
    cap = 1 + 3 * q + 64
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if args.cache else 0, max_rows=cap)
    try:
        height, prepared_round, new_round = 5, 1, 2
        msg, q, raw, addrs = closing_preprepare(bv, n, raw_len, height=height, prepared_round=prepared_round, new_round=new_round)
        bv.set_validators(height, addrs, np.ones(n, dtype=np.uint64))
        bv.set_kernel_timing(1)
        wb, off = np.frombuffer(msg, dtype=np.uint8), np.array([0, len(msg)], dtype=np.uint32)
        certs, dec = np.zeros(1 + q, dtype=V.CERT_VERDICT), np.zeros(1 + q, dtype=V.CERT_DECISION) if hasattr(V, "CERT_DECISION") else None
        n_rows, n_certs = C.c_size_t(0), C.c_size_t(0)
        p = V._p

        def judge():
            rc = bv._L.ibft_judge_certificates_wire(bv._h, p(wb), p(off), 1, cap, 1 + q, C.byref(n_rows), C.byref(n_certs), p(certs), None, None, None,
                                                    None, None, None)
            assert rc == 0, rc

        def decide():
            rc = bv._L.ibft_decide_certificates_wire(bv._h, p(wb), p(off), 1, cap, 1 + q, C.byref(n_rows), C.byref(n_certs), p(certs), p(dec), None, None,
                                                     None, None, None, None)
            assert rc == 0, rc

        def host_finish():
            """what the decision replaces: IsProposer per record, the highest prepared round (the last among equals), the hash"""
            proposer_of = lambda rnd: addrs[rnd % n].tobytes()
            best = None
            first = int(certs[0]["first_child_cert"])
            for k in range(first, first + int(certs[0]["n_children"])):
                c = certs[k]
                if c["pc"] == 1 and c["pc_from"].tobytes() == proposer_of(int(c["pc_round"])) and (best is None or c["pc_round"] >= certs[best]["pc_round"]):
                    best = k
            out = np.zeros(32, dtype=np.uint8)
            tail = np.frombuffer(int(certs[best]["pc_round"]).to_bytes(8, "big"), dtype=np.uint8)
            raw_a = np.frombuffer(raw, dtype=np.uint8)
            assert bv._L.ibft_keccak256(p(raw_a), len(raw_a), p(tail), 8, p(out)) == 0
            return best, out.tobytes() == certs[best]["pc_hash"].tobytes()

        call = decide if args.leg == "decide" else judge
        if args.leg == "decide":
            bv.set_proposers(height, 0, [addrs[r % n].tobytes() for r in range(8)])
        call()
        assert (int(n_rows.value), int(n_certs.value)) == (1 + 3 * q, 1 + q), (int(n_rows.value), int(n_certs.value), q)
        assert int(certs[0]["rcc"]) == 1 and int(certs[0]["cls"]) == 0, (int(certs[0]["rcc"]), int(certs[0]["cls"]), len(msg))
        assert certs[1:]["pc"].tolist() == [1] + [2] * (q - 2) + [1], np.unique(certs[1:]["pc"]).tolist()
        if args.leg == "decide":
            assert int(dec[0]["proposal"]) == 1 and int(dec[0]["prepared_record"]) == q and int(dec[0]["prepared_round"]) == prepared_round
            assert host_finish() == (q, True)
        for _ in range(args.warmup):
            call()
        bv.last_kernel_ms()
        t_call, k_call, k_judge, t_host = [], [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); call(); t_call.append(time.perf_counter() - t0)
            ms, pairs = bv.last_kernel_ms()
            assert pairs == (2 if args.leg == "decide" else 1)
            k_call.append(ms)
            if args.leg == "decide":
                judge()
                k_judge.append(bv.last_kernel_ms()[0])
                t0 = time.perf_counter(); host_finish(); t_host.append(time.perf_counter() - t0)
        out = {"validators": n, "raw_len": raw_len, "message_bytes": len(msg), "rows": int(n_rows.value), "records": 1 + q, "reps": args.reps,
               "call_ms_median": 1e3 * statistics.median(t_call), "call_ms_min": 1e3 * min(t_call), "call_ms_max": 1e3 * max(t_call),
               "timed_kernels_ms_median": statistics.median(k_call)}
        if args.leg == "decide":
            stage = [a - b for a, b in zip(k_call, k_judge)]
            out.update({"decision_stage_ms_median": statistics.median(stage), "decision_stage_ms_min": min(stage), "decision_stage_ms_max": max(stage),
                        "host_finish_ms_median": 1e3 * statistics.median(t_host), "host_finish_ms_min": 1e3 * min(t_host)})
        return out
    finally:
        bv.close()


if args.decide:
    import os
    print(json.dumps({"tool": "cert_verdict_rate --decide", "leg": args.leg, "library": os.environ.get("IBFT_GPU_LIB", "the tree's"),
                      "key_cache": bool(args.cache),
                      "sizes": [decide_leg(int(n), int(L)) for n in args.sizes.split(",") for L in args.raw_lens.split(",")]}))
    sys.exit(0)


def leg(n):
    q = (2 * n) // 3 + 1
    cap = q * (q + 1) + 64
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if args.cache else 0, max_rows=cap)
    try:
        r = S.make_round_change_round(bv, n, seed=5, distinct=True)
        bv.set_validators(r.height, r.addrs, r.power)
        bv.set_kernel_timing(1)

        # both legs through the C ABI into buffers allocated (and touched) once, as a caller that lives for more than one round has them
        import ctypes as C
        wb, off = np.frombuffer(r.wire, dtype=np.uint8), np.ascontiguousarray(r.off, dtype=np.uint32)
        words = (cap + 63) // 64
        nodes, rows, cls = np.zeros(cap, dtype=V.CERT_NODE), np.zeros(cap, dtype=V.WIRE_ROW), np.zeros(cap, dtype=np.uint8)
        ms, mh, mself = (np.zeros(words, dtype=np.uint64) for _ in range(3))
        certs_buf = np.zeros(r.q, dtype=V.CERT_VERDICT)
        n_rows, n_certs = C.c_size_t(0), C.c_size_t(0)
        p = V._p

        def rows_leg():
            rc = bv._L.ibft_verify_certificates_wire(bv._h, p(wb), p(off), r.q, cap, C.byref(n_rows), p(nodes), p(rows), p(cls), p(ms), p(mh), p(mself))
            assert rc == 0, rc
            return int(n_rows.value)

        def records_leg():
            rc = bv._L.ibft_judge_certificates_wire(bv._h, p(wb), p(off), r.q, cap, r.q, C.byref(n_rows), C.byref(n_certs), p(certs_buf), None, None, None,
                                                    None, None, None)
            assert rc == 0, rc
            return certs_buf[:int(n_certs.value)], int(n_rows.value), None
        k = rows_leg()
        sender = V.mask_to_bool(ms, k)
        certs, k2, _ = records_leg()
        assert k == k2 == r.rows and len(certs) == r.q and sender.all() and (certs["pc"] == 1).all() and (certs["pc_round"] == r.prepared_round).all()
        for _ in range(args.warmup):
            rows_leg(); records_leg()
        bv.last_kernel_ms()
        ta, tb, kern = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); rows_leg(); ta.append(time.perf_counter() - t0)
            bv.last_kernel_ms()
            certs_buf["pc"] = 0
            t0 = time.perf_counter(); got, _, _ = records_leg(); tb.append(time.perf_counter() - t0)
            assert (got["pc"] == 1).all()
            kernel_ms, pairs = bv.last_kernel_ms()
            assert pairs == 1
            kern.append(kernel_ms)
        words = (k + 63) // 64
        return {"validators": n, "messages": r.q, "rows": k, "records": len(certs), "wire_bytes": len(r.wire), "reps": args.reps,
                "rows_leg_ms_median": 1e3 * statistics.median(ta), "rows_leg_ms_min": 1e3 * min(ta), "rows_leg_ms_max": 1e3 * max(ta),
                "records_leg_ms_median": 1e3 * statistics.median(tb), "records_leg_ms_min": 1e3 * min(tb), "records_leg_ms_max": 1e3 * max(tb),
                "records_over_rows": statistics.median(tb) / statistics.median(ta),
                "rows_leg_bytes_back": k * (V.CERT_NODE.itemsize + V.WIRE_ROW.itemsize + 1) + 3 * 8 * words,
                "records_leg_bytes_back": len(certs) * V.CERT_VERDICT.itemsize,
                "record_kernels_ms_median": statistics.median(kern), "record_kernels_ms_max": max(kern)}
    finally:
        bv.close()


print(json.dumps({"tool": "cert_verdict_rate", "key_cache": bool(args.cache), "sizes": [leg(int(n)) for n in args.sizes.split(",")]}, indent=1))
