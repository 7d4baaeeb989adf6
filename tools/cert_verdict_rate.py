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
  --cache            contexts with the key cache (warm verdict kernels, two verdict launches) instead of cold ones"""
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
args = ap.parse_args()


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
