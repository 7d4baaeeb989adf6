#!/usr/bin/env python
"""tools/cert_dedup_rate.py — what IBFT_FLAG_CERT_DEDUP gains where nested messages repeat and costs where they do not, host
bytes → host-visible results through the C ABI (ibft_judge_certificates_wire, records only, buffers allocated once):

  (1) flag on against flag off on the ROUND_CHANGE batch of simulate.make_round_change_round (a certificate of its own per
      sender) at --sizes validators, cold contexts and contexts with the key cache.  Two contexts of one process on one device,
      the legs alternating (--reps of each, default 25, behind --warmup untimed pairs); medians and min–max, ibft_cert_stats of
      both, and the time of the dedup's own kernels by HIP events (ibft_last_kernel_ms after a flag-on
      ibft_verify_certificates_wire: two event pairs — table + compaction, scatter; the verdict launch between them is not timed).
      Before timing, the records and the sender masks of the two contexts are compared byte for byte.
  (2) the same two legs where nothing repeats: --distinct-roots ROUND_CHANGE messages of one sender, each with the certificate of
      another round (every nested message differs), at least 4 096 rows.
  (3) --against LIB: flag off in this build against flag off in another build of the library (the parent commit's), alternating
      PROCESSES (each loads one library through IBFT_GPU_LIB and prints its median), --rounds of each; the spread of LIB against
      LIB by the same procedure is what the difference has to stay inside.

Prints one JSON object and, with --out, writes it there; there is no threshold.

  --sizes N[,N…]       validators of (1) (default 256,1024)
  --reps R             timed calls per leg (default 25)
  --warmup W           untimed pairs first (default 3)
  --distinct-roots K   messages of (2) (default 64, with 97 validators: 66 rows each)
  --against LIB        run (3) at --against-size validators (default 1024), cold
  --rounds R           processes per library in (3) (default 3)
  --out PATH           also write the JSON there"""
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
import go_ibft_amd.simulate as S  # noqa: E402
import go_ibft_amd.verifier as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="256,1024")
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--distinct-roots", type=int, default=64)
ap.add_argument("--against", default=None)
ap.add_argument("--against-size", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--off-leg-only", type=int, default=0, help=argparse.SUPPRESS)   # (3)'s child process: print the flag-off median at N
args = ap.parse_args()
FLAG_DEDUP = getattr(V, "FLAG_CERT_DEDUP", 4)


class Caller:
    """one context and its output buffers; judge() = records only, verify() = the sender mask only"""

    def __init__(self, flags, cap, n_certs, addrs, power, height):
        self.bv = V.BatchVerifier(flags=flags, max_rows=cap)
        self.bv.set_validators(height, addrs, power)
        self.bv.set_kernel_timing(1)
        self.cap, self.certs = cap, np.zeros(n_certs, dtype=V.CERT_VERDICT)
        self.ms = np.zeros((cap + 63) // 64, dtype=np.uint64)
        self.n_rows, self.n_certs = C.c_size_t(0), C.c_size_t(0)

    def judge(self, wb, off):
        rc = self.bv._L.ibft_judge_certificates_wire(self.bv._h, V._p(wb), V._p(off), len(off) - 1, self.cap, len(self.certs), C.byref(self.n_rows),
                                                     C.byref(self.n_certs), V._p(self.certs), None, None, None, None, None, None)
        assert rc == 0, rc

    def verify(self, wb, off):
        rc = self.bv._L.ibft_verify_certificates_wire(self.bv._h, V._p(wb), V._p(off), len(off) - 1, self.cap, C.byref(self.n_rows), None, None, None,
                                                      V._p(self.ms), None, None)
        assert rc == 0, rc


def spread(ts):
    return {"ms_median": 1e3 * statistics.median(ts), "ms_min": 1e3 * min(ts), "ms_max": 1e3 * max(ts)}


def on_against_off(label, wire, off, addrs, power, height, rows, cache):
    wb, off = np.frombuffer(wire, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint32)
    cap, n = rows + 64, len(off) - 1
    base = V.FLAG_PUBKEY_CACHE if cache else 0
    a, b = Caller(base, cap, n, addrs, power, height), Caller(base | FLAG_DEDUP, cap, n, addrs, power, height)
    try:
        for _ in range(2 if cache else 1):                      # (the second call of a key-cache context is the warm one)
            for x in (a, b):
                x.verify(wb, off); x.judge(wb, off)
        assert a.n_rows.value == b.n_rows.value == rows and a.certs.tobytes() == b.certs.tobytes() and a.ms.tobytes() == b.ms.tobytes()
        stats = {"off": a.bv.cert_stats(), "on": b.bv.cert_stats()}
        for _ in range(args.warmup):
            a.judge(wb, off); b.judge(wb, off)
        ta, tb = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); a.judge(wb, off); ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); b.judge(wb, off); tb.append(time.perf_counter() - t0)
        kern = []
        b.bv.last_kernel_ms()
        for _ in range(5):
            b.verify(wb, off)
            ms, pairs = b.bv.last_kernel_ms()
            assert pairs == 2, pairs
            kern.append(ms)
        so, sn = spread(ta), spread(tb)
        return {"workload": label, "key_cache": cache, "messages": n, "rows": rows, "wire_bytes": len(wire), "reps": args.reps,
                "stats_off": dict(zip(("rows", "judged_rows", "verdict_rows", "unplaced_rows"), stats["off"])),
                "stats_on": dict(zip(("rows", "judged_rows", "verdict_rows", "unplaced_rows"), stats["on"])),
                "off": so, "on": sn, "on_over_off": sn["ms_median"] / so["ms_median"],
                "gain_ms": so["ms_median"] - sn["ms_median"], "off_spread_ms": so["ms_max"] - so["ms_min"],
                "dedup_kernels_ms_median": statistics.median(kern), "dedup_kernels_ms_max": max(kern),
                "dispatch_off": a.bv.last_dispatch(), "dispatch_on": b.bv.last_dispatch()}
    finally:
        a.bv.close(); b.bv.close()


def round_change_batch(n):
    q = (2 * n) // 3 + 1
    bv = V.BatchVerifier(max_rows=q * (q + 1) + 64)
    try:
        return S.make_round_change_round(bv, n, seed=5, distinct=True)
    finally:
        bv.close()


def distinct_batch(k, n=97):
    """k ROUND_CHANGE messages of validator 0, message j with the certificate of round 1 + j: no nested message repeats"""
    q = (2 * n) // 3 + 1
    bv = V.BatchVerifier(max_rows=q * (q + 1) + 64)
    try:
        msgs, r = [], None
        for j in range(k):
            r = S.make_round_change_round(bv, n, seed=5, prepared_round=1 + j, new_round=2 + j, raw_len=64)
            msgs.append(r.wire[int(r.off[0]):int(r.off[1])])
        off = np.zeros(k + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(m) for m in msgs])
        return b"".join(msgs), off, r.addrs, r.power, r.height, k * (q + 1)
    finally:
        bv.close()


def off_leg_only(n):
    r = round_change_batch(n)
    wb, off = np.frombuffer(r.wire, dtype=np.uint8), np.ascontiguousarray(r.off, dtype=np.uint32)
    a = Caller(0, r.rows + 64, r.q, r.addrs, r.power, r.height)
    try:
        for _ in range(args.warmup + 1):
            a.judge(wb, off)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); a.judge(wb, off); ts.append(time.perf_counter() - t0)
        return spread(ts)
    finally:
        a.bv.close()


if args.off_leg_only:
    print(json.dumps(off_leg_only(args.off_leg_only)))
    sys.exit(0)

out = {"tool": "cert_dedup_rate", "on_against_off": [], "nothing_repeats": []}
for n in (int(x) for x in args.sizes.split(",")):
    r = round_change_batch(n)
    for cache in (False, True):
        out["on_against_off"].append(dict(validators=n, **on_against_off("round change, a certificate per sender", r.wire, r.off, r.addrs, r.power,
                                                                        r.height, r.rows, cache)))
if args.distinct_roots:
    wire, off, addrs, power, height, rows = distinct_batch(args.distinct_roots)
    for cache in (False, True):
        out["nothing_repeats"].append(on_against_off("every nested message distinct", wire, off, addrs, power, height, rows, cache))
if args.against:
    # alternating processes: other, this, other, this, …; the other library's own run-to-run spread is the yardstick
    legs = {"other": [], "this": []}
    for _ in range(args.rounds):
        for name, lib in (("other", os.path.abspath(args.against)), ("this", None)):
            env = dict(os.environ)
            env.pop("IBFT_GPU_LIB", None)
            if lib:
                env["IBFT_GPU_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--off-leg-only", str(args.against_size), "--reps", str(args.reps),
                                "--warmup", str(args.warmup)], env=env, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
            legs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    med = {k: [x["ms_median"] for x in v] for k, v in legs.items()}
    out["off_against_other_build"] = {"validators": args.against_size, "rounds": args.rounds, "legs": legs,
                                      "other_medians_ms": med["other"], "this_medians_ms": med["this"],
                                      "other_against_other_spread_ms": max(med["other"]) - min(med["other"]),
                                      "this_minus_other_ms": statistics.median(med["this"]) - statistics.median(med["other"])}
text = json.dumps(out, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
