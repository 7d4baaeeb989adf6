#!/usr/bin/env python3
"""Chain sync from the proposals: what hashing the blocks' proposals on the device costs and saves.

    python tools/block_seals_raw_rate.py                     # the three legs, V=100 × 655 blocks of 1 KiB / 64 KiB, V=4 × 16 384 of 1 KiB
    python tools/block_seals_raw_rate.py --forms             # ibft_proposal_hashes alone, lane form against wavefront form, by batch size
    python tools/block_seals_raw_rate.py --hash-only --v 100 --blocks 655 --kib 1    # for rocprofv3 --kernel-trace --stats

Legs, alternated --alternations times on ONE context, every column in ibft_pinned_alloc memory, cold (no key cache) and warm
(IBFT_FLAG_PUBKEY_CACHE after the tables are built); median and min … max of the rounds:
  A  ibft_verify_block_seals_raw — proposals in, hashed on the device;
  B  what a caller had before: a loop of ibft_proposal_hash (one proposal per call, hashed on the calling host thread) into the
     block-hash column, then ibft_verify_block_seals;
  C  ibft_verify_block_seals with the hashes given — the floor.
A − C is what the device-side hashing adds (upload of the proposals + proposal_digest_kernel); B − C what the host loop adds.
Every block carries one seal of every validator over ITS proposal's hash (signed on the device, ibft_sign_seals).
--forms runs each form in a child process of its own (IBFT_PROPOSAL_LANES is read at ibft_ctx_create).
The lease's ibft_issue_probe value is in every record.  One JSON line per configuration, then a table."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, budget_s=0.15, max_reps=300):
    fn()
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(3, min(max_reps, int(budget_s / one)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def proposals(nb, kib, seed=5):
    """nb proposals of kib KiB ± a few bytes (so that starts fall on every offset mod 4), rounds 0 … nb − 1"""
    rng = np.random.default_rng(seed)
    lens = kib * 1024 + rng.integers(-3, 4, nb)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    raw = np.frombuffer(rng.bytes(int(off[-1])), np.uint8)
    return raw, off, np.arange(nb, dtype=np.uint64)


def measure(V_, nb, kib, warm, alternations):
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    r = W.make_round(V_, 7, raw_len=64)
    n = nb * V_
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if warm else 0, max_rows=65536)
    try:
        probe_ns = bv.issue_probe()[0]
        bv.set_validators(r.height, r.addrs, r.power)
        raw, roff, rnd = proposals(nb, kib)
        bh = bv.proposal_hashes((raw, roff), rnd)
        off = (np.arange(nb + 1) * V_).astype(np.uint32)
        sk = np.tile(np.frombuffer(b"".join(r.sks), np.uint8).reshape(V_, 32), (nb, 1))
        sig, signer, ok = bv.sign_seals(sk, np.repeat(bh, V_, axis=0))
        assert ok.all()
        raw, roff, rnd, off, sig, signer, bh_given = (V.pinned_copy(x) for x in (raw, roff, rnd, off, sig, signer, bh))
        bh_loop = V.pinned_copy(np.zeros_like(bh))
        L, h, p = bv._L, bv._h, V._p
        mask = np.zeros((n + 63) // 64, np.uint64)
        tal = (V.Tally * nb)()
        a_raw = (h, p(raw), p(roff), p(rnd), p(off), nb, p(sig), p(signer), None, None, p(mask), tal)
        a_given = (h, p(bh_given), p(off), nb, p(sig), p(signer), None, p(mask), tal)
        a_loop = (h, p(bh_loop), p(off), nb, p(sig), p(signer), None, p(mask), tal)
        import ctypes as C
        one = [(h, C.c_void_p(raw.ctypes.data + int(roff[b])), int(roff[b + 1] - roff[b]), int(rnd[b]),
                C.c_void_p(bh_loop.ctypes.data + 32 * b)) for b in range(nb)]

        def leg_a():
            assert L.ibft_verify_block_seals_raw(*a_raw) == 0

        def hash_loop():
            for a in one:
                assert L.ibft_proposal_hash(*a) == 0

        def leg_b():
            hash_loop()
            assert L.ibft_verify_block_seals(*a_loop) == 0

        def leg_c():
            assert L.ibft_verify_block_seals(*a_given) == 0

        def check():
            assert V.mask_to_bool(mask, n).all() and all(t.has_quorum == 1 for t in tal)

        legs = {"A_raw": leg_a, "B_host_loop": leg_b, "C_hashes_given": leg_c}
        leg_c()                                       # the key cache learns and builds here (warm); nothing changes cold
        check()
        times = {k: [] for k in legs}
        loop_only = []
        for _ in range(alternations):
            for name, fn in legs.items():
                times[name].append(timed(fn) * 1e3)
                check()
            loop_only.append(timed(hash_loop) * 1e3)
        assert (bh_loop == bh_given).all()
        res = {"v": V_, "blocks": nb, "rows": n, "kib": kib, "proposal_bytes": int(roff[-1]), "mode": "warm" if warm else "cold",
               "alternations": alternations, "issue_probe_ns": probe_ns, "cold_lanes": bv.last_dispatch()[0], "warm_lanes": bv.last_dispatch()[1],
               "proposal_lanes_env": os.environ.get("IBFT_PROPOSAL_LANES", "auto")}
        for name, ts in times.items():
            res[name + "_ms"] = float(np.median(ts))
            res[name + "_min_ms"] = min(ts)
            res[name + "_max_ms"] = max(ts)
        res["host_hash_loop_ms"] = float(np.median(loop_only))
        res["A_minus_C_ms"] = res["A_raw_ms"] - res["C_hashes_given_ms"]
        res["B_minus_C_ms"] = res["B_host_loop_ms"] - res["C_hashes_given_ms"]
        return res
    finally:
        bv.close()


def hash_only(nb, kib, reps=20):
    """ibft_proposal_hashes alone from pinned sources under the form the environment pins → one JSON line"""
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(max_rows=65536)
    try:
        raw, roff, rnd = (V.pinned_copy(x) for x in proposals(nb, kib))
        out = np.zeros((nb, 32), np.uint8)
        a = (bv._h, V._p(raw), V._p(roff), V._p(rnd), nb, V._p(out))

        def fn():
            assert bv._L.ibft_proposal_hashes(*a) == 0

        ts = [timed(fn, 0.1, reps) * 1e3 for _ in range(3)]
        print(json.dumps({"blocks": nb, "kib": kib, "proposal_lanes_env": os.environ.get("IBFT_PROPOSAL_LANES", "auto"),
                          "call_ms": float(np.median(ts)), "call_min_ms": min(ts), "call_max_ms": max(ts),
                          "issue_probe_ns": bv.issue_probe()[0]}), flush=True)
    finally:
        bv.close()


def main_forms(a):
    rows = []
    for kib in a.kib:
        for nb in a.counts:
            if nb * kib * 1024 > 200 << 20:
                continue
            rec = {"blocks": nb, "kib": kib}
            for lanes in ("1", "64", "1", "64"):      # alternated: each form twice
                env = dict(os.environ, IBFT_PROPOSAL_LANES=lanes)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--hash-only", "--blocks", str(nb), "--kib", str(kib)],
                                   capture_output=True, text=True, timeout=300, env=env)
                if p.returncode != 0:                 # (nothing more is started on the device after a child that failed)
                    raise RuntimeError(f"child failed ({p.returncode}): {p.stdout[-500:]}{p.stderr[-1500:]}")
                r = json.loads(p.stdout.strip().split("\n")[-1])
                rec.setdefault("lanes%s_ms" % lanes, []).append(round(r["call_ms"], 4))
                rec["issue_probe_ns"] = r["issue_probe_ns"]
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for rec in rows:
                f.write(json.dumps(rec) + "\n")
    print(f"{'KiB':>5} {'proposals':>9} {'lane form ms':>20} {'wavefront form ms':>20}")
    for r in rows:
        print(f"{r['kib']:>5} {r['blocks']:>9} {str(r['lanes1_ms']):>20} {str(r['lanes64_ms']):>20}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--v", type=int, default=None)
    ap.add_argument("--blocks", type=int, default=None)
    ap.add_argument("--kib", type=int, nargs="*", default=None)
    ap.add_argument("--modes", type=str, nargs="*", default=["cold", "warm"])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON lines here")
    ap.add_argument("--forms", action="store_true", help="ibft_proposal_hashes alone: lane form against wavefront form")
    ap.add_argument("--counts", type=int, nargs="*", default=[64, 655, 2048, 4096, 8192, 16384, 65536], help="--forms: proposals per call")
    ap.add_argument("--hash-only", action="store_true", help="one configuration of ibft_proposal_hashes (child of --forms; rocprofv3)")
    a = ap.parse_args()
    if a.hash_only:
        return hash_only(a.blocks or 655, (a.kib or [1])[0])
    if a.forms:
        a.kib = a.kib or [1]
        return main_forms(a)
    shapes = [(100, 655, 1), (100, 655, 64), (4, 16384, 1)]
    if a.v is not None:
        shapes = [(a.v, a.blocks or 65536 // a.v, k) for k in (a.kib or [1])]
    rows = []
    for V_, nb, kib in shapes:
        for mode in a.modes:
            res = measure(V_, nb, kib, mode == "warm", a.alternations)
            rows.append(res)
            print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for res in rows:
                f.write(json.dumps(res) + "\n")
    cell = lambda r, k: f"{r[k + '_ms']:.3f} ({r[k + '_min_ms']:.3f}…{r[k + '_max_ms']:.3f})"
    print(f"{'V':>5} {'blocks':>6} {'KiB':>4} {'mode':>5} {'probe ns':>8} {'A raw ms':>24} {'B host loop ms':>26} {'C hashes given ms':>24} "
          f"{'A−C':>7} {'B−C':>8} {'loop alone':>10}")
    for r in rows:
        print(f"{r['v']:>5} {r['blocks']:>6} {r['kib']:>4} {r['mode']:>5} {r['issue_probe_ns']:>8.3f} {cell(r, 'A_raw'):>24} {cell(r, 'B_host_loop'):>26} "
              f"{cell(r, 'C_hashes_given'):>24} {r['A_minus_C_ms']:>7.3f} {r['B_minus_C_ms']:>8.3f} {r['host_hash_loop_ms']:>10.3f}")


if __name__ == "__main__":
    main()
