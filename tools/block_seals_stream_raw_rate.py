#!/usr/bin/env python3
"""Streamed chain sync from proposals and from bare seals: time per batch of the streamed submits against what a streaming
syncer had before them.

    python tools/block_seals_stream_raw_rate.py                      # every shape below, proposals and bare seals
    python tools/block_seals_stream_raw_rate.py --only raw --v 100 --blocks 655 --mode cold   # one configuration
    python tools/block_seals_stream_raw_rate.py --only recover --parent-lib OLD/libibftgpu.so # leg B on another build too

One lease, one process; every column — the proposal bytes included — in ibft_pinned_alloc memory; every leg rotates three
distinct pre-signed batches; the legs are alternated --alternations times and the median (min … max) of the rounds is
reported; ibft_issue_probe of the lease is printed on every line.

From proposals (V = 100 × 655 blocks and V = 4 × 16 384 blocks with 1 KiB proposals, cold and warm; 64 KiB × 655 blocks):
  A_main / A_copy  ibft_block_seals_submit_raw / _collect_ex, one batch kept in flight, proposal_digest_kernel on the main /
                   on the copy stream (IBFT_STREAM_DIGEST is read at ibft_ctx_create: a context per setting, same process)
  B                what a streaming syncer had: ibft_proposal_hashes, then ibft_block_seals_submit / _collect per step
  C                the streamed hashes-given call alone (the floor: no hashing at all)
Bare seals (V = 100 × 655 blocks and V = 1 024 × 63 blocks, cold):
  A                ibft_recover_block_seals_submit / _collect_ex, one batch kept in flight
  B                the synchronous ibft_recover_block_seals from the same pinned sources — of this build, and with
                   --parent-lib of the parent commit's library as well, in child processes alternating with this build's
One JSON line per configuration, then a table."""
import argparse
import ctypes as C
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


def probe(bv):
    try:
        return round(float(bv.issue_probe()[0]), 3)
    except Exception:
        return None


def batches(bv, V_, nb, prop_len, with_raw=True):
    """three distinct batches in pinned memory: (raw, raw_off, round, bh, off, sig, signer) — every validator seals every block"""
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    r = W.make_round(V_, 7, raw_len=64)
    bv.set_validators(r.height, r.addrs, r.power)
    off = (np.arange(nb + 1) * V_).astype(np.uint32)
    sk = np.tile(np.frombuffer(b"".join(r.sks), np.uint8).reshape(V_, 32), (nb, 1))
    out = []
    rng = np.random.default_rng(11)
    for k in range(3):
        raw = rng.integers(0, 256, nb * prop_len, dtype=np.uint8)
        roff = (np.arange(nb + 1, dtype=np.uint64) * prop_len).astype(np.uint32)
        rnd = (np.arange(nb, dtype=np.uint64) + k)
        bh = bv.proposal_hashes((raw, roff), rnd).copy()   # (checked against the oracle by the test suite)
        sig, signer, ok = bv.sign_seals(sk, np.repeat(bh, V_, axis=0))
        assert ok.all()
        out.append(tuple(V.pinned_copy(a) for a in (raw, roff, rnd, bh, off, sig, signer)))
    return r, out


def summarise(res, times):
    for name, ts in times.items():
        res[name + "_ms"] = float(np.median(ts))
        res[name + "_min_ms"] = min(ts)
        res[name + "_max_ms"] = max(ts)


def measure_raw(V_, nb, prop_len, warm, alternations):
    import go_ibft_amd.verifier as V
    flags = V.FLAG_PUBKEY_CACHE if warm else 0
    ctx = {}
    for placement in ("main", "copy"):
        os.environ["IBFT_STREAM_DIGEST"] = placement
        ctx[placement] = V.BatchVerifier(flags=flags, max_rows=65536)
    os.environ.pop("IBFT_STREAM_DIGEST", None)
    try:
        main = ctx["main"]
        r, bt = batches(main, V_, nb, prop_len)
        ctx["copy"].set_validators(r.height, r.addrs, r.power)
        n = nb * V_
        L = main._L
        p = V._p
        mask = np.zeros((n + 63) // 64, np.uint64)
        tal = (V.Tally * nb)()
        hashes = np.zeros((nb, 32), np.uint8)
        state = {"k": 0}

        def nxt():
            state["k"] = (state["k"] + 1) % 3
            return bt[state["k"]]

        def a_submit(bv):
            raw, roff, rnd, bh, off, sig, signer = nxt()
            rc = L.ibft_block_seals_submit_raw(bv._h, p(raw), p(roff), p(rnd), p(off), nb, p(sig), p(signer), None)
            assert rc == 0, rc

        def a_collect(bv):
            rc = L.ibft_block_seals_collect_ex(bv._h, p(hashes), None, None, p(mask), tal)
            assert rc == 0, rc

        def c_submit(hash_first):
            raw, roff, rnd, bh, off, sig, signer = nxt()
            if hash_first:   # the synchronous hash call enqueues behind the batch in flight: the host waits for it
                rc = L.ibft_proposal_hashes(main._h, p(raw), p(roff), p(rnd), nb, p(hashes))
                assert rc == 0, rc
                bh = hashes
            rc = L.ibft_block_seals_submit(main._h, p(bh), p(off), nb, p(sig), p(signer), None)
            assert rc == 0, rc

        def c_collect():
            rc = L.ibft_block_seals_collect(main._h, p(mask), tal)
            assert rc == 0, rc

        legs = {
            "A_main": (lambda: a_submit(ctx["main"]), lambda: a_collect(ctx["main"])),
            "A_copy": (lambda: a_submit(ctx["copy"]), lambda: a_collect(ctx["copy"])),
            "B": (lambda: c_submit(True), c_collect),
            "C": (lambda: c_submit(False), c_collect),
        }

        def check():
            assert V.mask_to_bool(mask, n).all() and all(t.has_quorum == 1 for t in tal)

        for sub, col in legs.values():   # warm-up: buffers grow, the key cache learns and builds (warm)
            for _ in range(2):
                sub(); col(); check()
        times = {k: [] for k in legs}
        for _ in range(alternations):
            for name, (sub, col) in legs.items():
                sub()                     # prime: the timed steps always find one batch in flight

                def step():
                    sub()
                    col()
                times[name].append(timed(step) * 1e3)
                col()
                check()
        res = {"what": "raw", "v": V_, "blocks": nb, "rows": n, "proposal_bytes": prop_len, "mode": "warm" if warm else "cold",
               "alternations": alternations, "issue_probe_ns": probe(main)}
        summarise(res, times)
        return res
    finally:
        for bv in ctx.values():
            bv.close()


def measure_recover(V_, nb, alternations, sync_only=False):
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(max_rows=65536)
    try:
        r, bt = batches(bv, V_, nb, 64)
        n = nb * V_
        L = bv._L
        p = V._p
        mask = np.zeros((n + 63) // 64, np.uint64)
        tal = (V.Tally * nb)()
        out_signer = np.zeros((n, 20), np.uint8)
        out_vidx = np.zeros(n, np.int32)
        state = {"k": 0}

        def nxt():
            state["k"] = (state["k"] + 1) % 3
            return bt[state["k"]]

        def submit():
            _, _, _, bh, off, sig, _ = nxt()
            rc = L.ibft_recover_block_seals_submit(bv._h, p(bh), p(off), nb, p(sig), None)
            assert rc == 0, rc

        def collect():
            rc = L.ibft_block_seals_collect_ex(bv._h, None, p(out_signer), p(out_vidx), p(mask), tal)
            assert rc == 0, rc

        def sync():
            _, _, _, bh, off, sig, _ = nxt()
            rc = L.ibft_recover_block_seals(bv._h, p(bh), p(off), nb, p(sig), None, p(out_signer), p(out_vidx), p(mask), tal)
            assert rc == 0, rc

        def check():
            assert V.mask_to_bool(mask, n).all() and (out_vidx >= 0).all() and all(t.has_quorum == 1 for t in tal)

        sync(); check()
        times = {"B": []} if sync_only else {"A": [], "B": []}
        for _ in range(alternations):
            if not sync_only:
                submit()

                def step():
                    submit()
                    collect()
                times["A"].append(timed(step) * 1e3)
                collect()
                check()
            times["B"].append(timed(sync) * 1e3)
            check()
        res = {"what": "recover", "v": V_, "blocks": nb, "rows": n, "mode": "cold", "alternations": alternations,
               "issue_probe_ns": probe(bv), "lib": os.environ.get("IBFT_GPU_LIB", "this build")}
        summarise(res, times)
        return res
    finally:
        bv.close()


def child_sync(lib, V_, nb):
    """leg B of the recover measurement in a fresh process bound to `lib` (None: this build) → its result line"""
    env = dict(os.environ)
    if lib:
        env["IBFT_GPU_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-sync", "--v", str(V_), "--blocks", str(nb),
                          "--alternations", "1"], env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(out.stdout[-1000:] + out.stderr[-1000:])
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def cell(r, k):
    return f"{r[k + '_ms']:.3f} ({r[k + '_min_ms']:.3f} … {r[k + '_max_ms']:.3f})" if k + "_ms" in r else "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["raw", "recover"])
    ap.add_argument("--v", type=int)
    ap.add_argument("--blocks", type=int)
    ap.add_argument("--proposal-bytes", type=int, default=1024)
    ap.add_argument("--mode", choices=["cold", "warm"])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--parent-lib", help="recover: leg B on this other build of libibftgpu.so as well (child processes)")
    ap.add_argument("--child-sync", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_sync:
        print(json.dumps(measure_recover(a.v, a.blocks, a.alternations, sync_only=True)), flush=True)
        return 0
    rows = []
    if a.only != "recover":
        shapes = [(a.v, a.blocks, a.proposal_bytes)] if a.v and a.blocks else [(100, 655, 1024), (4, 16384, 1024), (100, 655, 65536)]
        for V_, nb, pl in shapes:
            for mode in ([a.mode] if a.mode else (["cold"] if pl > 1024 else ["cold", "warm"])):
                res = measure_raw(V_, nb, pl, mode == "warm", a.alternations)
                print(json.dumps(res), flush=True)
                rows.append(res)
    if a.only != "raw":
        for V_, nb in ([(a.v, a.blocks)] if a.v and a.blocks else [(100, 655), (1024, 63)]):
            res = measure_recover(V_, nb, a.alternations)
            if a.parent_lib:
                this, parent = [], []
                for _ in range(a.alternations):
                    parent.append(child_sync(a.parent_lib, V_, nb)["B_ms"])
                    this.append(child_sync(None, V_, nb)["B_ms"])
                summarise(res, {"B_parent_lib": parent, "B_this_lib_child": this})
            print(json.dumps(res), flush=True)
            rows.append(res)
    print()
    for r in rows:
        if r["what"] == "raw":
            print(f"raw      V {r['v']:>5} blocks {r['blocks']:>6} prop {r['proposal_bytes']:>6} B {r['mode']:>5}  A_main {cell(r, 'A_main')}  "
                  f"A_copy {cell(r, 'A_copy')}  B {cell(r, 'B')}  C {cell(r, 'C')}  ms/batch  probe {r['issue_probe_ns']} ns")
        else:
            print(f"recover  V {r['v']:>5} blocks {r['blocks']:>6} cold  A {cell(r, 'A')}  B {cell(r, 'B')}  B parent lib {cell(r, 'B_parent_lib')}  "
                  f"ms/batch  A/B {r['A_ms'] / r['B_ms']:.3f}  probe {r['issue_probe_ns']} ns")
    return 0


if __name__ == "__main__":
    sys.exit(main())
