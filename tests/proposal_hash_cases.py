"""Shared by tests/test_gpu_proposal_hashes.py and its child processes (one per pinned form of proposal_digest_kernel:
IBFT_PROPOSAL_LANES is read at ibft_ctx_create, and a fresh process is the clean way to pin it): batches of proposals and what
the ORACLE says their hashes are — oracle.binding.proposal_hash, never the call under test."""
from __future__ import annotations

import sys

import numpy as np

SEED = 1136
# every position of the round within a rate block (see tests/test_dev_proposal_digest_host.py), then long ones
EDGE_LENGTHS = list(range(0, 301)) + [1000, 4095] + [65536 + k for k in (0, 7, 8, 9, 15)]
MIB = 1 << 20
ROUNDS = [0, 1, 2**64 - 1, 7, 2**40 + 3]
SHORT_COUNTS = [1, 63, 64, 65, 4096, 65536]


def mixed_batch():
    """(proposals, rounds): the edge lengths in a shuffled order — so that starts fall on every offset mod 4 and long and short
    proposals share a wavefront — plus three proposals of 1 MiB (and 1 MiB ± 1)"""
    rng = np.random.default_rng(SEED)
    lens = EDGE_LENGTHS + [MIB, MIB + 1, MIB - 1]
    lens = [lens[i] for i in rng.permutation(len(lens))]
    raws = [rng.bytes(n) for n in lens]
    rounds = [ROUNDS[i % len(ROUNDS)] for i in range(len(raws))]
    return raws, rounds


def short_batch(n: int):
    """n proposals of 0 … 300 bytes (a block header's size), rounds 0 … 2⁶⁴ − 1"""
    rng = np.random.default_rng(SEED + n)
    lens = rng.integers(0, 301, n)
    blob = rng.bytes(int(lens.sum()))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    raws = [blob[off[i]:off[i + 1]] for i in range(n)]
    rounds = rng.integers(0, 2**64, n, dtype=np.uint64)
    rounds[:3] = [0, 2**64 - 1, 1][:min(n, 3)]
    return raws, [int(r) for r in rounds]


def expected(raws, rounds) -> np.ndarray:
    from oracle import binding as B
    return np.frombuffer(b"".join(B.proposal_hash(r, q) for r, q in zip(raws, rounds)), np.uint8).reshape(len(raws), 32)


def check_all(bv, V, label: str) -> int:
    """the mixed batch and every short count, from pageable and from pinned sources, against the oracle → cases checked"""
    done = 0
    batches = [("mixed", mixed_batch())] + [(f"short{n}", short_batch(n)) for n in SHORT_COUNTS]
    for name, (raws, rounds) in batches:
        want = expected(raws, rounds)
        got = bv.proposal_hashes(raws, rounds)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert got.shape == want.shape and not len(bad), f"{label} {name} pageable: rows {bad[:8]} (lengths {[len(raws[i]) for i in bad[:8]]})"
        raw, off, rnd = V.proposal_columns(raws, rounds)
        g0 = bv.gather_batches()
        got = bv.proposal_hashes((V.pinned_copy(raw), V.pinned_copy(off)), V.pinned_copy(rnd))
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert not len(bad), f"{label} {name} pinned: rows {bad[:8]}"
        assert bv.gather_batches() == g0 + 1, f"{label} {name}: pinned columns did not take the gather launch"
        done += 2
    return done


def main() -> int:
    """child process: the environment pins the form"""
    import os
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(max_rows=65536)
    try:
        done = check_all(bv, V, "IBFT_PROPOSAL_LANES=" + os.environ.get("IBFT_PROPOSAL_LANES", "auto"))
    finally:
        bv.close()
    print("PROPOSAL_HASHES_OK", done)
    return 0


if __name__ == "__main__":
    sys.exit(main())
