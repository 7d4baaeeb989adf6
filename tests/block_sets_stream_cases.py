"""Shared by tests/test_gpu_block_seals_sets_stream.py, its child processes (IBFT_STREAM_DIGEST and IBFT_PROPOSAL_LANES are read
at ibft_ctx_create) and tests/test_block_seals_sets_stream_inputs.py: block batches that carry their PROPOSALS and a set per
block, the six calls under test, their siblings, and the CPU oracle's answer.  Families and rows come from the generators of
tests/test_gpu_block_seals_sets.py (Fam, _fixture) — the fixture signs whatever _block_hashes hands it, so it is handed the
(seal digests of the) proposal hashes of proposals made here.
Shapes, the smallest at which this code can go wrong: 3 sets of 7 validators sliding over a pool of 11, 27 blocks — the
fixture's 13 row kinds, each under two different sets, the set changing every third block — plus one empty block; 70
validators per set and 5 blocks, where a block's rows span 64-bit verdict words and blocks straddle them; proposals of 0, 135,
136, 137 and 1 000 bytes (the Keccak rate is 136).  Expected values never come from the calls under test."""
from __future__ import annotations

import sys
from dataclasses import dataclass
from unittest import mock

import numpy as np

import block_stream_raw_cases as S
import test_gpu_block_seals_sets as T

LENGTHS = [0, 135, 136, 137, 1000]
ROUNDS = [0, 1, 2**64 - 1, 7, 2**40 + 3]
SUFFIX = S.SUFFIX
N_ORDER = S.N_ORDER
MAX_ROWS = 4096
KINDS = ("verify", "verify_raw", "recover", "recover_raw")
BATCH_SETS = 4
HIGH_S_KINDS = (3, 12)    # blocks of these fixture kinds get their last row (a plain valid one) flipped to its high-s twin

fields = S.fields
same = S.same
fingerprint = S.fingerprint


@dataclass
class Case:
    name: str
    f: object          # the family (T.Fam) that judges the batch
    bset: np.ndarray
    raws: list
    rounds: list
    bh: np.ndarray     # the oracle's proposal hashes of the blocks
    off: np.ndarray
    sig: np.ndarray
    signer: np.ndarray
    pre: np.ndarray | None
    kind_of_block: list   # the fixture's row kind (b % 13 of the fixture's own numbering), -1 for a block added here

    @property
    def n(self) -> int:
        return int(self.off[-1])


def proposals(nb: int, seed: int):
    from oracle import binding as B
    rng = np.random.default_rng(seed)
    raws = [rng.bytes(LENGTHS[(seed + b) % len(LENGTHS)]) for b in range(nb)]
    rounds = [ROUNDS[(seed + 2 * b) % len(ROUNDS)] ^ (b << 8) for b in range(nb)]   # (no two proposals alike)
    bh = np.frombuffer(b"".join(B.proposal_hash(x, q) for x, q in zip(raws, rounds)), np.uint8).reshape(nb, 32).copy()
    return raws, rounds, bh


def make_case(name: str, f, bset, seed: int, suffix=None, empty_at=None) -> Case:
    """the fixture's rows over proposals made here, signed under the given seal-digest convention; empty_at: a block without
    rows (judged under set 1) put in front of that block"""
    nb = len(bset)
    raws, rounds, bh = proposals(nb + (empty_at is not None), seed)
    keep = [b for b in range(len(bh)) if b != empty_at]
    signed = np.array([np.frombuffer(S.seal_digest(bytes(h), suffix), np.uint8) for h in bh[keep]], np.uint8).reshape(nb, 32)
    with mock.patch.object(T, "_block_hashes", lambda n_, seed_: signed):
        _, off, sig, signer, pre = T._fixture(f, list(bset), seed)
    kinds = [b % 13 for b in range(nb)]
    sig = sig.copy()
    for b in range(nb):   # high-s twins: valid rows that IBFT_FLAG_STRICT_LOW_S refuses
        if kinds[b] in HIGH_S_KINDS:
            row = int(off[b + 1]) - 1
            s = sig[row].tobytes()
            sig[row] = np.frombuffer(s[:32] + (N_ORDER - int.from_bytes(s[32:64], "big")).to_bytes(32, "big") + bytes([s[64] ^ 1]), np.uint8)
    bset = np.asarray(bset, np.uint32)
    if empty_at is not None:
        off = np.insert(off, empty_at, off[empty_at]).astype(np.uint32)
        bset = np.insert(bset, empty_at, 1).astype(np.uint32)
        kinds.insert(empty_at, -1)
    return Case(name, f, bset, raws, rounds, bh, off, sig, signer, pre, kinds)


def no_rows_case(f, seed: int) -> Case:
    """three blocks, no seal at all: their proposals are still hashed by a submit, and every tally carries its set's quorum"""
    raws, rounds, bh = proposals(3, seed)
    return Case("no_rows", f, np.array([2, 0, 2], np.uint32), raws, rounds, bh, np.zeros(4, np.uint32), np.zeros((0, 65), np.uint8),
                np.zeros((0, 20), np.uint8), None, [-1] * 3)


_MEMO: dict = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def family(big: bool = False):
    """3 sets of 7 sliding (by 2) over a pool of 11"""
    return _memo(("fam", big), lambda: T.Fam(11, 7, 2, 3, 4100, big=big))


def family70():
    """3 sets of 70 sliding (by 4) over a pool of 78"""
    return _memo("fam70", lambda: T.Fam(78, 70, 4, 3, 4170))


def other_family():
    """other keys, other powers, fewer sets: block_set entries of a batch made for family() are out of range here"""
    return _memo("other", lambda: T.Fam(11, 7, 4, 2, 4199))


def main_case(suffix=None, big: bool = False) -> Case:
    bset = [(b // 3) % 3 for b in range(27)]   # blocks b and b + 13 — the same row kind — lie in different sets
    return _memo(("main", suffix, big), lambda: make_case("sets27", family(big), bset, 4101, suffix, empty_at=14))


def wide_case() -> Case:
    return _memo("wide", lambda: make_case("sets70", family70(), [0, 1, 2, 1, 0], 4171))


def other_case() -> Case:
    return _memo("othercase", lambda: make_case("other", other_family(), [b % 2 for b in range(8)], 4198))


def empty_case() -> Case:
    return _memo("empty", lambda: no_rows_case(family(), 4102))


def pinned(c: Case):
    """(raw, raw_off) and the columns of the case — block_set included — in ibft_pinned_alloc memory"""
    import go_ibft_amd.verifier as V
    p = lambda a: a if a is None or not a.size else V.pinned_copy(a)
    raw, roff, _ = V.proposal_columns(c.raws, c.rounds)
    return Case(c.name + "/pinned", c.f, p(c.bset), (p(raw), p(roff)), c.rounds, p(c.bh), p(c.off), p(c.sig), p(c.signer), p(c.pre),
                c.kind_of_block)


def expect_cpu(c: Case, suffix=None, flags: int = 0, bare: bool = False):
    """the CPU oracle block by block under ValSet(set of b) → (bits, tally fields per block, recovered addresses, set indices).
    bare: bits and tallies of the recover forms — the rows judged with the RECOVERED address in the place of the claimed one
    (a stolen seal is a valid row of its true signer there)"""
    from oracle import binding as B
    digest = None if suffix is None else (lambda h: B.keccak256(h + suffix))
    if c.n == 0:
        q = [(0, 2 * sum(c.f.power[int(k)]) // 3 + 1, 0, 0, 0) for k in c.bset]
        return np.zeros(0, bool), q, np.zeros((0, 20), np.uint8), np.zeros(0, np.int32)
    bits, tallies, who, vidx = T._expect_cpu(c.f, c.bset, c.bh, c.off, c.sig, c.signer, c.pre, digest, flags, recover=True)
    if bare:
        bits, tallies = T._expect_cpu(c.f, c.bset, c.bh, c.off, c.sig, who, c.pre, digest, flags)
        assert (bits == (vidx >= 0)).all()     # recovered, and a member of the block's set
    return bits, tallies, who, vidx


def kind_bits(kind: str) -> int:
    return S.kind_bits(kind) | BATCH_SETS


def submit(bv, kind: str, c: Case) -> int:
    if kind == "verify":
        return bv.block_seals_submit_sets(c.bh, c.off, c.bset, c.sig, c.signer, c.pre)
    if kind == "verify_raw":
        return bv.block_seals_submit_sets_raw(c.raws, c.rounds, c.off, c.bset, c.sig, c.signer, c.pre)
    if kind == "recover":
        return bv.recover_block_seals_submit_sets(c.bh, c.off, c.bset, c.sig, c.pre)
    assert kind == "recover_raw"
    return bv.recover_block_seals_submit_sets_raw(c.raws, c.rounds, c.off, c.bset, c.sig, c.pre)


def sibling(bv, kind: str, c: Case) -> dict:
    """the synchronous sibling's result in the shape block_seals_collect_ex delivers"""
    k = kind_bits(kind)
    if kind == "verify":
        m, tl = bv.verify_block_seals_sets(c.bh, c.off, c.bset, c.sig, c.signer, c.pre)
        return {"kind": k, "verdict": m, "tallies": tl}
    if kind == "verify_raw":
        m, tl, bh = bv.verify_block_seals_sets_raw(c.raws, c.rounds, c.off, c.bset, c.sig, c.signer, c.pre)
        return {"kind": k, "verdict": m, "tallies": tl, "block_hash32": bh}
    if kind == "recover":
        a, v, m, tl = bv.recover_block_seals_sets(c.bh, c.off, c.bset, c.sig, c.pre)
        return {"kind": k, "verdict": m, "tallies": tl, "signer20": a, "vidx": v}
    a, v, m, tl, bh = bv.recover_block_seals_sets_raw(c.raws, c.rounds, c.off, c.bset, c.sig, c.pre)
    return {"kind": k, "verdict": m, "tallies": tl, "block_hash32": bh, "signer20": a, "vidx": v}


def hashes_route(bv, kind: str, c: Case) -> dict:
    """what exists without the _sets_raw calls: ibft_proposal_hashes, then the hashes-given _sets call with those hashes"""
    bh = bv.proposal_hashes(c.raws, c.rounds)
    k = kind_bits(kind)
    if kind == "verify_raw":
        m, tl = bv.verify_block_seals_sets(bh, c.off, c.bset, c.sig, c.signer, c.pre)
        return {"kind": k, "verdict": m, "tallies": tl, "block_hash32": bh}
    a, v, m, tl = bv.recover_block_seals_sets(bh, c.off, c.bset, c.sig, c.pre)
    return {"kind": k, "verdict": m, "tallies": tl, "block_hash32": bh, "signer20": a, "vidx": v}


def run_streamed(bv, kind: str, seq: list, in_flight: int = 1) -> list:
    """the cases through the pipeline with at most `in_flight` batches in flight (one family: installed by the caller): 1 —
    every batch is collected before the next submit; 2 — submit(k + 1), then collect(k)"""
    got, pend = [], 0

    def collect():
        k = seq[len(got)]
        assert bv.block_seals_pending_ex() == (pend, k.n, len(k.bh), kind_bits(kind))
        got.append(bv.block_seals_collect_ex())

    for c in seq:
        while pend >= in_flight:
            collect()
            pend -= 1
        assert submit(bv, kind, c) == c.n
        pend += 1
    while pend:
        collect()
        pend -= 1
    assert bv.block_seals_pending_ex() == (0, 0, 0, 0)
    return got


def main() -> int:
    """child process: the two raw kinds, streamed with one batch in flight under this process's environment → one fingerprint
    line per (kind, case)"""
    import go_ibft_amd.verifier as V
    seq = [main_case(), empty_case()]
    bv = V.BatchVerifier(max_rows=MAX_ROWS)
    try:
        family().install(bv)
        for kind in ("verify_raw", "recover_raw"):
            for c, g in zip(seq, run_streamed(bv, kind, seq, 1)):
                print("FP", kind, c.name, fingerprint(g))
    finally:
        bv.close()
    print("SETS_STREAM_CHILD_OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
