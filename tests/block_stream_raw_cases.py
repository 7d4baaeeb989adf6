"""Shared by tests/test_gpu_block_seals_stream_raw.py and its child processes (IBFT_STREAM_DIGEST and IBFT_PROPOSAL_LANES are
read at ibft_ctx_create: a fresh process is the clean way to set them): small block batches that carry their PROPOSALS, the
three streamed submits that take proposals or bare seals, their synchronous siblings, and a byte-exact fingerprint of a
result.  Shapes: V ∈ {4, 7}; 1, 3 and 40 blocks with empty blocks at the front, in the middle and at the end; no rows at all;
proposal lengths on both sides of every Keccak rate boundary; 600 and 2 100 rows so that AUTO passes through the
two-wavefront, one-wavefront and row-per-signature kernels.  Expected values never come from the streamed path."""
from __future__ import annotations

import hashlib
import sys
from dataclasses import dataclass

import numpy as np

SEED = 1311
LENGTHS = [0, 1, 135, 136, 137, 271, 272, 1000]   # rate boundaries (136), the splice of the round (128 … 136), ≈ 1 KiB
ROUNDS = [0, 1, 2**64 - 1, 7, 2**40 + 3]
SUFFIX = b"\x02commit"
N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
KINDS = ("verify_raw", "recover", "recover_raw")
MAX_ROWS = 4096


@dataclass
class Case:
    name: str
    r: object          # the round whose validator set judges the batch
    raws: list
    rounds: list
    bh: np.ndarray     # the oracle's proposal hashes of the blocks
    off: np.ndarray
    sig: np.ndarray
    signer: np.ndarray
    pre: np.ndarray | None

    @property
    def n(self) -> int:
        return int(self.off[-1])


_ROUNDS: dict = {}


def round_of(V_: int):
    from oracle import workload as W
    if V_ not in _ROUNDS:
        _ROUNDS[V_] = W.make_round(V_, SEED, raw_len=64)
    return _ROUNDS[V_]


def seal_digest(h: bytes, suffix) -> bytes:
    from oracle import binding as B
    return h if suffix is None else B.keccak256(h + suffix)


def _case(name, V_, sizes, suffix, byz, with_pre, k0):
    from oracle import binding as B
    import go_ibft_amd.verifier as V
    r = round_of(V_)
    rng = np.random.default_rng(SEED + k0)
    nb = len(sizes)
    raws = [rng.bytes(LENGTHS[(k0 + b) % len(LENGTHS)]) for b in range(nb)]
    rounds = [ROUNDS[(k0 + b) % len(ROUNDS)] for b in range(nb)]
    bh = np.frombuffer(b"".join(B.proposal_hash(x, q) for x, q in zip(raws, rounds)), np.uint8).reshape(nb, 32).copy() \
        if nb else np.zeros((0, 32), np.uint8)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(off[-1])
    sig = np.zeros((n, 65), np.uint8)
    signer = np.zeros((n, 20), np.uint8)
    pre = np.zeros(n, np.uint8) if with_pre else None
    for b in range(nb):
        d = seal_digest(bytes(bh[b]), suffix)
        who = rng.permutation(V_)
        for j, row in enumerate(range(int(off[b]), int(off[b + 1]))):
            i = int(who[j % V_])   # (more rows than validators: duplicate signers)
            s = bytearray(B.sign(r.sks[i], d))
            a = bytes(r.addrs[i])
            kind = int(rng.integers(0, 40)) if byz else 99
            if kind == 0:
                s[64] = 2                                   # v out of range
            elif kind == 1:
                s[:32] = bytes(32)                          # r = 0
            elif kind == 2:
                s[32:64] = (N_ORDER + 1).to_bytes(32, "big")   # s ≥ n
            elif kind == 3:
                s = bytearray(rng.bytes(65))                # random bytes
            elif kind == 4:
                a = bytes(r.addrs[(i + 1) % V_])            # a stolen seal
            elif kind == 5:
                a = bytes(rng.bytes(20))                    # From is no member
            elif kind == 6:                                 # the other s: valid, but high under IBFT_FLAG_STRICT_LOW_S
                s[32:64] = (N_ORDER - int.from_bytes(s[32:64], "big")).to_bytes(32, "big")
                s[64] ^= 1
            elif kind == 7 and row > int(off[b]):           # the seal of the row before, once more
                s, a = bytearray(sig[row - 1].tobytes()), signer[row - 1].tobytes()
            elif kind == 8 and b > 0 and off[b] > 0:        # a seal of an earlier block replayed here
                s = bytearray(sig[int(off[b]) - 1].tobytes())
            elif kind == 9 and with_pre:
                pre[row] = V.ROW_NIL if row & 1 else V.ROW_BADLEN
            sig[row] = np.frombuffer(bytes(s), np.uint8)
            signer[row] = np.frombuffer(a, np.uint8)
    return Case(name, r, raws, rounds, bh, off, sig, signer, pre)


_CASES: dict = {}


def cases(suffix=None) -> list[Case]:
    """the batches, their seals signed under the given seal-digest convention"""
    if suffix not in _CASES:
        forty = [(b * 5 + 3) % 8 for b in range(40)]
        forty[0] = forty[19] = forty[20] = forty[39] = 0
        _CASES[suffix] = [
            _case("v4_1x12", 4, [12], suffix, False, False, 0),
            _case("v7_front_empty", 7, [0, 7, 6], suffix, True, False, 1),
            _case("v7_middle_empty", 7, [7, 0, 6], suffix, False, True, 2),
            _case("v7_end_empty", 7, [9, 5, 0], suffix, True, True, 3),
            _case("no_rows", 7, [0, 0, 0], suffix, False, False, 4),
            _case("v7_40_blocks", 7, forty, suffix, True, True, 5),
            _case("v7_600", 7, [6] * 100, suffix, True, False, 6),
            _case("v4_2100", 4, [4] * 524 + [0, 4], suffix, True, True, 7),
        ]
        tot = [c.n for c in _CASES[suffix]]
        assert tot[5] in range(12, 281) and tot[6] == 600 and tot[7] == 2100 and tot[4] == 0
    return _CASES[suffix]


def pinned(c: Case):
    """(raw, raw_off) and the columns of the case in ibft_pinned_alloc memory"""
    import go_ibft_amd.verifier as V
    p = lambda a: a if a is None or not a.size else V.pinned_copy(a)
    raw, roff, _ = V.proposal_columns(c.raws, c.rounds)
    return (p(raw), p(roff)), Case(c.name + "/pinned", c.r, c.raws, c.rounds, p(c.bh), p(c.off), p(c.sig), p(c.signer), p(c.pre))


def fields(t):
    return (t.power, t.quorum, t.valid_rows, t.distinct_senders, t.has_quorum, t.shard_overlap, t.proposer_rows)


def submit(bv, kind: str, c: Case, raws=None) -> int:
    raws = c.raws if raws is None else raws
    if kind == "verify_raw":
        return bv.block_seals_submit_raw(raws, c.rounds, c.off, c.sig, c.signer, c.pre)
    if kind == "recover":
        return bv.recover_block_seals_submit(c.bh, c.off, c.sig, c.pre)
    if kind == "recover_raw":
        return bv.recover_block_seals_submit_raw(raws, c.rounds, c.off, c.sig, c.pre)
    assert kind == "verify"
    return bv.block_seals_submit(c.bh, c.off, c.sig, c.signer, c.pre)


def kind_bits(kind: str) -> int:
    return {"verify": 0, "verify_raw": 2, "recover": 1, "recover_raw": 3}[kind]


def sibling(bv, kind: str, c: Case) -> dict:
    """the synchronous sibling's result in the shape block_seals_collect_ex delivers"""
    if kind == "verify_raw":
        m, tl, bh = bv.verify_block_seals_raw(c.raws, c.rounds, c.off, c.sig, c.signer, c.pre)
        return {"kind": 2, "verdict": m, "tallies": tl, "block_hash32": bh}
    if kind == "recover":
        a, v, m, tl = bv.recover_block_seals(c.bh, c.off, c.sig, c.pre)
        return {"kind": 1, "verdict": m, "tallies": tl, "signer20": a, "vidx": v}
    if kind == "recover_raw":
        a, v, m, tl, bh = bv.recover_block_seals_raw(c.raws, c.rounds, c.off, c.sig, c.pre)
        return {"kind": 3, "verdict": m, "tallies": tl, "block_hash32": bh, "signer20": a, "vidx": v}
    m, tl = bv.verify_block_seals(c.bh, c.off, c.sig, c.signer, c.pre)
    return {"kind": 0, "verdict": m, "tallies": tl}


def same(got: dict, want: dict, what: str):
    """bit for bit: the same keys, the same bytes in every output"""
    assert sorted(got) == sorted(want), f"{what}: {sorted(got)} != {sorted(want)}"
    assert got["kind"] == want["kind"], what
    for k in ("verdict", "block_hash32", "signer20", "vidx"):
        if k in want:
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k} {g.shape} {g.dtype} != {w.shape} {w.dtype}"
            assert (g == w).all(), f"{what}: {k} differs at {np.argwhere(g != w)[:5].tolist()}"
    assert [fields(t) for t in got["tallies"]] == [fields(t) for t in want["tallies"]], f"{what}: tallies differ"


def fingerprint(res: dict) -> str:
    h = hashlib.sha256(str(res["kind"]).encode())
    for k in ("verdict", "block_hash32", "signer20", "vidx"):
        if k in res:
            h.update(k.encode() + np.ascontiguousarray(res[k]).tobytes())
    h.update(repr([fields(t) for t in res["tallies"]]).encode())
    return h.hexdigest()


def run_streamed(bv, kind: str, seq: list, in_flight: int = 1) -> list:
    """submit(k + 1), collect(k) over the cases; the validator set is changed in front of the submit that needs another one"""
    cur, got, pend = None, [], 0
    for c in seq:
        if cur is not c.r:
            bv.set_validators(c.r.height, c.r.addrs, c.r.power)
            cur = c.r
        assert submit(bv, kind, c) == c.n
        pend += 1
        while pend > in_flight:
            k = len(got)
            assert bv.block_seals_pending_ex() == (pend, seq[k].n, len(seq[k].bh), kind_bits(kind))
            got.append(bv.block_seals_collect_ex())
            pend -= 1
    while pend:
        k = len(got)
        assert bv.block_seals_pending_ex() == (pend, seq[k].n, len(seq[k].bh), kind_bits(kind))
        got.append(bv.block_seals_collect_ex())
        pend -= 1
    assert bv.block_seals_pending_ex() == (0, 0, 0, 0)
    return got


def run_sync(bv, kind: str, seq: list) -> list:
    cur, out = None, []
    for c in seq:
        if cur is not c.r:
            bv.set_validators(c.r.height, c.r.addrs, c.r.power)
            cur = c.r
        out.append(sibling(bv, kind, c))
    return out


def main() -> int:
    """child process: the two raw kinds, streamed with one batch in flight under this process's environment → one fingerprint
    line per (kind, case)"""
    import go_ibft_amd.verifier as V
    seq = cases(None)
    bv = V.BatchVerifier(max_rows=MAX_ROWS)
    try:
        for kind in ("verify_raw", "recover_raw"):
            for c, g in zip(seq, run_streamed(bv, kind, seq, 1)):
                print("FP", kind, c.name, fingerprint(g))
    finally:
        bv.close()
    print("STREAM_RAW_CHILD_OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
