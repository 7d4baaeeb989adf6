"""Shared by tests/test_gpu_block_seals_stream.py (and its IBFT_NO_HOST_DIRECT child process): a stream of block batches of
differing shape, what the oracle says about each, and a driver that keeps a given number of batches in flight through
ibft_block_seals_submit / ibft_block_seals_collect.  Expected values come from the CPU oracle (the way
tests/test_gpu_block_seals.py builds them) and from the synchronous ibft_verify_block_seals on a second context — never
from the streamed path."""
from __future__ import annotations

import sys
from dataclasses import dataclass, field

import numpy as np

SEED = 1201


@dataclass
class Batch:
    name: str
    r: object            # the round whose validator set (addrs, power) judges the batch
    bh: np.ndarray
    off: np.ndarray
    sig: np.ndarray
    signer: np.ndarray
    pre: np.ndarray | None = None
    _exp: tuple | None = field(default=None, repr=False)

    @property
    def n(self) -> int:
        return int(self.off[-1])

    def cols(self):
        return self.bh, self.off, self.sig, self.signer, self.pre


def fields(t):
    return (t.power, t.quorum, t.valid_rows, t.distinct_senders, t.has_quorum)


def expected(b: Batch):
    """(oracle verdicts bool[n], [tally fields per block])"""
    if b._exp is None:
        from oracle import binding as B
        import test_gpu_block_seals as BS
        vs = B.ValSet(b.r.addrs, b.r.power)
        if b.n:
            exp, te = BS._expect(vs, b.bh, b.off, b.sig, b.signer, b.pre)
            b._exp = (exp, [fields(t) for t in te])
        else:
            b._exp = (np.zeros(0, bool), [(0, vs.quorum, 0, 0, 0)] * len(b.bh))
    return b._exp


_ROUNDS: dict = {}


def round_of(V_: int, seed: int = SEED, weighted: bool = False):
    """validator i's key depends on (seed, i) only: the 4-validator set is a prefix of the 100- and the 1 024-validator one"""
    from oracle import workload as W
    k = (V_, seed, weighted)
    if k not in _ROUNDS:
        _ROUNDS[k] = W.make_round(V_, seed, raw_len=64, weighted=weighted)
    return _ROUNDS[k]


def _hashes(nb: int, tag: bytes) -> np.ndarray:
    from oracle import binding as B
    return np.frombuffer(b"".join(B.keccak256(tag + b.to_bytes(4, "little")) for b in range(nb)), np.uint8).reshape(nb, 32).copy()


def _signed(bv, r, bh, off, who):
    import test_gpu_block_seals as BS
    if int(off[-1]) <= 2048:   # small: the oracle signs
        from oracle import binding as B
        rh = BS._rows_hash(bh, off)
        sig = np.array([np.frombuffer(B.sign(r.sks[i], bytes(h)), np.uint8) for i, h in zip(who, rh)], np.uint8).reshape(-1, 65)
        return sig, r.addrs[np.asarray(who)].copy()
    return BS._device_signed(bv, r, bh, off, who)


_STREAM: list | None = None


def stream() -> list[Batch]:
    """nine batches: 64 × 100 with every kind of bad row, a ragged layout with empty blocks, no rows (three empty blocks),
    16 384 blocks of 4, one block of 65 536 rows, 4 rows straight after it, 655 × 100, no blocks at all, 16 × 100 weighted"""
    global _STREAM
    if _STREAM is not None:
        return _STREAM
    import go_ibft_amd.verifier as V
    import test_gpu_block_seals as BS
    rng = np.random.default_rng(SEED)
    out = []
    r100, r4, r1024 = round_of(100), round_of(4), round_of(1024)
    bv = V.BatchVerifier(max_rows=65536)   # signs the large batches (ibft_sign_seals)
    try:
        r, _, bh, off, sig, signer, pre = BS._sync_fixture(100, 64, SEED)
        assert r.addrs.tobytes() == r100.addrs.tobytes()
        out.append(Batch("64x100_bad_rows", r100, bh, off, sig, signer, pre))

        sizes = [0, 1, 0, 0, 3, 63, 64, 65, 1, 0, 130, 7, 0, 200, 1, 1, 0]
        bh = _hashes(len(sizes), b"rag")
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        who = rng.integers(0, 100, int(off[-1]))
        sig, signer = _signed(bv, r100, bh, off, who)
        sig[rng.random(len(who)) < 0.15, 64] = 2
        out.append(Batch("ragged", r100, bh, off, sig, signer))

        out.append(Batch("three_empty_blocks", r100, _hashes(3, b"emp"), np.zeros(4, np.uint32), np.zeros((0, 65), np.uint8),
                         np.zeros((0, 20), np.uint8)))

        nb = 16384
        bh = _hashes(nb, b"blk4")
        off = (np.arange(nb + 1) * 4).astype(np.uint32)
        sig, signer = _signed(bv, r4, bh, off, np.arange(nb * 4) % 4)
        sig[rng.integers(0, 4 * nb, 3000), 64] = 3     # some blocks fall below quorum (3 of 4)
        out.append(Batch("16384x4", r4, bh, off, sig, signer))

        bh = _hashes(1, b"one")
        off = np.array([0, 65536], np.uint32)
        sig, signer = _signed(bv, r1024, bh, off, np.arange(65536) % 1024)
        sig[::97, 0] ^= 0x55
        out.append(Batch("1x65536", r1024, bh, off, sig, signer))

        bh = _hashes(2, b"four")
        off = np.array([0, 3, 4], np.uint32)
        sig, signer = _signed(bv, r1024, bh, off, np.array([0, 1, 2, 3]))
        sig[1, 40] ^= 1
        out.append(Batch("4_rows_after_max_rows", r1024, bh, off, sig, signer))

        nb = 655
        bh = _hashes(nb, b"h100")
        off = (np.arange(nb + 1) * 100).astype(np.uint32)
        sig, signer = _signed(bv, r100, bh, off, np.arange(nb * 100) % 100)
        sig[np.unique(rng.integers(0, 100 * nb, 30000)), 3] ^= 0x10   # ≈ 37 bad rows per block (63 ± 5 valid) around the quorum of 67
        out.append(Batch("655x100", r100, bh, off, sig, signer, np.zeros(nb * 100, np.uint8)))

        out.append(Batch("no_blocks", r100, np.zeros((0, 32), np.uint8), np.zeros(1, np.uint32), np.zeros((0, 65), np.uint8),
                         np.zeros((0, 20), np.uint8)))

        r, _, bh, off, sig, signer, pre = BS._sync_fixture(100, 16, SEED + 1, weighted=True)
        out.append(Batch("16x100_weighted", r, bh, off, sig, signer, pre))
    finally:
        bv.close()
    _STREAM = out
    return out


def pinned(b: Batch) -> Batch:
    """the same batch with every column in ibft_pinned_alloc memory"""
    import go_ibft_amd.verifier as V
    p = lambda a: a if a is None or not a.size else V.pinned_copy(a)
    return Batch(b.name + "/pinned", b.r, p(b.bh), p(b.off), p(b.sig), p(b.signer), p(b.pre), b._exp)


def run_stream(bv, seq: list[Batch], in_flight: int = 1, on_collect=None) -> list:
    """submit every batch of seq with `in_flight` batches kept in flight (1: submit(k + 1), collect(k)); the validator set
    is changed in front of the submit that needs another one → [(verdicts, tallies)] per batch"""
    cur, got, pend = None, [], 0
    for b in seq:
        if cur is not b.r:
            bv.set_validators(b.r.height, b.r.addrs, b.r.power)
            cur = b.r
        assert bv.block_seals_submit(*b.cols()) == b.n
        pend += 1
        while pend > in_flight:
            k = len(got)
            assert bv.block_seals_pending() == (pend, seq[k].n, len(seq[k].bh))
            got.append(bv.block_seals_collect())
            pend -= 1
            if on_collect:
                on_collect(k)
    while pend:
        k = len(got)
        assert bv.block_seals_pending() == (pend, seq[k].n, len(seq[k].bh))
        got.append(bv.block_seals_collect())
        pend -= 1
        if on_collect:
            on_collect(k)
    assert bv.block_seals_pending() == (0, 0, 0)
    return got


def sync_results(seq: list[Batch], flags: int = 0) -> list:
    """the synchronous ibft_verify_block_seals over the same batches on a context of its own"""
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=flags, max_rows=65536)
    try:
        cur, out = None, []
        for b in seq:
            if cur is not b.r:
                bv.set_validators(b.r.height, b.r.addrs, b.r.power)
                cur = b.r
            out.append(bv.verify_block_seals(*b.cols()))
        return out
    finally:
        bv.close()


def compare(b: Batch, got, sync=None):
    m, tl = got
    exp, te = expected(b)
    assert m.dtype == bool and len(m) == b.n and len(tl) == len(b.bh), b.name
    assert (m == exp).all(), f"{b.name}: verdicts differ from the oracle at rows {np.nonzero(m != exp)[0][:10]}"
    for k, t in enumerate(tl):
        assert fields(t) == te[k], f"{b.name}: block {k}: {fields(t)} != {te[k]}"
        assert t.shard_overlap == 0 and t.proposer_rows == 0
    if sync is not None:
        ms, ts = sync
        assert (m == ms).all() and [fields(t) for t in tl] == [fields(t) for t in ts], f"{b.name}: differs from the synchronous call"


def main() -> int:
    """the whole stream, one batch kept in flight, against the oracle and the synchronous call (child process of the
    IBFT_NO_HOST_DIRECT test: the environment decides how results are delivered)"""
    import go_ibft_amd.verifier as V
    seq = stream()
    sync = sync_results(seq)
    bv = V.BatchVerifier(max_rows=65536)
    try:
        got = run_stream(bv, seq, 1)
    finally:
        bv.close()
    for b, g, s in zip(seq, got, sync):
        compare(b, g, s)
    print("BLOCK_STREAM_OK", len(seq))
    return 0


if __name__ == "__main__":
    sys.exit(main())
