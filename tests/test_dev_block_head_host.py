"""The per-row body of block_head_kernel (recover_dev.h: block_of_row, block_head_row), compiled for the host
(csrc/host_block_head_harness.hip), against the oracle's Keccak: every row gets the digest of ITS block — found through row
offsets with empty blocks at the front, in the middle and at the end — as it is under the identity convention, and
keccak256(digest ‖ suffix) under a suffix convention (1-byte and 64-byte suffixes; the nine suffix words are derived here the
way ibft_set_seal_digest derives them).  The digests themselves must come back untouched: the kernel only reads them."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as B


@pytest.fixture(scope="module")
def dev():
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_block_head_harness())
    vp = C.c_void_p
    L.bhh_rows.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.bhh_rows.restype = None
    return L


def suffix_words(suffix: bytes) -> np.ndarray:
    """suffix ‖ 0x01 ‖ 0… as nine little-endian words: bytes 32..103 of the one Keccak block"""
    block = bytearray(72)
    block[:len(suffix)] = suffix
    block[len(suffix)] = 0x01
    return np.frombuffer(bytes(block), "<u8").copy()


def p(a):
    return a.ctypes.data_as(C.c_void_p)


# rows per block: empty blocks at the front, in the middle, at the end; one block only; every block empty but one
SHAPES = {
    "plain": [3, 1, 4],
    "first_empty": [0, 5, 2],
    "last_empty": [4, 2, 0],
    "middle_empty": [2, 0, 0, 3, 0, 1],
    "both_ends_empty": [0, 0, 7, 0],
    "one_block": [9],
    "many": [(i * 7) % 5 for i in range(40)],
    "no_rows": [0, 0, 0],
}
SUFFIXES = {"identity": None, "suffix1": b"\x02", "suffix64": bytes(range(100, 164))}


@pytest.mark.parametrize("conv", sorted(SUFFIXES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rows_get_their_blocks_hash(dev, shape, conv):
    rows = SHAPES[shape]
    nb = len(rows)
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
    n = int(off[-1])
    rng = np.random.default_rng(len(shape) * 131 + len(conv))
    digests = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    before = digests.copy()
    suffix = SUFFIXES[conv]
    words = suffix_words(suffix if suffix is not None else b"")
    out = np.full((max(n, 1), 32), 0xEE, np.uint8)
    blk = np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
    dev.bhh_rows(p(digests), p(off), nb, n, 0 if suffix is None else 1, p(words), p(out), p(blk))
    assert (digests == before).all(), "the digests are read only"
    want_block = np.repeat(np.arange(nb, dtype=np.uint32), rows)
    assert (blk[:n] == want_block).all()
    for row in range(n):
        d = before[want_block[row]].tobytes()
        want = d if suffix is None else B.keccak256(d + suffix)
        assert out[row].tobytes() == want, (shape, conv, row)
    if n == 0:
        assert (out == 0xEE).all() and blk[0] == 0xFFFFFFFF
