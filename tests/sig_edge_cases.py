"""Signatures on the exact edges of the range checks (sig_in_range, verify_dev.h, and its second copy in recover_pubkey_with,
recover_dev.h): the full product of

  r ∈ {0, 1, 2, 3, n−3, n−2, n−1, n, n+1, p−1, p, 2^256−1}
  s ∈ {0, 1, 2, (n−1)/2 − 1, (n−1)/2, (n+1)/2, (n+1)/2 + 1, n−2, n−1, n, n+1, 2^256−1}
  z ∈ {0, 1, n−1, n, n+1, 2^256−1}
  v ∈ {0, 1, 2}

— 2 592 rows, each judged without and with IBFT_FLAG_STRICT_LOW_S.  Whoever sends a message chooses r, s and the digest; every
other corpus draws them at random, where an off-by-one in a comparison with n or with (n−1)/2 changes one verdict in 2^128 or
more.  The largest acceptable r is n − 2 (n − 1 is the x of no curve point), the largest acceptable s is n − 1, the strict rule
keeps s = (n−1)/2 and refuses (n+1)/2, and z = n, n + 1 must recover what z = 0, 1 recover.

Plain data and the oracle's answers (oracle.binding.recover_address / ecrecover); no call under test.
tests/test_sig_edge_inputs.py asserts that the grid holds both sides of every edge."""
import functools
from collections import namedtuple

from oracle import pyref

N, P = pyref.N, pyref.P
TOP = 2**256 - 1
HALF = (N - 1) // 2                     # the largest s the strict rule keeps

R_VALUES = (0, 1, 2, 3, N - 3, N - 2, N - 1, N, N + 1, P - 1, P, TOP)
S_VALUES = (0, 1, 2, HALF - 1, HALF, HALF + 1, HALF + 2, N - 2, N - 1, N, N + 1, TOP)
Z_VALUES = (0, 1, N - 1, N, N + 1, TOP)
V_VALUES = (0, 1, 2)
FLAGS = (0, 1)                          # 1: strict low s

Row = namedtuple("Row", "r s z v hash sig")


def make_row(r: int, s: int, z: int, v: int) -> Row:
    return Row(r, s, z, v, z.to_bytes(32, "big"), r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([v]))


@functools.lru_cache(None)
def grid():
    return tuple(make_row(r, s, z, v) for r in R_VALUES for s in S_VALUES for z in Z_VALUES for v in V_VALUES)


@functools.lru_cache(None)
def expected(flags: int):
    """the oracle's signer address of every row of the grid (None: refused)"""
    from oracle import binding as B
    return tuple(B.recover_address(row.hash, row.sig, flags) for row in grid())


@functools.lru_cache(None)
def expected_pub(flags: int):
    from oracle import binding as B
    return tuple(B.ecrecover(row.hash, row.sig, flags) for row in grid())


@functools.lru_cache(None)
def signers():
    """the distinct signers the oracle recovers anywhere in the grid, in order of first appearance"""
    seen, out = set(), []
    for a in expected(0) + expected(1):
        if a is not None and a not in seen:
            seen.add(a)
            out.append(a)
    return tuple(out)


def flipped(addr20: bytes) -> bytes:
    """the same address with one bit flipped: the neighbour every signer gets in the validator set"""
    return bytes([addr20[0] ^ 0x01]) + addr20[1:]


def index_of(r: int, s: int, z: int, v: int) -> int:
    return ((R_VALUES.index(r) * len(S_VALUES) + S_VALUES.index(s)) * len(Z_VALUES) + Z_VALUES.index(z)) * len(V_VALUES) + \
        V_VALUES.index(v)


@functools.lru_cache(None)
def wave_subset():
    """at most 48 rows for the emulated wavefront forms (a fraction of a second each): around an accepted row on the edges
    (r = n − 2, s = (n−1)/2, z = n) every value of r, of s, of z and of v in turn; then around the other accepted corner
    (r = n − 2, s = n − 1, z = n + 1, v = 1) every s once more and the r next to the edges — both sides of every edge of r,
    s, the strict rule and z.  The second round of s matters: with z ≡ 0 (mod n) a row with s ≡ 0 recovers the point at
    infinity and is refused whatever the range check says; with z ≡ 1 it would name a signer"""
    base = (N - 2, HALF, N, 0)
    idx = []
    for r in R_VALUES:
        idx.append(index_of(r, *base[1:]))
    for s in S_VALUES:
        idx.append(index_of(base[0], s, base[2], base[3]))
    for z in Z_VALUES:
        idx.append(index_of(base[0], base[1], z, base[3]))
    for v in V_VALUES:
        idx.append(index_of(*base[:3], v))
    for s in S_VALUES:
        idx.append(index_of(N - 2, s, N + 1, 1))
    for r in (1, N - 1, N):
        idx.append(index_of(r, N - 1, N + 1, 1))
    out = tuple(dict.fromkeys(idx))
    assert len(out) <= 48
    return out
