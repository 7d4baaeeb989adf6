"""The scalar stage of the row kernels (csrc/wave_fe_dev.h: row_scalars — r⁻¹ mod n, then ONE multiplication modulo n whose
lower half-row computes u2 = s/r and whose upper half-row computes z/r, then the GLV split with c1's products in one half
and c2's in the other), compiled for the host and run on the 64-coroutine lockstep wavefront emulator (csrc/wave_emul.h):
a whole wavefront with four different rows at once.  Checked against Python integers and against the lane-layout route
the function replaced (sc_mul twice, sc_split_lambda), in every lane that is supposed to hold the values.  The emulator
aborts the process when lanes disagree on a cross-lane primitive, so every call also checks that the control flow around
them is wave-uniform."""
import ctypes as C

import numpy as np
import pytest

import row_scalar_cases as RC
from go_ibft_amd import build as B

N = RC.N


@pytest.fixture(scope="module")
def dev():
    L = C.CDLL(B.build_row_scalars_harness())
    assert L.row_scalars_out_bytes() == 100
    return L


def _pack(t):
    z, r, s = t
    return z.to_bytes(32, "big") + r.to_bytes(32, "big") + s.to_bytes(32, "big")


def _unpack(b):
    b = bytes(b)
    i = lambda o: int.from_bytes(b[o:o + 32], "big")
    return i(0), i(32), i(64), bool(b[96]), bool(b[97])


def run_rows(dev, triples):
    """triples four per wavefront (the last wavefront padded with its last triple) → per triple (u1, |k1|, |k2|, k1 < 0,
    k2 < 0), after checking that all sixteen lanes of its row hold the same values and saw them at the hand-over"""
    n = len(triples)
    waves = (n + 3) // 4
    padded = list(triples) + [triples[-1]] * (waves * 4 - n)
    zrs = np.frombuffer(b"".join(_pack(t) for t in padded), dtype=np.uint8).copy()
    out = np.zeros((waves * 4, 16, 100), dtype=np.uint8)
    dev.row_scalars_waves(zrs.ctypes.data_as(C.c_void_p), waves, out.ctypes.data_as(C.c_void_p))
    assert (out == out[:, :1, :]).all(), "the lanes of a row disagree"
    assert (out[:, :, 98] == 1).all(), "the hand-over did not see the split the function returns"
    return [_unpack(out[i, 0]) for i in range(n)]


def lane_route(dev, t):
    out = np.zeros(100, dtype=np.uint8)
    dev.lane_scalars_one(C.c_char_p(_pack(t)), out.ctypes.data_as(C.c_void_p))
    return _unpack(out)


def check(dev, triples, against_lane_route=True):
    got = run_rows(dev, triples)
    for t, g in zip(triples, got):
        z, r, s = t
        u1, m1, m2, neg1, neg2 = g
        e1, e2 = RC.scalars(z, r, s)
        assert u1 == e1, ("u1", t)
        k1, k2 = (-m1 if neg1 else m1), (-m2 if neg2 else m2)
        assert (k1 + k2 * RC.LAMBDA) % N == e2, ("k1 + k2·λ", t)
        assert m1 < 1 << 128 and m2 < 1 << 128, ("bounds", t)
        assert (k1, k2) == RC.split(e2), ("the split's integers", t)
        if against_lane_route:
            assert g == lane_route(dev, t), ("lane-layout route", t)
    return got


def test_random_triples(dev):
    check(dev, RC.random_triples(2000, 1401))


def test_edges_in_every_row(dev):
    """each edge row in row 0 … 3 with random rows beside it, and once in all four rows"""
    filler = RC.random_triples(3 * 4 * 64, 1402)
    fi = iter(filler)
    for name, z, r, s in RC.edge_triples():
        e = (z, r, s)
        waves = []
        for row in range(4):
            w = [next(fi), next(fi), next(fi)]
            w.insert(row, e)
            waves += w
        waves += [e] * 4
        got = check(dev, waves)
        mine = [got[4 * row + row] for row in range(4)] + got[16:20]
        assert all(m == mine[0] for m in mine), name


def test_edges_are_what_they_claim():
    """the crafted inputs do reach what they were crafted for (in Python integers: the device code is not asked)"""
    names = [e[0] for e in RC.edge_triples()]
    assert sum(n.startswith("signs") for n in names) == 4
    for name, z, r, s in RC.edge_triples():
        if name.startswith("u2-wraps") or name.startswith("both-wrap"):
            assert RC.wraps(s, r)
        if name.startswith("z/r-wraps") or name.startswith("both-wrap"):
            assert RC.wraps(z, r)
    assert RC.scalars(0, 5, 7)[0] == 0 and RC.scalars(N, 5, 7)[0] == 0


def test_rows_are_independent(dev):
    """four different triples in one wavefront, in a few orders: a row's answer depends on nothing but its own triple (the
    half-row exchange and the broadcasts never reach into a neighbouring row)"""
    ts = RC.random_triples(4, 1403)
    want = check(dev, ts)
    assert len(set(want)) == 4
    for perm in ([3, 2, 1, 0], [1, 3, 0, 2], [2, 0, 3, 1], [0, 0, 1, 1], [3, 3, 3, 0]):
        assert run_rows(dev, [ts[i] for i in perm]) == [want[i] for i in perm], perm
