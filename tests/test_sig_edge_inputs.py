"""The signature edge grid (tests/sig_edge_cases.py) holds both sides of every edge, by the oracle's answers cross-checked
with the Python reference (oracle/pyref.py) — so the device tests that run the grid cannot quietly lose an edge."""
import sig_edge_cases as SE
from oracle import pyref

N, P, HALF = SE.N, SE.P, SE.HALF


def _accepted(flags, **fixed):
    return sum(1 for row, a in zip(SE.grid(), SE.expected(flags)) if a is not None
               and all(getattr(row, k) == v for k, v in fixed.items()))


def test_grid_shape_and_counts(oracle):
    g = SE.grid()
    assert len(g) == 12 * 12 * 6 * 3 == 2592 and len(set(g)) == 2592
    assert all(g[SE.index_of(row.r, row.s, row.z, row.v)] is row for row in g[::97])
    assert _accepted(0) == 480 and _accepted(1) == 240 and _accepted(0) + _accepted(1) == 720
    assert len(SE.signers()) == 160
    assert len({SE.flipped(a) for a in SE.signers()} | set(SE.signers())) == 320
    for row, a0, a1 in zip(g, SE.expected(0), SE.expected(1)):          # the strict rule only ever refuses
        assert a1 is None or a1 == a0


def test_oracle_agrees_with_the_python_reference(oracle):
    for flags in SE.FLAGS:
        for row, a, pub in zip(SE.grid(), SE.expected(flags), SE.expected_pub(flags)):
            assert pyref.recover_address(row.hash, row.sig, strict_low_s=bool(flags)) == a, (hex(row.r), hex(row.s), hex(row.z), row.v)
            assert (pub is None) == (a is None) and (a is None or oracle.address(pub) == a)


def test_both_sides_of_every_edge(oracle):
    # r: 0 | 1 and n − 2 | n − 1; n − 1 is in range but the x of no point, n − 2 is on the curve; r ≥ n refused whatever it is
    on_curve = lambda x: pow((pow(x, 3, P) + 7) % P, (P - 1) // 2, P) == 1
    assert on_curve(N - 2) and not on_curve(N - 1) and on_curve(1) and on_curve(N - 3)
    for flags, per_r in ((0, 96), (1, 48)):
        assert [_accepted(flags, r=r) for r in SE.R_VALUES] == [0, per_r, per_r, per_r, per_r, per_r, 0, 0, 0, 0, 0, 0]
    # s: 0 | 1 and n − 1 | n; the strict rule keeps (n−1)/2 and refuses (n+1)/2
    assert SE.S_VALUES[4] == HALF == (N - 1) // 2 and SE.S_VALUES[5] == (N + 1) // 2 and 2 * HALF + 1 == N
    assert [_accepted(0, s=s) for s in SE.S_VALUES] == [0, 60, 60, 60, 60, 60, 60, 60, 60, 0, 0, 0]
    assert [_accepted(1, s=s) for s in SE.S_VALUES] == [0, 60, 60, 60, 60, 0, 0, 0, 0, 0, 0, 0]
    # v: 0 and 1 accepted alike, 2 never
    assert [_accepted(0, v=v) for v in SE.V_VALUES] == [240, 240, 0]
    # z: every digest has accepted rows under both policies
    for flags, per_z in ((0, 80), (1, 40)):
        assert [_accepted(flags, z=z) for z in SE.Z_VALUES] == [per_z] * 6


def test_digests_at_n_and_beyond_reduce(oracle):
    """z = n and z = n + 1 name the signers of z = 0 and z = 1 in all 864 combinations; z = n − 1 and z = 2^256 − 1 do not"""
    e = {f: SE.expected(f) for f in SE.FLAGS}
    same = differ = 0
    for r in SE.R_VALUES:
        for s in SE.S_VALUES:
            for v in SE.V_VALUES:
                for f in SE.FLAGS:
                    for hi, lo in ((N, 0), (N + 1, 1)):
                        a, b = e[f][SE.index_of(r, s, hi, v)], e[f][SE.index_of(r, s, lo, v)]
                        assert a == b
                        same += f == 0
                    a, b, c = (e[f][SE.index_of(r, s, z, v)] for z in (N - 1, 0, SE.TOP))
                    if a is not None:
                        assert a != b and c not in (a, b) and b is not None and c is not None
                        differ += 1
    assert same == 864 and differ == 120


def test_wave_subset_holds_both_sides_of_every_edge(oracle):
    idx = SE.wave_subset()
    assert len(idx) <= 48 and len(set(idx)) == len(idx)
    rows = [SE.grid()[i] for i in idx]
    acc = {f: [SE.expected(f)[i] is not None for i in idx] for f in SE.FLAGS}
    side = lambda f, **fixed: {a for row, a in zip(rows, acc[f]) if all(getattr(row, k) == v for k, v in fixed.items())}
    assert side(0, r=0) == {False} and True in side(0, r=1) and True in side(0, r=N - 2) and side(0, r=N - 1) == {False}
    assert side(0, r=N) == {False} and side(0, r=P) == {False}
    assert side(0, s=0) == {False} and True in side(0, s=1) and True in side(0, s=N - 1) and side(0, s=N) == {False}
    assert True in side(1, s=HALF) and side(1, s=HALF + 1) == {False} and True in side(0, s=HALF + 1)
    for z in SE.Z_VALUES:
        assert True in side(0, z=z) and True in side(1, z=z)
    assert side(0, v=2) == {False} and True in side(0, v=0) and True in side(0, v=1)
    # s = 0 and s = n with everything else in order and z ≢ 0 (mod n): refused by the comparison with n ALONE (with z ≡ 0 such a
    # row recovers the point at infinity and is refused whatever the range check says)
    for s in (0, N):
        assert any(row.s == s and row.r == N - 2 and row.v <= 1 and row.z % N != 0 for row in rows)
