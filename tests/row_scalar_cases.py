"""Inputs for the scalar stage of the row kernels (csrc/wave_fe_dev.h: row_scalars), shared by
tests/test_dev_row_scalars_host.py (triples (z, r, s) for the host harness) and tests/test_gpu_rows_pair_scalars.py
((hash, seal) rows for the kernels), with the stage's arithmetic in Python integers."""
import random

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
C = (1 << 256) - N          # 2^256 mod n, 129 bits
# the lattice basis of the endomorphism and the two rounding constants (secp256k1_dev.h: sc_split_lambda)
A1 = 0x3086D221A7D46BCDE86C90E49284EB15
B1M = 0xE4437ED6010E88286F547FA90ABFE4C3     # −b1
A2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8
G1 = (A1 * (1 << 384) + N // 2) // N           # round(2^384·b2/n), b2 = a1
G2 = (B1M * (1 << 384) + N // 2) // N          # round(2^384·(−b1)/n)


def scalars(z, r, s):
    """(u1, u2) = (−z/r, s/r) mod n"""
    ri = pow(r, -1, N)
    return (-z * ri) % N, (s * ri) % N


def split(k):
    """the device's split in exact integers: (k1, k2) signed, k1 + k2·λ ≡ k (mod n)"""
    c1 = (k * G1 + (1 << 383)) >> 384
    c2 = (k * G2 + (1 << 383)) >> 384
    return k - c1 * A1 - c2 * A2, c1 * B1M - c2 * A1


def wraps(f, r):
    """does f·r⁻¹ take sc_canon's rare branch?  For a product below 2^260 the four fold rounds of sc_reduce_columns have
    nothing to fold, so the weak scalar IS the product x·2^256 + low, and the branch is the carry out of low + x·c."""
    p = f * pow(r, -1, N)
    assert p < 1 << 260
    return (p & ((1 << 256) - 1)) + (p >> 256) * C >= 1 << 256


def wrap_factors():
    """(f, r): f·r⁻¹ just below (x + 1)·2^256 with r⁻¹ < n — sc_canon's carry out of 2^256"""
    out = []
    for f, x in ((3, 1), (5, 3), (7, 2), (15, 13)):
        rinv = (((x + 1) << 256) - 1) // f
        assert rinv < N
        r = pow(rinv, -1, N)
        assert wraps(f, r)
        out.append((f, r))
    return out


def edge_triples(seed=1404):
    """(name, z, r, s): the edges of the stage; r, s in [1, n), z any 256-bit value"""
    rng = random.Random(seed)
    rnd = lambda: rng.randrange(1, N)
    out = [("z=0", 0, rnd(), rnd()), ("z=n", N, rnd(), rnd()), ("z=2^256-1", (1 << 256) - 1, rnd(), rnd()),
           ("s=1", rng.getrandbits(256), rnd(), 1), ("s=n-1", rng.getrandbits(256), rnd(), N - 1),
           ("r=1", rng.getrandbits(256), 1, rnd()), ("r=n-1", rng.getrandbits(256), N - 1, rnd()),
           ("all-small", 0, 1, 1), ("all-large", (1 << 256) - 1, N - 1, N - 1)]
    for f, r in wrap_factors():
        out.append((f"u2-wraps f={f}", rng.getrandbits(256), r, f))     # the lower half of the row takes the branch
        out.append((f"z/r-wraps f={f}", f, r, rnd()))                    # the upper half
        out.append((f"both-wrap f={f}", f, r, f))
    # every combination of signs of (k1, k2)
    want = {(a, b) for a in (False, True) for b in (False, True)}
    while want:
        z, r, s = rng.getrandbits(256), rnd(), rnd()
        k1, k2 = split(scalars(z, r, s)[1])
        sg = (k1 < 0, k2 < 0)
        if sg in want:
            want.discard(sg)
            out.append((f"signs {'-' if sg[0] else '+'}{'-' if sg[1] else '+'}", z, r, s))
    return out


def random_triples(count, seed):
    rng = random.Random(seed)
    return [(rng.getrandbits(256), rng.randrange(1, N), rng.randrange(1, N)) for _ in range(count)]
