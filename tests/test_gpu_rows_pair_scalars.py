"""GPU: the scalar stage the two row-per-signature cold kernels share (csrc/wave_fe_dev.h: row_scalars — one multiplication
modulo n for both halves of a row, the GLV split in halves, the split handed over before u1 is finished), through the
kernels that run it: ecrecover_rows_pair_kernel (IBFT_ROWS_PAIR=1, the helper wavefront) and ecrecover_rows_kernel
(IBFT_ROWS_PAIR=0), pinned with IBFT_COLD_LANES=16 at the small sizes — both pins select their kernel at every size, n = 1
included — and under AUTO at n = 2 049.  Sizes: one live row; one full wavefront; a second workgroup with a single live row
(a pair workgroup holds sixteen rows); 2 049.  Rows: a Byzantine round with the crafted rows of
tests/test_dev_row_scalars_host.py spliced in as (hash, seal) pairs next to the crafted rows of tests/test_gpu_rows_pair.py
(zero digest, s = ±k·z, edge u2); the last row of a batch stays the round's own.  Every size goes through the verdict mode,
the senders mode (the helper hashes the payload) and the emit mode; expected values are the oracle's."""
import numpy as np
import pytest

import row_scalar_cases as RC

pytestmark = pytest.mark.gpu


def _b(x):
    return x.to_bytes(32, "big")


def _crafted(rng):
    """(hash32, seal65): rare routes of the closing addition first (their R is a point of the curve), then the edges of
    the scalar stage, which the stage computes whatever becomes of the row"""
    from oracle import pyref
    n = pyref.N
    out = []
    for t in (1, 2**128 - 1):                       # u1 = 0 (zero digest), tiny / edge u2
        k = int.from_bytes(rng.bytes(32), "big") % (n - 1) + 1
        x, y = pyref.pt_mul(k, pyref.G)
        r = x % n
        out.append((bytes(32), _b(r) + _b((t * r) % n) + bytes([y & 1])))
    for sign in (1, -1):                            # s = ±k·z
        k = int.from_bytes(rng.bytes(32), "big") % (n - 1) + 1
        x, y = pyref.pt_mul(k, pyref.G)
        r, s = x % n, int.from_bytes(rng.bytes(32), "big") % (n - 1) + 1
        out.append((_b((sign * s * k) % n), _b(r) + _b(s) + bytes([y & 1])))
    for i, (_, z, r, s) in enumerate(RC.edge_triples()):
        out.append((_b(z), _b(r) + _b(s) + bytes([i & 1])))
    return out


_ROUNDS = {}


def _round(oracle, n):
    """the round of size n (made once, never changed afterwards): seals and envelope signatures with crafted rows spliced
    in; a crafted seal whose key recovers becomes that validator's"""
    from oracle import workload as W
    if n in _ROUNDS:
        return _ROUNDS[n]
    r = W.make_round(n, 7600 + n, byzantine=True, with_envelopes=True)
    rng = np.random.default_rng(7600 + n)
    crafted = _crafted(rng)
    rows = rng.permutation(n - 1)[:len(crafted)]     # (n = 1: none — its one row is an honest seal)
    for j, (h, sg) in zip(rows, crafted):
        r.hash32[j] = np.frombuffer(h, np.uint8)
        r.seal65[j] = np.frombuffer(sg, np.uint8)
        r.msg_sig65[j, :64] = np.frombuffer(sg[:64], np.uint8)    # senders mode: the digest is the payload's, (r, s) crafted
        r.pre_flags[j] = 0
        a = oracle.recover_address(h, sg)
        if a is not None:
            r.addrs[j] = np.frombuffer(a, np.uint8)
            r.signer20[j] = np.frombuffer(a, np.uint8)
    _ROUNDS[n] = r
    return r


def _expect_emit(oracle, vs, r):
    n = len(r.seal65)
    a = np.zeros((n, 20), np.uint8)
    for i in range(n):
        if not r.pre_flags[i]:
            got = oracle.recover_address(r.hash32[i].tobytes(), r.seal65[i].tobytes(), 0)
            if got is not None:
                a[i] = np.frombuffer(got, np.uint8)
    place = {}
    for x in r.addrs:
        place.setdefault(x.tobytes(), len(place))
    vidx = np.full(n, -1, np.int32)
    for i in range(n):
        if a[i].any() and vs.index(a[i].tobytes()) >= 0:
            vidx[i] = place[a[i].tobytes()]
    bit = vidx >= 0
    return a, vidx, bit, oracle.tally(vs, a, bit.astype(np.uint8))


def _fields(t):
    return (t.power, t.quorum, t.has_quorum, t.valid_rows, t.distinct_senders)


@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("n", [1, 4, 17, 2049])
def test_scalar_stage_in_both_row_forms(monkeypatch, oracle, n, pair):
    import go_ibft_amd.verifier as V
    r = _round(oracle, n)
    if n < 2049:
        monkeypatch.setenv("IBFT_COLD_LANES", "16")      # (read when the context is created)
        monkeypatch.setenv("IBFT_ROWS_PAIR", str(pair))
    elif not pair:
        monkeypatch.setenv("IBFT_ROWS_PAIR", "0")        # n = 2 049: AUTO picks the row kernels, and the pair form unless told
    vs = oracle.ValSet(r.addrs, r.power)
    bv = V.BatchVerifier(max_rows=4096)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        # verdict mode
        got, t = bv.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
        assert bv.last_dispatch() == (16, 0)
        exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=8).astype(bool)
        assert (got == exp).all(), np.nonzero(got != exp)[0][:10]
        assert _fields(t) == _fields(oracle.tally(vs, r.signer20, exp))
        # senders mode: the helper wavefront hashes the payload
        got, _ = bv.is_valid_validator(r.payload, r.off, r.msg_sig65, r.signer20, r.pre_flags)
        assert bv.last_dispatch() == (16, 0)
        exp = oracle.verify_senders(vs, r.payload, r.off, r.msg_sig65, r.signer20, r.pre_flags, nthreads=8).astype(bool)
        assert (got == exp).all(), np.nonzero(got != exp)[0][:10]
        # emit mode
        ga, gv, gm, gt = bv.recover_seals(r.hash32, r.seal65, r.pre_flags)
        assert bv.last_dispatch() == (16, 0)
        ea, ev, em, et = _expect_emit(oracle, vs, r)
        assert (ga[:n] == ea).all(), np.nonzero((ga[:n] != ea).any(axis=1))[0][:10]
        assert (gv[:n] == ev).all() and (gm == em).all()
        assert _fields(gt) == _fields(et)
    finally:
        bv.close()
