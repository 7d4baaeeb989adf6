"""GPU: the row-per-signature cold kernel with and without its helper wavefronts (ecrecover_rows_pair_kernel against
ecrecover_rows_kernel), each pinned by IBFT_ROWS_PAIR=1 / 0, against the oracle — at the sizes where AUTO picks the pair
form (2 048 < n ≤ 4 096), with ragged last wavefronts and workgroups, and above that range.  Rows: Byzantine, pre-flagged,
crafted rare scalars (u1 = 0, a closing doubling, a key at infinity), rows a warm pass already decided, senders mode."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [2049, 2050, 3000, 4095, 4096, 8192]


def _verifier(monkeypatch, pair, **kw):
    import go_ibft_amd.verifier as V
    monkeypatch.setenv("IBFT_ROWS_PAIR", "1" if pair else "0")   # read when the context is created
    return V.BatchVerifier(**kw)


def _crafted(oracle, rng):
    """(hash32, seal65) pairs whose recover takes the rare routes of the closing addition"""
    from oracle import pyref
    n = pyref.N
    out = []
    for sign in (1, -1):
        for flip in (0, 1):
            k = int.from_bytes(rng.bytes(32), "big") % (n - 1) + 1
            x, y = pyref.pt_mul(k, pyref.G)
            r, s = x % n, int.from_bytes(rng.bytes(32), "big") % (n - 1) + 1
            out.append((((sign * s * k) % n).to_bytes(32, "big"),
                        r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([(y & 1) ^ flip])))
    for t in (1, 2**64, 2**128 - 1, n - 1):      # u1 = 0 (zero digest), tiny / edge u2
        k = int.from_bytes(rng.bytes(32), "big") % (n - 1) + 1
        x, y = pyref.pt_mul(k, pyref.G)
        r = x % n
        out.append((bytes(32), r.to_bytes(32, "big") + ((t * r) % n).to_bytes(32, "big") + bytes([y & 1])))
    return out


def _round(oracle, n, seed):
    """a Byzantine round with crafted rows spliced in; a crafted row whose key recovers becomes that validator's seal"""
    from oracle import workload as W
    r = W.make_round(n, seed, byzantine=True)
    rng = np.random.default_rng(seed)
    rows = rng.choice(n, size=8, replace=False)
    for j, (h, sg) in zip(rows, _crafted(oracle, rng)):
        r.hash32[j] = np.frombuffer(h, np.uint8)
        r.seal65[j] = np.frombuffer(sg, np.uint8)
        r.pre_flags[j] = 0
        a = oracle.recover_address(h, sg)
        if a is not None:
            r.addrs[j] = np.frombuffer(a, np.uint8)
            r.signer20[j] = np.frombuffer(a, np.uint8)
    return r


def _check(bv, oracle, r):
    vs = oracle.ValSet(r.addrs, r.power)
    bv.set_validators(r.height, r.addrs, r.power)
    got, t = bv.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
    exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=8)
    assert (got == exp.astype(bool)).all(), np.nonzero(got != exp.astype(bool))[0][:10]
    te = oracle.tally(vs, r.signer20, exp)
    assert (t.power, t.quorum, t.has_quorum, t.valid_rows, t.distinct_senders) == \
           (te.power, te.quorum, te.has_quorum, te.valid_rows, te.distinct_senders)
    assert bv.last_dispatch() == (16, 0)
    return got


@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("n", SIZES)
def test_rows_forms_match_oracle(monkeypatch, oracle, n, pair):
    r = _round(oracle, n, 7100 + n)
    assert r.pre_flags.any() and any(r.kinds)
    bv = _verifier(monkeypatch, pair, max_rows=max(n, 4096))
    try:
        _check(bv, oracle, r)
    finally:
        bv.close()


@pytest.mark.parametrize("pair", [1, 0])
def test_rows_forms_after_a_warm_pass(monkeypatch, oracle, pair):
    """half the validators' keys known: the warm kernel decides their rows first, the cold kernel the rest"""
    import go_ibft_amd.verifier as V
    n = 3000
    r = _round(oracle, n, 7301)
    vs = oracle.ValSet(r.addrs, r.power)
    exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=8).astype(bool)
    bv = _verifier(monkeypatch, pair, flags=V.FLAG_PUBKEY_CACHE, max_rows=4096)
    try:
        bv.set_validators(1, r.addrs, r.power)
        even = np.arange(0, n, 2)
        got, _ = bv.is_valid_committed_seal(r.hash32[even], r.seal65[even], r.signer20[even], r.pre_flags[even])
        assert (got == exp[even]).all()
        for _ in range(2):     # mixed (warm rows decided first), then with every learned key's table built
            got, t = bv.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
            assert (got == exp).all(), np.nonzero(got != exp)[0][:10]
            assert t.valid_rows == int(exp.sum())
    finally:
        bv.close()


@pytest.mark.parametrize("pair", [1, 0])
def test_rows_forms_senders(monkeypatch, oracle, pair):
    """MODE 1: the digest is Keccak of the payload — only the helper wavefront hashes it"""
    from oracle import workload as W
    n = 3001
    r = W.make_round(n, 7402, byzantine=True, with_envelopes=True)
    vs = oracle.ValSet(r.addrs, r.power)
    bv = _verifier(monkeypatch, pair, max_rows=4096)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        got, _ = bv.is_valid_validator(r.payload, r.off, r.msg_sig65, r.signer20, r.pre_flags)
        exp = oracle.verify_senders(vs, r.payload, r.off, r.msg_sig65, r.signer20, r.pre_flags, nthreads=8)
        assert (got == exp.astype(bool)).all(), np.nonzero(got != exp.astype(bool))[0][:10]
        assert bv.last_dispatch() == (16, 0)
    finally:
        bv.close()
