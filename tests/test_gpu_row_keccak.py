"""GPU: the kernels whose tail is the row-layout address hash (csrc/keccak_row_dev.h) against the CPU oracle bit for bit:
verdict words, tally, distinct senders.  ecrecover_rows_pair_kernel at n = 2 049 (the smallest size it serves; 2 049 mod 4 = 1:
the last wavefront has three idle rows), ecrecover_rows_kernel at n = 2 049 and n = 4 100 (two wavefronts on some SIMDs; the
pair form ends at 4 096), pinned by IBFT_ROWS_PAIR; the one-wavefront forms ecrecover_wave_kernel and ecrecover_wave2_kernel,
pinned by IBFT_COLD_LANES = 64 / 128, at n = 5 (ragged: idle wavefronts in the last workgroup) and n = 64.  Every batch
carries a corrupted seal, a seal signed by a non-member, a wrong claimed signer and pre-flagged rows.  With the key cache on, the first pass learns the keys from the addresses and
points these kernels hand over and the second pass must find every one of them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROW_CASES = [(2049, 1), (2049, 0), (4100, 0)]      # (n, IBFT_ROWS_PAIR)
_rounds = {}
_small = {}


def _round(oracle, n):
    """one Byzantine round and its expected verdicts per size, shared by the tests and left unchanged"""
    if n not in _rounds:
        from oracle import workload as W
        r = W.make_round(n, 8200 + n, byzantine=True)
        assert {"random65", "non_validator", "stolen_seal"} <= set(r.kinds) and r.pre_flags.any()
        vs = oracle.ValSet(r.addrs, r.power)
        exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=8).astype(bool)
        bad = [i for i, k in enumerate(r.kinds) if k in ("random65", "non_validator", "stolen_seal")]
        assert not exp[bad].any() and not exp[r.pre_flags != 0].any() and exp.sum() > n // 2
        _rounds[n] = (r, vs, exp, oracle.tally(vs, r.signer20, exp))
    return _rounds[n]


def _verifier(monkeypatch, pair, **kw):
    import go_ibft_amd.verifier as V
    monkeypatch.setenv("IBFT_ROWS_PAIR", "1" if pair else "0")   # read when the context is created
    return V.BatchVerifier(**kw)


def _same_tally(t, te):
    assert (t.power, t.quorum, t.has_quorum, t.valid_rows, t.distinct_senders) == \
           (te.power, te.quorum, te.has_quorum, te.valid_rows, te.distinct_senders)


def _small_round(oracle, n):
    """n ≤ 64 rows, the bad rows put in by hand (the generator's Byzantine mix needs more rows than five): row 0 a corrupted
    seal, row 1 a seal by a key outside the set (over its own hash), row 2 an honest seal claimed by another member, row 3
    pre-flagged, the rest honest"""
    if n not in _small:
        from oracle import workload as W
        r = W.make_round(n, 8300 + n)
        f = W.make_round(n, 9300 + n)                    # other keys: nobody of this set
        assert not set(map(bytes, f.addrs)) & set(map(bytes, r.addrs))
        h, seal, signer, pre = r.hash32.copy(), r.seal65.copy(), r.signer20.copy(), np.zeros(n, np.uint8)
        seal[0, 7] ^= 0x40
        h[1], seal[1] = f.hash32[1], f.seal65[1]
        signer[2] = r.signer20[4]
        pre[3] = 1
        vs = oracle.ValSet(r.addrs, r.power)
        exp = oracle.verify_seals(vs, h, seal, signer, pre, nthreads=2).astype(bool)
        assert not exp[:4].any() and exp[4:].all()
        _small[n] = (r, h, seal, signer, pre, exp, oracle.tally(vs, signer, exp))
    return _small[n]


@pytest.mark.parametrize("lanes", [64, 128])
@pytest.mark.parametrize("n", [5, 64])
def test_one_wavefront_kernels_match_oracle(monkeypatch, oracle, n, lanes):
    import go_ibft_amd.verifier as V
    r, h, seal, signer, pre, exp, te = _small_round(oracle, n)
    monkeypatch.setenv("IBFT_COLD_LANES", str(lanes))   # read when the context is created
    bv = V.BatchVerifier(max_rows=1024)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        got, t = bv.is_valid_committed_seal(h, seal, signer, pre)
        assert bv.last_dispatch() == (lanes, 0)
        assert (got == exp).all(), np.nonzero(got != exp)[0][:10]
        _same_tally(t, te)
    finally:
        bv.close()


@pytest.mark.parametrize("n,pair", ROW_CASES)
def test_row_kernels_match_oracle(monkeypatch, oracle, n, pair):
    r, vs, exp, te = _round(oracle, n)
    bv = _verifier(monkeypatch, pair, max_rows=8192)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        got, t = bv.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
        assert bv.last_dispatch() == (16, 0)
        assert (got == exp).all(), np.nonzero(got != exp)[0][:10]
        _same_tally(t, te)
    finally:
        bv.close()


@pytest.mark.parametrize("pair", [1, 0])
def test_learned_keys_are_the_real_ones(monkeypatch, oracle, pair):
    """cache on: pass 1, the same validators' honest seals, goes through the row kernel, which hands every recovered key and
    address to the learn path; pass 2, the Byzantine batch, must then be decided by the warm kernel alone (every validator's
    key is known) — and a key or an address that was not the real one would turn its validator's good seal down there"""
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    n = 2049
    r, vs, exp, te = _round(oracle, n)
    h = W.make_round(n, 8200 + n)            # the same seed: the same validators, every seal honest
    assert (h.addrs == r.addrs).all() and not h.pre_flags.any()
    bv = _verifier(monkeypatch, pair, flags=V.FLAG_PUBKEY_CACHE, max_rows=8192)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        got, t = bv.is_valid_committed_seal(h.hash32, h.seal65, h.signer20, h.pre_flags)
        assert bv.last_dispatch() == (16, 0)
        assert got.all() and t.valid_rows == n and t.distinct_senders == n
        got2, t2 = bv.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
        cold, warm = bv.last_dispatch()
        print("pass 2 dispatch (cold, warm):", cold, warm, "cache:", bv.cache_stats())
        assert cold == 0 and warm != 0       # all-warm: no cold kernel ran
        assert bv.cache_stats()[0] == n
        assert (got2 == exp).all(), np.nonzero(got2 != exp)[0][:10]
        _same_tally(t2, te)
    finally:
        bv.close()
