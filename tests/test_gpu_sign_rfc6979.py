"""GPU: the device signer under the RFC 6979 nonce rule (ibft_sign_seals_ex / sign_lane_kernel<1>; sha256_dev.h and
rfc6979_drbg on gfx950).  References: the five published secp256k1 vectors (tests/golden/kats.json) — third-party bytes, no
oracle in between —, oracle/secp256k1.c:orc_sign_rfc6979, Python's own hmac / hashlib for the DRBG's candidates, and the verify
side of the library itself.  The Keccak rule must come out of the same context unchanged."""
import ctypes as C

import numpy as np
import pytest

import rfc6979_cases as RC

pytestmark = pytest.mark.gpu

N = RC.N


@pytest.fixture(scope="module")
def bv():
    import go_ibft_amd.verifier as V
    b = V.BatchVerifier(max_rows=1024)
    yield b
    b.close()


@pytest.fixture(scope="module")
def rows333():
    """the 50 edge rows and 283 random ones, with the oracle's RFC 6979 signature of each: computed once, never changed"""
    from oracle import binding as O
    sk, dg = RC.rows(333)
    want = [O.sign_rfc6979(sk[i].tobytes(), dg[i].tobytes()) for i in range(333)]
    sk.setflags(write=False)
    dg.setflags(write=False)
    return sk, dg, want


def test_published_vectors_from_a_partial_wavefront(bv):
    """n = 5: one partial wavefront whose 59 idle lanes sign the last row again"""
    vs = RC.vectors()
    sk = np.frombuffer(b"".join(v["private_key"] for v in vs), np.uint8).reshape(5, 32)
    dg = np.frombuffer(b"".join(v["digest"] for v in vs), np.uint8).reshape(5, 32)
    sig, signer, ok = bv.sign_seals(sk, dg, nonce="rfc6979")
    assert ok.all()
    for i, v in enumerate(vs):
        assert sig[i].tobytes() == v["sig65"], i
        assert signer[i].tobytes() == v["address"], i


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_lane_one_workgroup_and_one_lane_more(bv, rows333, n):
    sk, dg, want = rows333
    sig, signer, ok = bv.sign_seals(sk[:n], dg[:n], nonce="rfc6979")
    assert ok.all() and sig.shape == (n, 65)
    for i in range(n):
        assert sig[i].tobytes() == want[i], i


def test_edge_rows_match_the_oracle_and_the_keccak_rule_is_unchanged(bv, rows333):
    from oracle import binding as O
    sk, dg, want = rows333
    n = 333
    sig, signer, ok = bv.sign_seals(sk, dg, nonce="rfc6979")
    assert ok.all()
    for i in range(n):
        assert sig[i].tobytes() == want[i], i
        assert signer[i].tobytes() == O.address(O.pubkey(sk[i].tobytes())), i
    s_int = [int.from_bytes(sig[i, 32:64].tobytes(), "big") for i in range(n)]
    assert max(s_int) <= (N - 1) // 2 and set(sig[:, 64].tolist()) == {0, 1}
    # the same context, no nonce named: the library's own rule, byte for byte the oracle's orc_sign
    sig_k, signer_k, ok_k = bv.sign_seals(sk, dg)
    assert ok_k.all() and (signer_k == signer).all()
    for i in range(n):
        assert sig_k[i].tobytes() == O.sign(sk[i].tobytes(), dg[i].tobytes()), i
        assert sig_k[i, :32].tobytes() != sig[i, :32].tobytes(), i          # another nonce, another r …
        d = dg[i].tobytes()
        assert O.recover_address(d, sig_k[i].tobytes()) == O.recover_address(d, sig[i].tobytes()) == signer[i].tobytes(), i   # … the same key


def test_seal_digest_convention_applies_before_the_nonce():
    """h1 is the digest AFTER the convention: row i = orc_sign_rfc6979(sk_i, keccak256(hash_i ‖ 0x02)), and the staged batch verifies"""
    import go_ibft_amd.verifier as V
    from oracle import binding as O
    n = 70
    sk, hs = RC.rows(n, seed=70)
    b = V.BatchVerifier(max_rows=256)
    try:
        b.set_seal_digest(b"\x02")
        sig, signer, ok = b.sign_seals(sk, hs, nonce="rfc6979")
        assert ok.all()
        for i in range(n):
            assert sig[i].tobytes() == O.sign_rfc6979(sk[i].tobytes(), O.keccak256(hs[i].tobytes() + b"\x02")), i
        uniq = np.unique(signer, axis=0)
        b.set_validators(1, uniq, np.ones(len(uniq), np.uint64))
        verdict, t = b.seals_run()
        assert verdict.all() and t.valid_rows == n
    finally:
        b.close()


def test_refusals():
    import go_ibft_amd.verifier as V
    n = 70
    sk, hs = RC.rows(n, seed=5)
    bad = dict(zip((4, 17, 40, 69), RC.BAD_KEYS))
    for i, k in bad.items():
        sk[i] = np.frombuffer(RC.b32(k), np.uint8)
    b = V.BatchVerifier(max_rows=256)
    try:
        sig, signer, ok = b.sign_seals(sk, hs, nonce="rfc6979")
        for i in range(n):
            assert ok[i] == (i not in bad), i
            assert (i in bad) == (not sig[i].any()) == (not signer[i].any()), i
        # an unknown rule through the raw call: refused, nothing written, the staged batch as it was
        L = b._L
        rows_before, pre_before = C.c_uint32(), C.c_uint32()
        b._chk(L.ibft_seals_rows(b._h, C.byref(rows_before), C.byref(pre_before)), "ibft_seals_rows")
        assert rows_before.value == n
        o_sig, o_signer, o_ok = np.full((n, 65), 0xA5, np.uint8), np.full((n, 20), 0xA5, np.uint8), np.full(n, 0xA5, np.uint8)
        for unknown in (2, 0xFFFFFFFF):
            rc = L.ibft_sign_seals_ex(b._h, V._p(sk), V._p(hs), n, unknown, V._p(o_sig), V._p(o_signer), V._p(o_ok))
            assert rc == -1   # IBFT_E_INVAL
            assert str(unknown).encode() in L.ibft_last_error(b._h)
        assert (o_sig == 0xA5).all() and (o_signer == 0xA5).all() and (o_ok == 0xA5).all()
        rows_after, pre_after = C.c_uint32(), C.c_uint32()
        b._chk(L.ibft_seals_rows(b._h, C.byref(rows_after), C.byref(pre_after)), "ibft_seals_rows")
        assert (rows_after.value, pre_after.value) == (rows_before.value, pre_before.value)
        good = np.array([i not in bad for i in range(n)])
        uniq = np.unique(signer[good], axis=0)
        b.set_validators(1, uniq, np.ones(len(uniq), np.uint64))
        verdict, t = b.seals_run()                         # … and it still is the batch signed above
        assert (verdict == good).all() and t.valid_rows == n - len(bad)
        sig0, signer0, ok0 = b.sign_seals(np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8), nonce="rfc6979")
        assert sig0.shape == (0, 65) and signer0.shape == (0, 20) and ok0.shape == (0,)
    finally:
        b.close()


def test_sign_then_verify_resident_round_trip():
    """test_gpu_sign.py's round trip under the new rule at n = 1 000: sign → (staged) → verify cold and warm; one flipped bit in
    37 rows breaks exactly those rows"""
    import go_ibft_amd.verifier as V
    n = 1000
    rng = np.random.default_rng(n)
    sk = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(-1, 32).copy()
    sk[:, 0] &= 0x7F                       # < 2^255 < n: every key usable
    sk[:, 31] |= 1
    hs = np.tile(np.frombuffer(rng.bytes(32), np.uint8), (n, 1))
    for flags in (0, V.FLAG_PUBKEY_CACHE):
        b = V.BatchVerifier(max_rows=1024, flags=flags)
        try:
            sig, signer, ok = b.sign_seals(sk, hs, nonce="rfc6979")
            assert ok.all() and len({s.tobytes() for s in signer}) == n
            b.set_validators(7, signer, np.ones(n, np.uint64))
            for _ in range(3):             # with the cache: the cold pass learns the keys, later passes run the warm kernels
                verdict, t = b.seals_run()
                assert verdict.all() and t.valid_rows == n and t.distinct_senders == n and t.has_quorum
            sig2 = sig.copy()
            rows = rng.choice(n, size=37, replace=False)
            for j, i in enumerate(rows):
                sig2[i, j % 65] ^= 1 << (j % 8) if j % 65 != 64 else 1
            verdict, t = b.is_valid_committed_seal(hs, sig2, signer)
            want = np.ones(n, bool)
            want[rows] = False
            assert (verdict == want).all() and t.valid_rows == n - 37
        finally:
            b.close()


def test_drbg_candidates_and_reseed_on_the_device():
    """devtest_rfc6979: one lane per row returns the first three candidates, so the reseed step runs as gfx950 code"""
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_devtest())
    L.devtest_rfc6979.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.devtest_rfc6979.restype = C.c_int
    n, m = 70, 3
    sk, dg = RC.rows(n)
    out = np.zeros((n, m, 32), np.uint8)
    assert L.devtest_rfc6979(n, m, sk.ctypes.data, dg.ctypes.data, out.ctypes.data) == 0
    for i in range(n):
        assert out[i].tobytes() == b"".join(RC.candidates(sk[i].tobytes(), dg[i].tobytes(), m)), i
