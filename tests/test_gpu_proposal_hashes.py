"""GPU: chain sync from the PROPOSALS — ibft_proposal_hashes (n proposal hashes in one launch, the round spliced in on the device,
two kernel forms) and the two block calls that take proposals in place of hashes (ibft_verify_block_seals_raw,
ibft_recover_block_seals_raw).  Expected values: the CPU oracle (oracle.binding.proposal_hash / verify_seals / tally) and the
existing hashes-given calls — never the calls under test."""
import os
import subprocess
import sys

import numpy as np
import pytest

import proposal_hash_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_NOVALSET, E_TOOBIG = -1, -5, -7


def _V():
    import go_ibft_amd.verifier as V
    return V


def _fields(t):
    return (t.power, t.quorum, t.valid_rows, t.distinct_senders, t.has_quorum, t.shard_overlap, t.proposer_rows)


# ---- (a) the hashes themselves ---------------------------------------------------------------------------------------
def test_hashes_equal_the_oracle_auto_form_pageable_and_pinned():
    V = _V()
    bv = V.BatchVerifier(max_rows=65536)
    try:
        assert PC.check_all(bv, V, "auto") == 2 * (1 + len(PC.SHORT_COUNTS))
        assert len(bv.proposal_hashes([], [])) == 0                      # n = 0 is legal
        rc = bv._L.ibft_proposal_hashes(bv._h, None, None, None, 0, None)
        assert rc == 0
    finally:
        bv.close()


@pytest.mark.parametrize("lanes", ["1", "64"])
def test_hashes_equal_the_oracle_with_the_form_pinned(lanes):
    """IBFT_PROPOSAL_LANES is read at ibft_ctx_create: a fresh child process per form"""
    env = dict(os.environ, IBFT_PROPOSAL_LANES=lanes)
    code = ("import sys; sys.path[:0] = [%r, %r]; import proposal_hash_cases as S; sys.exit(S.main())" % (ROOT, os.path.join(ROOT, "tests")))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0 and "PROPOSAL_HASHES_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_row_equals_ibft_proposal_hash_byte_for_byte():
    """the defining property, against the one-proposal call of the same library (host route) on a sample of the edge lengths"""
    V = _V()
    raws, rounds = PC.mixed_batch()
    pick = [i for i, r in enumerate(raws) if len(r) in (0, 1, 120, 127, 128, 129, 135, 136, 264, 300, 4095, 65536 + 8, PC.MIB)]
    assert len(pick) == 13
    bv = V.BatchVerifier(max_rows=4096)
    try:
        got = bv.proposal_hashes([raws[i] for i in pick], [rounds[i] for i in pick])
        for k, i in enumerate(pick):
            assert got[k].tobytes() == bv.proposal_hash(raws[i], rounds[i]), len(raws[i])
    finally:
        bv.close()


# ---- (b) the _raw block calls = hashes + the existing call -----------------------------------------------------------
def _suffix_digest(suffix):
    from oracle import binding as B
    return None if suffix is None else (lambda h: B.keccak256(h + suffix))


def _fixture(seed: int, suffix: bytes | None = None):
    """blocks with proposals of differing length (0 … 1 200 bytes; starts on every offset mod 4), signed by a 20-validator
    set over what the convention says a seal signs: empty blocks, a seal placed in the wrong block, duplicate signers, a
    non-member's valid seal, corrupted seals, NIL / BADLEN pre-flags, blocks below, at and above quorum (14 of 20)"""
    from oracle import binding as B, workload as W
    V = _V()
    r = W.make_round(20, seed, raw_len=64)
    vs = B.ValSet(r.addrs, r.power)
    rng = np.random.default_rng(seed)
    sizes = [0, 14, 13, 20, 0, 0, 15, 14, 1, 16, 20, 0]
    lens = [0, 1, 127, 128, 129, 135, 136, 700, 1200, 33, 264, 5]
    raws = [rng.bytes(n) for n in lens]
    rounds = [0, 1, 2**64 - 1, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    bh = PC.expected(raws, rounds)
    dg = _suffix_digest(suffix) or (lambda h: h)
    outsider = W.validator_key(seed ^ 0x55, 1 << 41)
    rows, off = [], [0]
    for b, cnt in enumerate(sizes):
        H = dg(bytes(bh[b]))
        who = rng.permutation(20)[:cnt]
        blk = [(B.sign(r.sks[i], H), bytes(r.addrs[i]), 0) for i in who]
        if b == 1:    # the seal of ANOTHER block, placed here
            blk[0] = (B.sign(r.sks[who[0]], dg(bytes(bh[3]))), bytes(r.addrs[who[0]]), 0)
        elif b == 3:  # duplicate signers and a non-member
            blk += [blk[0], blk[1], (B.sign(outsider, H), B.address(B.pubkey(outsider)), 0)]
        elif b == 6:  # pre-flagged rows (their seals are good)
            blk[0] = (blk[0][0], blk[0][1], V.ROW_NIL)
            blk[1] = (blk[1][0], blk[1][1], V.ROW_BADLEN)
        elif b == 7:  # a corrupted seal: the block falls below quorum
            s = bytearray(blk[2][0]); s[5] ^= 0x40
            blk[2] = (bytes(s), blk[2][1], 0)
        elif b == 9:  # v = 2, a stolen seal
            blk[0] = (blk[0][0][:64] + b"\x02", blk[0][1], 0)
            blk[1] = (blk[2][0], blk[1][1], 0)
        rows += blk
        off.append(len(rows))
    sig = np.frombuffer(b"".join(x[0] for x in rows), np.uint8).reshape(-1, 65).copy()
    signer = np.frombuffer(b"".join(x[1] for x in rows), np.uint8).reshape(-1, 20).copy()
    pre = np.array([x[2] for x in rows], np.uint8)
    return r, vs, raws, rounds, bh, np.array(off, np.uint32), sig, signer, pre


def _sync_fixture_with_proposals(seed: int, nb: int = 64):
    """the fixture of tests/test_gpu_block_seals.py (100 validators, every kind of bad row) with the proposals its block
    hashes were made from (test_gpu_block_seals._block_hashes)"""
    import test_gpu_block_seals as BS
    r, vs, bh, off, sig, signer, pre = BS._sync_fixture(100, nb, seed)
    raws = [seed.to_bytes(8, "little") + b.to_bytes(8, "little") * 3 for b in range(nb)]
    rounds = list(range(nb))
    assert (PC.expected(raws, rounds) == bh).all()
    return r, vs, raws, rounds, bh, off, sig, signer, pre


def _check_raw_equals_hashes_given(bv, fx, suffix=None, oracle=True):
    import test_gpu_block_seals as BS
    r, vs, raws, rounds, bh, off, sig, signer, pre = fx
    # the existing calls, with the ORACLE's hashes
    m0, t0 = bv.verify_block_seals(bh, off, sig, signer, pre)
    if oracle:
        exp, te = BS._expect(vs, bh, off, sig, signer, pre, _suffix_digest(suffix))
        assert (m0 == exp).all() and [_fields(t)[:5] for t in t0] == [BS._fields(t) for t in te]
    # ibft_proposal_hashes, then the existing call with ITS hashes: the same
    hs = bv.proposal_hashes(raws, rounds)
    assert (hs == bh).all()
    # the _raw verify call
    for want_hashes in (True, False):
        m, tl, got_bh = bv.verify_block_seals_raw(raws, rounds, off, sig, signer, pre, want_hashes=want_hashes)
        assert (m == m0).all(), np.nonzero(m != m0)[0][:10]
        assert [_fields(t) for t in tl] == [_fields(t) for t in t0]
        assert (got_bh is None) if not want_hashes else (got_bh == bh).all()   # the hashes BEFORE the seal-digest convention
    # … leaves the rows resident, as the hashes-given call does
    assert bv.seals_rows()[0] == int(off[-1])
    m1, _ = bv.seals_run()
    assert (m1 == m0).all()
    # the _raw recover call against the hashes-given one
    s0, v0, rm0, rt0 = bv.recover_block_seals(bh, off, sig, pre)
    for want_hashes in (True, False):
        s1, v1, rm1, rt1, got_bh = bv.recover_block_seals_raw(raws, rounds, off, sig, pre, want_hashes=want_hashes)
        assert (s1 == s0).all() and (v1 == v0).all() and (rm1 == rm0).all()
        assert [_fields(t) for t in rt1] == [_fields(t) for t in rt0]
        assert (got_bh is None) if not want_hashes else (got_bh == bh).all()
    assert bv.seals_rows()[0] == 0                                            # bare rows are no resident batch
    return m0, t0


@pytest.mark.parametrize("suffix", [None, b"\x02", bytes(range(64))])
def test_raw_calls_equal_hashes_plus_existing_call_cold(suffix):
    V = _V()
    fx = _fixture(2101, suffix)
    bv = V.BatchVerifier(max_rows=4096)
    try:
        bv.set_validators(fx[0].height, fx[0].addrs, fx[0].power)
        bv.set_seal_digest(suffix)
        m0, t0 = _check_raw_equals_hashes_given(bv, fx, suffix)
        hq = [t.has_quorum for t in t0]
        assert 0 < sum(hq) < len(hq) and m0.sum() > 0 and (~m0).sum() >= 6   # the fixture has what it claims
        assert bv.cache_stats()[1] == 0                                       # no warm pass: the context has no key cache
    finally:
        bv.close()


@pytest.mark.parametrize("suffix", [None, b"\x02"])
def test_raw_calls_equal_hashes_plus_existing_call_warm(suffix):
    V = _V()
    fx = _fixture(2102, suffix)
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=4096)
    try:
        bv.set_validators(fx[0].height, fx[0].addrs, fx[0].power)
        bv.set_seal_digest(suffix)
        # the FIRST call of the context is the _raw one: cold, and it teaches the device the keys …
        r, vs, raws, rounds, bh, off, sig, signer, pre = fx
        import test_gpu_block_seals as BS
        exp, te = BS._expect(vs, bh, off, sig, signer, pre, _suffix_digest(suffix))
        m, tl, got_bh = bv.verify_block_seals_raw(raws, rounds, off, sig, signer, pre)
        assert (m == exp).all() and [_fields(t)[:5] for t in tl] == [BS._fields(t) for t in te] and (got_bh == bh).all()
        # … so that everything after it runs warm
        w0 = bv.cache_stats()[1]
        _check_raw_equals_hashes_given(bv, fx, suffix)
        assert bv.cache_stats()[0] == 20 and bv.cache_stats()[1] > w0
    finally:
        bv.close()


@pytest.mark.parametrize("flags_name", ["cold", "warm"])
def test_raw_calls_on_the_shapes_of_the_block_seals_suite(flags_name):
    V = _V()
    fx = _sync_fixture_with_proposals(11)
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if flags_name == "warm" else 0, max_rows=65536)
    try:
        bv.set_validators(fx[0].height, fx[0].addrs, fx[0].power)
        if flags_name == "warm":
            bv.verify_block_seals(*fx[4:9])
        _check_raw_equals_hashes_given(bv, fx)
        if flags_name == "warm":
            assert bv.cache_stats()[1] > 0
    finally:
        bv.close()


def test_no_rows_and_no_blocks():
    V = _V()
    fx = _fixture(2103)
    bv = V.BatchVerifier(max_rows=1024)
    try:
        bv.set_validators(fx[0].height, fx[0].addrs, fx[0].power)
        raws, rounds, bh = fx[2][:3], fx[3][:3], fx[4][:3]
        m, tl, got = bv.verify_block_seals_raw(raws, rounds, [0, 0, 0, 0], np.zeros((0, 65), np.uint8), np.zeros((0, 20), np.uint8))
        assert len(m) == 0 and [t.has_quorum for t in tl] == [0, 0, 0] and (got == bh).all()   # hashed although no seal waits
        assert all(t.quorum == fx[1].quorum and t.power == 0 for t in tl)
        s, v, m, tl, got = bv.recover_block_seals_raw(raws, rounds, [0, 0, 0, 0], np.zeros((0, 65), np.uint8), want_hashes=False)
        assert len(m) == 0 and len(s) == 0 and got is None and [t.has_quorum for t in tl] == [0, 0, 0]
        m, tl, got = bv.verify_block_seals_raw([], [], [0], np.zeros((0, 65), np.uint8), np.zeros((0, 20), np.uint8))
        assert len(m) == 0 and tl == [] and len(got) == 0
    finally:
        bv.close()


# ---- (c) a proposal altered in one byte, a round off by one ----------------------------------------------------------
def test_altered_proposal_or_round_flips_exactly_that_block():
    V = _V()
    fx = _fixture(2104)
    r, vs, raws, rounds, bh, off, sig, signer, pre = fx
    bv = V.BatchVerifier(max_rows=4096)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        m0, t0, _ = bv.verify_block_seals_raw(raws, rounds, off, sig, signer, pre)
        for b in (3, 7 - 1, 9, 10):                 # blocks with rows and (3, 6, 10) with a quorum
            assert int(off[b + 1]) > int(off[b]) and m0[off[b]:off[b + 1]].any()
            variants = [(raws[:b] + [raws[b][:-1] + bytes([raws[b][-1] ^ 1])] + raws[b + 1:], rounds),
                        (raws[:b] + [bytes([raws[b][0] ^ 0x80]) + raws[b][1:]] + raws[b + 1:], rounds),
                        (raws, rounds[:b] + [(rounds[b] + 1) % 2**64] + rounds[b + 1:]),
                        (raws, rounds[:b] + [(rounds[b] - 1) % 2**64] + rounds[b + 1:])]
            for rw, rd in variants:
                m, tl, got = bv.verify_block_seals_raw(rw, rd, off, sig, signer, pre)
                lo, hi = int(off[b]), int(off[b + 1])
                assert not m[lo:hi].any() and tl[b].has_quorum == 0 and tl[b].valid_rows == 0
                keep = np.ones(len(m), bool); keep[lo:hi] = False
                assert (m[keep] == m0[keep]).all()
                assert [_fields(t) for k, t in enumerate(tl) if k != b] == [_fields(t) for k, t in enumerate(t0) if k != b]
                assert (got[b] != bh[b]).any() and (np.delete(got, b, 0) == np.delete(bh, b, 0)).all()
                s, v, rm, rt, _ = bv.recover_block_seals_raw(rw, rd, off, sig, pre)
                assert not rm[lo:hi].any() and rt[b].has_quorum == 0     # whoever those seals recover to is no member
        assert any(t0[b].has_quorum for b in (3, 6, 10))
    finally:
        bv.close()


# ---- (d) every error code, out buffers untouched ---------------------------------------------------------------------
def test_error_codes_and_untouched_outputs():
    V = _V()
    fx = _fixture(2105)
    r, vs, raws, rounds, bh, off, sig, signer, pre = fx
    raw, roff, rnd = V.proposal_columns(raws, rounds)
    nb, n = len(rounds), int(off[-1])
    p = V._p
    out = np.full((nb, 32), 0xA5, np.uint8)
    so = np.full((n, 20), 0xA5, np.uint8)
    vi = np.full(n, 77, np.int32)
    mask = np.full((n + 63) // 64, 0x0707, np.uint64)
    tal = (V.Tally * nb)()
    for t in tal:
        t.power_lo = 0x1234

    def untouched():
        return ((out == 0xA5).all() and (so == 0xA5).all() and (vi == 77).all() and (mask == 0x0707).all()
                and all(t.power_lo == 0x1234 and t.quorum_lo == 0 for t in tal))

    os.environ["IBFT_PROPOSAL_BYTES_MAX"] = "4096"     # read at ibft_ctx_create; the fixture's proposals are 2 858 bytes
    try:
        bv = V.BatchVerifier(max_rows=128)
    finally:
        del os.environ["IBFT_PROPOSAL_BYTES_MAX"]
    try:
        L, h = bv._L, bv._h

        def hashes(raw_=raw, roff_=roff, rnd_=rnd, n_=nb, out_=out):
            return L.ibft_proposal_hashes(h, p(raw_), p(roff_), p(rnd_), n_, p(out_))

        def verify(raw_=raw, roff_=roff, rnd_=rnd, off_=off, nb_=nb, sig_=sig, signer_=signer, mask_=mask):
            return L.ibft_verify_block_seals_raw(h, p(raw_), p(roff_), p(rnd_), p(off_), nb_, p(sig_), p(signer_), p(pre), p(out),
                                                 p(mask_), tal)

        def recover(raw_=raw, roff_=roff, rnd_=rnd, off_=off, nb_=nb, so_=so):
            return L.ibft_recover_block_seals_raw(h, p(raw_), p(roff_), p(rnd_), p(off_), nb_, p(sig), p(pre), p(out), p(so_), p(vi),
                                                  p(mask), tal)

        # the existing order first: no validator set yet
        assert verify() == E_NOVALSET and recover() == E_NOVALSET and untouched()
        assert hashes() == 0 and (out == bh).all()                         # … which ibft_proposal_hashes does not need
        out[:] = 0xA5
        bv.set_validators(r.height, r.addrs, r.power)
        bad0 = roff.copy(); bad0[0] = 1
        dec = roff.copy(); dec[5] = dec[4] - 1
        big = roff.copy(); big[-1] = 4097
        many_off = np.zeros(130, np.uint32)
        for call in (hashes, verify, recover):
            assert call(roff_=None) == E_INVAL                             # NULL raw_off
            assert call(rnd_=None) == E_INVAL                              # NULL round
            assert call(raw_=None) == E_INVAL                              # NULL raw with raw_off[n] > 0
            assert call(roff_=bad0) == E_INVAL                             # raw_off[0] ≠ 0
            assert call(roff_=dec) == E_INVAL                              # decreasing
            assert call(roff_=big) == E_TOOBIG                             # above the byte budget
            assert untouched(), call.__name__
        assert hashes(out_=None) == E_INVAL
        assert hashes(roff_=many_off, rnd_=np.zeros(129, np.uint64), n_=129, out_=np.zeros((129, 32), np.uint8)) == E_TOOBIG   # n > max_rows
        # the block calls' own checks come first, with their codes
        soff_bad = off.copy(); soff_bad[0] = 1
        assert verify(off_=soff_bad) == E_INVAL and verify(off_=None) == E_INVAL and verify(sig_=None) == E_INVAL
        assert verify(signer_=None) == E_INVAL and verify(mask_=None) == E_INVAL and recover(so_=None) == E_INVAL
        assert verify(off_=many_off, nb_=129) == E_TOOBIG and recover(off_=many_off, nb_=129) == E_TOOBIG
        assert untouched()
        # NULL raw is fine when every proposal is empty; and the context still works
        z = np.zeros(nb + 1, np.uint32)
        assert L.ibft_proposal_hashes(h, None, p(z), p(rnd), nb, p(out)) == 0
        assert (out == PC.expected([b""] * nb, rounds)).all()
        assert verify() == 0 and (out == bh).all() and not untouched()
    finally:
        bv.close()


# ---- (e) the remembered proposal of ibft_verify_hashes survives ------------------------------------------------------
def test_remembered_proposal_survives_a_batch_call():
    from oracle import binding as B
    V = _V()
    rng = np.random.default_rng(2106)
    raw, rnd = rng.bytes(500), 9
    H = B.proposal_hash(raw, rnd)
    h32 = np.frombuffer(H + B.proposal_hash(raw, rnd + 1) + H, np.uint8).reshape(3, 32).copy()
    hl = np.array([32, 32, 32], np.uint8)
    bv = V.BatchVerifier(max_rows=1024)
    try:
        assert bv.is_valid_proposal_hash(raw, rnd, h32, hl).tolist() == [True, False, True]      # hashed and remembered
        # a batch that holds the same bytes under another round, other proposals, and enough of them to reuse every buffer
        raws = [raw, raw[:-1], rng.bytes(136), b""] * 16
        rounds = [rnd + 1, rnd, 0, 1] * 16
        assert (bv.proposal_hashes(raws, rounds) == PC.expected(raws, rounds)).all()
        # the remembered digest is still the one of (raw, rnd): the compare that skips the hash gives the same verdicts
        assert bv.is_valid_proposal_hash(raw, rnd, h32, hl).tolist() == [True, False, True]
        assert bv.proposal_hash(raw, rnd) == H
        bv.forget_proposal()                                                                         # semantics untouched
        assert (bv.proposal_hashes(raws, rounds) == PC.expected(raws, rounds)).all()
        assert bv.is_valid_proposal_hash(raw, rnd, h32, hl).tolist() == [True, False, True]
    finally:
        bv.close()


# ---- (f) between a streamed submit and its collect -------------------------------------------------------------------
def test_calls_between_submit_and_collect_leave_the_batch_in_flight_intact():
    import test_gpu_block_seals as BS
    V = _V()
    big = _sync_fixture_with_proposals(12, 32)
    r, vs, raws, rounds, bh, off, sig, signer, pre = big
    exp, te = BS._expect(vs, bh, off, sig, signer, pre)
    # a second, smaller batch judged by the same validator set through the calls under test
    sraws, srounds = raws[:5], rounds[:5]
    soff = off[:6].copy()
    ns = int(soff[-1])
    bv = V.BatchVerifier(max_rows=65536)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        keep = [V.pinned_copy(x) for x in (bh, off, sig, signer, pre)]
        assert bv.block_seals_submit(*keep) == int(off[-1])
        hs = bv.proposal_hashes(raws, rounds)
        m, tl, got = bv.verify_block_seals_raw(sraws, srounds, soff, sig[:ns], signer[:ns], pre[:ns])
        s, v, rm, rt, got2 = bv.recover_block_seals_raw(sraws, srounds, soff, sig[:ns], pre[:ns])
        assert bv.block_seals_pending() == (1, int(off[-1]), len(bh))
        cm, ct = bv.block_seals_collect()
        assert (cm == exp).all() and [_fields(t)[:5] for t in ct] == [BS._fields(t) for t in te]
        assert (hs == bh).all() and (got == bh[:5]).all() and (got2 == bh[:5]).all()
        assert (m == exp[:ns]).all() and [_fields(t)[:5] for t in tl] == [BS._fields(t) for t in te[:5]]
        assert (rm[exp[:ns]]).all()                  # every seal its signer verified recovers to a member
    finally:
        bv.close()
