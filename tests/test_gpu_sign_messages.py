"""GPU: ibft_sign_messages_wire / sign_message_lane_kernel<NONCE> — whole PREPARE / COMMIT messages built, hashed, signed and
encoded on gfx950.  References: oracle/wire.py + oracle.binding (the expected bytes of every row, sign_message_cases.expected),
the library's own verify side (ibft_verify_senders_wire, ibft_wire_stage_seals + ibft_seals_run), ibft_sign_seals_ex for the
seals, and oracle.binding.verify_senders for the simulator's rounds."""
import ctypes as C

import numpy as np
import pytest

import sign_message_cases as SM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bv():
    import go_ibft_amd.verifier as V
    b = V.BatchVerifier(max_rows=256)
    yield b
    b.close()


_cache = {}


def _case(n, nonce, suffix=None):
    """(columns, the oracle's rows) of a batch: computed once per (n, nonce, suffix), never changed"""
    key = (n, nonce, suffix)
    if key not in _cache:
        cols = SM.batch(n)
        for c in cols:
            c.setflags(write=False)
        _cache[key] = (cols, SM.expected_batch(cols, nonce, suffix))
    return _cache[key]


def _check_bytes(cols, want, got):
    wire, off, frm, ok = got
    n = len(want)
    assert off.dtype == np.uint32 and len(off) == n + 1
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).tolist()
    assert len(wire) == int(off[n])
    for i, (w_wire, _, w_from, _, w_ok) in enumerate(want):
        assert wire[off[i]:off[i + 1]] == w_wire, (i, int(cols[1][i]), int(cols[2][i]), int(cols[3][i]))
        assert frm[i].tobytes() == w_from, i
        assert bool(ok[i]) == w_ok, i


@pytest.mark.parametrize("nonce", SM.NONCES)
@pytest.mark.parametrize("n", SM.BATCH_SIZES)
def test_byte_parity_with_the_oracle(bv, n, nonce):
    cols, want = _case(n, nonce)
    got = bv.sign_messages(*cols, nonce=nonce)
    _check_bytes(cols, want, got)
    if n == 130:
        assert [i for i in range(n) if not got[3][i]] == [5, 70, 129]
        assert set(cols[1][:64].tolist()) == {1} and set(cols[1][64:128].tolist()) == {2} and set(cols[1][128:].tolist()) == {1, 2}


@pytest.mark.parametrize("nonce", SM.NONCES)
def test_every_row_case_under_the_edge_keys(bv, nonce):
    """the nine row cases under key 1 and key n − 1 (the batches above put SplitMix keys on most cases)"""
    keys = [SM.b32(1), SM.b32(SM.N - 1)]
    rows = [(k, c) for c in SM.ROW_CASES for k in keys]
    sk = np.frombuffer(b"".join(k for k, _ in rows), np.uint8).reshape(-1, 32)
    typ = np.array([c[0] for _, c in rows], np.uint8)
    height = np.array([c[1] for _, c in rows], np.uint64)
    round_ = np.array([c[2] for _, c in rows], np.uint64)
    hs = np.tile(np.arange(32, dtype=np.uint8), (len(rows), 1))
    cols = (sk, typ, height, round_, hs)
    got = bv.sign_messages(*cols, nonce=nonce)
    _check_bytes(cols, SM.expected_batch(cols, nonce), got)
    assert np.diff(got[1].astype(np.int64)).tolist() == [c[4] for _, c in rows]


@pytest.mark.parametrize("nonce", SM.NONCES)
@pytest.mark.parametrize("suffix", [None, b"\x02"], ids=["identity", "suffix_02"])
def test_round_trip_through_the_verify_side(suffix, nonce):
    import go_ibft_amd.verifier as V
    n = 130
    cols, want = _case(n, nonce, suffix)
    sk, typ, height, round_, hs = cols
    b = V.BatchVerifier(max_rows=256)
    try:
        b.set_seal_digest(suffix)
        got = b.sign_messages(*cols, nonce=nonce)
        _check_bytes(cols, want, got)
        wire, off, frm, ok = got
        # the call leaves no staged seal batch and no resident wire batch
        rows_res = C.c_uint32(99)
        b._chk(b._L.ibft_seals_rows(b._h, C.byref(rows_res), None), "ibft_seals_rows")
        assert rows_res.value == 0
        with pytest.raises(RuntimeError):
            b.wire_stage_seals()
        uniq = np.unique(frm[ok], axis=0)
        b.set_validators(1, uniq, np.ones(len(uniq), np.uint64))
        verdict, rows, t = b.is_valid_validator_wire(wire, off)
        assert (rows["status"] == V.WIRE_OK).all()
        assert (verdict == ok).all() and t.valid_rows == int(ok.sum())
        assert (rows["height"] == height).all() and (rows["round"] == round_).all() and (rows["type"] == typ).all()
        assert (rows["from"] == frm).all() and (rows["proposal_hash"] == hs).all()
        assert (rows["hash_len"] == 32).all() and (rows["from_len"] == 20).all() and (rows["sig_len"] == 65).all()
        assert (rows["seal_len"] == np.where(typ == SM.COMMIT, 65, 0)).all()
        b.wire_stage_seals()
        seals, _ = b.seals_run()
        assert (seals == (ok & (typ == SM.COMMIT))).all()
    finally:
        b.close()


@pytest.mark.parametrize("nonce", SM.NONCES)
def test_seals_equal_ibft_sign_seals_ex(nonce):
    import go_ibft_amd.verifier as V
    n = 130
    cols, _ = _case(n, nonce, b"\x02")
    sk, typ, height, round_, hs = cols
    b = V.BatchVerifier(max_rows=256)
    try:
        for suffix in (None, b"\x02"):
            b.set_seal_digest(suffix)
            wire, off, frm, ok = b.sign_messages(*cols, nonce=nonce)
            sig, signer, ok2 = b.sign_seals(sk, hs, nonce=nonce)
            assert (ok2 == ok).all() and (signer == frm).all()
            commits = np.flatnonzero(typ == SM.COMMIT)
            assert len(commits) > 64
            for i in commits:
                assert wire[off[i + 1] - 67:off[i + 1] - 65] == b"\x12\x41"
                assert wire[off[i + 1] - 65:off[i + 1]] == sig[i].tobytes(), i
    finally:
        b.close()


def _decode(wire, off):
    """PayloadNoSig, signature and From of every message, through the oracle's parser"""
    from oracle import wire_parse as WP
    pns, sigs, frm = [], [], []
    for i in range(len(off) - 1):
        m = wire[off[i]:off[i + 1]]
        e = WP.expected(m)
        assert e.status == WP.OK, i
        cut = m.index(b"\x1a\x41" + e.signature)
        pns.append(m[:cut] + m[cut + 67:])
        sigs.append(np.frombuffer(e.signature, np.uint8))
        frm.append(np.frombuffer(e.sender, np.uint8))
    poff = np.concatenate([[0], np.cumsum([len(p) for p in pns])]).astype(np.uint32)
    return b"".join(pns), poff, np.array(sigs), np.array(frm)


@pytest.mark.parametrize("kind,byzantine,nonce", [("commit", False, "keccak"), ("commit", True, "rfc6979"), ("prepare", True, "keccak")])
def test_simulated_message_round(bv, kind, byzantine, nonce):
    import go_ibft_amd.simulate as S
    from oracle import binding as O
    n = 130
    r = S.make_message_round(bv, n, seed=3, kind=kind, height=7, round_=2, byzantine=byzantine, nonce=nonce)
    assert r.n == n and len(r.off) == n + 1 and len(r.wire) == int(r.off[n])
    assert r.expect.all() != byzantine
    if byzantine:
        spoiled = [k for k in r.kinds if k]
        assert len(spoiled) == int((~r.expect).sum()) >= 6 and set(spoiled) == set(S.MESSAGE_CORRUPTIONS)
    bv.set_validators(r.height, r.addrs, r.power)
    verdict, rows, t = bv.is_valid_validator_wire(r.wire, r.off)
    assert (rows["status"] == 0).all() and (rows["height"] == 7).all() and (rows["round"] == 2).all()
    assert (rows["type"] == S.MESSAGE_KINDS[kind]).all() and (rows["proposal_hash"] == np.frombuffer(r.proposal_hash, np.uint8)).all()
    assert (verdict == r.expect).all(), np.flatnonzero(verdict != r.expect)
    payload, poff, sigs, frm = _decode(r.wire, r.off)
    want = O.verify_senders(O.ValSet(r.addrs, r.power), payload, poff, sigs, frm).astype(bool)
    assert (verdict == want).all()
    assert t.valid_rows == int(r.expect.sum()) and t.distinct_senders == int(r.expect.sum())


def test_simulated_round_in_pieces_of_max_rows():
    """a context of 64 rows signs 130 messages in three pieces: the same bytes as one piece"""
    import go_ibft_amd.simulate as S
    import go_ibft_amd.verifier as V
    small, big = V.BatchVerifier(max_rows=64), V.BatchVerifier(max_rows=256)
    try:
        a = S.make_message_round(small, 130, seed=4, kind="commit", byzantine=True)
        b = S.make_message_round(big, 130, seed=4, kind="commit", byzantine=True)
        assert a.wire == b.wire and (a.off == b.off).all() and (a.addrs == b.addrs).all() and (a.expect == b.expect).all()
    finally:
        small.close()
        big.close()


def test_refusals_in_order_and_untouched_outputs(bv):
    import go_ibft_amd.verifier as V
    E_INVAL, E_TOOBIG = -1, -7
    L, p = bv._L, V._p
    n = 65
    cols, want = _case(n, "keccak")
    sk, typ, height, round_, hs = (np.array(c) for c in cols)
    total = sum(len(w[0]) for w in want)
    wire = np.full(n * 218, 0xA5, np.uint8)
    off = np.full(n + 1, 0xA5A5A5A5, np.uint32)
    frm = np.full((n, 20), 0xA5, np.uint8)
    ok = np.full(n, 0xA5, np.uint8)

    def call(sk=sk, typ=typ, height=height, round_=round_, hs=hs, n=n, nonce=0, wire=wire, cap=wire.size, off=off):
        return L.ibft_sign_messages_wire(bv._h, p(sk), p(typ), p(height), p(round_), p(hs), n, nonce, p(wire), cap, p(off), p(frm), p(ok))

    bad_type = typ.copy()
    bad_type[[9, 40]] = (3, 0)
    # 1. a NULL column (before anything else: the nonce is unknown too, the error text is not the nonce's)
    for kw in ({"sk": None}, {"typ": None}, {"height": None}, {"round_": None}, {"hs": None}, {"wire": None}, {"off": None}):
        assert call(nonce=9, **kw) == E_INVAL
    # 2. an unknown nonce rule, named — before the row count, the types and the capacity are looked at
    for unknown in (2, 0xFFFFFFFF):
        assert call(nonce=unknown, n=bv.max_rows + 1, typ=bad_type, cap=0) == E_INVAL
        assert str(unknown).encode() in L.ibft_last_error(bv._h)
    # 3. more rows than the context holds — before the types and the capacity
    assert call(n=bv.max_rows + 1, typ=bad_type, cap=0) == E_TOOBIG
    # 4. a type other than PREPARE / COMMIT: the first such row is named — before the capacity
    assert call(typ=bad_type, cap=0) == E_INVAL
    assert b"row 9 " in L.ibft_last_error(bv._h)
    # 5. wire_cap one byte short
    assert call(cap=total - 1) == E_TOOBIG
    assert (wire == 0xA5).all() and (off == 0xA5A5A5A5).all() and (frm == 0xA5).all() and (ok == 0xA5).all()
    # exactly enough is enough; n = 0 is legal and sets out_off[0]
    assert call(cap=total) == 0
    assert int(off[n]) == total and bytes(wire[:total]) == b"".join(w[0] for w in want) and (wire[total:] == 0xA5).all()
    off0 = np.full(1, 0xA5A5A5A5, np.uint32)
    assert call(n=0, cap=0, off=off0) == 0 and off0[0] == 0 and int(off[n]) == total
    assert L.ibft_sign_messages_wire(bv._h, None, None, None, None, None, 0, 0, None, 0, None, None, None) == 0
    w0, o0, f0, k0 = bv.sign_messages(np.zeros((0, 32), np.uint8), 2, 1, 0, np.zeros((0, 32), np.uint8))
    assert w0 == b"" and o0.tolist() == [0] and f0.shape == (0, 20) and k0.shape == (0,)
