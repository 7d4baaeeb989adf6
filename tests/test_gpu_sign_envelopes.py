"""GPU: ibft_sign_envelopes_wire — PREPREPARE / ROUND_CHANGE envelopes around given bodies: heads built, bodies copied, envelopes
hashed (a lane or a wavefront per message) and signed on gfx950.  Signer and verifier share their hashing code, so the reference
of every byte is the ORACLE (sign_envelope_cases.expected: oracle/wire.py + oracle.binding); the library's own verify side
(ibft_verify_certificates_wire, ibft_verify_senders_wire) comes on top of that, never instead."""
import os

import numpy as np
import pytest

import sign_envelope_cases as SE

pytestmark = pytest.mark.gpu
E_INVAL, E_TOOBIG = -1, -7


@pytest.fixture(scope="module")
def bv():
    import go_ibft_amd.verifier as V
    b = V.BatchVerifier(max_rows=256)
    yield b
    b.close()


_cache = {}


def _case(n, nonce):
    """(columns, the oracle's rows) of a batch: computed once per (n, nonce), never changed"""
    if (n, nonce) not in _cache:
        cols = SE.batch(n)
        for c in cols:
            if isinstance(c, np.ndarray):
                c.setflags(write=False)
        _cache[(n, nonce)] = (cols, SE.expected_batch(cols, nonce))
    return _cache[(n, nonce)]


def _check_bytes(want, got):
    wire, off, frm, ok = got
    n = len(want)
    assert off.dtype == np.uint32 and len(off) == n + 1
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).tolist()
    assert len(wire) == int(off[n])
    for i, (w_wire, _, w_from, w_ok) in enumerate(want):
        got_i = wire[off[i]:off[i + 1]]
        if got_i != w_wire:
            d = next(k for k in range(len(w_wire)) if got_i[k] != w_wire[k])
            raise AssertionError(f"row {i} of {n} ({len(w_wire)} bytes) differs from byte {d} on")
        assert frm[i].tobytes() == w_from, i
        assert bool(ok[i]) == w_ok, i


@pytest.mark.parametrize("lanes", [None, "1", "64"], ids=["auto", "lane", "wave"])
@pytest.mark.parametrize("nonce", SE.NONCES)
def test_case_table_byte_parity_with_the_oracle(nonce, lanes):
    """the CPU case table at n = 1, 64, 65, 130 under each digest form: every row byte-identical to the oracle's message"""
    import go_ibft_amd.verifier as V
    old = os.environ.pop("IBFT_ENVELOPE_LANES", None)
    if lanes:
        os.environ["IBFT_ENVELOPE_LANES"] = lanes     # read at ibft_ctx_create
    try:
        b = V.BatchVerifier(max_rows=256)
    finally:
        os.environ.pop("IBFT_ENVELOPE_LANES", None)
        if old is not None:
            os.environ["IBFT_ENVELOPE_LANES"] = old
    try:
        for n in SE.BATCH_SIZES:
            cols, want = _case(n, nonce)
            _check_bytes(want, b.sign_envelopes(*cols, nonce=nonce))
            if n == 130:
                typ = cols[1]
                assert set(typ[:64].tolist()) == {0} and set(typ[64:128].tolist()) == {3} and set(typ[128:].tolist()) == {0, 3}
                assert [i for i, w in enumerate(want) if not w[3]] == [5, 70]
            else:
                assert n == 1 or set(cols[1].tolist()) == {0, 3}
        # row boundaries at every offset mod 4, also across wavefronts (rows 64, 128) and inside one
        offs = np.concatenate([np.cumsum([len(w[0]) for w in _case(n, nonce)[1]]) for n in (65, 130)])
        assert set((offs % 4).tolist()) == {0, 1, 2, 3}
    finally:
        b.close()


@pytest.mark.parametrize("nonce", SE.NONCES)
def test_rows_that_share_one_body(bv, nonce):
    """65 rows over ONE 16 384-byte body, and 65 rows over overlapping ranges of it"""
    n = 65
    body, canonical = SE.make_body(SE.ROUND_CHANGE, 16384, 77)
    assert canonical
    keys = SE.good_keys(n, seed=13)
    sk = np.frombuffer(b"".join(keys), np.uint8).reshape(n, 32)
    typ = np.where(np.arange(n) % 3 == 0, 0, 3).astype(np.uint8)
    height = np.full(n, 5, np.uint64)
    round_ = np.arange(n, dtype=np.uint64)
    for at, ln in ((np.zeros(n, np.uint32), np.full(n, 16384, np.uint32)),
                   ((np.arange(n) * 37).astype(np.uint32), (16384 - np.arange(n) * 101).astype(np.uint32))):
        assert int((at.astype(np.uint64) + ln).max()) <= len(body)
        cols = (sk, typ, height, round_, body, at, ln)
        _check_bytes(SE.expected_batch(cols, nonce), bv.sign_envelopes(*cols, nonce=nonce))


@pytest.mark.parametrize("nonce", SE.NONCES)
def test_round_trip_through_the_verify_side(bv, nonce):
    """the produced bytes through ibft_verify_certificates_wire: sender bit 1 for every signed row, 0 for the refused-key rows,
    class 0.  ibft_verify_senders_wire hands EVERY PREPREPARE / ROUND_CHANGE payload to the host by contract (status
    IBFT_WIRE_NEEDS_HOST, verdict 0: include/ibftgpu.h) — that is what it must answer here too —, and the call it sends the host
    to, ibft_verify_senders over the oracle's PayloadNoSig and the produced signatures, gives the same bits as the tree."""
    import go_ibft_amd.verifier as V
    from oracle import wire as W, wire_cert as WC
    n = 130
    cols, want = _case(n, nonce)
    keep = [i for i in range(n) if SE.make_body(int(cols[1][i]), int(cols[6][i]))[1]]     # (the 1-byte body is no protobuf message)
    assert len(keep) >= n - 12 and 5 in keep and 70 in keep
    sub = tuple(c[keep] if isinstance(c, np.ndarray) else c for c in cols)
    wire, off, frm, ok = bv.sign_envelopes(*sub, nonce=nonce)
    _check_bytes([want[i] for i in keep], (wire, off, frm, ok))
    assert int((~ok).sum()) == 2
    uniq = np.unique(frm[ok], axis=0)
    bv.set_validators(5, uniq, np.ones(len(uniq), np.uint64))
    rows_n, nodes, rows, cls, sender, hb, sb = bv.verify_certificates_wire(wire, off, rows_cap=4096)
    assert rows_n == len(keep), "no body of the table nests a message"
    assert (cls[:rows_n] == 0).all() and (rows["status"][:rows_n] == V.WIRE_OK).all()
    assert (sender[:rows_n] == ok).all()
    assert (rows["from"][:rows_n] == frm).all() and (rows["type"][:rows_n] == sub[1]).all()
    assert (rows["height"][:rows_n] == sub[2]).all() and (rows["round"][:rows_n] == sub[3]).all()
    msgs = [wire[off[i]:off[i + 1]] for i in range(len(keep))]
    exp = WC.expected_tree(msgs, uniq)
    assert exp.sender_ok == ok.tolist() and not any(exp.cls)
    verdict, wrows, _ = bv.is_valid_validator_wire(wire, off)
    assert (wrows["status"] == V.WIRE_NEEDS_HOST).all() and not verdict.any()
    pns = [want[i][1] for i in keep]
    poff = np.concatenate([[0], np.cumsum([len(x) for x in pns])]).astype(np.uint32)
    cut = [len(W._len_field(1, W.View(int(h), int(r)).encode(), emit_empty=True)) + 22 for h, r in zip(sub[2], sub[3])]   # View ‖ From
    sigs = np.array([np.frombuffer(m[c + 2:c + 67], np.uint8) for m, c in zip(msgs, cut)])
    assert all(m[:c] + m[c + 67:] == x for m, c, x in zip(msgs, cut, pns))
    verdict, t = bv.is_valid_validator(b"".join(pns), poff, sigs, frm)
    assert (verdict == ok).all() and t.valid_rows == int(ok.sum())


def test_refusals_in_order_and_untouched_outputs(bv):
    import go_ibft_amd.verifier as V
    L, p = bv._L, V._p
    n = 65
    cols, want = _case(n, "keccak")
    sk, typ, height, round_, body, at, ln = cols
    bb = np.frombuffer(body, np.uint8)
    total = sum(len(w[0]) for w in want)
    wire = np.full(total + 64, 0xA5, np.uint8)
    off = np.full(n + 1, 0xA5A5A5A5, np.uint32)
    frm = np.full((n, 20), 0xA5, np.uint8)
    ok = np.full(n, 0xA5, np.uint8)

    def call(sk=sk, typ=typ, height=height, round_=round_, body=bb, body_bytes=len(body), at=at, ln=ln, n=n, nonce=0, wire=wire,
             cap=wire.size, off=off):
        return L.ibft_sign_envelopes_wire(bv._h, p(sk), p(typ), p(height), p(round_), p(body), body_bytes, p(at), p(ln), n, nonce,
                                          p(wire), cap, p(off), p(frm), p(ok))

    bad_type = typ.copy()
    bad_type[[9, 40]] = (1, 2)
    past = ln.copy()
    past[7] = len(body) - int(at[7]) + 1                 # one byte past body_bytes
    wrap_at, wrap_ln = at.copy(), ln.copy()
    wrap_at[11], wrap_ln[11] = 0xFFFFFFF0, 0x20          # at + len wraps 2^32 (and would look like 0x10 in 32 bits)
    # 1. a NULL column (before anything else: the nonce is unknown too, the error text is not the nonce's)
    for kw in ({"sk": None}, {"typ": None}, {"height": None}, {"round_": None}, {"at": None}, {"ln": None}, {"wire": None}, {"off": None}):
        assert call(nonce=9, **kw) == E_INVAL
    # 2. a NULL body with body_bytes > 0 — before the nonce
    assert call(nonce=9, body=None) == E_INVAL
    # 3. an unknown nonce rule, named — before the row count, the types, the ranges and the capacity are looked at
    for unknown in (2, 0xFFFFFFFF):
        assert call(nonce=unknown, n=bv.max_rows + 1, typ=bad_type, ln=past, cap=0) == E_INVAL
        assert str(unknown).encode() in L.ibft_last_error(bv._h)
    # 4. more rows than the context holds — before the types, the ranges and the capacity
    assert call(n=bv.max_rows + 1, typ=bad_type, ln=past, cap=0) == E_TOOBIG
    # 5. a type other than PREPREPARE / ROUND_CHANGE: the first such row is named — before the ranges and the capacity
    assert call(typ=bad_type, ln=past, cap=0) == E_INVAL
    assert b"row 9 " in L.ibft_last_error(bv._h)
    # 6. a body range past body_bytes, or one whose end wraps 2^32 — before the capacity
    assert call(ln=past, cap=0) == E_INVAL
    assert b"row 7 " in L.ibft_last_error(bv._h)
    assert call(at=wrap_at, ln=wrap_ln, cap=0) == E_INVAL
    assert b"row 11 " in L.ibft_last_error(bv._h)
    # 7. wire_cap one byte short
    assert call(cap=total - 1) == E_TOOBIG
    assert (wire == 0xA5).all() and (off == 0xA5A5A5A5).all() and (frm == 0xA5).all() and (ok == 0xA5).all()
    # the next good call is correct; exactly enough is enough; n = 0 is legal and sets out_off[0]
    assert call(cap=total) == 0
    assert int(off[n]) == total and bytes(wire[:total]) == b"".join(w[0] for w in want) and (wire[total:] == 0xA5).all()
    off0 = np.full(1, 0xA5A5A5A5, np.uint32)
    assert call(n=0, cap=0, off=off0) == 0 and off0[0] == 0 and int(off[n]) == total
    assert L.ibft_sign_envelopes_wire(bv._h, None, None, None, None, None, 0, None, None, 0, 0, None, 0, None, None, None) == 0
    w0, o0, f0, k0 = bv.sign_envelopes(np.zeros((0, 32), np.uint8), 3, 1, 0, b"", 0, 0)
    assert w0 == b"" and o0.tolist() == [0] and f0.shape == (0, 20) and k0.shape == (0,)


def test_byte_budget_is_the_proposal_budget():
    """body_bytes or the total output beyond IBFT_PROPOSAL_BYTES_MAX: IBFT_E_TOOBIG, and the context goes on working"""
    import go_ibft_amd.verifier as V
    os.environ["IBFT_PROPOSAL_BYTES_MAX"] = "4096"     # read at ibft_ctx_create
    try:
        b = V.BatchVerifier(max_rows=64)
    finally:
        del os.environ["IBFT_PROPOSAL_BYTES_MAX"]
    try:
        sk = np.frombuffer(b"".join(SE.good_keys(3)), np.uint8).reshape(3, 32)
        big = bytes(4097)
        with pytest.raises(RuntimeError, match="-7"):
            b.sign_envelopes(sk[:1], 3, 5, 2, big, 0, 10)               # body_bytes over the budget
        with pytest.raises(RuntimeError, match="-7"):
            b.sign_envelopes(sk, 3, 5, 2, big[:2000], 0, 2000)          # 3 × (2 000 + head) bytes out over the budget
        body, _ = SE.make_body(3, 1000)
        cols = (sk, np.full(3, 3, np.uint8), np.full(3, 5, np.uint64), np.full(3, 2, np.uint64), body, np.zeros(3, np.uint32),
                np.full(3, 1000, np.uint32))
        _check_bytes(SE.expected_batch(cols, "keccak"), b.sign_envelopes(*cols))
    finally:
        b.close()
