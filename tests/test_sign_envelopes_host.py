"""The envelope signer's device code (csrc/sign_envelope_dev.h: head, body copy, digest in the lane and in the wavefront form,
signature — the four steps ibft_sign_envelopes_wire launches), compiled for the host by csrc/host_sign_envelope_harness.hip (the
wavefront form through wave_emul.h), against the oracle: oracle/wire.py for the bytes, oracle.binding for From, digest and
signature, and the oracle's parser for what a verifier reads.  No GPU.

The parser is oracle/wire_cert.py (own / expected_tree), the walk of oracle/wire_parse.py one level deeper: wire_parse.expected
itself answers NEEDS_HOST for EVERY PrePrepareMessage / RoundChangeMessage payload by design (it judges flat PREPARE / COMMIT bodies
only), so "parses as IBFT_WIRE_OK" is asked of the parser that does judge these two types — status OK, class 0, the sender
recovered over its digest."""
import ctypes as C

import numpy as np
import pytest

import sign_envelope_cases as SE
from oracle import binding as O, wire as W, wire_cert as WC

NONCE_ID = {"keccak": 0, "rfc6979": 1}
FORMS = (1, 64)
SENT = 0xEE
PAD = 64     # sentinel bytes on either side of a row


@pytest.fixture(scope="module")
def dev():
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_sign_envelope_harness())
    L.dev_envelope_cut.argtypes = [C.c_uint64, C.c_uint64]
    L.dev_envelope_cut.restype = C.c_uint32
    L.dev_message_front.argtypes = [C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p]
    L.dev_message_front.restype = C.c_uint32
    L.dev_envelope_head_len.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]
    L.dev_envelope_head_len.restype = C.c_uint32
    L.dev_envelope_wire_len.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]
    L.dev_envelope_wire_len.restype = C.c_uint64
    vp = C.c_void_p
    L.dev_sign_envelope.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint64, C.c_uint64, vp, C.c_uint32, C.c_uint32,
                                    vp, C.c_uint32, C.POINTER(C.c_uint32), C.c_char_p, C.c_char_p]
    L.dev_sign_envelope.restype = C.c_int
    L.dev_envelope_digest.argtypes = [C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_char_p]
    L.dev_envelope_digest.restype = None
    L.dev_envelope_copy.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32]
    L.dev_envelope_copy.restype = None
    return L


def _aligned(nbytes, fill):
    """a 16-byte aligned u8 array of nbytes (what hipMalloc gives the device buffers)"""
    raw = np.full(nbytes + 16, fill, np.uint8)
    shift = (-raw.ctypes.data) % 16
    return raw[shift:shift + nbytes]


def _row(dev, nonce, form, sk, typ, height, round_, body, src_mis=0, dst_mis=0):
    """one row through the harness: the body lies at offset 16 + src_mis of its buffer, the message goes to PAD + dst_mis of a
    buffer of sentinels → (ok, message, digest, From); asserts that nothing but the row was stored"""
    src_at, dst_at = 16 + src_mis, PAD + dst_mis
    bbuf = _aligned(src_at + len(body) + 32, 0x77)
    bbuf[src_at:src_at + len(body)] = np.frombuffer(body, np.uint8)
    want_len = dev.dev_envelope_wire_len(typ, height, round_, len(body))
    wbuf = _aligned(dst_at + want_len + PAD + 16, SENT)
    wl = C.c_uint32()
    dg, frm = C.create_string_buffer(32), C.create_string_buffer(20)
    ok = dev.dev_sign_envelope(NONCE_ID[nonce], form, sk, typ, height, round_, bbuf.ctypes.data, src_at, len(body), wbuf.ctypes.data,
                               dst_at, C.byref(wl), dg, frm)
    assert ok >= 0 and wl.value == want_len
    assert (wbuf[:dst_at] == SENT).all() and (wbuf[dst_at + want_len:] == SENT).all(), "stores outside the row"
    return ok, wbuf[dst_at:dst_at + want_len].tobytes(), dg.raw, frm.raw


def _check(dev, nonce, form, sk, typ, height, round_, body, **kw):
    want_wire, want_pns, want_from, want_ok = SE.expected(sk, typ, height, round_, body, nonce)
    ok, wire, dg, frm = _row(dev, nonce, form, sk, typ, height, round_, body, **kw)
    where = (typ, height, round_, len(body), nonce, form, kw)
    assert bool(ok) == want_ok, where
    cut = dev.dev_envelope_cut(height, round_)
    assert wire[:cut] + wire[cut + 67:] == want_pns, where          # PayloadNoSig
    assert dg == O.keccak256(want_pns), where                       # the digest that was signed
    assert wire == want_wire, where
    assert frm == want_from, where
    return wire


def test_case_table_is_what_the_issue_asks_for():
    """both types, the five views, PayloadNoSig of 135 … 273 bytes under each type, the body lengths; the oracle's lengths"""
    for t in SE.TYPES:
        rows = [c for c in SE.ROW_CASES if c[0] == t]
        assert {(h, r) for _, h, r, _ in rows} >= set(SE.VIEWS)
        assert {SE.payload_len(*c) for c in rows} >= set(SE.RATE_LENGTHS)
        assert {c[3] for c in rows} >= set(SE.BODY_LENGTHS)
    m = W.IbftMessage(view=W.View(0, 0), sender=bytes(20), signature=bytes(65), type=SE.PREPREPARE, payload=b"")
    assert m.encode()[:2] == b"\x0a\x00" and b"\x20" not in m.encode()[2 + 22 + 67:]      # empty View present, no Type field
    assert m.encode().endswith(b"\x2a\x00")                                                  # the empty body is emitted


def test_length_function(dev):
    for typ in SE.TYPES:
        for height, round_ in SE.VIEWS + [(2**35, 1), (127, 128)]:
            for blen in (0, 1, 127, 128, 16383, 16384, 2097151, 2097152):
                m = W.IbftMessage(view=W.View(height, round_), sender=bytes(20), signature=bytes(65), type=typ, payload=bytes(blen))
                assert dev.dev_envelope_wire_len(typ, height, round_, blen) == len(m.encode()), (typ, height, round_, blen)
                assert dev.dev_envelope_head_len(typ, height, round_, blen) == len(m.encode()) - blen
    assert dev.dev_envelope_head_len(3, SE.M64, SE.M64, 2**32 - 1) == 121       # ENVELOPE_HEAD_MAX


def test_message_front_is_the_front_of_both_signers_messages(dev):
    """put_message_front (View ‖ From, shared by sign_message_row and envelope_head) under the nine views of the message
    signer's row cases and under height = round = 2^64 − 1: the offset it returns is envelope_cut, and its bytes open the oracle's
    PREPARE and the oracle's ROUND_CHANGE of that row"""
    import sign_message_cases as SM
    sk = SE.good_keys(3)[2]
    frm = O.address(O.pubkey(sk))
    views = [(h, r) for _, h, r, _, _ in SM.ROW_CASES] + [(SE.M64, SE.M64)]
    assert len(views) == 10
    for height, round_ in views:
        out = C.create_string_buffer(b"\xee" * 64, 64)
        cut = dev.dev_message_front(height, round_, frm, out)
        assert cut == dev.dev_envelope_cut(height, round_), (height, round_)
        assert out.raw[cut:] == b"\xee" * (64 - cut), "stores behind From"
        prepare = SM.expected(sk, SM.PREPARE, height, round_, bytes(range(32)), "keccak")[0]
        round_change = SE.expected(sk, SE.ROUND_CHANGE, height, round_, SE.make_body(SE.ROUND_CHANGE, 40)[0], "keccak")[0]
        assert out.raw[:cut] == prepare[:cut], (height, round_)
        assert out.raw[:cut] == round_change[:cut], (height, round_)


@pytest.mark.parametrize("form", FORMS, ids=["lane", "wave"])
@pytest.mark.parametrize("nonce", SE.NONCES)
def test_row_parity_with_the_oracle(dev, nonce, form):
    """every row case: PayloadNoSig, digest, wire and From byte for byte; the message parses as IBFT_WIRE_OK and recovers its sender"""
    keys = SE.good_keys(len(SE.ROW_CASES) + 2)
    for i, (typ, height, round_, blen) in enumerate(SE.ROW_CASES):
        body, canonical = SE.make_body(typ, blen, i)
        assert canonical or blen == 1      # (no protobuf message is one byte long: the row is still carried byte for byte)
        wire = _check(dev, nonce, form, keys[2 + i], typ, height, round_, body, src_mis=i % 4, dst_mis=(i // 4) % 4)
        if not canonical:
            continue
        frm = O.address(O.pubkey(keys[2 + i]))
        t = WC.expected_tree([wire], [frm])
        e = t.rows[0]
        assert t.status[0] == WC.OK and t.cls[0] == 0 and (e.height, e.round, e.type, e.kind) == (height, round_, typ, 5 + typ), i
        assert e.sender == frm and t.sender_ok[0] and O.recover_address(t.digest[0], e.signature) == frm, i
        if typ == SE.PREPREPARE:
            cut = dev.dev_envelope_cut(height, round_)
            assert wire[cut + 67] == 0x2A, "no 20 xx field in a PREPREPARE"
        else:
            cut = dev.dev_envelope_cut(height, round_)
            assert wire[cut + 67:cut + 70] == b"\x20\x03\x42"


@pytest.mark.parametrize("nonce", SE.NONCES)
def test_edge_keys(dev, nonce):
    """keys 1 and n − 1 sign; 0 and n are refused: normal length, zero From and Signature, body present"""
    for typ, height, round_, blen in ((SE.PREPREPARE, 5, 2, 106), (SE.ROUND_CHANGE, 5, 2, 239)):
        body, canonical = SE.make_body(typ, blen)
        assert canonical
        for sk in SE.good_keys(2):
            _check(dev, nonce, 1, sk, typ, height, round_, body)
        for key in SE.REFUSED_KEYS:
            want_wire, _, _, _ = SE.expected(SE.b32(key), typ, height, round_, body, nonce)
            ok, wire, _, frm = _row(dev, nonce, 64, SE.b32(key), typ, height, round_, body, src_mis=1, dst_mis=3)
            assert ok == 0 and frm == bytes(20) and wire == want_wire and wire.endswith(body)
            t = WC.expected_tree([wire], [bytes(20)])
            assert t.status[0] == WC.OK and t.rows[0].sender == bytes(20) and t.rows[0].signature == bytes(65) and not t.sender_ok[0]


@pytest.mark.parametrize("blen", [0, 1, 3, 4, 5, 15, 16, 17, 31, 33, 70])
def test_every_alignment_of_source_and_destination(dev, blen):
    """the body copy at every (source offset mod 4) × (destination offset mod 16): the bytes arrive, the neighbours stay"""
    src = SE.pool(16 + 4 + blen + 32, seed=blen)
    for s in range(4):
        for d in range(16):
            sbuf = _aligned(len(src), 0)
            sbuf[:] = np.frombuffer(src, np.uint8)
            wbuf = _aligned(PAD + 16 + blen + PAD, SENT)
            dev.dev_envelope_copy(wbuf.ctypes.data, sbuf.ctypes.data, PAD + d, 16 + s, blen)
            assert wbuf[PAD + d:PAD + d + blen].tobytes() == src[16 + s:16 + s + blen], (s, d)
            assert (wbuf[:PAD + d] == SENT).all() and (wbuf[PAD + d + blen:] == SENT).all(), (s, d)


def test_copy_across_pieces(dev):
    """a body longer than one workgroup's 4 096 bytes of output, at every alignment pair mod 4"""
    blen = 2 * 4096 + 37
    src = SE.pool(16 + 4 + blen + 32, seed=99)
    for s in range(4):
        for d in range(4):
            sbuf = _aligned(len(src), 0)
            sbuf[:] = np.frombuffer(src, np.uint8)
            wbuf = _aligned(PAD + 16 + blen + PAD, SENT)
            dev.dev_envelope_copy(wbuf.ctypes.data, sbuf.ctypes.data, PAD + 13 + d, 16 + s, blen)
            lo = PAD + 13 + d
            assert wbuf[lo:lo + blen].tobytes() == src[16 + s:16 + s + blen], (s, d)
            assert (wbuf[:lo] == SENT).all() and (wbuf[lo + blen:] == SENT).all(), (s, d)


@pytest.mark.parametrize("typ", SE.TYPES)
def test_alignment_through_the_whole_row(dev, typ):
    """every body start offset mod 4 crossed with every destination offset mod 4, a two-block row, both digest forms"""
    sk = SE.good_keys(4)[3]
    body = SE.pool(SE.body_len_for(typ, 5, 2, 273))
    for s in range(4):
        for d in range(4):
            _check(dev, "keccak", 1 if (s + d) % 2 else 64, sk, typ, 5, 2, body, src_mis=s, dst_mis=d)


def test_both_sponge_forms_give_the_oracles_digest(dev):
    """oracle messages of every rate-boundary length and of 16 KB, hashed in place at every offset mod 4"""
    sk = SE.good_keys(3)[2]
    for typ, height, round_, blen in SE.ROW_CASES:
        wire, pns, _, _ = SE.expected(sk, typ, height, round_, SE.pool(blen), "keccak")
        cut = dev.dev_envelope_cut(height, round_)
        for mis in range(4) if blen < 1000 else (1,):
            buf = _aligned(mis + len(wire) + 32, 0x33)
            buf[mis:mis + len(wire)] = np.frombuffer(wire, np.uint8)
            for form in FORMS:
                out = C.create_string_buffer(32)
                dev.dev_envelope_digest(form, buf.ctypes.data + mis, len(wire), cut, out)
                assert out.raw == O.keccak256(pns), (typ, height, round_, blen, mis, form)
