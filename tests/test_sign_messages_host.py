"""The message-signing row (csrc/sign_message_dev.h: encode, hash, sign, store — what sign_message_lane_kernel runs per lane),
compiled for the host by csrc/host_sign_message_harness.hip, against the oracle: oracle/wire.py for the bytes,
oracle.binding.sign / sign_rfc6979 for seal and signature, address(pubkey(sk)) for From.  No GPU."""
import ctypes as C

import pytest

import sign_message_cases as SM
from oracle import binding as O, wire as W, wire_parse as WP

NONCE_ID = {"keccak": 0, "rfc6979": 1}


@pytest.fixture(scope="module")
def dev():
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_sign_message_harness())
    for f in (L.dev_message_payload_len, L.dev_message_wire_len):
        f.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64]
        f.restype = C.c_uint32
    L.dev_sign_message.argtypes = [C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint32,
                                   C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p]
    L.dev_sign_message.restype = C.c_int
    return L


def _row(dev, nonce, sk, typ, height, round_, h, suffix=None):
    wire, pns, frm = C.create_string_buffer(b"\xee" * 256, 256), C.create_string_buffer(b"\xee" * 256, 256), C.create_string_buffer(20)
    wl, pl = C.c_uint32(), C.c_uint32()
    ok = dev.dev_sign_message(NONCE_ID[nonce], sk, typ, height, round_, h, suffix, len(suffix or b""), wire, C.byref(wl), pns,
                              C.byref(pl), frm)
    assert wire.raw[wl.value:] == b"\xee" * (256 - wl.value), "nothing is stored behind the message"
    return ok, wire.raw[:wl.value], pns.raw[:pl.value], frm.raw


def test_case_table_is_what_the_oracle_encodes():
    """the lengths of the table are oracle/wire.py's, and such a message parses as IBFT_WIRE_OK and recovers its sender"""
    sk, h = SM.good_keys(3)[2], bytes(range(32))
    for nonce in SM.NONCES:
        for typ, height, round_, plen, wlen in SM.ROW_CASES:
            wire, pns, frm, seal, ok = SM.expected(sk, typ, height, round_, h, nonce)
            assert (len(pns), len(wire)) == (plen, wlen) and ok
            e = WP.expected(wire)
            assert e.status == WP.OK and (e.height, e.round, e.type) == (height, round_, typ) and e.sender == frm
            assert O.recover_address(e.digest, e.signature) == frm


@pytest.mark.parametrize("suffix", SM.SUFFIXES, ids=["identity", "suffix1", "suffix64"])
@pytest.mark.parametrize("nonce", SM.NONCES)
def test_row_parity_with_the_oracle(dev, nonce, suffix):
    keys = SM.good_keys(len(SM.ROW_CASES) + 2)
    for i, (typ, height, round_, plen, wlen) in enumerate(SM.ROW_CASES):
        # every case under a SplitMix key; the first under key 1, the last under key n − 1 as well
        for sk in [keys[2 + i]] + ([keys[0]] if i == 0 else []) + ([keys[1]] if i == len(SM.ROW_CASES) - 1 else []):
            h = O.keccak256(bytes([i]) + sk)
            want_wire, want_pns, want_from, _, _ = SM.expected(sk, typ, height, round_, h, nonce, suffix)
            ok, wire, pns, frm = _row(dev, nonce, sk, typ, height, round_, h, suffix)
            assert ok == 1
            assert (len(pns), len(wire)) == (plen, wlen)
            assert pns == want_pns, (i, pns.hex(), want_pns.hex())
            assert wire == want_wire, (i, wire.hex(), want_wire.hex())
            assert frm == want_from


@pytest.mark.parametrize("nonce", SM.NONCES)
def test_rate_boundary_rows_recover_their_sender(dev, nonce):
    """the 135-, 136- and 137-byte payloads: the envelope signature recovers From over keccak256(PayloadNoSig) computed by the oracle"""
    sk = SM.good_keys(5)[4]
    frm_want = O.address(O.pubkey(sk))
    for typ, height, round_, plen, _ in SM.ROW_CASES:
        if plen not in (135, 136, 137):
            continue
        ok, wire, pns, frm = _row(dev, nonce, sk, typ, height, round_, b"\x5a" * 32)
        e = WP.expected(wire)
        assert ok == 1 and e.status == WP.OK and len(pns) == plen and frm == frm_want
        assert O.recover_address(O.keccak256(pns), e.signature) == frm_want
        assert O.recover_address(b"\x5a" * 32, e.committed_seal) == frm_want


@pytest.mark.parametrize("key", SM.REFUSED_KEYS, ids=["0", "n", "2^256-1"])
def test_refused_keys_keep_the_length_and_carry_zeros(dev, key):
    for nonce in SM.NONCES:
        for typ, height, round_, plen, wlen in (SM.ROW_CASES[1], SM.ROW_CASES[5]):
            h = bytes(range(32, 64))
            want_wire, want_pns, _, _, want_ok = SM.expected(SM.b32(key), typ, height, round_, h, nonce)
            ok, wire, pns, frm = _row(dev, nonce, SM.b32(key), typ, height, round_, h)
            assert ok == 0 and not want_ok and frm == bytes(20)
            assert (len(pns), len(wire)) == (plen, wlen) and wire == want_wire and pns == want_pns
            e = WP.expected(wire)
            assert e.status == WP.OK and e.sender == bytes(20) and e.signature == bytes(65)


def test_length_function_at_every_varint_width(dev):
    """height and round independently at each of the ten varint widths (and 0: the field is omitted), both types"""
    h, frm, sig = bytes(32), bytes(20), bytes(65)
    for typ, body in ((W.PREPARE, W.prepare_body(h)), (W.COMMIT, W.commit_body(h, sig))):
        for height in SM.VARINT_EDGES:
            for round_ in SM.VARINT_EDGES:
                m = W.IbftMessage(view=W.View(height, round_), sender=frm, signature=sig, type=typ, payload=body)
                assert dev.dev_message_wire_len(typ, height, round_) == len(m.encode()), (typ, height, round_)
                assert dev.dev_message_payload_len(typ, height, round_) == len(m.payload_no_sig()), (typ, height, round_)
    assert dev.dev_message_wire_len(W.COMMIT, SM.M64, SM.M64) == 218   # IBFT_SIGN_MESSAGE_MAX
