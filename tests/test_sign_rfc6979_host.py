"""The RFC 6979 nonce rule of the device signer, compiled for the host (csrc/host_sign_nonce_harness.hip: sha256_dev.h and
sign_dev.h as the gfx950 kernels compile them), against references that share no code with it: the compression function and
HMAC against Python's hashlib / hmac, the DRBG's candidates — the reseed step included — against the derivation of
rfc6979_cases.py, and the signing row against the five published vectors, the oracle's signer and oracle.pyref.sign with an
explicit nonce."""
import ctypes as C
import hashlib
import hmac
import struct

import numpy as np
import pytest

import rfc6979_cases as RC
from oracle import binding as O, pyref as R

IV = (0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19)


@pytest.fixture(scope="module")
def dev():
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_sign_nonce_harness())
    L.dev_sha256_compress.argtypes = [C.c_void_p, C.c_void_p]
    L.dev_sha256_compress.restype = None
    L.dev_hmac32.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p]
    L.dev_hmac32.restype = C.c_int
    L.dev_rfc6979_candidates.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p]
    L.dev_rfc6979_candidates.restype = None
    L.dev_sign_rfc6979.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p]
    L.dev_sign_rfc6979.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def rows300():
    return RC.rows(300)


def _pad(msg: bytes) -> bytes:
    """SHA-256's padding, done here: the device code never pads a free-form message"""
    return msg + b"\x80" + bytes((55 - len(msg)) % 64) + struct.pack(">Q", 8 * len(msg))


def _digest_by_compress(dev, msg: bytes) -> bytes:
    padded = _pad(msg)
    state = np.array(IV, np.uint32)
    for i in range(0, len(padded), 64):
        block = np.array(struct.unpack(">16I", padded[i:i + 64]), np.uint32)
        dev.dev_sha256_compress(state.ctypes.data, block.ctypes.data)
    return struct.pack(">8I", *state.tolist())


@pytest.mark.parametrize("msg", [b"abc", b"", bytes(range(55))], ids=["abc", "empty", "55_bytes"])
def test_compress_one_block(dev, msg):
    assert len(_pad(msg)) == 64
    assert _digest_by_compress(dev, msg) == hashlib.sha256(msg).digest()


def test_compress_two_blocks_chained(dev):
    msg = bytes(range(100, 156))   # 56 bytes: the padding no longer fits the first block
    assert len(_pad(msg)) == 128
    assert _digest_by_compress(dev, msg) == hashlib.sha256(msg).digest()


def _sign(dev, sk: bytes, dg: bytes, mask: int):
    sig, addr = C.create_string_buffer(b"\xee" * 65, 65), C.create_string_buffer(b"\xee" * 20, 20)
    ok = dev.dev_sign_rfc6979(sk, dg, mask, sig, addr)
    return ok, sig.raw, addr.raw


@pytest.mark.parametrize("length", [32, 33, 97])
def test_hmac_three_shapes(dev, length):
    rng = np.random.default_rng(length)
    fills = {"zero": lambda n: bytes(n), "ones": lambda n: b"\xff" * n, "random": lambda n: rng.bytes(n)}
    for kname, kf in fills.items():
        for mname, mf in fills.items():
            for tag in ((0, 1) if length == 97 else (0,)):
                key, msg = kf(32), bytearray(mf(length))
                if length > 32:
                    msg[32] = tag   # the byte behind V is 0x00 or 0x01 in every message RFC 6979 forms
                out = C.create_string_buffer(32)
                assert dev.dev_hmac32(key, bytes(msg), length, out) == 1
                assert out.raw == hmac.new(key, bytes(msg), hashlib.sha256).digest(), (kname, mname, tag)
    sentinel = C.create_string_buffer(b"\x5a" * 32, 32)
    assert dev.dev_hmac32(bytes(32), bytes(64), 64, sentinel) == 0 and sentinel.raw == b"\x5a" * 32   # not a shape it has


def test_candidates_with_reseed_match_python(dev, rows300):
    sk, dg = rows300
    for i in range(RC.N_EDGE_ROWS):
        out = C.create_string_buffer(96)
        dev.dev_rfc6979_candidates(sk[i].tobytes(), dg[i].tobytes(), 3, out)
        assert out.raw == b"".join(RC.candidates(sk[i].tobytes(), dg[i].tobytes(), 3)), i


def test_published_vectors(dev):
    for v in RC.vectors():
        ok, sig, addr = _sign(dev, v["private_key"], v["digest"], 0)
        assert ok == 1 and sig == v["sig65"] and addr == v["address"]


def test_python_derivation_reproduces_vectors_and_oracle(rows300):
    """the references agree with each other: hmac / hashlib nonce → pyref.sign = the oracle's RFC 6979 signer = the vectors"""
    for v in RC.vectors():
        k = int.from_bytes(RC.candidates(v["private_key"], v["digest"], 1)[0], "big")
        assert R.sign(int.from_bytes(v["private_key"], "big"), v["digest"], k) == v["sig65"] == O.sign_rfc6979(v["private_key"], v["digest"])
    sk, dg = rows300
    for i in list(range(0, RC.N_EDGE_ROWS, 7)) + [60, 299]:
        s, d = sk[i].tobytes(), dg[i].tobytes()
        k = int.from_bytes(RC.candidates(s, d, 1)[0], "big")
        assert 0 < k < RC.N
        assert R.sign(int.from_bytes(s, "big"), d, k) == O.sign_rfc6979(s, d), i


def test_sign_matches_oracle_on_300_rows(dev, rows300):
    sk, dg = rows300
    assert len(sk) == 300
    for i in range(300):
        s, d = sk[i].tobytes(), dg[i].tobytes()
        ok, sig, addr = _sign(dev, s, d, 0)
        assert ok == 1, i
        assert sig == O.sign_rfc6979(s, d), i
        assert addr == O.address(O.pubkey(s)), i


@pytest.mark.parametrize("mask,which", [(1, 1), (3, 2)])
def test_rejected_candidates_take_the_next_after_reseed(dev, rows300, mask, which):
    sk, dg = rows300
    for i in list(range(0, RC.N_EDGE_ROWS, 5)) + list(range(RC.N_EDGE_ROWS, RC.N_EDGE_ROWS + 10)):   # 20 rows, edge and random
        s, d = sk[i].tobytes(), dg[i].tobytes()
        k = int.from_bytes(RC.candidates(s, d, which + 1)[which], "big")
        assert 0 < k < RC.N
        ok, sig, addr = _sign(dev, s, d, mask)
        assert ok == 1 and sig == R.sign(int.from_bytes(s, "big"), d, k), i
        assert addr == O.address(O.pubkey(s)), i


@pytest.mark.parametrize("key", RC.BAD_KEYS, ids=["0", "n", "n+1", "2^256-1"])
def test_refused_keys_return_zero_bytes(dev, key):
    for mask in (0, 1):
        ok, sig, addr = _sign(dev, RC.b32(key), hashlib.sha256(b"refused").digest(), mask)
        assert ok == 0 and sig == bytes(65) and addr == bytes(20)
