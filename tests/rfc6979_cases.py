"""Shared rows and the independent derivation for the RFC 6979 signer tests (test_sign_rfc6979_host.py on the CPU,
test_gpu_sign_rfc6979.py on the device): the DRBG of RFC 6979 §3.2 restated with Python's own hmac / hashlib, the ten edge keys
of test_gpu_sign.py combined with the edge digests 0, 0xFF…FF, n, n + 1, n − 1, random rows behind them, and the five published
secp256k1 vectors of tests/golden/kats.json.  A case module, not a test file."""
import hashlib
import hmac
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
EDGE_KEYS = [1, 2, 3, N - 1, N - 2, (N - 1) // 2, (N + 1) // 2, 2**255 % N, 2**128, 2**128 - 1]
EDGE_DIGESTS = [0, 2**256 - 1, N, N + 1, N - 1]
BAD_KEYS = [0, N, N + 1, 2**256 - 1]


def b32(x: int) -> bytes:
    return x.to_bytes(32, "big")


def _mac(key: bytes, msg: bytes) -> bytes:
    return hmac.new(key, msg, hashlib.sha256).digest()


def candidates(sk: bytes, digest: bytes, m: int) -> list:
    """the first m nonce candidates (32 big-endian bytes each) of RFC 6979 §3.2 with bits2octets(h1) = h1 mod n, every
    candidate treated as unusable so that each next one comes after the reseed step (h.3)"""
    h1 = b32(int.from_bytes(digest, "big") % N)
    K, V = bytes(32), b"\x01" * 32
    for tag in (b"\x00", b"\x01"):
        K = _mac(K, V + tag + sk + h1)
        V = _mac(K, V)
    out = []
    for _ in range(m):
        V = _mac(K, V)
        out.append(V)
        K = _mac(K, V + b"\x00")
        V = _mac(K, V)
    return out


def rows(n: int, seed: int = 6979):
    """(sk u8[n, 32], digest u8[n, 32]): edge keys × edge digests first (50 rows), random usable keys and digests behind"""
    rng = np.random.default_rng(seed)
    pairs = [(k, d) for k in EDGE_KEYS for d in EDGE_DIGESTS]
    while len(pairs) < n:
        pairs.append((int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1, int.from_bytes(rng.bytes(32), "big")))
    pairs = pairs[:n]
    sk = np.frombuffer(b"".join(b32(k) for k, _ in pairs), np.uint8).reshape(-1, 32).copy()
    dg = np.frombuffer(b"".join(b32(d) for _, d in pairs), np.uint8).reshape(-1, 32).copy()
    return sk, dg


N_EDGE_ROWS = len(EDGE_KEYS) * len(EDGE_DIGESTS)


def vectors() -> list:
    """the five published RFC 6979 secp256k1 vectors: dicts with private_key, digest, sig65, address (bytes)"""
    with open(os.path.join(HERE, "golden", "kats.json")) as f:
        k = json.load(f)
    vs = [{f: bytes.fromhex(v[f]) for f in ("private_key", "digest", "sig65", "address")}
          for v in k["public_recover_vectors"] if "message" in v]
    assert len(vs) == 5
    return vs
