"""Shared cases of the message signer (ibft_sign_messages_wire / sign_message_dev.h): the row cases with the lengths
oracle/wire.py gives them, the keys, the batches, and the expected bytes of a row built with nothing but the oracle."""
import numpy as np

from oracle import binding as O, wire as W

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
M64 = 2**64 - 1
PREPARE, COMMIT = W.PREPARE, W.COMMIT

# (type, height, round, len(PayloadNoSig), len(wire)); the COMMIT rows of 135, 136 and 137 bytes sit on the Keccak rate
ROW_CASES = [
    (PREPARE, 0, 0, 62, 129),
    (PREPARE, 16384, 128, 69, 136),
    (PREPARE, M64, M64, 84, 151),
    (COMMIT, 0, 0, 129, 196),
    (COMMIT, 16384, 1, 135, 202),
    (COMMIT, 16384, 128, 136, 203),
    (COMMIT, 2097152, 128, 137, 204),
    (COMMIT, M64, 0, 140, 207),
    (COMMIT, M64, M64, 151, 218),
]
# every varint width: 0 (field omitted), then the smallest and the largest value of 1 … 10 bytes
VARINT_EDGES = [0, 1] + [v for k in range(1, 10) for v in (2**(7 * k) - 1, 2**(7 * k))] + [M64]
REFUSED_KEYS = [0, N, 2**256 - 1]
NONCES = ("keccak", "rfc6979")
BATCH_SIZES = (1, 64, 65, 130)
SUFFIXES = (None, b"\x02", bytes(range(1, 65)))   # identity, KECCAK_SUFFIX of 1 byte and of 64 bytes


def b32(x: int) -> bytes:
    return int(x).to_bytes(32, "big")


def good_keys(count: int, seed: int = 7) -> list:
    """1, n − 1, then SplitMix keys from simulate.secret_keys"""
    import go_ibft_amd.simulate as S
    sm = S.secret_keys(seed, max(count, 2))
    return ([b32(1), b32(N - 1)] + [sm[i].tobytes() for i in range(len(sm))])[:count]


def _sign(nonce: str, sk: bytes, digest: bytes) -> bytes:
    return O.sign(sk, digest) if nonce == "keccak" else O.sign_rfc6979(sk, digest)


def expected(sk: bytes, typ: int, height: int, round_: int, h: bytes, nonce: str, suffix: bytes | None = None):
    """(wire bytes, PayloadNoSig, From, seal or None, ok) of one row, from the oracle alone"""
    key = int.from_bytes(sk, "big")
    ok = 0 < key < N
    frm = O.address(O.pubkey(sk)) if ok else bytes(20)
    seal = None
    if typ == COMMIT:
        seal = _sign(nonce, sk, h if suffix is None else O.keccak256(h + suffix)) if ok else bytes(65)
        body = W.commit_body(h, seal)
    else:
        body = W.prepare_body(h)
    m = W.IbftMessage(view=W.View(height, round_), sender=frm, type=typ, payload=body)
    pns = m.payload_no_sig()
    m.signature = _sign(nonce, sk, O.keccak256(pns)) if ok else bytes(65)
    return m.encode(), pns, frm, seal, ok


def batch(n: int, seed: int = 11):
    """n rows as columns (sk u8[n,32], type u8[n], height u64[n], round u64[n], hash u8[n,32]).  The row cases cycle; n = 130
    is laid out as one wavefront all PREPARE, one all COMMIT and a partial third with both types alternating, and carries the
    three refused keys inside wavefronts of good ones (rows 5, 70 and 129)."""
    prep = [c for c in ROW_CASES if c[0] == PREPARE]
    comm = [c for c in ROW_CASES if c[0] == COMMIT]
    keys = good_keys(n, seed)
    rng = np.random.default_rng(seed)
    sk = np.zeros((n, 32), np.uint8)
    typ = np.zeros(n, np.uint8)
    height = np.zeros(n, np.uint64)
    round_ = np.zeros(n, np.uint64)
    hs = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32).copy()
    for i in range(n):
        if n == 130:
            case = prep[i % len(prep)] if i < 64 else comm[i % len(comm)] if i < 128 else (prep, comm)[i % 2][i % 3]
        else:
            case = ROW_CASES[(i * 5 + n) % len(ROW_CASES)]
        sk[i] = np.frombuffer(keys[i], np.uint8)
        typ[i], height[i], round_[i] = case[0], case[1], case[2]
    if n == 130:
        for i, k in zip((5, 70, 129), REFUSED_KEYS):
            sk[i] = np.frombuffer(b32(k), np.uint8)
    return sk, typ, height, round_, hs


def expected_batch(cols, nonce: str, suffix: bytes | None = None):
    """[(wire, pns, from, seal, ok)] per row of a batch"""
    sk, typ, height, round_, hs = cols
    return [expected(sk[i].tobytes(), int(typ[i]), int(height[i]), int(round_[i]), hs[i].tobytes(), nonce, suffix)
            for i in range(len(typ))]
