"""ibft_recover_seals / ibft_recover_block_seals (bare committed seals: who signed?) without a GPU: the library exports and the
header declares the two symbols, the C entry points refuse NULL arguments before touching the device and leave the out buffers
alone, the binding names the symbols and raises GpuUnavailable against a library without them, and the emitting kernels' shared
epilogue (recover_dev.h: emit_row), compiled for the host, equals oracle.recover_address + ValSet.index on honest rows, on
every rejection class, on a non-member's valid signature and on a pre-flagged row.  Its sibling for the rows that CLAIM a signer
(recover_dev.h: claim_row, the decision of the other two modes of the same kernels) is held to oracle.verify_seals the same way."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import binding as B, pyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibft_recover_seals", "ibft_recover_block_seals")
STRICT_LOW_S = 1   # IBFT_FLAG_STRICT_LOW_S


@pytest.fixture(scope="module")
def V():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    V.load_library()
    return V


@pytest.fixture(scope="module")
def dev():
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_host_harness())
    L.dev_emit_row.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_char_p, C.POINTER(C.c_int32)]
    L.dev_emit_row.restype = C.c_int
    L.dev_claim_row.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_char_p, C.POINTER(C.c_int32)]
    L.dev_claim_row.restype = C.c_int
    return L


def test_symbols_exported_and_declared(V):
    L = V.load_library()
    with open(os.path.join(ROOT, "include", "ibftgpu.h")) as f:
        header = f.read()
    for name, argc in zip(NAMES, (9, 10)):
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in V.EXPORTS and name in V.OPTIONAL_EXPORTS
        assert len(getattr(L, name).argtypes) == argc
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4   # new entry points, no new version
    assert V.FLAG_STRICT_LOW_S == STRICT_LOW_S
    for m in ("recover_seals", "recover_block_seals"):
        assert callable(getattr(V.BatchVerifier, m))


def test_null_arguments_are_invalid_and_outputs_untouched(V):
    L = V.load_library()
    h = np.zeros((1, 32), np.uint8)
    sig = np.zeros((1, 65), np.uint8)
    off = np.array([0, 1], np.uint32)
    signer = np.full((1, 20), 0xA5, np.uint8)
    vidx = np.full(1, 77, np.int32)
    mask = np.full(1, 7, np.uint64)
    tal = (V.Tally * 1)()
    tal[0].power_lo = 0x1234

    def untouched():
        return (signer == 0xA5).all() and vidx[0] == 77 and mask[0] == 7 and tal[0].power_lo == 0x1234 and tal[0].quorum_lo == 0

    # NULL context, with every other argument in order and with NULL columns / out buffers
    assert L.ibft_recover_seals(None, V._p(h), V._p(sig), None, 1, V._p(signer), V._p(vidx), V._p(mask), tal) == -1
    assert L.ibft_recover_seals(None, None, None, None, 1, None, None, None, None) == -1
    assert L.ibft_recover_block_seals(None, V._p(h), V._p(off), 1, V._p(sig), None, V._p(signer), V._p(vidx), V._p(mask), tal) == -1
    assert L.ibft_recover_block_seals(None, None, None, 1, None, None, None, None, None, None) == -1
    assert untouched()


def test_library_without_the_symbols_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    with pytest.raises(V.GpuUnavailable):
        bv.recover_seals(np.zeros((1, 32), np.uint8), np.zeros((1, 65), np.uint8))
    with pytest.raises(V.GpuUnavailable):
        bv.recover_block_seals(np.zeros((1, 32), np.uint8), [0, 0], np.zeros((0, 65), np.uint8))


# ---- the shared epilogue on the host ---------------------------------------------------------------------------------
def _emit(dev, digest, sig, flags, pre, addrs):
    out = C.create_string_buffer(20)
    vi = C.c_int32(12345)
    bit = dev.dev_emit_row(digest, sig, flags, pre, addrs.ctypes.data, len(addrs), out, C.byref(vi))
    return out.raw, vi.value, bit


def _expect(vs, digest, sig, flags, pre):
    """(address bytes, validator index, bit) from the oracle alone"""
    a = None if pre else B.recover_address(digest, sig, flags)
    if a is None:
        return bytes(20), -1, 0
    vi = set_index(vs, a)
    return a, vi, 1 if vi >= 0 else 0


def set_index(vs, addr20):
    """ValSet.index answers in the oracle's own (sorted) order; the library numbers the validators in the caller's order,
    a repeated address keeping its first place: membership from the oracle, the position from the caller's list."""
    if vs.index(addr20) < 0:
        return -1
    seen = []
    for a in vs.addrs:
        a = a.tobytes()
        if a == addr20:
            return len(seen)
        if a not in seen:
            seen.append(a)
    raise AssertionError("the oracle names a member that is not in its own list")


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    sks = [(int.from_bytes(rng.bytes(32), "big") % (R.N - 1) + 1).to_bytes(32, "big") for _ in range(n)]
    addrs = np.frombuffer(b"".join(B.address(B.pubkey(sk)) for sk in sks), np.uint8).reshape(n, 20).copy()
    return sks, addrs


def test_epilogue_honest_rows(dev):
    sks, addrs = _keys(9, 3)
    vs = B.ValSet(addrs, np.ones(len(addrs), np.uint64))
    rng = np.random.default_rng(4)
    for i, sk in enumerate(sks):
        d = rng.bytes(32)
        sig = B.sign(sk, d)
        got = _emit(dev, d, sig, 0, 0, addrs)
        assert got == _expect(vs, d, sig, 0, 0)
        assert got == (addrs[i].tobytes(), i, 1)


def test_epilogue_rejection_classes_non_member_and_pre_flag(dev):
    sks, addrs = _keys(5, 11)
    vs = B.ValSet(addrs, np.ones(len(addrs), np.uint64))
    outsider, _ = _keys(1, 12)
    rng = np.random.default_rng(13)
    d = rng.bytes(32)
    sig = B.sign(sks[2], d)
    n32 = R.N.to_bytes(32, "big")

    def with_(r=None, s=None, v=None):
        b = bytearray(sig)
        if r is not None:
            b[0:32] = r
        if s is not None:
            b[32:64] = s
        if v is not None:
            b[64] = v
        return bytes(b)

    assert pow(5 ** 3 + 7, (R.P - 1) // 2, R.P) != 1      # x = 5 is on no curve point
    rejected = {"r = 0": with_(r=bytes(32)), "r = n": with_(r=n32), "r > n": with_(r=b"\xff" * 32), "s = 0": with_(s=bytes(32)),
                "s = n": with_(s=n32), "s > n": with_(s=b"\xff" * 32), "v = 2": with_(v=2), "v = 27": with_(v=27),
                "no square root": with_(r=(5).to_bytes(32, "big"))}
    for name, bad in rejected.items():
        for flags in (0, STRICT_LOW_S):
            assert B.recover_address(d, bad, flags) is None, name
            assert _emit(dev, d, bad, flags, 0, addrs) == (bytes(20), -1, 0), name

    # high s (the other recovery id): the same key — accepted by default, nothing recovered under the strict flag
    s_int = int.from_bytes(sig[32:64], "big")
    low = sig if s_int <= R.N // 2 else with_(s=(R.N - s_int).to_bytes(32, "big"), v=sig[64] ^ 1)
    low_s = int.from_bytes(low[32:64], "big")
    high = bytes(low[0:32]) + (R.N - low_s).to_bytes(32, "big") + bytes([low[64] ^ 1])
    for flags in (0, STRICT_LOW_S):
        assert _emit(dev, d, low, flags, 0, addrs) == (addrs[2].tobytes(), 2, 1)
        assert _emit(dev, d, low, flags, 0, addrs) == _expect(vs, d, low, flags, 0)
        assert _emit(dev, d, high, flags, 0, addrs) == _expect(vs, d, high, flags, 0)
    assert _emit(dev, d, high, 0, 0, addrs) == (addrs[2].tobytes(), 2, 1)
    assert _emit(dev, d, high, STRICT_LOW_S, 0, addrs) == (bytes(20), -1, 0)

    # a non-member's valid signature: the address is emitted, no index, no bit
    osig = B.sign(outsider[0], d)
    oaddr = B.address(B.pubkey(outsider[0]))
    assert _emit(dev, d, osig, 0, 0, addrs) == (oaddr, -1, 0) == _expect(vs, d, osig, 0, 0)
    # a member's signature over ANOTHER digest recovers some other address: whatever the oracle says
    d2 = rng.bytes(32)
    assert _emit(dev, d2, sig, 0, 0, addrs) == _expect(vs, d2, sig, 0, 0)
    assert _emit(dev, d2, sig, 0, 0, addrs)[1:] == (-1, 0)
    # a pre-flagged row: zeros, -1, 0 — although its signature is a member's
    assert _emit(dev, d, sig, 0, 1, addrs) == (bytes(20), -1, 0)
    # a validator whose address is twenty zero bytes is not "found" by a row that recovered nothing
    with_zero = np.concatenate([np.zeros((1, 20), np.uint8), addrs])
    assert _emit(dev, d, with_(v=2), 0, 0, with_zero) == (bytes(20), -1, 0)
    assert _emit(dev, d, sig, 0, 1, with_zero) == (bytes(20), -1, 0)
    assert _emit(dev, d, sig, 0, 0, with_zero) == (addrs[2].tobytes(), 3, 1)
    # a repeated address keeps its first index (ibft_set_validators / the oracle's ValSet)
    rep = np.concatenate([addrs, addrs[1:2]])
    vs_rep = B.ValSet(rep, np.ones(len(rep), np.uint64))
    s1 = B.sign(sks[1], d)
    assert _emit(dev, d, s1, 0, 0, rep) == _expect(vs_rep, d, s1, 0, 0)


# ---- the claimed-signer form of the same epilogue ----------------------------------------------------------------------
def _claim(dev, digest, sig, flags, pre, addrs, claimed):
    vi = C.c_int32(12345)
    bit = dev.dev_claim_row(digest, sig, flags, pre, addrs.ctypes.data, len(addrs), claimed, C.byref(vi))
    return vi.value, bit


def test_claimed_signer_decision_equals_the_oracle(dev):
    sks, addrs = _keys(6, 21)
    vs = B.ValSet(addrs, np.ones(len(addrs), np.uint64))
    outsider, oaddrs = _keys(1, 22)
    rng = np.random.default_rng(23)
    d, d2 = rng.bytes(32), rng.bytes(32)

    def check(digest, sig, claimed, flags=0, pre=0):
        exp = int(B.verify_seals(vs, np.frombuffer(digest, np.uint8), np.frombuffer(sig, np.uint8), np.frombuffer(claimed, np.uint8),
                                 np.array([pre], np.uint8), flags=flags)[0])
        vi, bit = _claim(dev, digest, sig, flags, pre, addrs, claimed)
        assert vi == set_index(vs, claimed) and bit == exp, (vi, bit, exp)
        return bit

    for i, sk in enumerate(sks):                                                   # honest rows
        assert check(d, B.sign(sk, d), addrs[i].tobytes()) == 1
    sig = B.sign(sks[2], d)
    me, other = addrs[2].tobytes(), addrs[3].tobytes()
    assert check(d, sig, other) == 0                                               # a stolen seal: valid, but not the claimed member's
    assert check(d2, sig, me) == 0                                                 # over another digest
    assert check(d, sig, me, pre=1) == 0                                           # pre-flagged although valid
    osig, oaddr = B.sign(outsider[0], d), oaddrs[0].tobytes()
    assert check(d, osig, oaddr) == 0 and _claim(dev, d, osig, 0, 0, addrs, oaddr) == (-1, 0)   # a non-member, signed correctly
    assert check(d, osig, me) == 0                                                 # ... and claiming to be a member
    for bad in (bytes(32) + sig[32:], sig[:32] + bytes(32) + sig[64:], sig[:64] + b"\x02", sig[:64] + bytes([sig[64] ^ 1])):
        assert check(d, bad, me) == 0                                              # r = 0, s = 0, v = 2, the other recovery id
    s_int = int.from_bytes(sig[32:64], "big")                                      # the high-s twin under both policies
    twin = sig[:32] + (R.N - s_int).to_bytes(32, "big") + bytes([sig[64] ^ 1])
    high = twin if s_int <= R.N // 2 else sig
    assert check(d, high, me, flags=0) == 1 and check(d, high, me, flags=STRICT_LOW_S) == 0
    # a validator whose address is twenty zero bytes: a row that recovered nothing does not become "its" row
    with_zero = np.concatenate([np.zeros((1, 20), np.uint8), addrs])
    assert _claim(dev, d, sig[:64] + b"\x02", 0, 0, with_zero, bytes(20)) == (0, 0)
