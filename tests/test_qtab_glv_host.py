"""The GLV table form of the warm path (IBFT_QTAB_FORM=glv) on the CPU, through csrc/host_qtab_glv_harness.hip: the exact
device source of the recoding helper, of the table build and of the two warm forms that run on one lane and on one wavefront
(the latter through the 64-coroutine emulator).

  * the recoding of a half reconstructs it and keeps the digit ranges, read by position and from a shift register alike;
  * table entries equal big-integer arithmetic (oracle/pyref);
  * the verdicts of both forms equal the oracle's recover-and-compare over the rows of
    test_dev_arith_host.py::test_warm_path_verify_equals_recover_and_compare."""
import ctypes as C
import random

import numpy as np
import pytest

import row_scalar_cases as RC
from oracle import pyref as R

N = R.N
WINDOWS = 16
SLOT_BYTES = 174080


def b32(x):
    return x.to_bytes(32, "big")


@pytest.fixture(scope="module")
def qgh():
    import go_ibft_amd.build as B
    h = C.CDLL(B.build_qtab_glv_harness())
    h.qgh_init_gtab()
    h.qgh_slot_dwords.restype = C.c_uint32
    h.qgh_points.restype = C.c_uint32
    return h


def _split(qgh, u2):
    k1, k2, neg = C.create_string_buffer(16), C.create_string_buffer(16), (C.c_int * 3)()
    qgh.qgh_split(b32(u2), k1, k2, neg)
    assert neg[2] == 0, hex(u2)                                 # both halves below 2^128
    return int.from_bytes(k1.raw, "little"), int.from_bytes(k2.raw, "little"), bool(neg[0]), bool(neg[1])


def _recode(qgh, k, lam, neg):
    digit, index, flags = (C.c_int32 * WINDOWS)(), (C.c_uint32 * WINDOWS)(), (C.c_uint32 * WINDOWS)()
    assert qgh.qgh_recode(k.to_bytes(16, "little"), int(lam), int(neg), digit, index, flags) == 0, hex(k)
    return list(digit), list(index), list(flags)


def _check_half(qgh, k):
    """digits of k < 2^128: ranges, reconstruction, and what the helper says about each (entry, non-zero, ·β, negate)"""
    want = []                                                    # the recoding restated: b = k + Σ_{i<15} 128·256^i
    b = k + sum(128 << (8 * i) for i in range(15))
    for i in range(15):
        want.append(((b >> (8 * i)) & 255) - 128)
    want.append(b >> 120)
    assert all(-128 <= d <= 127 for d in want[:15]) and 0 <= want[15] <= 256
    assert sum(d << (8 * i) for i, d in enumerate(want)) == k
    for lam in (False, True):
        for neg in (False, True):
            digit, index, flags = _recode(qgh, k, lam, neg)
            assert digit == want, (hex(k), lam, neg)
            for w, d in enumerate(want):
                assert index[w] == 128 * w + max(abs(d), 1) - 1 and index[w] < 2176
                assert flags[w] == (d != 0) | (lam << 1) | (((d < 0) != neg) << 2), (hex(k), w, lam, neg)


def test_geometry(qgh):
    assert qgh.qgh_points() == 15 * 128 + 256 == 2176
    assert qgh.qgh_slot_dwords() * 4 == SLOT_BYTES and 655360 / SLOT_BYTES > 3.76


def test_recoding_reconstructs_the_half_and_keeps_the_digit_ranges(qgh):
    fixed = [0, 1, (1 << 120) - 1, 1 << 120, (1 << 128) - 1,
             int.from_bytes(b"\x7f" * 16, "little"), int.from_bytes(b"\x80" * 16, "little"), int.from_bytes(b"\xff" * 16, "little")]
    for k in fixed:
        _check_half(qgh, k)
    rng = random.Random(2201)
    u2s = [1, RC.LAMBDA, N - 1, N - RC.LAMBDA] + [rng.randrange(1, N) for _ in range(10000)]
    for u2 in u2s:
        k1, k2, n1, n2 = _split(qgh, u2)
        s1, s2 = RC.split(u2)                                    # the device's split in exact integers
        assert (k1, n1 and k1 != 0) == (abs(s1), s1 < 0) and (k2, n2 and k2 != 0) == (abs(s2), s2 < 0), hex(u2)
        assert ((-k1 if n1 else k1) + (-k2 if n2 else k2) * RC.LAMBDA) % N == u2
        for k in (k1, k2):
            _check_half(qgh, k)
    assert _split(qgh, RC.LAMBDA)[:2] == (0, 1) and _split(qgh, 1)[:2] == (1, 0)


def _pub_point(pub):
    return (int.from_bytes(pub[:32], "big"), int.from_bytes(pub[32:], "big"))


def _table(qgh, pub):
    t = np.zeros(SLOT_BYTES // 4, dtype=np.uint32)
    qgh.qgh_build_qtab(pub, t.ctypes.data_as(C.c_void_p))
    return t


def test_table_entries_against_big_integers(qgh, oracle):
    rng = np.random.default_rng(2202)
    for _ in range(3):
        sk = b32(int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1)
        pub = oracle.pubkey(sk)
        t = _table(qgh, pub)
        Q = _pub_point(pub)
        for w, m in ((0, 1), (0, 128), (7, 64), (14, 128), (15, 1), (15, 255), (15, 256)):
            o = C.create_string_buffer(64)
            qgh.qgh_entry(t.ctypes.data_as(C.c_void_p), w, m, o)
            assert o.raw == R.pub_bytes(R.pt_mul(m << (8 * w), Q)), (w, m)
        assert t.reshape(-1, 20).any(axis=1).all()               # no entry is ∞ (none was left zeroed)


def test_verdicts_equal_recover_and_compare(qgh, oracle):
    """the rows of test_dev_arith_host.py::test_warm_path_verify_equals_recover_and_compare: honest rows, every corruption
    kind, both low-s policies — the lane form and the emulated wavefront form"""
    rng = np.random.default_rng(14)
    for key in range(2):
        sk = b32(int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1)
        pub, addr = oracle.pubkey(sk), oracle.address(oracle.pubkey(sk))
        t = _table(qgh, pub)
        tp = t.ctypes.data_as(C.c_void_p)
        accepted = 0
        for i in range(48):
            d = rng.bytes(32)
            sig = oracle.sign(sk, d)
            if i % 5 == 1: sig = sig[:64] + bytes([sig[64] ^ 1])
            if i % 7 == 2: sig = rng.bytes(64) + bytes([i & 1])
            if i % 11 == 3: sig = bytes(32) + sig[32:]
            if i % 13 == 4: sig = sig[:32] + b32(N) + sig[64:]
            if i % 17 == 5: sig = sig[:64] + b"\x02"
            if i % 19 == 6:
                s_ = int.from_bytes(sig[32:64], "big")
                sig = sig[:32] + b32(N - s_) + bytes([sig[64] ^ 1])
            if i % 23 == 7: sig = oracle.sign(b32(4242 + i), d)          # valid, but another key
            for fl in (0, 1):
                rec = oracle.recover_address(d, sig, fl)
                want = int(rec is not None and rec == addr)
                accepted += want
                assert qgh.qgh_verify_lane(tp, d, sig, fl) == want, ("lane", key, i, fl)
                ok = np.zeros(64, dtype=np.int32)
                qgh.qgh_verify_wave(tp, d, sig, fl, ok.ctypes.data_as(C.c_void_p))
                assert (ok == want).all(), ("wave", key, i, fl)
        assert accepted > 40
