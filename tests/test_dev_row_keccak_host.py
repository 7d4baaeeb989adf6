"""The row-layout address hash of the row kernels (csrc/keccak_row_dev.h: the Keccak state of one 64-byte key spread over five
lanes of a row, θ by DPP, π through wave-private scratch), compiled for the host and run on the 64-coroutine lockstep
wavefront emulator (csrc/wave_emul.h) — the exact source the gfx950 kernels wrap — against the lane-layout
keccak::address_from_xy and the oracle's Keccak.  The emulator aborts the process when lanes disagree on a cross-lane
primitive, so every call here also checks that the control flow around them is wave-uniform."""
import ctypes as C
import random

import numpy as np
import pytest

from go_ibft_amd import build as B
from oracle import binding as OB

GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8


@pytest.fixture(scope="module")
def dev():
    return C.CDLL(B.build_row_keccak_harness())


def row_addresses(dev, keys):
    """keys: 64-byte X‖Y strings, four per wavefront (the last wavefront padded) → each key's address, after checking that
    all sixteen lanes of its row hold the same one"""
    n = len(keys)
    waves = (n + 3) // 4
    xy = np.zeros((waves * 4, 64), dtype=np.uint8)
    for i, k in enumerate(keys):
        xy[i] = np.frombuffer(k, dtype=np.uint8)
    out = np.zeros((waves * 4, 16, 20), dtype=np.uint8)
    dev.row_keccak_addresses(xy.ctypes.data_as(C.c_void_p), waves, out.ctypes.data_as(C.c_void_p))
    assert (out == out[:, :1, :]).all(), "the lanes of a row disagree"
    return [out[i, 0].tobytes() for i in range(n)]


def lane_address(dev, key):
    out = np.zeros(20, dtype=np.uint8)
    dev.lane_keccak_address(C.c_char_p(key), out.ctypes.data_as(C.c_void_p))
    return out.tobytes()


def check(dev, keys):
    got = row_addresses(dev, keys)
    for k, g in zip(keys, got):
        assert g == OB.keccak256(k)[12:], k.hex()
        assert g == lane_address(dev, k), k.hex()


def test_generator_point_is_the_address_of_key_one(dev):
    key = GX.to_bytes(32, "big") + GY.to_bytes(32, "big")
    assert row_addresses(dev, [key])[0] == bytes.fromhex("7E5F4552091A69125d5DfCb7b8C2659029395Bdf")
    check(dev, [key])


def test_all_zero_and_all_ones(dev):
    check(dev, [bytes(64), b"\xff" * 64, bytes(32) + b"\xff" * 32, b"\xff" * 32 + bytes(32)])


def test_every_single_bit(dev):
    check(dev, [(1 << b).to_bytes(64, "big") for b in range(512)])


def test_random_inputs(dev):
    rng = random.Random(1207)
    check(dev, [bytes(rng.randrange(256) for _ in range(64)) for _ in range(400)])


def test_rows_are_independent(dev):
    """four different keys in one wavefront, in every order of a few: a row's answer depends on nothing but its own key
    (lane 15 of a row never leaks into lane 0 of the next, a row's scratch is its own)"""
    rng = random.Random(99)
    keys = [GX.to_bytes(32, "big") + GY.to_bytes(32, "big"), bytes(64), b"\xff" * 64, bytes(rng.randrange(256) for _ in range(64))]
    want = [OB.keccak256(k)[12:] for k in keys]
    assert len(set(want)) == 4
    for perm in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [2, 0, 3, 1], [0, 0, 1, 1], [3, 3, 3, 0]):
        assert row_addresses(dev, [keys[i] for i in perm]) == [want[i] for i in perm], perm


def test_scratch_fits_the_window_table(dev):
    assert dev.row_keccak_scratch_dwords() <= 32 * 64   # wv::ROW_TAB_SLOTS × 64: what the row kernels hand over
