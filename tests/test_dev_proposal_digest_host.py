"""The absorb-with-spliced-tail routines behind proposal_digest_kernel (ibft_proposal_hashes, the _raw block calls), compiled for the
host (csrc/host_proposal_digest_harness.hip): the lane form — keccak::hash_range_tail_dwords, called directly — and the wavefront
form — cw::sponge_message with a tail, on the 64-coroutine lockstep emulator of csrc/wave_emul.h — against the oracle.

The eight bytes of the round are not in memory behind the proposal; the absorb step splices them in.  Where they fall is decided by
len mod 136 (the rate): inside a block (≤ 128), across two blocks (129 … 135), in front of a block that holds nothing but the
padding (len + 8 ≡ 0), with the two padding bits in one byte (len + 8 ≡ 135).  Every length 0 … 300 holds each of those at least
twice; 1 000, 4 095 and 65 536 + k repeat them behind many whole blocks — 65 536 ≡ 120 (mod 136), so k = 0 is "inside", k = 7 is
len + 8 ≡ 135, k = 8 is len + 8 ≡ 0, k = 9 and k = 15 are the first and the last straddling length.  Each at start addresses
0 … 3 mod 4 (the dword loads are realigned with funnel shifts) and with rounds 0, 1 and 2⁶⁴ − 1."""
import ctypes as C
import random

import numpy as np
import pytest

from go_ibft_amd import build as B
from oracle import binding as OB
from oracle import pyref

LENGTHS = list(range(0, 301)) + [1000, 4095] + [65536 + k for k in (0, 7, 8, 9, 15)]
ROUNDS = [0, 1, 2**64 - 1]
SLACK = 16  # what the routines may read past the proposal: ≤ 7 bytes (the staged buffer carries 256)


@pytest.fixture(scope="module")
def dev():
    return C.CDLL(B.build_proposal_digest_harness())


@pytest.fixture(scope="module")
def material():
    """one random byte string per length, and its expected digests per round from the oracle"""
    rng = random.Random(1136)
    raws = {n: rng.randbytes(n) for n in LENGTHS}
    want = {(n, r): OB.proposal_hash(raws[n], r) for n in LENGTHS for r in ROUNDS}
    return raws, want


def _placed(data: bytes, lead: int):
    """data at (a 16-byte aligned address) + lead; the bytes around it are NOT zero, so a routine that takes a byte too many
    from memory — in front of the proposal, behind it, or in place of the round — computes another digest"""
    buf = np.full(len(data) + 32 + SLACK + lead, 0xA5, dtype=np.uint8)
    base = (-buf.ctypes.data) % 16 + lead
    buf[base:base + len(data)] = np.frombuffer(data, dtype=np.uint8)
    return buf, base


def _run(fn, data: bytes, lead: int, rnd: int) -> bytes:
    buf, base = _placed(data, lead)
    out = np.zeros(32, dtype=np.uint8)
    fn(C.c_void_p(buf.ctypes.data + base), C.c_uint32(len(data)), C.c_uint64(rnd), out.ctypes.data_as(C.c_void_p))
    return out.tobytes()


def test_the_case_set_holds_every_position_of_the_round():
    mods = {n % 136 for n in LENGTHS}
    assert set(range(136)) <= mods                                     # every position of the tail within a block
    big = {n % 136 for n in LENGTHS if n > 65000}
    assert {120, 127, 128, 129, 135} <= big                            # … and the four kinds behind 481 whole blocks
    for n in (0, 135, 136 - 8, 2 * 136 - 8, 136 - 9, 129, 265):
        assert n in LENGTHS


def test_oracles_agree(material):
    raws, want = material
    for n in (0, 1, 127, 128, 129, 135, 136, 264, 300, 1000):
        for r in ROUNDS:
            assert pyref.proposal_hash(raws[n], r) == want[(n, r)]
    assert OB.proposal_hash(b"", 0) == OB.keccak256(bytes(8))


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_spliced_tail_every_length_offset_and_round(dev, material, form):
    raws, want = material
    fn = dev.pdh_lane if form == "lane" else dev.pdh_wave
    fn.restype = None
    bad = []
    for n in LENGTHS:
        for lead in range(4):
            for r in ROUNDS:
                if _run(fn, raws[n], lead, r) != want[(n, r)]:
                    bad.append((n, lead, r))
    assert not bad, f"{form} form: {len(bad)} of {len(LENGTHS) * 12} cases differ from the oracle, first {bad[:8]}"


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_a_flipped_bit_anywhere_changes_the_digest(dev, form):
    """the digest depends on every byte of the proposal and of the round — nothing is dropped at a block or dword seam"""
    fn = dev.pdh_lane if form == "lane" else dev.pdh_wave
    fn.restype = None
    rng = random.Random(77)
    for n in (131, 136, 270):
        raw = rng.randbytes(n)
        base = _run(fn, raw, 1, 5)
        assert base == OB.proposal_hash(raw, 5)
        for i in range(n):
            alt = raw[:i] + bytes([raw[i] ^ 0x10]) + raw[i + 1:]
            assert _run(fn, alt, 1, 5) == OB.proposal_hash(alt, 5) != base
        for bit in range(64):
            assert _run(fn, raw, 1, 5 ^ (1 << bit)) == OB.proposal_hash(raw, 5 ^ (1 << bit)) != base
