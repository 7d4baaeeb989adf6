"""The rows pair (wave_fe_dev.h: recover_pubkey_row<…, PAIR = true> + recover_helper_row) on the CPU.

The helper wavefront's half (r⁻¹, u1, u2, GLV split, u1·G) runs first, then the main wavefront's half, on one emulated
wavefront each with the hand-over in plain memory — sequential here, concurrent on the device.  Every row must answer
as the oracle does and exactly as the single-wavefront form (recover_pubkey_row) does.  Test infrastructure only.
"""
import ctypes

import numpy as np
import pytest

from go_ibft_amd import build as B


@pytest.fixture(scope="module")
def wh():
    lib = ctypes.CDLL(B.build_wave_harness())
    lib.wvh_init_gtab()
    return lib


def _run(fn, hs, sigs):
    addr = np.zeros((64, 20), dtype=np.uint8)
    ok = np.zeros(64, dtype=np.int32)
    fn(b"".join(hs), b"".join(sigs), addr.ctypes.data_as(ctypes.c_void_p), ok.ctypes.data_as(ctypes.c_void_p))
    for row in range(4):
        lanes = slice(16 * row, 16 * row + 16)
        assert (ok[lanes] == ok[16 * row]).all() and (addr[lanes] == addr[16 * row]).all(), "lanes of a row disagree"
    return [(bool(ok[16 * r]), addr[16 * r].tobytes()) for r in range(4)]


def _check(wh, oracle, hs, sigs, tag=""):
    pair = _run(wh.wvh_recover4_pair, hs, sigs)
    single = _run(wh.wvh_recover4, hs, sigs)
    for row in range(4):
        want = oracle.recover_address(hs[row], sigs[row])
        assert pair[row][0] == (want is not None), (tag, row)
        if want is not None:
            assert pair[row][1] == want, (tag, row)
        assert pair[row] == single[row], (tag, row)


def _rand_scalar(rng, n):
    return int.from_bytes(rng.bytes(32), "big") % (n - 1) + 1


def test_rows_pair_honest_and_invalid_rows(wh, oracle):
    from oracle import pyref
    n = pyref.N
    rng = np.random.default_rng(4096)
    for _ in range(2):
        hs, sigs = [], []
        for i in range(4):
            sk = _rand_scalar(rng, n).to_bytes(32, "big")
            h = rng.bytes(32)
            sg = bytearray(oracle.sign(sk, h))
            if i == 2:      # high s, other recovery id: the same key
                sg[32:64] = (n - int.from_bytes(sg[32:64], "big")).to_bytes(32, "big")
                sg[64] ^= 1
            hs.append(h)
            sigs.append(bytes(sg))
        _check(wh, oracle, hs, sigs, "honest")
    # a good row, a tiny u2, x = 5 (not on the curve), a zero digest (u1 = 0)
    sk = _rand_scalar(rng, n).to_bytes(32, "big")
    h0 = rng.bytes(32)
    x, _ = pyref.pt_mul(_rand_scalar(rng, n), pyref.G)
    s0 = oracle.sign(sk, h0)
    hs = [h0, rng.bytes(32), rng.bytes(32), bytes(32)]
    sigs = [s0, (x % n).to_bytes(32, "big") + ((17 * x) % n).to_bytes(32, "big") + b"\x01",
            (5).to_bytes(32, "big") + s0[32:64] + b"\x00", oracle.sign(sk, bytes(32))]
    _check(wh, oracle, hs, sigs, "mixed")


def test_rows_pair_crafted_scalars(wh, oracle):
    """u2 tiny / near 2^64, 2^128, n (digit-32 carries, both signs of the split), u1 = 0, and the rare closing additions:
    u1·G = u2·R (a doubling), u1·G = −u2·R (the key would be ∞: rejected)."""
    from oracle import pyref
    n = pyref.N
    rng = np.random.default_rng(77)
    rows = []
    for i, t in enumerate([1, 16, 2**64 - 1, 2**64, 2**128 - 1, n - 1, n - 2**64, int("8" * 64, 16) % n]):
        k = _rand_scalar(rng, n)
        x, y = pyref.pt_mul(k, pyref.G)
        r = x % n
        z = 0 if i < 2 else int.from_bytes(rng.bytes(32), "big")
        rows.append((z.to_bytes(32, "big"), r.to_bytes(32, "big") + ((t * r) % n).to_bytes(32, "big") + bytes([y & 1])))
    for sign in (1, -1):
        for flip in (0, 1):
            k = _rand_scalar(rng, n)
            x, y = pyref.pt_mul(k, pyref.G)
            r, s = x % n, _rand_scalar(rng, n)
            rows.append((((sign * s * k) % n).to_bytes(32, "big"),
                         r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([(y & 1) ^ flip])))
    assert len(rows) % 4 == 0
    for g in range(0, len(rows), 4):
        _check(wh, oracle, [h for h, _ in rows[g:g + 4]], [sg for _, sg in rows[g:g + 4]], f"crafted {g}")


def test_rows_pair_byzantine_rows(wh, oracle):
    """one row of every corruption kind of the synthetic workload, four to an emulated wavefront"""
    from oracle import workload as W
    r = W.make_round(64, 8191, byzantine=True)
    picked, seen = [], set()
    for i, kind in enumerate(r.kinds):
        if kind not in seen and not r.pre_flags[i]:
            seen.add(kind)
            picked.append(i)
    assert len(seen) >= 8
    honest = [i for i in range(r.n) if i not in picked]
    while len(picked) % 4:
        picked.append(honest.pop())
    for g in range(0, len(picked), 4):
        rows = picked[g:g + 4]
        _check(wh, oracle, [r.hash32[i].tobytes() for i in rows], [r.seal65[i].tobytes() for i in rows],
               ",".join(str(r.kinds[i]) for i in rows))
