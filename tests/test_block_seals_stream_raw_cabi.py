"""The streamed submits from proposals and bare seals (ibft_block_seals_submit_raw, ibft_recover_block_seals_submit,
ibft_recover_block_seals_submit_raw) with ibft_block_seals_collect_ex / _pending_ex, without a GPU: the five symbols are
exported, declared in the header, bound in verifier.py and in the Go shim; the version stays 4; a NULL context and NULL
required arguments are refused with IBFT_E_INVAL before any device is touched and nothing is written."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibft_block_seals_submit_raw", "ibft_recover_block_seals_submit", "ibft_recover_block_seals_submit_raw",
         "ibft_block_seals_collect_ex", "ibft_block_seals_pending_ex")
ARGC = (9, 6, 8, 6, 5)
METHODS = ("block_seals_submit_raw", "recover_block_seals_submit", "recover_block_seals_submit_raw", "block_seals_collect_ex",
           "block_seals_pending_ex")


@pytest.fixture(scope="module")
def V():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    V.load_library()
    return V


def test_symbols_exported_and_bound(V):
    L = V.load_library()
    for name, argc in zip(NAMES, ARGC):
        assert name in V.EXPORTS and name in V.OPTIONAL_EXPORTS
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == argc
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4   # new entry points, no new version
    for m in METHODS:
        assert callable(getattr(V.BatchVerifier, m))
    assert (V.BatchVerifier.BATCH_RECOVER, V.BatchVerifier.BATCH_RAW) == (1, 2)


def test_header_declares_them():
    with open(os.path.join(ROOT, "include", "ibftgpu.h")) as f:
        h = f.read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(ibft_ctx \*ctx", h, re.M), name
    assert re.search(r"#define IBFT_BATCH_RECOVER 1u", h) and re.search(r"#define IBFT_BATCH_RAW 2u", h)
    # the synchronous siblings point at their streamed forms (only the _sets calls have none)
    assert "Streamed form: ibft_recover_block_seals_submit" in h
    assert "Streamed forms: ibft_block_seals_submit_raw and" in h
    assert h.count("no streamed (submit / collect) form") == 1


def test_go_shim_binds_them():
    with open(os.path.join(ROOT, "shim", "go", "ibftgpu", "ibftgpu.go")) as f:
        g = f.read()
    for name in NAMES:
        assert "C." + name + "(" in g, name


def test_null_context_is_invalid(V):
    L = V.load_library()
    off = np.array([0, 1], np.uint32)
    raw = np.zeros(8, np.uint8)
    roff = np.array([0, 8], np.uint32)
    rnd = np.zeros(1, np.uint64)
    bh = np.zeros((1, 32), np.uint8)
    sig = np.zeros((1, 65), np.uint8)
    signer = np.zeros((1, 20), np.uint8)
    p = V._p
    assert L.ibft_block_seals_submit_raw(None, p(raw), p(roff), p(rnd), p(off), 1, p(sig), p(signer), None) == -1
    assert L.ibft_recover_block_seals_submit(None, p(bh), p(off), 1, p(sig), None) == -1
    assert L.ibft_recover_block_seals_submit_raw(None, p(raw), p(roff), p(rnd), p(off), 1, p(sig), None) == -1
    mask = np.full(1, 7, np.uint64)
    out_h = np.full((1, 32), 9, np.uint8)
    out_s = np.full((1, 20), 9, np.uint8)
    out_v = np.full(1, 5, np.int32)
    tal = (V.Tally * 1)()
    tal[0].power_lo = 0x1234
    assert L.ibft_block_seals_collect_ex(None, p(out_h), p(out_s), p(out_v), p(mask), tal) == -1
    assert mask[0] == 7 and tal[0].power_lo == 0x1234 and tal[0].quorum_lo == 0
    assert (out_h == 9).all() and (out_s == 9).all() and out_v[0] == 5
    a, b, c, k = C.c_uint32(11), C.c_uint32(12), C.c_uint32(13), C.c_uint32(14)
    assert L.ibft_block_seals_pending_ex(None, C.byref(a), C.byref(b), C.byref(c), C.byref(k)) == -1
    assert (a.value, b.value, c.value, k.value) == (11, 12, 13, 14)


def test_library_without_the_symbols_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    sig0 = np.zeros((0, 65), np.uint8)
    with pytest.raises(V.GpuUnavailable):
        bv.block_seals_submit_raw([b"x"], [0], [0, 0], sig0, np.zeros((0, 20), np.uint8))
    with pytest.raises(V.GpuUnavailable):
        bv.recover_block_seals_submit(np.zeros((1, 32), np.uint8), [0, 0], sig0)
    with pytest.raises(V.GpuUnavailable):
        bv.recover_block_seals_submit_raw([b"x"], [0], [0, 0], sig0)
    with pytest.raises(V.GpuUnavailable):
        bv.block_seals_collect_ex()
    with pytest.raises(V.GpuUnavailable):
        bv.block_seals_pending_ex()
