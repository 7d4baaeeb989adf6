"""ibft_block_seals_submit / _collect / _pending (streamed chain sync) without a GPU: the C entry points refuse a NULL
context before touching the device and leave the out buffers alone, the binding declares and names the three symbols, and
a library without them makes the three methods raise GpuUnavailable."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("ibft_block_seals_submit", "ibft_block_seals_collect", "ibft_block_seals_pending")


@pytest.fixture(scope="module")
def V():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    V.load_library()
    return V


def test_null_context_is_invalid(V):
    L = V.load_library()
    off = np.array([0, 1], np.uint32)
    bh = np.zeros((1, 32), np.uint8)
    sig = np.zeros((1, 65), np.uint8)
    signer = np.zeros((1, 20), np.uint8)
    assert L.ibft_block_seals_submit(None, V._p(bh), V._p(off), 1, V._p(sig), V._p(signer), None) == -1
    mask = np.full(1, 7, np.uint64)
    tal = (V.Tally * 1)()
    tal[0].power_lo = 0x1234
    assert L.ibft_block_seals_collect(None, V._p(mask), tal) == -1
    assert mask[0] == 7 and tal[0].power_lo == 0x1234 and tal[0].quorum_lo == 0
    a, b, c = C.c_uint32(11), C.c_uint32(12), C.c_uint32(13)
    assert L.ibft_block_seals_pending(None, C.byref(a), C.byref(b), C.byref(c)) == -1
    assert (a.value, b.value, c.value) == (11, 12, 13)


def test_binding_names_the_symbols(V):
    L = V.load_library()
    for name, argc in zip(NAMES, (7, 3, 4)):
        assert name in V.EXPORTS and name in V.OPTIONAL_EXPORTS
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == argc
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4   # new entry points, no new version
    for m in ("block_seals_submit", "block_seals_collect", "block_seals_pending"):
        assert callable(getattr(V.BatchVerifier, m))


def test_library_without_the_symbols_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    with pytest.raises(V.GpuUnavailable):
        bv.block_seals_submit(np.zeros((1, 32), np.uint8), [0, 0], np.zeros((0, 65), np.uint8), np.zeros((0, 20), np.uint8))
    with pytest.raises(V.GpuUnavailable):
        bv.block_seals_collect()
    with pytest.raises(V.GpuUnavailable):
        bv.block_seals_pending()
