"""ibft_verify_block_seals (chain sync) without a GPU: the C entry point refuses a NULL context before touching the
device, the binding declares and names the symbol, and a library without it makes the method raise GpuUnavailable."""
import ctypes as C

import numpy as np
import pytest


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
    mask = np.full(1, 7, np.uint64)
    tal = (V.Tally * 1)()
    assert L.ibft_verify_block_seals(None, V._p(bh), V._p(off), 1, V._p(sig), V._p(signer), None, V._p(mask), tal) == -1
    assert mask[0] == 7 and tal[0].quorum_lo == 0


def test_binding_names_the_symbol(V):
    L = V.load_library()
    assert "ibft_verify_block_seals" in V.EXPORTS
    assert hasattr(L, "ibft_verify_block_seals") and len(L.ibft_verify_block_seals.argtypes) == 9
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4   # a new entry point, no new version
    assert callable(V.BatchVerifier.verify_block_seals)


def test_library_without_the_symbol_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    with pytest.raises(V.GpuUnavailable):
        bv.verify_block_seals(np.zeros((1, 32), np.uint8), [0, 0], np.zeros((0, 65), np.uint8), np.zeros((0, 20), np.uint8))
