"""ibft_proposal_hashes / ibft_verify_block_seals_raw / ibft_recover_block_seals_raw (chain sync from the proposals) without a GPU:
the library exports and the header declares the three symbols with the arities of the issue, the version stays 4, a NULL context is
IBFT_E_INVAL before anything else is looked at and no out buffer is written, the binding names the symbols, flattens a list of
proposals into the columns of the C ABI and raises GpuUnavailable against a library without them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibft_proposal_hashes", "ibft_verify_block_seals_raw", "ibft_recover_block_seals_raw")
E_INVAL = -1


@pytest.fixture(scope="module")
def V():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    V.load_library()
    return V


def test_symbols_exported_and_declared(V):
    L = V.load_library()
    with open(os.path.join(ROOT, "include", "ibftgpu.h")) as f:
        header = f.read()
    for name, argc in zip(NAMES, (6, 12, 13)):
        assert hasattr(L, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        assert len(m.group(1).split(",")) == argc        # the prototype of the header …
        assert len(getattr(L, name).argtypes) == argc    # … and the binding's
        assert name in V.EXPORTS and name in V.OPTIONAL_EXPORTS
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4   # new entry points, no new version
    for m in ("proposal_hashes", "verify_block_seals_raw", "recover_block_seals_raw"):
        assert callable(getattr(V.BatchVerifier, m))
    # the header says what the issue asks it to say
    assert "IBFT_PROPOSAL_LANES" in header and "IBFT_PROPOSAL_BYTES_MAX" in header
    assert re.search(r"no streamed \(submit / collect\) form of these calls", header)


def test_null_context_is_invalid_and_outputs_untouched(V):
    L = V.load_library()
    raw = np.frombuffer(b"abc", np.uint8).copy()
    roff = np.array([0, 3], np.uint32)
    rnd = np.array([1], np.uint64)
    soff = np.array([0, 1], np.uint32)
    sig = np.zeros((1, 65), np.uint8)
    f20 = np.zeros((1, 20), np.uint8)
    out = np.full((1, 32), 0xA5, np.uint8)
    signer = np.full((1, 20), 0xA5, np.uint8)
    vidx = np.full(1, 77, np.int32)
    mask = np.full(1, 7, np.uint64)
    tal = (V.Tally * 1)()
    tal[0].power_lo = 0x1234
    p = V._p

    def untouched():
        return ((out == 0xA5).all() and (signer == 0xA5).all() and vidx[0] == 77 and mask[0] == 7 and tal[0].power_lo == 0x1234
                and tal[0].quorum_lo == 0)

    assert L.ibft_proposal_hashes(None, p(raw), p(roff), p(rnd), 1, p(out)) == E_INVAL
    assert L.ibft_proposal_hashes(None, None, None, None, 0, None) == E_INVAL
    assert L.ibft_proposal_hashes(None, None, None, None, 1, None) == E_INVAL
    assert L.ibft_verify_block_seals_raw(None, p(raw), p(roff), p(rnd), p(soff), 1, p(sig), p(f20), None, p(out), p(mask), tal) == E_INVAL
    assert L.ibft_verify_block_seals_raw(None, None, None, None, None, 1, None, None, None, None, None, None) == E_INVAL
    assert L.ibft_recover_block_seals_raw(None, p(raw), p(roff), p(rnd), p(soff), 1, p(sig), None, p(out), p(signer), p(vidx),
                                          p(mask), tal) == E_INVAL
    assert L.ibft_recover_block_seals_raw(None, None, None, None, None, 1, None, None, None, None, None, None, None) == E_INVAL
    assert untouched()


def test_proposal_columns_flattens_lists_and_keeps_given_columns(V):
    raw, off, rnd = V.proposal_columns([b"ab", b"", b"cde"], [1, 2, 2**64 - 1])
    assert raw.tobytes() == b"abcde" and off.tolist() == [0, 2, 2, 5] and off.dtype == np.uint32
    assert rnd.dtype == np.uint64 and rnd.tolist() == [1, 2, 2**64 - 1]
    raw, off, rnd = V.proposal_columns([], [])
    assert off.tolist() == [0] and len(rnd) == 0 and raw.size >= 1     # (a pointer the C side never follows)
    col = np.frombuffer(b"abcde", np.uint8).copy()
    raw, off, rnd = V.proposal_columns((col, [0, 2, 5]), [7, 8])
    assert raw.ctypes.data == col.ctypes.data                            # not copied: a pinned column stays pinned
    assert off.tolist() == [0, 2, 5]
    raw, off, rnd = V.proposal_columns((b"ab", b"cd"), [0, 0])           # a tuple of two proposals is a list of two proposals
    assert off.tolist() == [0, 2, 4]
    with pytest.raises(ValueError):
        V.proposal_columns([b"a", b"b"], [1])


def test_library_without_the_symbols_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    with pytest.raises(V.GpuUnavailable):
        bv.proposal_hashes([b"x"], [0])
    with pytest.raises(V.GpuUnavailable):
        bv.verify_block_seals_raw([b"x"], [0], [0, 0], np.zeros((0, 65), np.uint8), np.zeros((0, 20), np.uint8))
    with pytest.raises(V.GpuUnavailable):
        bv.recover_block_seals_raw([b"x"], [0], [0, 0], np.zeros((0, 65), np.uint8))
