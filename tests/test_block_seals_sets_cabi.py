"""The validator-set family (ibft_set_validator_sets[_u256], ibft_validator_sets_info) and the block calls that take a set per
block (ibft_verify_block_seals_sets, ibft_recover_block_seals_sets) without a GPU: the library exports and the header declares
the five symbols with the documented parameter lists, the C entry points refuse what is decided before a context is looked at
and leave every out buffer alone, the version stays 4, and the binding raises GpuUnavailable — from these methods only — against
a library without the symbols.  (Every check that needs a context — their order included — is in tests/test_gpu_block_seals_sets.py:
a context cannot be created without a device.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name → the parameter list of include/ibftgpu.h (types only, in order)
SIGNATURES = {
    "ibft_set_validator_sets": ["ibft_ctx *", "size_t", "const uint64_t *", "const uint32_t *", "const uint8_t *", "const uint64_t *"],
    "ibft_set_validator_sets_u256": ["ibft_ctx *", "size_t", "const uint64_t *", "const uint32_t *", "const uint8_t *", "const uint8_t *"],
    "ibft_validator_sets_info": ["ibft_ctx *", "uint32_t *", "uint32_t *", "uint64_t *"],
    "ibft_verify_block_seals_sets": ["ibft_ctx *", "const uint8_t *", "const uint32_t *", "const uint32_t *", "size_t", "const uint8_t *",
                                     "const uint8_t *", "const uint8_t *", "uint64_t *", "ibft_tally_t *"],
    "ibft_recover_block_seals_sets": ["ibft_ctx *", "const uint8_t *", "const uint32_t *", "const uint32_t *", "size_t", "const uint8_t *",
                                      "const uint8_t *", "uint8_t *", "int32_t *", "uint64_t *", "ibft_tally_t *"],
}
E_INVAL = -1


@pytest.fixture(scope="module")
def V():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    V.load_library()
    return V


def _header_params(header: str, name: str):
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/ibftgpu.h"
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        out.append(re.sub(r"\s*\w+$", "", p).strip())   # drop the parameter's name
    return out


def test_symbols_exported_with_the_headers_signatures(V):
    L = V.load_library()
    with open(os.path.join(ROOT, "include", "ibftgpu.h")) as f:
        header = f.read()
    for name, params in SIGNATURES.items():
        assert hasattr(L, name), name
        assert _header_params(header, name) == params, name
        assert name in V.EXPORTS and name in V.OPTIONAL_EXPORTS
        assert len(getattr(L, name).argtypes) == len(params), name
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4   # new entry points, no new version
    for m in ("set_validator_sets", "set_validator_sets_u256", "validator_sets_info", "verify_block_seals_sets", "recover_block_seals_sets"):
        assert callable(getattr(V.BatchVerifier, m))


def test_header_states_the_rules(V):
    with open(os.path.join(ROOT, "include", "ibftgpu.h")) as f:
        header = " ".join(f.read().split())
    for phrase in ("IBFT_VALSETS_BYTES_MAX", "a refused install leaves the previous one in place", "NOT a resident staged batch",
                   "never read the context's single set", "Out of scope: streamed"):
        assert phrase in header, phrase


def test_null_context_is_invalid_and_outputs_untouched(V):
    L = V.load_library()
    h = np.zeros((1, 32), np.uint8)
    sig = np.zeros((1, 65), np.uint8)
    who = np.zeros((1, 20), np.uint8)
    off = np.array([0, 1], np.uint32)
    bset = np.zeros(1, np.uint32)
    signer = np.full((1, 20), 0xA5, np.uint8)
    vidx = np.full(1, 77, np.int32)
    mask = np.full(1, 7, np.uint64)
    tal = (V.Tally * 1)()
    tal[0].power_lo = 0x1234
    n_sets, union = C.c_uint32(91), C.c_uint32(92)
    nbytes = C.c_uint64(93)

    def untouched():
        return ((signer == 0xA5).all() and vidx[0] == 77 and mask[0] == 7 and tal[0].power_lo == 0x1234 and tal[0].quorum_lo == 0
                and (n_sets.value, union.value, nbytes.value) == (91, 92, 93))

    p = V._p
    # NULL context, with every other argument in order …
    assert L.ibft_verify_block_seals_sets(None, p(h), p(off), p(bset), 1, p(sig), p(who), None, p(mask), tal) == E_INVAL
    assert L.ibft_recover_block_seals_sets(None, p(h), p(off), p(bset), 1, p(sig), None, p(signer), p(vidx), p(mask), tal) == E_INVAL
    # … and with NULL columns / out buffers
    assert L.ibft_verify_block_seals_sets(None, None, None, None, 1, None, None, None, None, None) == E_INVAL
    assert L.ibft_recover_block_seals_sets(None, None, None, None, 1, None, None, None, None, None, None) == E_INVAL
    assert L.ibft_validator_sets_info(None, C.byref(n_sets), C.byref(union), C.byref(nbytes)) == E_INVAL
    heights = np.zeros(1, np.uint64)
    soff = np.array([0, 1], np.uint32)
    power = np.ones(1, np.uint64)
    be = np.zeros((1, 32), np.uint8)
    assert L.ibft_set_validator_sets(None, 1, p(heights), p(soff), p(who), p(power)) == E_INVAL
    assert L.ibft_set_validator_sets_u256(None, 1, p(heights), p(soff), p(who), p(be)) == E_INVAL
    assert L.ibft_set_validator_sets(None, 0, None, None, None, None) == E_INVAL
    assert L.ibft_set_validator_sets_u256(None, 0, None, None, None, None) == E_INVAL
    assert untouched()


def test_library_without_the_symbols_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    one = [(np.zeros((1, 20), np.uint8), [1])]
    with pytest.raises(V.GpuUnavailable):
        bv.set_validator_sets(one)
    with pytest.raises(V.GpuUnavailable):
        bv.set_validator_sets_u256(one)
    with pytest.raises(V.GpuUnavailable):
        bv.validator_sets_info()
    with pytest.raises(V.GpuUnavailable):
        bv.verify_block_seals_sets(np.zeros((1, 32), np.uint8), [0, 0], [0], np.zeros((0, 65), np.uint8), np.zeros((0, 20), np.uint8))
    with pytest.raises(V.GpuUnavailable):
        bv.recover_block_seals_sets(np.zeros((1, 32), np.uint8), [0, 0], [0], np.zeros((0, 65), np.uint8))


def test_binding_flattens_a_family_into_the_c_columns(V):
    a0 = np.arange(40, dtype=np.uint8).reshape(2, 20)
    a1 = np.arange(60, dtype=np.uint8).reshape(3, 20) + 100
    h, off, a, pw = V.BatchVerifier._set_columns([(a0, [5, 6]), (7, a1, [1, 2, 3])], False)
    assert h.tolist() == [0, 7] and off.tolist() == [0, 2, 5] and off.dtype == np.uint32
    assert (a == np.concatenate([a0, a1])).all() and pw.tolist() == [5, 6, 1, 2, 3] and pw.dtype == np.uint64
    h, off, a, pw = V.BatchVerifier._set_columns([(a0, [1 << 200, 6])], True)
    assert pw.shape == (2, 32) and int.from_bytes(pw[0].tobytes(), "big") == 1 << 200
    with pytest.raises(ValueError):
        V.BatchVerifier._set_columns([(a0, [1])], False)
