"""ibft_sign_seals_ex (the device signer under a chosen nonce rule) without a GPU: the library exports and the header declares
the symbol with its eight parameters and the two IBFT_SIGN_NONCE_* constants, the binding names it (as an optional export: no
new version), and the C entry point refuses a NULL context before touching the device and leaves the out buffers alone."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ibft_sign_seals_ex"
E_INVAL = -1


@pytest.fixture(scope="module")
def V():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    V.load_library()
    return V


def test_symbol_exported_declared_and_bound(V):
    L = V.load_library()
    with open(os.path.join(ROOT, "include", "ibftgpu.h")) as f:
        header = f.read()
    assert hasattr(L, NAME)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", header)
    assert m, "the header declares it"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 8 and params[4] == "uint32_t nonce"
    assert re.search(r"^#define\s+IBFT_SIGN_NONCE_KECCAK\s+0u\b", header, re.M)
    assert re.search(r"^#define\s+IBFT_SIGN_NONCE_RFC6979\s+1u\b", header, re.M)
    assert NAME in V.EXPORTS and NAME in V.OPTIONAL_EXPORTS
    assert len(getattr(L, NAME).argtypes) == 8
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4   # a new entry point, no new version
    assert V.SIGN_NONCES == {"keccak": 0, "rfc6979": 1}


def test_null_context_is_invalid_and_outputs_untouched(V):
    L = V.load_library()
    sk = np.ones((1, 32), np.uint8)
    h = np.zeros((1, 32), np.uint8)
    sig = np.full((1, 65), 0xA5, np.uint8)
    signer = np.full((1, 20), 0xA5, np.uint8)
    ok = np.full(1, 0xA5, np.uint8)
    for nonce in (0, 1, 7):
        assert L.ibft_sign_seals_ex(None, V._p(sk), V._p(h), 1, nonce, V._p(sig), V._p(signer), V._p(ok)) == E_INVAL
        assert L.ibft_sign_seals_ex(None, None, None, 1, nonce, None, None, None) == E_INVAL
        assert L.ibft_sign_seals_ex(None, None, None, 0, nonce, None, None, None) == E_INVAL
    assert (sig == 0xA5).all() and (signer == 0xA5).all() and ok[0] == 0xA5


def test_binding_refuses_unknown_rule_and_old_library(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = None
    with pytest.raises(ValueError):
        bv.sign_seals(np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8), nonce="rfc-6979")
    with pytest.raises(V.GpuUnavailable):
        bv.sign_seals(np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8), nonce="rfc6979")
