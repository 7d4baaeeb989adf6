"""ibft_sign_envelopes_wire (the device signer for PREPREPARE / ROUND_CHANGE envelopes around given bodies) without a GPU: the
library exports and the header declares the symbol with its sixteen parameters, the binding names it (as an optional export: no new
version), the C entry point refuses a NULL context before touching the device and leaves the out buffers alone, the binding
refuses an unknown rule and a library without the symbol, and simulate.py offers make_round_change_round without importing the
oracle."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ibft_sign_envelopes_wire"
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
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["ibft_ctx *ctx", "const uint8_t *sk32", "const uint8_t *type", "const uint64_t *height", "const uint64_t *round",
                      "const uint8_t *body", "size_t body_bytes", "const uint32_t *body_at", "const uint32_t *body_len", "size_t n",
                      "uint32_t nonce", "uint8_t *out_wire", "size_t wire_cap", "uint32_t *out_off", "uint8_t *out_from20",
                      "uint8_t *out_ok"]
    doc = header[header.index("The signing side two layers up"):m.start()]
    assert "NOT for a production validator's key" in doc and "NO staged seal batch" in doc   # the warning and the staged state
    assert "same or overlapping ranges" in " ".join(doc.replace("*", " ").split())                # why (at, len) columns, not offsets
    assert "IBFT_CERT_CLASS_DIGEST_BY_HOST" in doc and "IBFT_ENVELOPE_LANES" in doc and "IBFT_PROPOSAL_BYTES_MAX" in doc
    assert NAME in V.EXPORTS and NAME in V.OPTIONAL_EXPORTS
    assert len(getattr(L, NAME).argtypes) == 16
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4   # a new entry point, no new version


def test_null_context_is_invalid_and_outputs_untouched(V):
    L = V.load_library()
    fn = getattr(L, NAME)
    sk = np.ones((1, 32), np.uint8)
    ty = np.zeros(1, np.uint8)
    hh = np.ones(1, np.uint64)
    rr = np.zeros(1, np.uint64)
    body = np.zeros(8, np.uint8)
    at = np.zeros(1, np.uint32)
    ln = np.full(1, 8, np.uint32)
    wire = np.full(256, 0xA5, np.uint8)
    off = np.full(2, 0xA5A5A5A5, np.uint32)
    frm = np.full((1, 20), 0xA5, np.uint8)
    ok = np.full(1, 0xA5, np.uint8)
    p = V._p
    for nonce in (0, 1, 7):
        assert fn(None, p(sk), p(ty), p(hh), p(rr), p(body), 8, p(at), p(ln), 1, nonce, p(wire), 256, p(off), p(frm), p(ok)) == E_INVAL
        assert fn(None, p(sk), p(ty), p(hh), p(rr), p(body), 8, p(at), p(ln), 1, nonce, p(wire), 0, p(off), None, None) == E_INVAL
        assert fn(None, None, None, None, None, None, 8, None, None, 1, nonce, None, 0, None, None, None) == E_INVAL
        assert fn(None, None, None, None, None, None, 0, None, None, 0, nonce, None, 0, None, None, None) == E_INVAL
    assert (wire == 0xA5).all() and (off == 0xA5A5A5A5).all() and (frm == 0xA5).all() and ok[0] == 0xA5


def test_binding_refuses_unknown_rule_and_old_library(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = None
    cols = (np.zeros((1, 32), np.uint8), 0, 1, 0, b"\x12\x00", 0, 2)
    with pytest.raises(ValueError):
        bv.sign_envelopes(*cols, nonce="rfc-6979")
    for nonce in ("keccak", "rfc6979"):
        with pytest.raises(V.GpuUnavailable):
            bv.sign_envelopes(*cols, nonce=nonce)
    assert list(inspect.signature(V.BatchVerifier.sign_envelopes).parameters) == \
        ["self", "sk32", "type", "height", "round", "body", "body_at", "body_len", "nonce"]


def test_simulate_offers_the_round_change_round_and_imports_no_oracle():
    with open(os.path.join(ROOT, "go-ibft_amd", "simulate.py")) as f:
        src = f.read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M)
    import go_ibft_amd.simulate as S
    assert callable(S.make_round_change_round)
    sig = inspect.signature(S.make_round_change_round)
    assert list(sig.parameters) == ["bv", "n", "seed", "height", "prepared_round", "new_round", "distinct", "byzantine", "nonce", "raw_len"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["seed"], d["height"], d["prepared_round"], d["new_round"], d["distinct"], d["byzantine"], d["nonce"], d["raw_len"]) == \
        (1, 5, 1, 2, False, False, "keccak", 1024)
