"""IBFT_FLAG_CERT_DEDUP and ibft_cert_stats at the C boundary, without a device: the symbol is exported, declared with its five
parameters and bound as an optional export of ABI version 4; a NULL context is refused and nothing is written; the binding and
the Go shim name the flag and the call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ibft_cert_stats"


@pytest.fixture(scope="module")
def lib():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    return V.load_library()


def header():
    return open(os.path.join(ROOT, "include", "ibftgpu.h")).read()


def test_exported_declared_and_bound_as_optional(lib):
    import go_ibft_amd.verifier as V
    assert hasattr(lib, NAME)
    assert lib.ibft_version() == 4 == V.ABI_VERSION                       # no version step: an older build simply lacks the symbol
    assert NAME in V.EXPORTS and NAME in V.OPTIONAL_EXPORTS and NAME not in V.EXPORTS_SINCE
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, re.sub(r"/\*.*?\*/", "", header(), flags=re.S), re.S)
    assert proto, "not declared"
    params = [" ".join(p.split()) for p in proto.group(1).split(",")]
    assert params == ["ibft_ctx *ctx", "uint32_t *rows", "uint32_t *judged_rows", "uint32_t *verdict_rows", "uint32_t *unplaced_rows"]
    assert len(getattr(lib, NAME).argtypes) == 5
    assert callable(V.BatchVerifier.cert_stats)


def test_the_flag():
    import go_ibft_amd.verifier as V
    m = re.search(r"#define\s+IBFT_FLAG_CERT_DEDUP\s+(\w+)", header())
    assert m and int(m.group(1).rstrip("u"), 0) == 4 == V.FLAG_CERT_DEDUP
    assert V.FLAG_CERT_DEDUP not in (V.FLAG_STRICT_LOW_S, V.FLAG_PUBKEY_CACHE)
    hdr = header()
    for word in ("IBFT_CERT_DEDUP=0|1", "bit for bit the flag-off output", "ibft_last_dispatch, ibft_last_kernel_ms and", "IBFT_CERT_DEDUP_SLOTS"):
        assert word in hdr, word


def test_null_context_is_refused_and_nothing_is_written(lib):
    f = getattr(lib, NAME)
    v = [C.c_uint32(0x7777) for _ in range(4)]
    assert f(None, *(C.byref(x) for x in v)) == -1                        # IBFT_E_INVAL
    assert f(None, None, None, None, None) == -1
    assert [x.value for x in v] == [0x7777] * 4


def test_the_go_shim_names_them():
    go = open(os.path.join(ROOT, "shim", "go", "ibftgpu", "ibftgpu.go")).read()
    assert "FlagCertDedup = uint32(C.IBFT_FLAG_CERT_DEDUP)" in go and "cfg.flags |= C.IBFT_FLAG_CERT_DEDUP" in go
    assert "C.ibft_cert_stats(" in go and "func (c *Ctx) CertStats(" in go
