"""ibft_pipeline_stats_ex at the C boundary, without a device: the symbol is exported, declared with its four parameters and bound
as an optional export of ABI version 4 (ibft_pipeline_stats keeps its signature); a NULL context is refused and nothing is
written; the header names the pin, the binding and the Go shim name the call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ibft_pipeline_stats_ex"


@pytest.fixture(scope="module")
def lib():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    return V.load_library()


def header():
    return open(os.path.join(ROOT, "include", "ibftgpu.h")).read()


def params_of(name):
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", header(), flags=re.S), re.S)
    assert proto, name + " is not declared"
    return [" ".join(p.split()) for p in proto.group(1).split(",")]


def test_exported_declared_and_bound_as_optional(lib):
    import go_ibft_amd.verifier as V
    assert hasattr(lib, NAME)
    assert lib.ibft_version() == 4 == V.ABI_VERSION                       # no version step: an older build simply lacks the symbol
    assert NAME in V.EXPORTS and NAME in V.OPTIONAL_EXPORTS and NAME not in V.EXPORTS_SINCE
    assert params_of(NAME) == ["ibft_ctx *ctx", "uint32_t *side_tallies", "uint32_t *split_batches", "uint32_t *alt_verdicts"]
    assert params_of("ibft_pipeline_stats") == ["ibft_ctx *ctx", "uint32_t *side_tallies", "uint32_t *split_batches"]
    assert len(getattr(lib, NAME).argtypes) == 4 and len(lib.ibft_pipeline_stats.argtypes) == 3
    assert callable(V.BatchVerifier.alt_verdict_passes)
    assert "IBFT_ALT_VERDICT=0" in header()


def test_null_context_is_refused_and_nothing_is_written(lib):
    f = getattr(lib, NAME)
    v = [C.c_uint32(0x7777) for _ in range(3)]
    assert f(None, *(C.byref(x) for x in v)) == -1                        # IBFT_E_INVAL
    assert f(None, None, None, None) == -1
    assert [x.value for x in v] == [0x7777] * 3


def test_the_go_shim_names_it():
    go = open(os.path.join(ROOT, "shim", "go", "ibftgpu", "ibftgpu.go")).read()
    assert "C.ibft_pipeline_stats_ex(" in go and "func (c *Ctx) AltVerdictPasses(" in go
