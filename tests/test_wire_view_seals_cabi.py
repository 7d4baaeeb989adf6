"""The C ABI of ibft_verify_messages_wire_views and ibft_wire_seal_stats: exported with the header's parameter lists and bound,
ibft_wire_view_t untouched (the seal rule is pad[0], named by IBFT_WIRE_VIEW_SEAL_RULE), a NULL context refused with nothing
written, a library without the symbol.  What needs a context is marked gpu: every refusal of ibft_verify_senders_wire_views, in
its order, with the same answer from both calls, and out_seal NULL."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_wire_views_cabi as VT
import wire_view_seals_model as SM

ROOT = VT.ROOT
NAME, VIEWS, STATS = "ibft_verify_messages_wire_views", "ibft_verify_senders_wire_views", "ibft_wire_seal_stats"
PARAMS = VT.PARAMS + ["uint64_t *"]

V = VT.V       # the module fixture: the library built and loaded


def _params(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/ibftgpu.h"
    return [re.sub(r"\s*\w+$", "", " ".join(p.split())).strip() for p in m.group(1).split(",")]


def test_symbols_exported_with_the_headers_signatures(V):
    L = V.load_library()
    header = VT._header()
    assert _params(header, NAME) == PARAMS
    assert _params(header, STATS) == ["ibft_ctx *", "uint32_t *", "uint32_t *"]
    for name, n_args in ((NAME, len(PARAMS)), (STATS, 3)):
        assert hasattr(L, name) and name in V.EXPORTS and name in V.OPTIONAL_EXPORTS
        assert len(getattr(L, name).argtypes) == n_args
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4          # new entry points, no new version
    assert callable(V.BatchVerifier.verify_messages_wire_views) and callable(V.BatchVerifier.wire_seal_stats)


def test_the_struct_keeps_its_layout_and_the_rule_is_pad_0(V):
    header = VT._header()
    m = re.search(r"#define\s+IBFT_WIRE_VIEW_SEAL_RULE\s+(\d+)", header)
    assert m and int(m.group(1)) == 0 == V.WIRE_VIEW_SEAL_RULE == SM.SEAL_RULE
    assert re.search(r"uint8_t pad\[5\];", re.search(r"typedef struct \{([^}]*)\} ibft_wire_view_t;", header).group(1))
    assert V.WIRE_VIEW.fields["pad"][1] == 35 and V.WIRE_VIEW["pad"].shape == (5,) and V.WIRE_VIEW.itemsize == 128
    VT.test_struct_layout_agrees_everywhere(V)                   # field for field what the views call's test pins
    src = open(os.path.join(ROOT, "go-ibft_amd", "csrc", "ibftgpu.hip")).read()
    assert "static_assert(IBFT_WIRE_VIEW_SEAL_RULE == wviews::SEAL_RULE" in src


class _Outs(VT._Outs):
    def __init__(self, V, n_sets=2):
        super().__init__(V, n_sets)
        self.seal = np.full(2, 3, np.uint64)

    def args(self, p):
        return super().args(p) + (p(self.seal),)

    def untouched(self):
        return super().untouched() and (self.seal == 3).all()


def test_null_context_is_invalid_and_outputs_untouched(V):
    L, p, o = V.load_library(), V._p, _Outs(V)
    wire, off = np.zeros(8, np.uint8), np.array([0, 4, 8], np.uint32)
    assert SM.check_call(False, 2, True, True, 4, True, True, 64, True, True) == SM.E_INVAL
    assert getattr(L, NAME)(None, p(wire), p(off), 2, 4, *o.args(p)) == SM.E_INVAL
    assert getattr(L, NAME)(None, None, None, 2, 0, *([None] * 10)) == SM.E_INVAL
    a, b = C.c_uint32(5), C.c_uint32(6)
    assert getattr(L, STATS)(None, C.byref(a), C.byref(b)) == SM.E_INVAL and (a.value, b.value) == (5, 6)
    assert o.untouched()


def test_library_without_the_symbols_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    with pytest.raises(V.GpuUnavailable):
        bv.verify_messages_wire_views(b"", [0], 4)
    with pytest.raises(V.GpuUnavailable):
        bv.wire_seal_stats()


@pytest.mark.gpu
def test_refusals_are_the_views_calls_in_its_order(V):
    L, p = V.load_library(), V._p
    seals, views = getattr(L, NAME), getattr(L, VIEWS)
    bv = V.BatchVerifier(max_rows=64)
    try:
        h = bv._h
        o = _Outs(V)
        a = o.args(p)
        wire, off = np.zeros(8, np.uint8), np.array([0, 4, 8], np.uint32)
        down, many = np.array([0, 4, 2], np.uint32), np.zeros(66, np.uint32)
        addrs = np.arange(60, dtype=np.uint8).reshape(3, 20)
        state = dict(have_family=False, have_map=False)

        def both(want, *front, args=None):
            """the same refusal from both calls, and the one the model names"""
            args = a if args is None else args
            assert seals(h, *front, *args) == views(h, *front, *args[:9]) == want

        def want(n=2, have_off=True, have_mask=True, cap=4, offsets_ok=True, bytes_ok=True):
            return SM.check_call(True, n, have_off, have_mask, cap, offsets_ok, bytes_ok, 64, **state)

        def sweep():
            both(want(have_off=False), p(wire), None, 2, 4)
            both(want(have_mask=False), p(wire), p(off), 2, 4, args=(None,) + a[1:])
            both(want(cap=0), p(wire), p(off), 2, 0)
            both(want(n=65, cap=0), None, p(many), 65, 0)                                      # before IBFT_E_TOOBIG
            both(want(offsets_ok=False), p(wire), p(down), 2, 4)
            both(want(bytes_ok=False), None, p(off), 2, 4)
            both(want(n=65), None, p(many), 65, 4)
            assert want(have_off=False) == want(cap=0) == want(offsets_ok=False) == SM.E_INVAL and want(n=65) == SM.E_TOOBIG
            assert o.untouched()

        sweep()
        both(want(), p(wire), p(off), 2, 4)                                                      # no family
        assert want() == SM.E_NOVALSET
        bv.set_validator_sets([(addrs[:2], [1, 2]), (addrs[1:], [3, 4])])
        state["have_family"] = True
        both(want(), p(wire), p(off), 2, 4)                                                      # a family, no map
        assert want() == SM.E_NOVALSET and o.untouched()
        bv.set_height_sets([1, 5, 9], [0, 1])
        state["have_map"] = True
        sweep()
        # every out buffer but the mask may be NULL, out_seal among them; garbage rows are NEEDS_HOST rows: no view, no seal
        mask = np.full(1, 7, np.uint64)
        assert seals(h, p(wire), p(off), 2, 10**9, p(mask), *([None] * 9)) == want(cap=10**9) == SM.E_OK
        assert mask[0] == 0 and bv.wire_seal_stats() == (0, 0)
        out = bv.verify_messages_wire_views(wire.tobytes(), off, 1)
        assert not out[0].any() and out[5].tolist() == [-1, -1] and not out[6].any() and out[8] == 0 and not out[9].any()
        # n = 0 with views_cap = 0 is legal
        nv = C.c_uint32(91)
        assert seals(h, None, p(np.zeros(1, np.uint32)), 0, 0, *([None] * 8), C.byref(nv), None) == want(n=0, cap=0, have_mask=False) == SM.E_OK
        assert nv.value == 0
    finally:
        bv.close()
