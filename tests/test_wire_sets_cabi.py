"""The C ABI of the wire route under a family of sets: ibft_set_height_sets, ibft_height_sets_info and
ibft_verify_senders_wire_sets are exported with the header's parameter lists and bound; every refusal of the two calls comes
in the documented order — the order of tests/wire_sets_model.py: check_height_sets — and a refused call writes nothing.
What needs no context runs without a GPU; the refusals behind the NULL-context check need one and are marked gpu."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wire_sets_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "ibft_set_height_sets": ["ibft_ctx *", "size_t", "const uint64_t *", "const uint32_t *"],
    "ibft_height_sets_info": ["ibft_ctx *", "uint32_t *", "uint64_t *", "uint64_t *"],
    "ibft_verify_senders_wire_sets": ["ibft_ctx *", "const uint8_t *", "const uint32_t *", "size_t", "uint64_t *", "ibft_wire_row_t *",
                                      "int32_t *", "int32_t *", "ibft_tally_t *"],
}


@pytest.fixture(scope="module")
def V():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    V.load_library()
    return V


def _header():
    with open(os.path.join(ROOT, "include", "ibftgpu.h")) as f:
        return f.read()


def _header_params(header: str, name: str):
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/ibftgpu.h"
    return [re.sub(r"\s*\w+$", "", " ".join(p.split())).strip() for p in m.group(1).split(",")]


def test_symbols_exported_with_the_headers_signatures(V):
    L = V.load_library()
    header = _header()
    for name, params in SIGNATURES.items():
        assert hasattr(L, name), name
        assert _header_params(header, name) == params, name
        assert name in V.EXPORTS and name in V.OPTIONAL_EXPORTS
        assert len(getattr(L, name).argtypes) == len(params), name
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4   # new entry points, no new version
    for m in ("set_height_sets", "height_sets_info", "verify_senders_wire_sets"):
        assert callable(getattr(V.BatchVerifier, m))
    assert int(re.search(r"#define IBFT_HEIGHT_RANGES_MAX (\d+)u", header).group(1)) == M.RANGES_MAX


class _Outs:
    def __init__(self, V, n_sets=4):
        self.mask = np.full(2, 7, np.uint64)
        self.rows = np.full(3, 0xA5, np.uint8).repeat(80).view(V.WIRE_ROW)
        self.rset = np.full(3, 55, np.int32)
        self.vidx = np.full(3, 77, np.int32)
        self.tal = (V.Tally * n_sets)()
        for t in self.tal:
            t.power_lo = 0x1234
        self.info = (C.c_uint32(91), C.c_uint64(92), C.c_uint64(93))

    def untouched(self):
        return ((self.mask == 7).all() and (self.rows.view(np.uint8) == 0xA5).all() and (self.rset == 55).all() and (self.vidx == 77).all()
                and all(t.power_lo == 0x1234 and t.quorum_lo == 0 for t in self.tal)
                and tuple(x.value for x in self.info) == (91, 92, 93))


def test_null_context_is_invalid_and_outputs_untouched(V):
    L, p, o = V.load_library(), V._p, _Outs(V)
    wire = np.zeros(8, np.uint8)
    off = np.array([0, 4, 8], np.uint32)
    first = np.array([1, 2], np.uint64)
    rs = np.zeros(1, np.uint32)
    assert M.check_height_sets(False, 1, first.tolist(), rs.tolist(), 1)[0] == M.E_INVAL
    assert L.ibft_set_height_sets(None, 1, p(first), p(rs)) == M.E_INVAL
    assert L.ibft_set_height_sets(None, 0, None, None) == M.E_INVAL        # the NULL ctx comes before "0 clears"
    assert L.ibft_height_sets_info(None, C.byref(o.info[0]), C.byref(o.info[1]), C.byref(o.info[2])) == M.E_INVAL
    assert L.ibft_verify_senders_wire_sets(None, p(wire), p(off), 2, p(o.mask), p(o.rows), p(o.rset), p(o.vidx), o.tal) == M.E_INVAL
    assert L.ibft_verify_senders_wire_sets(None, None, None, 2, None, None, None, None, None) == M.E_INVAL
    assert o.untouched()


def test_library_without_the_symbols_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    with pytest.raises(V.GpuUnavailable):
        bv.set_height_sets([1, 2], [0])
    with pytest.raises(V.GpuUnavailable):
        bv.height_sets_info()
    with pytest.raises(V.GpuUnavailable):
        bv.verify_senders_wire_sets(b"", [0])


def test_model_orders_its_checks():
    inc, bad = [1, 5, 9], [1, 5, 5]
    assert M.check_height_sets(True, 0, None, None, None) == (M.E_OK, True)
    assert M.check_height_sets(True, 2, None, [0, 0], 3)[0] == M.E_INVAL
    assert M.check_height_sets(True, 2, bad, [0, 9], None)[0] == M.E_INVAL
    big = list(range(M.RANGES_MAX + 2))
    assert M.check_height_sets(True, M.RANGES_MAX + 1, big, [0] * (M.RANGES_MAX + 1), None)[0] == M.E_TOOBIG
    assert M.check_height_sets(True, 2, inc, [0, 9], None)[0] == M.E_NOVALSET
    assert M.check_height_sets(True, 2, inc, [0, 3], 3)[0] == M.E_INVAL
    assert M.check_height_sets(True, 2, inc, [0, 2], 3) == (M.E_OK, False)


@pytest.mark.gpu
def test_refusals_in_the_documented_order(V):
    L, p = V.load_library(), V._p
    bv = V.BatchVerifier(max_rows=64)
    try:
        h = bv._h
        addrs = np.arange(60, dtype=np.uint8).reshape(3, 20)
        inc, bad = np.array([1, 5, 9], np.uint64), np.array([1, 5, 5], np.uint64)
        big = np.arange(M.RANGES_MAX + 2, dtype=np.uint64)
        big_rs = np.full(M.RANGES_MAX + 1, 9, np.uint32)
        cap = np.arange(M.RANGES_MAX + 1, dtype=np.uint64)
        rs_ok, rs_out = np.array([0, 1], np.uint32), np.array([0, 2], np.uint32)

        def set_map(n, first, rs, n_sets):
            want = M.check_height_sets(True, n, None if first is None else first.tolist(), None if rs is None else rs.tolist(), n_sets)[0]
            assert L.ibft_set_height_sets(h, n, p(first), p(rs)) == want
            return want

        # ---- no family yet: every check in front of IBFT_E_NOVALSET answers first
        assert set_map(0, None, None, None) == M.E_OK
        assert set_map(2, None, rs_out, None) == M.E_INVAL
        assert set_map(2, inc, None, None) == M.E_INVAL
        assert set_map(2, bad, rs_out, None) == M.E_INVAL
        assert set_map(M.RANGES_MAX + 1, big, big_rs, None) == M.E_TOOBIG     # (its entries are ≥ n_sets too: the cap comes first)
        assert set_map(2, inc, rs_out, None) == M.E_NOVALSET
        o = _Outs(V, 2)
        wire, off = np.zeros(8, np.uint8), np.array([0, 4, 8], np.uint32)
        outs = (p(o.mask), p(o.rows), p(o.rset), p(o.vidx), o.tal)
        call = L.ibft_verify_senders_wire_sets
        assert call(h, p(wire), p(off), 2, *outs) == M.E_NOVALSET               # no family
        bv.set_validator_sets([(addrs[:2], [1, 2]), (addrs[1:], [3, 4])])
        assert call(h, p(wire), p(off), 2, *outs) == M.E_NOVALSET               # a family, no map
        # ---- a family of two sets
        assert set_map(2, inc, rs_out, 2) == M.E_INVAL                         # an entry ≥ n_sets
        assert bv.height_sets_info() == (0, 0, 0)
        assert set_map(M.RANGES_MAX, cap, np.zeros(M.RANGES_MAX, np.uint32), 2) == M.E_OK    # the cap itself is legal
        assert set_map(2, inc, rs_ok, 2) == M.E_OK
        assert bv.height_sets_info() == (2, 1, 9)
        for n, first, rs in ((2, bad, rs_ok), (2, inc, rs_out), (2, None, rs_ok), (M.RANGES_MAX + 1, big, big_rs)):
            assert set_map(n, first, rs, 2) != M.E_OK
            assert bv.height_sets_info() == (2, 1, 9)                          # a refused install leaves the old map in place
        # ---- the call's own refusals, in ibft_verify_senders_wire's order; nothing is written
        down = np.array([0, 4, 2], np.uint32)
        many = np.zeros(66, np.uint32)
        assert call(h, p(wire), None, 2, *outs) == M.E_INVAL                    # NULL off
        assert call(h, p(wire), p(off), 2, None, *outs[1:]) == M.E_INVAL        # NULL out_mask
        assert call(h, p(wire), p(down), 2, *outs) == M.E_INVAL                 # decreasing offsets
        assert call(h, None, p(off), 2, *outs) == M.E_INVAL                     # bytes promised, none given
        assert call(h, None, p(many), 65, *outs) == M.E_TOOBIG                  # n > max_rows
        assert o.untouched()
        assert set_map(0, None, None, 2) == M.E_OK                             # cleared
        assert bv.height_sets_info() == (0, 0, 0)
        assert call(h, p(wire), p(off), 2, *outs) == M.E_NOVALSET
        assert call(h, None, p(many), 65, *outs) == M.E_TOOBIG                  # … which comes behind the row count
        assert o.untouched()
        # every out buffer but the mask may be NULL; garbage rows are NEEDS_HOST rows without a set
        assert set_map(2, inc, rs_ok, 2) == M.E_OK
        mask = np.full(1, 7, np.uint64)
        assert call(h, p(wire), p(off), 2, p(mask), None, None, None, None) == M.E_OK
        assert mask[0] == 0
        got, rows, rset, vidx, tl = bv.verify_senders_wire_sets(wire.tobytes(), off)
        assert not got.any() and rset.tolist() == [-1, -1] and vidx.tolist() == [-1, -1] and (rows["status"] == 1).all()
        assert [(t.quorum, t.valid_rows, t.has_quorum) for t in tl] == [(3, 0, 0), (5, 0, 0)]
    finally:
        bv.close()
