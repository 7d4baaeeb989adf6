"""The C ABI of ibft_verify_senders_wire_views: exported with the header's parameter list and bound, ibft_wire_view_t laid out
as the header, the Python dtype and the device source agree, every refusal in the documented order — the order of
tests/wire_views_model.py: check_call — and a refused call writes nothing.  What needs no context runs without a GPU; the
refusals behind the NULL-context check need one and are marked gpu."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wire_views_harness as H
import wire_views_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ibft_verify_senders_wire_views"
PARAMS = ["ibft_ctx *", "const uint8_t *", "const uint32_t *", "size_t", "size_t", "uint64_t *", "ibft_wire_row_t *", "int32_t *", "int32_t *",
          "ibft_tally_t *", "int32_t *", "uint64_t *", "ibft_wire_view_t *", "uint32_t *"]
# ibft_wire_view_t: (type, name, array length or 0), in the header's order
FIELDS = [("uint64_t", "height", 0), ("uint64_t", "round", 0), ("int32_t", "set", 0), ("uint32_t", "first_row", 0), ("uint32_t", "rows", 0),
          ("uint32_t", "stored_rows", 0), ("uint8_t", "type", 0), ("uint8_t", "hash_len", 0), ("uint8_t", "prepare_rule", 0),
          ("uint8_t", "pad", 5), ("uint8_t", "proposal_hash", 32), ("ibft_tally_t", "tally", 0)]


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


def test_symbol_exported_with_the_headers_signature(V):
    L = V.load_library()
    header = _header()
    m = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", header, re.S)
    assert m, f"{NAME} is not declared in include/ibftgpu.h"
    assert [re.sub(r"\s*\w+$", "", " ".join(p.split())).strip() for p in m.group(1).split(",")] == PARAMS
    assert hasattr(L, NAME) and NAME in V.EXPORTS and NAME in V.OPTIONAL_EXPORTS
    assert len(getattr(L, NAME).argtypes) == len(PARAMS)
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4          # a new entry point, no new version
    assert callable(V.BatchVerifier.verify_senders_wire_views)


def test_struct_layout_agrees_everywhere(V):
    header = _header()
    m = re.search(r"typedef struct \{([^}]*)\} ibft_wire_view_t;", header)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    got = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        typ, names = decl.split(None, 1)
        for nm in names.split(","):
            a = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            got.append((typ, a.group(1), int(a.group(2) or 0)))
    assert got == FIELDS
    assert V.WIRE_VIEW.itemsize == 128 and V.WIRE_VIEW.itemsize % 8 == 0 and C.sizeof(V.Tally) == 56
    assert [n for n in V.WIRE_VIEW.names] == [f[1] for f in FIELDS]
    assert V.WIRE_VIEW.fields["tally"][1] == 72 and V.WIRE_VIEW.fields["proposal_hash"][1] == 40
    assert [n for n in V.WIRE_VIEW["tally"].names] == [f[0] for f in V.Tally._fields_]
    assert H.WIRE_VIEW == V.WIRE_VIEW
    assert H.load().wvh_sizeof_view() == 128                     # the device source's mirror (static_asserted against the header's in the library)
    src = open(os.path.join(ROOT, "go-ibft_amd", "csrc", "ibftgpu.hip")).read()
    assert re.search(r"static_assert\(sizeof\(ibft_wire_view_t\) == sizeof\(wviews::view_t\) && sizeof\(ibft_wire_view_t\) == 128", src)


class _Outs:
    def __init__(self, V, n_sets=2):
        self.mask = np.full(2, 7, np.uint64)
        self.rows = np.full(3, 0xA5, np.uint8).repeat(80).view(V.WIRE_ROW)
        self.rset = np.full(3, 55, np.int32)
        self.vidx = np.full(3, 77, np.int32)
        self.tal = (V.Tally * n_sets)()
        for t in self.tal:
            t.power_lo = 0x1234
        self.view = np.full(3, 66, np.int32)
        self.stored = np.full(2, 5, np.uint64)
        self.views = np.full(3 * 128, 0x5A, np.uint8).view(V.WIRE_VIEW)
        self.nv = C.c_uint32(91)

    def args(self, p):
        return (p(self.mask), p(self.rows), p(self.rset), p(self.vidx), self.tal, p(self.view), p(self.stored), p(self.views), C.byref(self.nv))

    def untouched(self):
        return ((self.mask == 7).all() and (self.rows.view(np.uint8) == 0xA5).all() and (self.rset == 55).all() and (self.vidx == 77).all()
                and all(t.power_lo == 0x1234 and t.quorum_lo == 0 for t in self.tal) and (self.view == 66).all() and (self.stored == 5).all()
                and (self.views.view(np.uint8) == 0x5A).all() and self.nv.value == 91)


def test_null_context_is_invalid_and_outputs_untouched(V):
    L, p, o = V.load_library(), V._p, _Outs(V)
    wire, off = np.zeros(8, np.uint8), np.array([0, 4, 8], np.uint32)
    assert VM.check_call(False, 2, True, True, 4, True, True, 64, True, True) == VM.E_INVAL
    assert getattr(L, NAME)(None, p(wire), p(off), 2, 4, *o.args(p)) == VM.E_INVAL
    assert getattr(L, NAME)(None, None, None, 2, 0, *([None] * 9)) == VM.E_INVAL
    assert o.untouched()


def test_library_without_the_symbol_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    with pytest.raises(V.GpuUnavailable):
        bv.verify_senders_wire_views(b"", [0], 4)


def test_model_orders_its_checks():
    ok = dict(have_ctx=True, n=2, have_off=True, have_mask=True, views_cap=4, offsets_ok=True, bytes_ok=True, max_rows=64, have_family=True,
              have_map=True)
    call = lambda **kw: VM.check_call(**{**ok, **kw})  # noqa: E731
    assert call() == VM.E_OK
    assert call(have_ctx=False, views_cap=0, n=65, have_family=False) == VM.E_INVAL
    assert call(have_off=False) == VM.E_INVAL and call(have_mask=False) == VM.E_INVAL
    assert call(views_cap=0) == VM.E_INVAL
    assert call(views_cap=0, n=65) == VM.E_INVAL                 # the cap comes before the row count …
    assert call(views_cap=0, have_family=False) == VM.E_INVAL    # … and before the family and the map
    assert call(views_cap=0, n=0, have_off=False, have_mask=False) == VM.E_OK     # no rows: nothing to cap
    assert call(offsets_ok=False, n=65) == VM.E_INVAL and call(bytes_ok=False, have_map=False) == VM.E_INVAL
    assert call(n=65, have_family=False) == VM.E_TOOBIG
    assert call(have_family=False) == VM.E_NOVALSET and call(have_map=False) == VM.E_NOVALSET
    assert call(views_cap=10**9) == VM.E_OK                      # a cap above n behaves as n


@pytest.mark.gpu
def test_refusals_in_the_documented_order(V):
    L, p = V.load_library(), V._p
    call = getattr(L, NAME)
    bv = V.BatchVerifier(max_rows=64)
    try:
        h = bv._h
        o = _Outs(V)
        a = o.args(p)
        wire, off = np.zeros(8, np.uint8), np.array([0, 4, 8], np.uint32)
        down, many = np.array([0, 4, 2], np.uint32), np.zeros(66, np.uint32)
        addrs = np.arange(60, dtype=np.uint8).reshape(3, 20)
        state = dict(have_family=False, have_map=False)

        def want(n=2, have_off=True, have_mask=True, cap=4, offsets_ok=True, bytes_ok=True):
            return VM.check_call(True, n, have_off, have_mask, cap, offsets_ok, bytes_ok, 64, **state)

        def sweep():
            assert call(h, p(wire), None, 2, 4, *a) == want(have_off=False) == VM.E_INVAL
            assert call(h, p(wire), p(off), 2, 4, None, *a[1:]) == want(have_mask=False) == VM.E_INVAL
            assert call(h, p(wire), p(off), 2, 0, *a) == want(cap=0) == VM.E_INVAL
            assert call(h, None, p(many), 65, 0, *a) == want(n=65, cap=0) == VM.E_INVAL          # before IBFT_E_TOOBIG
            assert call(h, p(wire), p(down), 2, 4, *a) == want(offsets_ok=False) == VM.E_INVAL
            assert call(h, None, p(off), 2, 4, *a) == want(bytes_ok=False) == VM.E_INVAL
            assert call(h, None, p(many), 65, 4, *a) == want(n=65) == VM.E_TOOBIG
            assert o.untouched()

        sweep()
        assert call(h, p(wire), p(off), 2, 4, *a) == want() == VM.E_NOVALSET                     # no family
        bv.set_validator_sets([(addrs[:2], [1, 2]), (addrs[1:], [3, 4])])
        state["have_family"] = True
        assert call(h, p(wire), p(off), 2, 4, *a) == want() == VM.E_NOVALSET                     # a family, no map
        assert o.untouched()
        bv.set_height_sets([1, 5, 9], [0, 1])
        state["have_map"] = True
        sweep()
        # every out buffer but the mask may be NULL; garbage rows are NEEDS_HOST rows: no view, no record
        mask = np.full(1, 7, np.uint64)
        assert call(h, p(wire), p(off), 2, 10**9, p(mask), *([None] * 8)) == want(cap=10**9) == VM.E_OK
        assert mask[0] == 0
        got, rows, rset, vidx, tl, view, stored, views, n_views = bv.verify_senders_wire_views(wire.tobytes(), off, 1)
        assert not got.any() and view.tolist() == [-1, -1] and not stored.any() and n_views == 0 and len(views) == 0
        assert [(t.quorum, t.valid_rows, t.has_quorum) for t in tl] == [(3, 0, 0), (5, 0, 0)]
        # n = 0 with views_cap = 0 is legal
        nv = C.c_uint32(91)
        assert call(h, None, p(np.zeros(1, np.uint32)), 0, 0, *([None] * 8), C.byref(nv)) == want(n=0, cap=0, have_mask=False) == VM.E_OK
        assert nv.value == 0
    finally:
        bv.close()
