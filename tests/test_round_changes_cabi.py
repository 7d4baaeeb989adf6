"""The C ABI of ibft_decide_round_changes_wire: exported with the header's parameter list, bound and optional; ibft_rc_query_t /
ibft_rc_record_t / ibft_rc_answer_t are 32 / 128 / 64 bytes in the header, the library, the device source's mirror, the Python
dtypes and the Go shim; every refusal leaves every buffer as it was.  What needs no context runs without a GPU; the refusals
behind the NULL-context check need one and are marked gpu."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ibft_decide_round_changes_wire"
DECIDE_PARAMS = ["ibft_ctx *", "const uint8_t *", "const uint32_t *", "size_t", "size_t", "size_t", "size_t *", "size_t *", "ibft_cert_verdict_t *",
                 "ibft_cert_decision_t *", "ibft_cert_node_t *", "ibft_wire_row_t *", "uint8_t *", "uint64_t *", "uint64_t *", "uint64_t *"]
PARAMS = DECIDE_PARAMS + ["const ibft_rc_query_t *", "int32_t *", "uint64_t *", "ibft_rc_record_t *", "size_t", "size_t *", "ibft_rc_answer_t *"]
C_SIZES = {"uint64_t": 8, "uint32_t": 4, "int8_t": 1, "uint8_t": 1, "ibft_tally_t": 56}
E_INVAL, E_NOVALSET, E_TOOBIG = -1, -5, -7


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


def _params(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/ibftgpu.h"
    return [re.sub(r"\s*\w+$", "", " ".join(p.split())).strip() for p in m.group(1).split(",")]


def test_symbol_exported_declared_and_optional(V):
    L = V.load_library()
    header = _header()
    assert _params(header, "ibft_decide_certificates_wire") == DECIDE_PARAMS
    assert _params(header, NAME) == PARAMS                        # the decide call's list, one input and the outputs behind it
    assert hasattr(L, NAME) and NAME in V.EXPORTS and NAME in V.OPTIONAL_EXPORTS
    assert len(getattr(L, NAME).argtypes) == len(PARAMS)
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4          # a new entry point, no new version
    assert callable(V.BatchVerifier.decide_round_changes_wire) and callable(V.DeviceGroup.decide_round_changes_wire)


def _struct_fields(header, name):
    m = re.search(r"typedef struct \{([^}]*)\} " + name + ";", header)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        typ, names = decl.split(None, 1)
        for nm in names.split(","):
            a = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            out.append((typ, a.group(1), int(a.group(2) or 0)))
    return out


def test_struct_sizes_agree_everywhere(V):
    import go_ibft_amd.build as build
    header = _header()
    for name, dtype, size in (("ibft_rc_query_t", V.RC_QUERY, 32), ("ibft_rc_record_t", V.RC_RECORD, 128), ("ibft_rc_answer_t", V.RC_ANSWER, 64)):
        fields = _struct_fields(header, name)
        assert [f[1] for f in fields] == list(dtype.names), name                     # the header's fields in the header's order
        assert sum(C_SIZES[t] * (k or 1) for t, _, k in fields) == size == dtype.itemsize, name   # (no padding: every field on its own alignment)
        off = 0
        for t, nm, k in fields:
            assert dtype.fields[nm][1] == off, (name, nm)
            off += C_SIZES[t] * (k or 1)
    assert V.RC_RECORD.fields["tally"][1] == 56 and [n for n in V.RC_RECORD["tally"].names] == [f[0] for f in V.Tally._fields_]
    H = C.CDLL(build.build_round_change_harness())
    H.rch_sizeof.restype = C.c_uint32
    assert [H.rch_sizeof(i) for i in range(3)] == [32, 128, 64]   # the device source's mirrors (static_asserted against the header's in the library)
    src = open(os.path.join(ROOT, "go-ibft_amd", "csrc", "ibftgpu.hip")).read()
    for name, mirror, size in (("ibft_rc_query_t", "rcd::query", 32), ("ibft_rc_record_t", "rcd::record", 128), ("ibft_rc_answer_t", "rcd::answer", 64)):
        assert f"static_assert(sizeof({name}) == sizeof({mirror}) && sizeof({name}) == {size}" in src, name
    go = open(os.path.join(ROOT, "shim", "go", "ibftgpu", "ibftgpu.go")).read()
    for name, size in (("RCQuery", 32), ("RCRecord", 128), ("RCAnswer", 64)):
        assert f"_ = unsafe.Sizeof({name}{{}}) - {size}\n" in go and f"_ = {size} - unsafe.Sizeof({name}{{}})\n" in go, name
    assert "C.ibft_decide_round_changes_wire(" in go


class _Outs:
    """every out buffer of the call, filled with a pattern"""

    def __init__(self, V):
        self.n_rows, self.n_certs, self.n_rc = C.c_size_t(7), C.c_size_t(8), C.c_size_t(9)
        self.cert = np.full(4 * 128, 0x5A, np.uint8).view(V.CERT_VERDICT)
        self.dec = np.full(4 * 64, 0x5B, np.uint8).view(V.CERT_DECISION)
        self.nodes = np.full(4 * 56, 0x5C, np.uint8).view(V.CERT_NODE)
        self.rows = np.full(4 * 80, 0x5D, np.uint8).view(V.WIRE_ROW)
        self.cls = np.full(4, 0x5E, np.uint8)
        self.masks = [np.full(1, 0x5F, np.uint64) for _ in range(3)]
        self.view = np.full(4, 66, np.int32)
        self.stored = np.full(1, 5, np.uint64)
        self.recs = np.full(4 * 128, 0x6A, np.uint8).view(V.RC_RECORD)
        self.answer = np.full(64, 0x6B, np.uint8).view(V.RC_ANSWER)
        self.query = V.rc_query(5, 0)

    def call(self, L, p, h, wire, off, n, rows_cap=64, certs_cap=4, rc_cap=4, query=True, n_rc=True, recs=True, dec=True):
        return getattr(L, NAME)(h, p(wire), p(off), n, rows_cap, certs_cap, C.byref(self.n_rows), C.byref(self.n_certs), p(self.cert),
                                p(self.dec) if dec else None, p(self.nodes), p(self.rows), p(self.cls), *(p(m) for m in self.masks),
                                p(self.query) if query else None, p(self.view), p(self.stored), p(self.recs) if recs else None, rc_cap,
                                C.byref(self.n_rc) if n_rc else None, p(self.answer))

    def untouched(self):
        return ((self.n_rows.value, self.n_certs.value, self.n_rc.value) == (7, 8, 9) and (self.cert.view(np.uint8) == 0x5A).all()
                and (self.dec.view(np.uint8) == 0x5B).all() and (self.nodes.view(np.uint8) == 0x5C).all() and (self.rows.view(np.uint8) == 0x5D).all()
                and (self.cls == 0x5E).all() and all((m == 0x5F).all() for m in self.masks) and (self.view == 66).all() and (self.stored == 5).all()
                and (self.recs.view(np.uint8) == 0x6A).all() and (self.answer.view(np.uint8) == 0x6B).all())


WIRE, OFF = np.zeros(8, np.uint8), np.array([0, 4, 8], np.uint32)


def test_null_context_is_invalid_and_outputs_untouched(V):
    L, o = V.load_library(), _Outs(V)
    assert o.call(L, V._p, None, WIRE, OFF, 2) == E_INVAL
    assert o.untouched()


def test_library_without_the_symbol_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    bv.max_rows = 64
    with pytest.raises(V.GpuUnavailable):
        bv.decide_round_changes_wire(b"", [0])


@pytest.mark.gpu
def test_refusals_leave_every_buffer_as_it_was(V):
    L, p = V.load_library(), V._p
    bv = V.BatchVerifier(max_rows=64)
    try:
        h, o = bv._h, _Outs(V)
        down, many = np.array([0, 4, 2], np.uint32), np.zeros(66, np.uint32)

        def sweep():
            assert o.call(L, p, h, WIRE, OFF, 2, n_rc=False) == E_INVAL                    # a NULL out_n_rc
            assert o.call(L, p, h, WIRE, OFF, 2, recs=False) == E_INVAL                    # a NULL out_rc with n > 0
            assert o.call(L, p, h, WIRE, OFF, 2, rc_cap=0) == E_INVAL                      # rc_cap == 0 with n > 0 …
            assert o.call(L, p, h, None, many, 65, rc_cap=0) == E_INVAL                    # … before IBFT_E_TOOBIG
            assert o.call(L, p, h, WIRE, OFF, 2, dec=False) == E_INVAL                     # the decide call's own
            o.query["reserved"] = 1
            assert o.call(L, p, h, WIRE, OFF, 2) == E_INVAL
            o.query["reserved"], o.query["has_accepted_proposal"] = 0, 2
            assert o.call(L, p, h, WIRE, OFF, 2) == E_INVAL
            o.query["has_accepted_proposal"] = 0
            assert o.call(L, p, h, WIRE, down, 2) == E_INVAL                               # offsets that run backwards
            assert o.untouched()

        sweep()
        # behind the argument checks the counts are zeroed, as the decide call zeroes its own; nothing else is written
        assert o.call(L, p, h, None, many, 65) == E_TOOBIG
        assert o.call(L, p, h, WIRE, OFF, 2) == E_NOVALSET
        assert (o.n_rows.value, o.n_certs.value, o.n_rc.value) == (0, 0, 0)
        o.n_rows.value, o.n_certs.value, o.n_rc.value = 7, 8, 9
        assert o.untouched()
        bv.set_validators(5, np.arange(60, dtype=np.uint8).reshape(3, 20), np.array([1, 2, 3], dtype=np.uint64))
        sweep()
        assert o.call(L, p, h, WIRE, OFF, 2, rows_cap=1) == E_TOOBIG                       # n above rows_cap
        o.n_rows.value, o.n_certs.value, o.n_rc.value = 7, 8, 9
        assert o.untouched()
        # garbage messages are rows for the host: they take no part, and the answer says how many there are
        assert o.call(L, p, h, WIRE, OFF, 2) == 0
        assert (o.n_rows.value, o.n_certs.value, o.n_rc.value) == (2, 2, 0)
        assert o.view[:2].tolist() == [-1, -1] and o.stored[0] == 0 and not o.recs[:2].view(np.uint8).any()
        a = o.answer[0]
        assert (int(a["extended"]), int(a["record"]), int(a["most_record"]), int(a["unjudged_rows"]), int(a["flags"])) == (0, V.CERT_NO_RECORD, V.CERT_NO_RECORD, 2, 0)
        # n = 0 with rc_cap = 0 and no out_rc is legal: no records, the answer over nothing
        o2 = _Outs(V)
        assert o2.call(L, p, h, None, np.zeros(1, np.uint32), 0, rc_cap=0, recs=False) == 0
        assert o2.n_rc.value == 0 and int(o2.answer[0]["extended"]) == 0 and int(o2.answer[0]["record"]) == V.CERT_NO_RECORD
        assert not o2.answer[0]["reserved"].any() and (o2.recs.view(np.uint8) == 0x6A).all()
    finally:
        bv.close()
