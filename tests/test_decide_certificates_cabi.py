"""ibft_set_proposers, ibft_proposers_info and ibft_decide_certificates_wire at the C boundary, without a device: the three
symbols are exported, declared with their parameter lists and bound as optional exports of ABI version 4; a refused call leaves
every out buffer as it was; the decision is 64 bytes in the header, in the library, in Python and in Go."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ibft_set_proposers", "ibft_proposers_info", "ibft_decide_certificates_wire"]
PARAMS = {
    "ibft_set_proposers": ["ibft_ctx *ctx", "uint64_t height", "uint64_t first_round", "const uint8_t *proposer20", "size_t n_rounds"],
    "ibft_proposers_info": ["ibft_ctx *ctx", "uint64_t *height", "uint64_t *first_round", "uint32_t *n_rounds"],
    "ibft_decide_certificates_wire": ["ibft_ctx *ctx", "const uint8_t *wire", "const uint32_t *off", "size_t n", "size_t rows_cap", "size_t certs_cap",
                                      "size_t *out_n_rows", "size_t *out_n_certs", "ibft_cert_verdict_t *out_cert", "ibft_cert_decision_t *out_decision",
                                      "ibft_cert_node_t *out_nodes", "ibft_wire_row_t *out_rows", "uint8_t *out_class", "uint64_t *out_sender_mask",
                                      "uint64_t *out_hash_mask", "uint64_t *out_self_mask"],
}


@pytest.fixture(scope="module")
def lib():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    return V.load_library()


def header():
    hdr = open(os.path.join(ROOT, "include", "ibftgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_exported_declared_and_bound_as_optional(lib, name):
    import go_ibft_amd.verifier as V
    assert hasattr(lib, name)
    assert lib.ibft_version() == 4 == V.ABI_VERSION                       # no version step: an older build simply lacks the symbols
    assert name in V.EXPORTS and name in V.OPTIONAL_EXPORTS and name not in V.EXPORTS_SINCE
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header(), re.S)
    assert proto, "not declared"
    assert [" ".join(p.split()) for p in proto.group(1).split(",")] == PARAMS[name]
    assert len(getattr(lib, name).argtypes) == len(PARAMS[name])


def test_the_binding_has_the_three_calls_on_both_classes():
    import go_ibft_amd.verifier as V
    for cls in (V.BatchVerifier, V.DeviceGroup):
        assert callable(cls.set_proposers) and callable(cls.proposers_info) and callable(cls.decide_certificates_wire)
    assert "#define IBFT_PROPOSER_ROUNDS_MAX 4096u" in open(os.path.join(ROOT, "include", "ibftgpu.h")).read() and V.PROPOSER_ROUNDS_MAX == 4096


def test_refusals_leave_every_buffer_untouched(lib):
    import go_ibft_amd.verifier as V
    f = lib.ibft_decide_certificates_wire
    wire = np.full(64, 0x5A, dtype=np.uint8)
    off = np.array([0, 10], dtype=np.uint32)
    bufs = {"cert": np.full(4, 0x77, dtype=np.uint8).repeat(128).view(V.CERT_VERDICT), "dec": np.full(4, 0x77, dtype=np.uint8).repeat(64).view(V.CERT_DECISION),
            "nodes": np.full(8 * 56, 0x77, dtype=np.uint8), "rows": np.full(8 * 80, 0x77, dtype=np.uint8), "cls": np.full(8, 0x77, dtype=np.uint8),
            "ms": np.full(2, 0x7777777777777777, dtype=np.uint64), "mh": np.full(2, 0x7777777777777777, dtype=np.uint64),
            "mself": np.full(2, 0x7777777777777777, dtype=np.uint64)}
    n_rows, n_certs = C.c_size_t(0x7777), C.c_size_t(0x7777)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(ctx, out_n_rows=C.byref(n_rows), out_n_certs=C.byref(n_certs), cert=p(bufs["cert"]), dec=p(bufs["dec"])):
        return f(ctx, p(wire), p(off), 1, 8, 4, out_n_rows, out_n_certs, cert, dec, p(bufs["nodes"]), p(bufs["rows"]), p(bufs["cls"]), p(bufs["ms"]),
                 p(bufs["mh"]), p(bufs["mself"]))
    assert call(None) == -1                                               # IBFT_E_INVAL: no context
    assert call(None, dec=None) == -1 and call(None, out_n_certs=None) == -1 and call(None, cert=None) == -1 and call(None, out_n_rows=None) == -1
    assert (n_rows.value, n_certs.value) == (0x7777, 0x7777)
    for name, b in bufs.items():
        assert (b.view(np.uint8) == 0x77).all(), name
    assert wire.tolist() == [0x5A] * 64 and off.tolist() == [0, 10]
    # the table calls: no context, and the caller's memory is only read
    addrs = np.full(40, 0x33, dtype=np.uint8)
    assert lib.ibft_set_proposers(None, 5, 0, p(addrs), 2) == -1 and lib.ibft_set_proposers(None, 5, 0, None, 0) == -1
    h, fr, nr = C.c_uint64(0x7777), C.c_uint64(0x7777), C.c_uint32(0x7777)
    assert lib.ibft_proposers_info(None, C.byref(h), C.byref(fr), C.byref(nr)) == -1
    assert (h.value, fr.value, nr.value) == (0x7777, 0x7777, 0x7777) and (addrs == 0x33).all()


def test_decision_size_agrees_everywhere():
    import go_ibft_amd.verifier as V
    assert V.CERT_DECISION.itemsize == 64
    hdr = header()
    body = hdr[hdr.index("typedef struct {\n  int8_t valid_pc, round_change, proposal;"):hdr.index("} ibft_cert_decision_t;")]
    names = re.findall(r"\b(valid_pc|round_change|proposal|flags|prepared_record|prepared_round|prepared_hash|reserved)\b(?=[,;\[])", body)
    assert names == list(V.CERT_DECISION.names)
    # the header's struct, laid out by its field types: every member naturally aligned, no hole, 64 bytes
    size = {"uint32_t": 4, "int8_t": 1, "uint8_t": 1, "uint64_t": 8}
    at = 0
    for ctype, decl in re.findall(r"\b(uint32_t|int8_t|uint8_t|uint64_t)\s+([^;]+);", body):
        for d in decl.split(","):
            name, count = re.match(r"\s*(\w+)(?:\[(\d+)\])?", d).groups()
            assert at % size[ctype] == 0 and V.CERT_DECISION.fields[name][1] == at, name
            at += size[ctype] * int(count or 1)
    assert at == 64
    src = open(os.path.join(ROOT, "go-ibft_amd", "csrc", "ibftgpu.hip")).read()
    assert "static_assert(sizeof(ibft_cert_decision_t) == sizeof(certd::decision) && sizeof(ibft_cert_decision_t) == 64" in src
    dev = open(os.path.join(ROOT, "go-ibft_amd", "csrc", "cert_decide_dev.h")).read()
    assert 'static_assert(sizeof(decision) == 64, "ABI");' in dev
    go = open(os.path.join(ROOT, "shim", "go", "ibftgpu", "ibftgpu.go")).read()
    assert "type CertDecision struct" in go and "unsafe.Sizeof(CertDecision{}) - 64" in go and "64 - unsafe.Sizeof(CertDecision{})" in go
    assert "C.ibft_decide_certificates_wire(" in go and "C.ibft_set_proposers(" in go
    body = go[go.index("type CertDecision struct"):]
    body = body[:body.index("\n}")]
    go_size = {"uint32": 4, "int8": 1, "uint8": 1, "uint64": 8}
    total = 0
    for line in body.splitlines()[1:]:
        line = line.split("//")[0].strip()
        if not line:
            continue
        m = re.match(r"([\w, ]+?)\s+(?:\[(\d+)\])?(uint32|int8|uint8|uint64|byte)$", line)
        assert m, line
        total += len(m.group(1).split(",")) * int(m.group(2) or 1) * go_size.get(m.group(3), 1)
    assert total == 64
