"""ibft_judge_certificates_wire at the C boundary, without a device: the symbol is exported, declared with its fifteen
parameters and bound as an optional export of ABI version 4; a refused call leaves every out buffer as it was; the record is 128
bytes in the header, in the library, in Python and in Go."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ibft_judge_certificates_wire"


@pytest.fixture(scope="module")
def lib():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    return V.load_library()


def header():
    hdr = open(os.path.join(ROOT, "include", "ibftgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_exported_declared_and_bound_as_optional(lib):
    import go_ibft_amd.verifier as V
    assert hasattr(lib, NAME)
    assert lib.ibft_version() == 4 == V.ABI_VERSION                       # no version step: an older build simply lacks the symbol
    assert NAME in V.EXPORTS and NAME in V.OPTIONAL_EXPORTS and NAME not in V.EXPORTS_SINCE
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, header(), re.S)
    assert proto, "not declared"
    params = [" ".join(p.split()) for p in proto.group(1).split(",")]
    assert params == ["ibft_ctx *ctx", "const uint8_t *wire", "const uint32_t *off", "size_t n", "size_t rows_cap", "size_t certs_cap",
                      "size_t *out_n_rows", "size_t *out_n_certs", "ibft_cert_verdict_t *out_cert", "ibft_cert_node_t *out_nodes",
                      "ibft_wire_row_t *out_rows", "uint8_t *out_class", "uint64_t *out_sender_mask", "uint64_t *out_hash_mask",
                      "uint64_t *out_self_mask"]
    assert len(getattr(lib, NAME).argtypes) == 15
    assert callable(V.BatchVerifier.judge_certificates_wire) and callable(V.DeviceGroup.judge_certificates_wire)


def test_refusals_leave_every_buffer_untouched(lib):
    import go_ibft_amd.verifier as V
    f = getattr(lib, NAME)
    wire = np.full(64, 0x5A, dtype=np.uint8)
    off = np.array([0, 10], dtype=np.uint32)
    bufs = {"cert": np.full(4, 0x77, dtype=np.uint8).repeat(128).view(V.CERT_VERDICT), "nodes": np.full(8 * 56, 0x77, dtype=np.uint8),
            "rows": np.full(8 * 80, 0x77, dtype=np.uint8), "cls": np.full(8, 0x77, dtype=np.uint8),
            "ms": np.full(2, 0x7777777777777777, dtype=np.uint64), "mh": np.full(2, 0x7777777777777777, dtype=np.uint64),
            "mself": np.full(2, 0x7777777777777777, dtype=np.uint64)}
    n_rows, n_certs = C.c_size_t(0x7777), C.c_size_t(0x7777)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(ctx, out_n_rows=C.byref(n_rows), out_n_certs=C.byref(n_certs), cert=p(bufs["cert"])):
        return f(ctx, p(wire), p(off), 1, 8, 4, out_n_rows, out_n_certs, cert, p(bufs["nodes"]), p(bufs["rows"]), p(bufs["cls"]), p(bufs["ms"]),
                 p(bufs["mh"]), p(bufs["mself"]))
    assert call(None) == -1                                               # IBFT_E_INVAL: no context
    assert call(None, out_n_certs=None) == -1 and call(None, cert=None) == -1 and call(None, out_n_rows=None) == -1
    assert (n_rows.value, n_certs.value) == (0x7777, 0x7777)
    for name, b in bufs.items():
        assert (b.view(np.uint8) == 0x77).all(), name
    assert wire.tolist() == [0x5A] * 64 and off.tolist() == [0, 10]


def test_record_size_agrees_everywhere():
    import go_ibft_amd.verifier as V
    assert V.CERT_VERDICT.itemsize == 128
    hdr = header()
    body = hdr[hdr.index("typedef struct {\n  uint32_t row, first_child, n_children;"):hdr.index("} ibft_cert_verdict_t;")]
    names = re.findall(r"\b(row|first_child|n_children|first_child_cert|rcc_rows|pc|rcc|cls|bits|type|role|level|from_len|reserved|height|round|"
                       r"pc_round|from|pc_from|pc_hash)\b(?=[,;\[])", body)
    assert names == list(V.CERT_VERDICT.names)
    # the header's struct, laid out by its field types: every member naturally aligned, no hole, 128 bytes
    size = {"uint32_t": 4, "int8_t": 1, "uint8_t": 1, "uint64_t": 8}
    at = 0
    for ctype, decl in re.findall(r"\b(uint32_t|int8_t|uint8_t|uint64_t)\s+([^;]+);", body):
        for d in decl.split(","):
            name, count = re.match(r"\s*(\w+)(?:\[(\d+)\])?", d).groups()
            assert at % size[ctype] == 0 and V.CERT_VERDICT.fields[name][1] == at, name
            at += size[ctype] * int(count or 1)
    assert at == 128
    src = open(os.path.join(ROOT, "go-ibft_amd", "csrc", "ibftgpu.hip")).read()
    assert "static_assert(sizeof(ibft_cert_verdict_t) == sizeof(certv::record) && sizeof(ibft_cert_verdict_t) == 128" in src
    go = open(os.path.join(ROOT, "shim", "go", "ibftgpu", "ibftgpu.go")).read()
    assert "type CertVerdict struct" in go and "unsafe.Sizeof(CertVerdict{}) - 128" in go and "128 - unsafe.Sizeof(CertVerdict{})" in go and "C.ibft_judge_certificates_wire(" in go
    body = go[go.index("type CertVerdict struct"):]
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
    assert total == 128
