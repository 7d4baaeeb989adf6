"""Driver of csrc/host_wire_view_seals_harness.hip (csrc/wire_seals_dev.h and the seal form of csrc/wire_views_dev.h compiled
for the host) for tests/test_dev_wire_view_seals_host.py, and what the seal tests share: the records in the model's form, the
columns the device stages read, the byte strings the outputs are compared as.  The family's tables are wire_views_harness's."""
import ctypes as C

import numpy as np

import wire_views_cases as VC
import wire_views_harness as H

NONE = 0xFFFFFFFF
ROW_COMMIT, ROW_SEALABLE = 1, 2


def load():
    """→ (the seal harness, the views harness — which builds the tables)"""
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_wire_view_seals_harness())
    vp, u32 = C.c_void_p, C.c_uint32
    L.wsh_stage.argtypes = [vp, vp, u32, C.POINTER(H.Family), vp, vp, vp, vp]
    L.wsh_stage.restype = None
    L.wsh_combine.argtypes = [vp, vp, u32, vp, vp]
    L.wsh_combine.restype = None
    L.wsh_run.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u32, C.POINTER(H.Family), vp, vp, vp, C.POINTER(u32)]
    L.wsh_run.restype = C.c_int
    return L, H.load()


_p = H._p


def pack_bits(bits):
    n = len(bits)
    w = np.zeros(max((n + 63) // 64, 1), np.uint64)
    for i, b in enumerate(bits):
        if b:
            w[i >> 6] |= np.uint64(1 << (i & 63))
    return w


def unpack_bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool).tolist()


def parsed_columns(parsed):
    """oracle.wire_parse rows → ibft_wire_row_t as the walks leave them (the fields the seal and views stages read)"""
    rows = np.zeros(len(parsed), VC.WS_WIRE_ROW)
    for j, p in enumerate(parsed):
        r = rows[j]
        r["height"], r["round"], r["type"], r["status"], r["payload_kind"], r["has_view"] = p.height, p.round, p.type, p.status, p.payload_kind, p.has_view
        r["hash_len"], r["seal_len"], r["from_len"], r["sig_len"] = (len(p.proposal_hash), min(len(p.committed_seal), 255), min(len(p.sender), 255),
                                                                     min(len(p.signature), 255))
        r["from"][:min(len(p.sender), 20)] = np.frombuffer(p.sender[:20], np.uint8)
        r["proposal_hash"][:len(p.proposal_hash)] = np.frombuffer(p.proposal_hash, np.uint8)
    return rows


def stage(L, tables, rows, rset):
    """mark + scan → (flags list, seal_row list, src list of the sealable rows, sealable rows, COMMIT rows)"""
    n = len(rows)
    flags, seal_row, src = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    counts = np.zeros(2, np.uint32)
    L.wsh_stage(_p(np.ascontiguousarray(rows)), _p(np.ascontiguousarray(rset, np.int32)), n, C.byref(tables.fam), _p(flags), _p(seal_row), _p(src),
                _p(counts))
    return flags[:n].tolist(), seal_row[:n].tolist(), src[:int(counts[0])].tolist(), int(counts[0]), int(counts[1])


def combine(L, valid, seal_row, seal_verdicts):
    """valid: the final sender bits; seal_verdicts[k]: the verdict bit of seal row k → the rows' seal bits"""
    n = len(valid)
    out = np.zeros(max((n + 63) // 64, 1), np.uint64)
    L.wsh_combine(_p(np.array(valid, np.uint8)), _p(np.array(seal_row, np.uint32)), n, _p(pack_bits(seal_verdicts)), _p(out))
    return unpack_bits(out, n)


def run(L, tables, rows, valid, vidx, rset, seal, views_cap, slots, salt):
    """the views stage in its seal form → None when a table was exhausted, else (out_view, stored, n_views, records)"""
    n = len(rows)
    view = np.full(max(n, 1), 99, np.int32)
    stored = np.zeros(max((n + 63) // 64, 1), np.uint64)
    cap = min(views_cap, n)
    recs = np.zeros(max(cap, 1), H.WIRE_VIEW)
    nv = C.c_uint32(0)
    err = L.wsh_run(_p(np.ascontiguousarray(rows)), _p(np.ascontiguousarray(vidx, np.int32)), _p(np.ascontiguousarray(rset, np.int32)),
                    _p(np.ascontiguousarray(valid, np.uint8)), _p(pack_bits(seal)), n, slots, salt, views_cap, C.byref(tables.fam), _p(view),
                    _p(stored), _p(recs), C.byref(nv))
    if err:
        return None
    return view[:n].tolist(), unpack_bits(stored, n), nv.value, [H.record_dict(r) for r in recs[:min(nv.value, cap)]]


def model_record(w):
    """a record of wire_view_seals_model.views (or, with no pad of its own, of wire_views_model.views) as H.record_dict gives
    the device's"""
    return dict(H.model_record(w), pad=w.get("pad", bytes(5)))


def output_bytes(out):
    """everything a views call returned — either of the two — as bytes"""
    got, rows, rset, vidx, tl, view, stored, views, n_views = out[:9]
    tail = [np.packbits(out[9]).tobytes()] if len(out) > 9 else []
    return b"".join([np.packbits(got).tobytes(), rows.tobytes(), rset.tobytes(), vidx.tobytes(), b"".join(bytes(t) for t in tl),
                     view.tobytes(), np.packbits(stored).tobytes(), views.tobytes(), int(n_views).to_bytes(4, "little")] + tail)
