"""Driver of csrc/host_wire_views_harness.hip (the row bodies of csrc/wire_views_dev.h compiled for the host) for
tests/test_dev_wire_views_host.py and tests/test_wire_views_inputs.py: the family's tables built the way
ibft_set_validator_sets documents them, one run of the whole stage, the records back as dictionaries in the model's form."""
import ctypes as C

import numpy as np

U64_MAX = 2**64 - 1
EMPTY = 0xFFFFFFFF
WIRE_VIEW = np.dtype([("height", "<u8"), ("round", "<u8"), ("set", "<i4"), ("first_row", "<u4"), ("rows", "<u4"), ("stored_rows", "<u4"),
                      ("type", "u1"), ("hash_len", "u1"), ("prepare_rule", "u1"), ("pad", "u1", 5), ("proposal_hash", "u1", 32),
                      ("tally", [("quorum_lo", "<u8"), ("quorum_hi", "<u8"), ("power_lo", "<u8"), ("power_hi", "<u8"),
                                 ("valid_rows", "<u4"), ("distinct_senders", "<u4"), ("has_quorum", "<u4"), ("shard_overlap", "<u4"),
                                 ("proposer_rows", "<u4"), ("reserved", "<u4")])])
LOW128 = 2**128 - 1


class Family(C.Structure):
    _fields_ = [("setidx", C.c_void_p), ("set_meta", C.c_void_p), ("vpower32", C.c_void_p), ("quorum", C.c_void_p), ("vtab", C.c_void_p),
                ("vslot_mask", C.c_uint32), ("n_union", C.c_uint32), ("n_pieces", C.c_uint32),
                ("t_height", C.c_uint64), ("t_first", C.c_uint64), ("t_addr20", C.c_void_p), ("t_rounds", C.c_uint32)]


def load():
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_wire_views_harness())
    vp, u32 = C.c_void_p, C.c_uint32
    L.wvh_table_slots.argtypes = [u32, u32]
    L.wvh_table_slots.restype = u32
    L.wvh_sizeof_view.restype = u32
    L.wvh_hashes.argtypes = [vp, vp, u32, u32, vp, vp]
    L.wvh_hashes.restype = None
    L.wvh_run.argtypes = [vp, vp, vp, vp, u32, vp, u32, u32, u32, C.POINTER(Family), vp, vp, vp, vp, C.POINTER(u32)]
    L.wvh_run.restype = C.c_int
    L.wvh_build_vtab.argtypes = [vp, u32, vp, u32]
    L.wvh_build_vtab.restype = u32
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Tables:
    """[wire_sets_model.Set] → union, setidx (n_sets × n_union), set_meta, vpower32 (entries × 2·pw), quorum (n_sets × 5), the
    union's address table; proposers: wire_views_model.Proposers or None"""

    def __init__(self, L, sets, pw, proposers=None):
        self.pw = pw
        union = []
        for st in sets:
            for a in st.order:
                if a not in union:
                    union.append(a)
        self.union = union
        self.setidx = np.full((len(sets), max(len(union), 1)), -1, np.int32)
        meta, pieces, quorum = [], [], []
        for k, st in enumerate(sets):
            meta.append((len(pieces), len(st.order)))
            for i, a in enumerate(st.order):
                self.setidx[k, union.index(a)] = i
                pieces.append([(st.power[a] >> (32 * j)) & 0xFFFFFFFF for j in range(2 * pw)])
            quorum.append([(st.quorum >> (64 * j)) & U64_MAX for j in range(5)])
        self.meta = np.array(meta, np.uint32).reshape(-1, 2)
        self.vp32 = np.array(pieces, np.uint32).reshape(-1, 2 * pw)
        self.quorum = np.array(quorum, np.uint64).reshape(-1, 5)
        slots = 64
        while slots < 2 * len(union):
            slots *= 2
        self.vtab = np.zeros(6 * slots, np.uint32)
        addrs = np.frombuffer(b"".join(union) or bytes(20), np.uint8).copy()
        self.vslot_mask = L.wvh_build_vtab(_p(addrs), len(union), _p(self.vtab), slots)
        self.t_addrs = np.frombuffer(b"".join(proposers.addrs) if proposers and proposers.addrs else bytes(20), np.uint8).copy()
        self.fam = Family(_p(self.setidx).value, _p(self.meta).value, _p(self.vp32).value, _p(self.quorum).value, _p(self.vtab).value,
                          self.vslot_mask, len(union), 2 * pw, proposers.height if proposers else 0,
                          proposers.first_round if proposers else 0, _p(self.t_addrs).value,
                          len(proposers.addrs) if proposers else 0)


def run(L, tables, rows, valid, vidx, rset, views_cap, slots, salt, order=None):
    """one run of the stage → None when a table was exhausted, else (out_view list, stored [bool], n_views, records [dict],
    tables as filled)"""
    n = len(rows)
    order = np.arange(n, dtype=np.uint32) if order is None else np.ascontiguousarray(order, np.uint32)
    rows = np.ascontiguousarray(rows)
    tab = np.zeros(2 * slots, np.uint32)
    view = np.full(max(n, 1), 99, np.int32)
    stored = np.zeros(max((n + 63) // 64, 1), np.uint64)
    cap = min(views_cap, n)
    recs = np.zeros(max(cap, 1), WIRE_VIEW)
    nv = C.c_uint32(0)
    err = L.wvh_run(_p(rows), _p(vidx), _p(rset), _p(valid), n, _p(order), slots, salt, views_cap, C.byref(tables.fam), _p(tab), _p(view),
                    _p(stored), _p(recs), C.byref(nv))
    if err:
        return None
    bits = np.unpackbits(stored.view(np.uint8), bitorder="little")[:n].astype(bool).tolist()
    return view[:n].tolist(), bits, nv.value, [record_dict(r) for r in recs[:min(nv.value, cap)]], tab


def record_dict(r):
    """an ibft_wire_view_t (numpy record) in the model's form"""
    t = r["tally"]
    return dict(height=int(r["height"]), round=int(r["round"]), type=int(r["type"]), hash=bytes(r["proposal_hash"][:int(r["hash_len"])]),
                tail=bytes(r["proposal_hash"][int(r["hash_len"]):]), pad=bytes(r["pad"]), set=int(r["set"]), first_row=int(r["first_row"]),
                rows=int(r["rows"]), stored_rows=int(r["stored_rows"]), prepare_rule=int(r["prepare_rule"]),
                tally=dict(power=int(t["power_lo"]) | (int(t["power_hi"]) << 64), quorum=int(t["quorum_lo"]) | (int(t["quorum_hi"]) << 64),
                           valid_rows=int(t["valid_rows"]), distinct_senders=int(t["distinct_senders"]), has_quorum=int(t["has_quorum"]),
                           proposer_rows=int(t["proposer_rows"]), shard_overlap=int(t["shard_overlap"]), reserved=int(t["reserved"])))


def model_record(w):
    """a record of wire_views_model.views as record_dict gives the device's"""
    t = w["tally"]
    return dict(height=w["height"], round=w["round"], type=w["type"], hash=w["hash"], tail=bytes(32 - len(w["hash"])), pad=bytes(5),
                set=w["set"], first_row=w["first_row"], rows=w["rows"], stored_rows=w["stored_rows"], prepare_rule=w["prepare_rule"],
                tally=dict(power=t["power"] & LOW128, quorum=t["quorum"] & LOW128, valid_rows=t["valid_rows"],
                           distinct_senders=t["distinct_senders"], has_quorum=t["has_quorum"], proposer_rows=t["proposer_rows"],
                           shard_overlap=0, reserved=0))


def longest_run(table):
    """the longest circular run of occupied slots of a filled table"""
    occ = np.asarray(table) != EMPTY
    if occ.all():
        return len(occ)
    k = int(np.argmin(occ))                       # start behind a free slot
    best = cur = 0
    for x in np.roll(occ, -k):
        cur = cur + 1 if x else 0
        best = max(best, cur)
    return best
