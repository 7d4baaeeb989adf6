"""round_change_dev.h over wire_views_dev.h's tables on the CPU (host_round_change_harness.hip, hipcc's host pass — the exact
source the round_change_*_kernel launches run): every case of tests/round_change_cases.py against tests/round_change_model.py,
with the row order shuffled into the tables, the slot count down to the smallest allowed and several salts; the answer's
selection on the wave emulator; and an independent check through the host mirror's store."""
import ctypes as C
import random

import numpy as np
import pytest

import go_ibft_amd.build as build
import go_ibft_amd.hostlib as hostlib
import go_ibft_amd.verifier as V
from oracle import wire_cert as WC

import cert_cases as CC
import cert_decision_model as DM
import cert_verdict_cases as K
import cert_verdict_model as M
import round_change_cases as RK
import round_change_model as RM
from test_dev_cert_decide_host import judge_lib, records  # noqa: F401  (the records of cert_verdict_dev.h over the model's rows)


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(build.build_round_change_harness())
    vp, u32 = C.c_void_p, C.c_uint32
    L.rch_sizeof.restype = u32
    L.rch_build_vtab.argtypes = [vp, u32, vp, u32]
    L.rch_build_vtab.restype = u32
    L.rch_run.argtypes = [vp, vp, vp, u32, vp, u32, u32, u32, vp, u32, u32, vp, u32, vp, vp, vp, vp, vp, vp, C.POINTER(u32), vp]
    L.rch_select.argtypes = [vp, u32, u32, u32, u32, vp, vp]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pieces(powers, n_pieces):
    out = np.zeros((len(powers), n_pieces), dtype=np.uint32)
    for i, p in enumerate(powers):
        for k in range(n_pieces):
            out[i, k] = (int(p) >> (32 * k)) & 0xFFFFFFFF
    return out


def query_of(c):
    return V.rc_query(*c.query[:2], has_accepted_proposal=c.query[2], min_round=c.query[3])


_world = {}


def world(judge_lib, r, powers, c):
    """(rows model, records, decisions under the case's table), once per (case, table)"""
    key = (c.label, c.table)
    if key not in _world:
        addrs = [a.tobytes() for a in r.addrs]
        wire, _ = CC.pack(c.msgs)
        cv = M.rows_from_tree(WC.expected_tree(c.msgs, r.addrs), addrs, powers)
        n = len(c.msgs)
        if max(powers) < 2**64:
            certs = records(judge_lib, cv, n, addrs, powers)
        else:
            certs = None  # (certs_for)
        table = dict(DM.tables_for(addrs, RK.H, 2))[c.table]
        dec = DM.expected_decisions(cv, n, table, wire)
        _world[key] = (cv, certs, dec)
    return _world[key]


def run(lib, r, powers, cv, certs, dec, n, query, rc_cap, order=None, hook=0, salt=0x1234):
    """the harness over the level-0 rows → the tuple round_change_model.check takes"""
    addrs = np.ascontiguousarray(r.addrs, dtype=np.uint8)
    vslots = 64
    while vslots < 2 * len(powers):
        vslots *= 2
    vtab = np.zeros(6 * vslots, dtype=np.uint32)
    vmask = lib.rch_build_vtab(_p(addrs), len(powers), _p(vtab), vslots)
    n_pieces = 2 if max(powers) < 2**64 else 8
    pw = pieces(powers, n_pieces)
    q = 2 * sum(int(p) for p in powers) // 3 + 1
    quorum = np.array([(q >> (64 * i)) & (2**64 - 1) for i in range(5)], dtype=np.uint64)
    slots = table_slots(n, hook)
    tables = np.zeros(2 * slots, dtype=np.uint32)
    order = np.arange(n, dtype=np.uint32) if order is None else np.asarray(order, dtype=np.uint32)
    cap = n if rc_cap is None else min(rc_cap, n)
    view = np.full(max(n, 1), 77, dtype=np.int32)
    stored = np.full((n + 63) // 64 or 1, 0x7777777777777777, dtype=np.uint64)
    recs = np.zeros(max(cap, 1), dtype=V.RC_RECORD)
    ans = np.zeros(1, dtype=V.RC_ANSWER)
    n_rc = C.c_uint32(0)
    rows = np.ascontiguousarray(cv.rows[:n])
    rc = lib.rch_run(_p(rows), _p(np.ascontiguousarray(certs[:n])), _p(np.ascontiguousarray(dec[:n])), n, _p(order), slots, salt, cap, _p(vtab), vmask,
                     len(powers), _p(pw), n_pieces, _p(quorum), _p(query), _p(tables), _p(view), _p(stored), _p(recs), C.byref(n_rc), _p(ans))
    assert rc == 0, "a table was exhausted"
    filled = min(int(n_rc.value), cap)
    assert not recs[filled:cap].tobytes().strip(b"\0"), "records past the number of keys are zeroed"
    return view[:n], V.mask_to_bool(stored, n), recs[:filled], int(n_rc.value), (None if query is None else ans[0])


def table_slots(n, hook):
    """wviews::table_slots"""
    s = 64
    while s < 2 * n:
        s *= 2
    if hook:
        floor_ = 1
        while floor_ <= n:
            floor_ *= 2
        c = 1
        while c <= hook // 2:
            c *= 2
        s = min(s, max(c, floor_))
    return s


def level0_records(cv, n):
    """what round_change_dev.h reads of a level-0 record — its class and its sender bit —, and the rest of the record's own part,
    straight from the model's rows"""
    out = np.zeros(n, dtype=V.CERT_VERDICT)
    for i in range(n):
        w, o = cv.rows[i], out[i]
        o["row"], o["cls"], o["bits"] = i, cv.cls[i], (V.CERT_BIT_SENDER if cv.sender[i] else 0)
        o["type"], o["from_len"], o["height"], o["round"], o["from"] = w["type"], w["from_len"], w["height"], w["round"], w["from"]
    return out


def certs_for(cv, n, certs):
    """u64 sets: the records of cert_verdict_dev.h, which must carry the class and the sender bit of level0_records; a u256 set
    (the verdict harness of this module takes u64 powers): level0_records itself"""
    own = level0_records(cv, n)
    if certs is None:
        return own
    for f in ("row", "cls", "type", "from_len", "height", "round"):
        assert (certs[:n][f] == own[f]).all(), f
    assert ((certs[:n]["bits"] & V.CERT_BIT_SENDER) == own["bits"]).all() and certs[:n]["from"].tobytes() == own["from"].tobytes()
    return certs


def test_struct_sizes_agree(lib):
    assert [lib.rch_sizeof(i) for i in range(3)] == [V.RC_QUERY.itemsize, V.RC_RECORD.itemsize, V.RC_ANSWER.itemsize] == [32, 128, 64]


def test_every_case_against_the_model_in_any_order(lib, judge_lib):
    seen = {"has_quorum": set(), "extended": set()}
    for c in RK.all_cases():
        r, powers = RK.make_round(c.powers), RK.powers_of(c.powers)
        cv, certs, dec = world(judge_lib, r, powers, c)
        n = len(c.msgs)
        certs = certs_for(cv, n, certs)
        q = query_of(c)
        want = RM.expected(cv, n, dec["round_change"], q[0], c.rc_cap)
        RK.check_construction(c, want)             # the model alone reaches what the construction fixes
        if c.label.startswith("two heights"):      # … and the mixed batch has its PREPREPARE root and its root for the host
            assert [int(x != 0) for x in cv.cls[:n]] == [0, 0, 0, 0, 0, 1, 0, 0] and not RM.takes_part(cv, 2) and not RM.takes_part(cv, 5)
        seen["has_quorum"] |= {int(x) for x in want.records["has_quorum"]}
        seen["extended"].add(int(want.answer["extended"]))
        rng = random.Random(len(c.label))
        first = None
        for hook, salt in ((0, 0x1234), (1, 0), (1, 0xDEADBEEF), (4 * n, 7)):
            order = list(range(n))
            rng.shuffle(order)
            got = run(lib, r, powers, cv, certs, dec, n, q, c.rc_cap, order, hook, salt)
            RM.check((c.label, hook, salt), want, got)
            blob = b"".join(np.asarray(x).tobytes() for x in got[:3]) + got[4].tobytes()
            assert first is None or blob == first, (c.label, "outputs differ between table sizes, salts or insert orders")
            first = blob
        no_answer = run(lib, r, powers, cv, certs, dec, n, None, c.rc_cap)
        RM.check((c.label, "no query"), RM.expected(cv, n, dec["round_change"], None, c.rc_cap), no_answer)
    assert seen["has_quorum"] == {-1, 0, 1} and seen["extended"] == {-1, 0, 1}


def test_seventy_senders_of_one_round(lib, judge_lib):
    r, powers, c = RK.seventy_senders_case()
    cv, certs, dec = world(judge_lib, r, powers, c)
    n = len(c.msgs)
    q = query_of(c)
    want = RM.expected(cv, n, dec["round_change"], q[0], None)
    RK.check_construction(c, want)
    order = list(range(n))
    random.Random(5).shuffle(order)
    RM.check(c.label, want, run(lib, r, powers, cv, certs, dec, n, q, None, order, 1, 99))


# ---- the selection on the emulated wavefront -----------------------------------------------------------------------------------
def records_of(rounds, quorums, stored, height=5):
    recs = np.zeros(len(rounds), dtype=V.RC_RECORD)
    recs["height"], recs["round"], recs["has_quorum"], recs["stored_rows"] = height, rounds, quorums, stored
    return recs


def select(lib, recs, query, n_keys=None, cap=None, unjudged=3):
    out = np.zeros(1, dtype=V.RC_ANSWER)
    n_keys = len(recs) if n_keys is None else n_keys
    cap = len(recs) if cap is None else cap
    assert lib.rch_select(_p(recs), len(recs), n_keys, cap, unjudged, _p(query), _p(out)) == 0, "the lanes disagree"
    return out[0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 + 7, 200])
def test_selection_across_lanes(lib, n):
    rng = random.Random(n)
    q = V.rc_query(5, 0)
    spots = sorted({0, 63 % n, n - 1, (64 + 7) % n})      # lane 0, lane 63, record 64 + k, the last
    for spot in spots:
        for hq in (1, -1):
            rounds = np.array(rng.sample(range(1, 10 * n + 1), n), dtype=np.uint64)
            rounds[spot] = 20 * n                                        # the winner sits at `spot`
            quorums = np.array([rng.choice([0, 0, 1, -1]) for _ in range(n)], dtype=np.int8)
            quorums[spot] = hq
            stored = np.array([rng.randrange(1, 5) for _ in range(n)], dtype=np.uint32)
            recs = records_of(rounds, quorums, stored)
            got = select(lib, recs, q)
            want = RM.answer(recs, n, n, 3, q[0])
            assert got.tobytes() == want.tobytes(), (n, spot, hq, got, want)
            assert int(got["extended"]) == hq
    # equal stored_rows everywhere: the LOWEST round wins most_*, wherever it sits
    for spot in spots:
        rounds = np.arange(2, n + 2, dtype=np.uint64)
        rounds[spot], rounds[0] = 1, rounds[spot] if spot else 1
        recs = records_of(rounds, np.zeros(n, dtype=np.int8), np.full(n, 4, dtype=np.uint32))
        got = select(lib, recs, q)
        assert got.tobytes() == RM.answer(recs, n, n, 3, q[0]).tobytes()
        assert (int(got["most_record"]), int(got["most_round"]), int(got["most_rows"])) == (spot, 1, 4), (n, spot, got)
    # other heights, round 0, the accepted round and min_round take no part; rounds beyond 32 bits compare in full
    rounds = np.array([(2**40 + k) if k % 3 else k for k in range(n)], dtype=np.uint64)
    recs = records_of(rounds, np.ones(n, dtype=np.int8), np.arange(n, dtype=np.uint32) % 7)
    recs["height"][::2] = 6
    for query in (V.rc_query(5, int(rounds[n - 1]), True, 2**40), V.rc_query(6, 0, False, 0), V.rc_query(7, 0)):
        got = select(lib, recs, query, n_keys=n + 5, cap=n)
        assert got.tobytes() == RM.answer(recs, n + 5, n, 3, query[0]).tobytes(), (n, query, got)


# ---- an independent check through the host mirror ------------------------------------------------------------------------------
def test_answers_against_the_mirrors_store(lib, judge_lib):
    for c in RK.all_cases():
        if c.rc_cap is not None:
            continue                                   # (the store knows no cap)
        r, powers = RK.make_round(c.powers), RK.powers_of(c.powers)
        cv, certs, dec = world(judge_lib, r, powers, c)
        n = len(c.msgs)
        q = query_of(c)
        want = RM.expected(cv, n, dec["round_change"], q[0], None)
        host = hostlib.Host()
        closure = {}
        for i in range(n):
            if RM.takes_part(cv, i):
                host.store_add(c.msgs[i])
                closure[c.msgs[i]] = int(dec["round_change"][i])
        height = c.query[0]
        quorum_of = {int(x["round"]): int(x["has_quorum"]) for x in want.records if int(x["height"]) == height}
        accepted_round = c.query[1] if c.query[2] else None
        ext = int(want.answer["extended"])
        if ext in (0, 1):
            # the message predicate: the decision; the RCC predicate: the model's quorum (and the node's own accepted round never counts)
            got = host.store_get_extended_rcc(height, lambda m: closure[m] == 1, lambda rnd, k: rnd != accepted_round and quorum_of.get(rnd) == 1)
            rec = int(want.answer["record"])
            held = [] if ext == 0 else [c.msgs[i] for i in sorted(want.keys[rec].stored.values()) if int(dec["round_change"][i]) == 1]
            assert sorted(got) == sorted(held), (c.label, len(got), len(held))
        most = host.store_get_most_rc(c.query[3], height)
        assert len(most) == int(want.answer["most_rows"]), (c.label, len(most), int(want.answer["most_rows"]))
