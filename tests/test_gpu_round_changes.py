"""ibft_decide_round_changes_wire on the GPU (round_change_*_kernel, round_change_dev.h): every case of
tests/round_change_cases.py through the C ABI against tests/round_change_model.py applied to what
ibft_verify_certificates_wire and ibft_decide_certificates_wire answer for the same bytes on the same context; every record's
tally against ibft_tally over its stored yes rows; every shared output against the decide call's, byte for byte."""
import numpy as np
import pytest

import cert_cases as CC
import cert_decision_model as DM
import cert_verdict_cases as K
import round_change_cases as RK
import round_change_model as RM
from test_dev_round_change_host import query_of
from test_gpu_decide_certificates import install, make_bv, rows_of

pytestmark = pytest.mark.gpu
CAP = 4096
TALLY_FIELDS = ("quorum_lo", "quorum_hi", "power_lo", "power_hi", "valid_rows", "distinct_senders", "has_quorum", "shard_overlap", "proposer_rows")


def tables(r):
    return dict(DM.tables_for([a.tobytes() for a in r.addrs], RK.H, 2))


def same_as_decide(label, decide_out, got):
    dc, dd, dn, drow = decide_out
    assert got[2] == dn and got[0].tobytes() == dc.tobytes() and got[1].tobytes() == dd.tobytes(), (label, "records / decisions")
    for a, b in zip(drow, got[3]):
        assert a.tobytes() == b.tobytes(), (label, "per-row outputs")


def run_case(bv, r, powers, c, table, check_tally=True):
    addrs = [a.tobytes() for a in r.addrs]
    buf, off = CC.pack(c.msgs)
    n = len(c.msgs)
    install(bv, table)
    cv = rows_of(bv, c.msgs, addrs, powers)
    decide_out = bv.decide_certificates_wire(buf, off, rows_cap=CAP, per_row=True)
    q = query_of(c)
    got = bv.decide_round_changes_wire(buf, off, q, rows_cap=CAP, rc_cap=c.rc_cap, per_row=True)
    same_as_decide(c.label, decide_out, got)
    dec = got[1]
    DM.check_decisions(c.label, cv, n, table, buf, got[0], dec)
    want = RM.expected(cv, n, dec["round_change"][:n], q[0], c.rc_cap)
    RK.check_construction(c, want)
    RM.check(c.label, want, got[4])
    if check_tally:
        for v, key in enumerate(want.keys):
            yes = [i for i in sorted(key.stored.values()) if int(dec[i]["round_change"]) == 1]
            col = np.ascontiguousarray(cv.rows["from"][yes], dtype=np.uint8).reshape(-1, 20)
            t = bv.has_quorum(col, np.ones(len(yes), dtype=bool))
            rec = got[4][2][v]["tally"]
            full_q, full_p = int(t.quorum), int(t.power)
            want_t = (full_q & (2**64 - 1), (full_q >> 64) & (2**64 - 1), full_p & (2**64 - 1), (full_p >> 64) & (2**64 - 1), int(t.valid_rows),
                      int(t.distinct_senders), int(t.has_quorum), int(t.shard_overlap), int(t.proposer_rows))
            assert tuple(int(rec[f]) for f in TALLY_FIELDS) == want_t and int(rec["reserved"]) == 0, (c.label, "record", v, rec, want_t)
    return got


def blob(got):
    view, stored, recs, n_rc, ans = got[4]
    return view.tobytes() + stored.tobytes() + recs.tobytes() + bytes([n_rc & 0xFF]) + (ans.tobytes() if ans is not None else b"")


def test_every_case_against_the_model():
    seen = {"has_quorum": set(), "extended": set()}
    bvs = {}
    try:
        for c in RK.all_cases():
            r, powers = RK.make_round(c.powers), RK.powers_of(c.powers)
            if c.powers not in bvs:
                bvs[c.powers] = make_bv(powers, r.addrs, u256=c.powers == "u256")
            got = run_case(bvs[c.powers], r, powers, c, tables(r)[c.table])
            seen["has_quorum"] |= {int(x) for x in got[4][2]["has_quorum"]}
            seen["extended"].add(int(got[4][4]["extended"]))
    finally:
        for bv in bvs.values():
            bv.close()
    assert seen["has_quorum"] == {-1, 0, 1} and seen["extended"] == {-1, 0, 1}


def test_seventy_senders_of_one_round():
    r, powers, c = RK.seventy_senders_case()
    bv = make_bv(powers, r.addrs)
    try:
        got = run_case(bv, r, powers, c, None)
        assert int(got[4][2][0]["stored_rows"]) == RK.SEVENTY and int(got[4][2][0]["has_quorum"]) == 1
    finally:
        bv.close()


def chosen_cases():
    keep = ("a sender twice, valid then invalid", "a later row with a spoiled", "two heights interleaved", "more keys than rc_cap",
            "70 rounds from one sender", "a batch of 257")
    return [c for c in RK.all_cases() if c.label.startswith(keep)]


@pytest.mark.parametrize("dedup,overlap,slots", [("1", "1", None), ("0", "0", None), ("1", "0", "1"), ("0", "1", "1")],
                         ids=["dedup", "one stream", "dedup, one stream, slot floor", "slot floor"])
def test_combinations_that_change_no_byte(monkeypatch, dedup, overlap, slots):
    """dedup × overlap, a warm context on its second call, the slot hook at its floor: the new outputs are the plain context's"""
    import go_ibft_amd.verifier as V
    r = RK.make_round("u64")
    for name in ("IBFT_CERT_DEDUP", "IBFT_CERT_OVERLAP", "IBFT_ROUND_CHANGE_SLOTS"):
        monkeypatch.delenv(name, raising=False)
    plain = make_bv(K.POWERS, r.addrs)
    monkeypatch.setenv("IBFT_CERT_DEDUP", dedup)
    monkeypatch.setenv("IBFT_CERT_OVERLAP", overlap)
    if slots:
        monkeypatch.setenv("IBFT_ROUND_CHANGE_SLOTS", slots)
    other = make_bv(K.POWERS, r.addrs, flags=V.FLAG_PUBKEY_CACHE)
    try:
        for c in chosen_cases():
            table = tables(r)[c.table]
            a = run_case(plain, r, K.POWERS, c, table, check_tally=False)
            for call in ("cold", "warm"):                      # the second call of `other` runs the known-key kernels
                b = run_case(other, r, K.POWERS, c, table, check_tally=call == "warm")
                assert blob(a) == blob(b), (c.label, call)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (c.label, call)
    finally:
        plain.close(); other.close()


def test_two_batches_in_sequence_with_a_views_call_between():
    """nothing stale: tables, accumulators and words of the first batch do not reach the second, whatever ran between them"""
    r = RK.make_round("u64")
    cases = {c.label: c for c in RK.all_cases()}
    first, second = cases["70 rounds from one sender beside a quorum"], cases["one power short of the quorum"]
    bv = make_bv(K.POWERS, r.addrs)
    fresh = make_bv(K.POWERS, r.addrs)
    try:
        table = tables(r)["covering"]
        run_case(bv, r, K.POWERS, first, table, check_tally=False)
        # a views call on the same context: the same tables' code over other buffers
        bv.set_validator_sets([(r.addrs, np.asarray(K.POWERS, dtype=np.uint64))])
        bv.set_height_sets([0, 2**63], [0])
        buf, off = CC.pack(second.msgs)
        bv.verify_senders_wire_views(buf, off, len(second.msgs))
        bv.set_validators(K.H, r.addrs, np.asarray(K.POWERS, dtype=np.uint64))
        a = run_case(bv, r, K.POWERS, second, table)
        b = run_case(fresh, r, K.POWERS, second, table)
        assert blob(a) == blob(b)
        c = run_case(bv, r, K.POWERS, first, table, check_tally=False)      # and the long batch again behind the short one
        assert blob(c) == blob(run_case(fresh, r, K.POWERS, first, table, check_tally=False))
    finally:
        bv.close(); fresh.close()


def test_device_group_on_its_first_context():
    import go_ibft_amd.verifier as V
    r = RK.make_round("u64")
    c = next(x for x in RK.all_cases() if x.label.startswith("two rounds with a quorum"))
    buf, off = CC.pack(c.msgs)
    table = tables(r)["covering"]
    g = V.DeviceGroup([0, 0], max_rows_total=2 * CAP)
    try:
        g.set_validators(K.H, r.addrs, np.asarray(K.POWERS, dtype=np.uint64))
        g.set_proposers(table.height, table.first_round, table.addrs)
        certs, dec, n_rows, _, rc = g.decide_round_changes_wire(buf, off, query_of(c), rows_cap=CAP)
        dc, dd, dn, _ = g.decide_certificates_wire(buf, off, rows_cap=CAP)
        assert dc.tobytes() == certs.tobytes() and dd.tobytes() == dec.tobytes() and dn == n_rows
        assert rc[3] == 2 and (int(rc[4]["extended"]), int(rc[4]["round"]), int(rc[4]["record"])) == (1, 3, 1)
    finally:
        g.close()


def test_a_null_query_and_null_optional_outputs():
    import ctypes as C
    import go_ibft_amd.verifier as V
    r = RK.make_round("u64")
    c = next(x for x in RK.all_cases() if x.label.startswith("two rounds with a quorum"))
    buf, off = CC.pack(c.msgs)
    n = len(c.msgs)
    bv = make_bv(K.POWERS, r.addrs)
    try:
        install(bv, tables(r)["covering"])
        with_q = bv.decide_round_changes_wire(buf, off, query_of(c), rows_cap=CAP)
        without = bv.decide_round_changes_wire(buf, off, None, rows_cap=CAP)
        assert without[4][4] is None and blob(with_q)[:-64] == blob(without)
        # the answer buffer of a call without a query stays as it was; view, stored and answer may be NULL
        L, p = bv._L, V._p
        wb = np.frombuffer(buf, dtype=np.uint8)
        certs, decs = np.zeros(n, dtype=V.CERT_VERDICT), np.zeros(n, dtype=V.CERT_DECISION)
        recs, ans = np.zeros(n, dtype=V.RC_RECORD), np.full(64, 0x6B, np.uint8)
        a, b, k = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        args = (bv._h, p(wb), p(off), n, CAP, n, C.byref(a), C.byref(b), p(certs), p(decs), None, None, None, None, None, None)
        assert L.ibft_decide_round_changes_wire(*args, None, None, None, p(recs), n, C.byref(k), p(ans)) == 0
        assert (ans == 0x6B).all() and k.value == 2 and recs[:2].tobytes() == with_q[4][2].tobytes()
        assert L.ibft_decide_round_changes_wire(*args, p(query_of(c)), None, None, p(recs), 10**9, C.byref(k), None) == 0      # a cap above n behaves as n
        assert k.value == 2 and recs[:2].tobytes() == with_q[4][2].tobytes() and not recs[2:].view(np.uint8).any()
    finally:
        bv.close()
