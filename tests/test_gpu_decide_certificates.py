"""ibft_decide_certificates_wire on the GPU: one decision per record under the proposer table of ibft_set_proposers
(cert_decide_records_kernel, cert_decide_proposals_kernel, cert_decide_dev.h) against tests/cert_decision_model.py applied to
what ibft_verify_certificates_wire answers for the same bytes on the same context; every output the judge call has equals the
judge call's, byte for byte."""
import numpy as np
import pytest

import cert_cases as CC
import cert_decision_cases as DK
import cert_decision_model as DM
import cert_verdict_cases as K
import cert_verdict_model as M

pytestmark = pytest.mark.gpu
CAP = 4096


def make_bv(powers, addrs, flags=0, u256=False):
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=flags, max_rows=CAP)
    if u256:
        bv.set_validators_u256(K.H, addrs, powers)
    else:
        bv.set_validators(K.H, addrs, np.asarray(powers, dtype=np.uint64))
    return bv


def install(bv, table):
    if table is None:
        bv.set_proposers(0, 0, [])
        assert bv.proposers_info() == (0, 0, 0)
    else:
        bv.set_proposers(table.height, table.first_round, table.addrs)
        assert bv.proposers_info() == (table.height, table.first_round, len(table.addrs))


def rows_of(bv, msgs, addrs, powers):
    """ibft_verify_certificates_wire's answer as the models read it"""
    buf, off = CC.pack(msgs)
    n, nodes, rows, cls, sender, hb, sb = bv.verify_certificates_wire(buf, off, rows_cap=CAP)
    pw = {bytes(a): int(p) for a, p in zip(addrs, powers)}
    return M.Rows(n, nodes, rows, cls, sender, hb, sb, pw, 2 * sum(pw.values()) // 3 + 1)


def same_as_judge(label, judge_out, decide_out):
    """out_cert and every per-row output: the judge call's bytes"""
    jc, jn, jrow = judge_out
    dc, _, dn, drow = decide_out
    assert jn == dn and jc.tobytes() == dc.tobytes(), (label, "records")
    for a, b in zip(jrow, drow):
        assert a.tobytes() == b.tobytes(), (label, "per-row outputs")


def check_case(bv, r, powers, c, tables, seen=None, cv=None):
    """the case under every table: decisions against the model, everything else against the judge call → decisions by table name"""
    addrs = [a.tobytes() for a in r.addrs]
    buf, off = CC.pack(c.msgs)
    cv = cv or rows_of(bv, c.msgs, addrs, powers)
    judge_out = bv.judge_certificates_wire(buf, off, rows_cap=CAP, per_row=True)
    out = {}
    for name, table in tables:
        install(bv, table)
        got = bv.decide_certificates_wire(buf, off, rows_cap=CAP, per_row=True)
        same_as_judge((c.label, name), judge_out, got)
        certs, dec = got[0], got[1]
        want = DM.check_decisions((c.label, name), cv, len(c.msgs), table, buf, certs, dec)
        for i, (fld, v) in (c.expect if name == "covering" else c.expect_under.get(name, {})).items():
            assert int(dec[i][fld]) == v, (c.label, name, i, fld, int(dec[i][fld]), v)
        if name == "covering":
            for i, (k, rnd) in c.prepared.items():
                assert (int(dec[i]["prepared_record"]), int(dec[i]["prepared_round"])) == (int(certs[i]["first_child_cert"]) + k, rnd), (c.label, i)
            for i in range(len(c.msgs)):
                w = cv.rows[i]
                if seen is not None and w["status"] == 0 and w["type"] == M.ROUND_CHANGE:
                    seen["round_change"].add(int(dec[i]["round_change"]))
                    assert c.irregular or int(dec[i]["round_change"]) != -1, (c.label, i)
                if seen is not None and w["status"] == 0 and w["type"] == M.PREPREPARE and w["payload_kind"] == 5 and w["has_view"]:
                    seen["proposal"].add(int(dec[i]["proposal"]))
                    assert c.irregular or int(dec[i]["proposal"]) != -1, (c.label, i)
        out[name] = want
    # the judge call with a table installed: what it was without one
    again = bv.judge_certificates_wire(buf, off, rows_cap=CAP, per_row=True)
    assert again[0].tobytes() == judge_out[0].tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(again[2], judge_out[2])), c.label
    return out


def test_every_case_under_every_table():
    r, cases = DK.all_cases()
    addrs = [a.tobytes() for a in r.addrs]
    tables = DM.tables_for(addrs, DK.H, DK.RND)
    seen = {"round_change": set(), "proposal": set()}
    bv = make_bv(K.POWERS, r.addrs)
    try:
        for c in cases:
            check_case(bv, r, K.POWERS, c, tables, seen)
    finally:
        bv.close()
    assert seen["round_change"] == {-1, 0, 1} and seen["proposal"] == {-1, 0, 1}


def chosen_cases():
    """what the variants below run: the mixed roots, the proposal cases and one batch of the length sweep"""
    r, cases = DK.all_cases()
    keep = [c for c in cases if c.label == "mixed roots" or c.prepared or c.label.startswith("round 0") or c.label.startswith("from is not")]
    sweeps = [c for c in keep if c.label.startswith("proposal lengths")]
    return r, [c for c in keep if c not in sweeps[1:]]


@pytest.mark.parametrize("dedup,overlap", [("1", "1"), ("0", "0"), ("1", "0")], ids=["dedup", "one stream", "dedup, one stream"])
def test_dedup_and_overlap_change_no_byte(monkeypatch, dedup, overlap):
    import go_ibft_amd.verifier as V
    r, cases = chosen_cases()
    addrs = [a.tobytes() for a in r.addrs]
    tables = DM.tables_for(addrs, DK.H, DK.RND)[:2]
    monkeypatch.delenv("IBFT_CERT_DEDUP", raising=False)
    monkeypatch.delenv("IBFT_CERT_OVERLAP", raising=False)
    plain = make_bv(K.POWERS, r.addrs, flags=V.FLAG_PUBKEY_CACHE)
    monkeypatch.setenv("IBFT_CERT_DEDUP", dedup)
    monkeypatch.setenv("IBFT_CERT_OVERLAP", overlap)
    other = make_bv(K.POWERS, r.addrs, flags=V.FLAG_PUBKEY_CACHE)
    try:
        for c in cases:
            buf, off = CC.pack(c.msgs)
            cv = rows_of(plain, c.msgs, addrs, K.POWERS)
            for name, table in tables:
                install(plain, table), install(other, table)
                a = plain.decide_certificates_wire(buf, off, rows_cap=CAP, per_row=True)
                b = other.decide_certificates_wire(buf, off, rows_cap=CAP, per_row=True)   # (from its second call on: warm kernels, two verdict launches)
                DM.check_decisions((c.label, name), cv, len(c.msgs), table, buf, a[0], a[1])
                assert a[1].tobytes() == b[1].tobytes() and a[0].tobytes() == b[0].tobytes() and a[2] == b[2], (c.label, name)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a[3], b[3])), (c.label, name)
    finally:
        plain.close(); other.close()


def test_u256_set():
    r, cases = chosen_cases()
    addrs = [a.tobytes() for a in r.addrs]
    tables = DM.tables_for(addrs, DK.H, DK.RND)[:1]
    bv = make_bv(K.POWERS_U256, r.addrs, u256=True)
    try:
        for c in cases:
            check_case(bv, r, K.POWERS_U256, c, tables)
    finally:
        bv.close()


def test_seventy_round_changes():
    """a RoundChangeCertificate of 70 messages: the winner sits at child k + 64 of a lane, or in another lane than its equals"""
    r, powers, cases = DK.big_tree_cases()
    addrs = [a.tobytes() for a in r.addrs]
    tables = [t for t in DM.tables_for(addrs, DK.H, DK.RND) if t[0] in ("covering", "shifted", "no table")]
    bv = make_bv(powers, r.addrs)
    try:
        for c in cases:
            check_case(bv, r, powers, c, tables)
    finally:
        bv.close()


def test_the_table_is_replaced_cleared_and_left_alone_by_set_validators():
    import go_ibft_amd.verifier as V
    r, cases = DK.all_cases()
    addrs = [a.tobytes() for a in r.addrs]
    c = next(x for x in cases if x.label == "re-proposal of the highest prepared round")
    buf, off = CC.pack(c.msgs)
    named = dict(DM.tables_for(addrs, DK.H, DK.RND))
    bv = make_bv(K.POWERS, r.addrs)
    try:
        cv = rows_of(bv, c.msgs, addrs, K.POWERS)
        assert bv.proposers_info() == (0, 0, 0)

        def decide(table):
            certs, dec, _, _ = bv.decide_certificates_wire(buf, off, rows_cap=CAP)
            DM.check_decisions(c.label, cv, 1, table, buf, certs, dec)
            return int(dec[0]["proposal"])
        assert decide(None) == -1                                   # before any table
        install(bv, named["covering"])
        assert decide(named["covering"]) == 1
        install(bv, named["shifted"])                               # replaced between two calls
        assert decide(named["shifted"]) == 0
        install(bv, named["covering"])
        bv.set_validators(K.H, r.addrs, np.asarray(K.POWERS, dtype=np.uint64))      # the validator set again: the table stays
        assert bv.proposers_info() == (DK.H, 0, 8) and decide(named["covering"]) == 1
        # refused calls leave the table in place
        for height, first, table_addrs, code in ((DK.H, 2**64 - 3, addrs[:4], "-1"), (DK.H, 0, addrs * 410, "-7")):
            with pytest.raises(RuntimeError):
                bv.set_proposers(height, first, table_addrs)
        rc = bv._L.ibft_set_proposers(bv._h, DK.H, 0, None, 3)
        assert rc == -1 and bv.proposers_info() == (DK.H, 0, 8) and decide(named["covering"]) == 1
        assert bv._L.ibft_set_proposers(bv._h, DK.H, 2**64 - 3, V._p(np.zeros(80, dtype=np.uint8)), 4) == -1       # the range runs past 2^64
        assert bv._L.ibft_set_proposers(bv._h, DK.H, 0, V._p(np.zeros(20 * 4097, dtype=np.uint8)), 4097) == -7     # IBFT_E_TOOBIG
        assert decide(named["covering"]) == 1
        # the largest table, its last round asked
        last = DM.Table(DK.H, 0, [addrs[0]] * 4095 + [addrs[(DK.H + 0) % len(addrs)]])
        bv.set_proposers(DK.H, 2**64 - 4097, last.addrs)
        assert bv.proposers_info() == (DK.H, 2**64 - 4097, 4096)
        install(bv, None)                                           # cleared
        assert decide(None) == -1
        # a NULL out_decision with n > 0
        import ctypes as C
        a, b = C.c_size_t(7), C.c_size_t(7)
        cert = np.zeros(64, dtype=V.CERT_VERDICT)
        wb = np.frombuffer(buf, dtype=np.uint8)
        assert bv._L.ibft_decide_certificates_wire(bv._h, V._p(wb), V._p(off), 1, CAP, 64, C.byref(a), C.byref(b), V._p(cert), None,
                                                   None, None, None, None, None, None) == -1
        assert (a.value, b.value) == (7, 7) and not cert.view(np.uint8).any()
    finally:
        bv.close()


def test_device_group_decides_on_its_first_context():
    import go_ibft_amd.verifier as V
    r, cases = DK.all_cases()
    addrs = [a.tobytes() for a in r.addrs]
    c = next(x for x in cases if x.label == "one round prepared twice, the last proposed")
    buf, off = CC.pack(c.msgs)
    name, table = DM.tables_for(addrs, DK.H, DK.RND)[0]
    g = V.DeviceGroup([0, 0], max_rows_total=2 * CAP)
    try:
        g.set_validators(K.H, r.addrs, np.asarray(K.POWERS, dtype=np.uint64))
        g.set_proposers(table.height, table.first_round, table.addrs)
        assert g.proposers_info() == (table.height, table.first_round, len(table.addrs))
        certs, dec, n_rows, _ = g.decide_certificates_wire(buf, off, rows_cap=CAP)
        jc, jn, _ = g.judge_certificates_wire(buf, off, rows_cap=CAP)
        assert jc.tobytes() == certs.tobytes() and jn == n_rows
        assert int(dec[0]["proposal"]) == 1 and int(dec[0]["flags"]) == V.CERT_DECISION_HAS_PREPARED
    finally:
        g.close()
