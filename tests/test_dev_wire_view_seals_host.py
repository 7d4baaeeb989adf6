"""The row bodies of the wire_seals_*_kernel launches (csrc/wire_seals_dev.h) and the seal form of the views stage
(csrc/wire_views_dev.h), compiled for the host (csrc/host_wire_view_seals_harness.hip), against the plain model of
tests/wire_view_seals_model.py on corpora S and C: the sealable decision with its membership lookup and the dense order of the
seal rows, how seal verdicts and final sender bits combine into seal bits, and the records — PREPARE records the views
stage's, COMMIT records over stored ∧ sealed — at several table sizes, salts and caps, u64 and u256 pieces."""
import random

import numpy as np
import pytest

import wire_sets_cases as WS
import wire_view_seals_cases as SC
import wire_view_seals_harness as SH
import wire_view_seals_model as SM
import wire_views_cases as VC
import wire_views_harness as H


@pytest.fixture(scope="module")
def dev():
    return SH.load()


def _columns(e):
    return SH.parsed_columns(e["parsed"]), np.array(e["bits"], np.uint8), np.array(e["vidx"], np.int32), np.array(e["set"], np.int32)


CASES = [("s", False, False), ("s", False, True), ("s", True, False), ("c", False, False)]


def _case(name, big, recode):
    c = SC.corpus_s(big) if name == "s" else SC.corpus_c()
    cap = len(c.msgs) if name == "s" else SC.C_CAP
    return c, cap, SC.expected(c, WS.MAP_A, recode, cap)


@pytest.mark.parametrize("name,big,recode", CASES)
def test_sealable_decision_and_dense_order(dev, oracle, name, big, recode):
    L, LV = dev
    c, cap, e = _case(name, big, recode)
    t = H.Tables(LV, c.model_sets(), 4 if big else 1, VC.proposers(c))
    rows, valid, vidx, rset = _columns(e)
    flags, seal_row, src, seal_rows, commit_rows = SH.stage(L, t, rows, rset)
    sets = c.model_sets()
    want = [(SH.ROW_COMMIT if SM.is_commit(p, e["set"][j]) else 0) | (SH.ROW_SEALABLE if SM.is_sealable(p, e["set"][j], sets) else 0)
            for j, p in enumerate(e["parsed"])]
    assert flags == want
    assert src == e["dense"] and (seal_rows, commit_rows) == (e["seal_rows"], e["commit_rows"])
    assert [seal_row[j] for j in src] == list(range(len(src)))
    assert all(seal_row[j] == SH.NONE for j in range(len(rows)) if j not in set(src))


@pytest.mark.parametrize("name,big,recode", CASES)
def test_seal_bits_combine(dev, oracle, name, big, recode):
    """the verdict bit of a seal row is the bare seal check (the verdict launch knows nothing of the envelope): the row's seal
    bit needs the final sender bit as well"""
    L, LV = dev
    c, cap, e = _case(name, big, recode)
    t = H.Tables(LV, c.model_sets(), 4 if big else 1)
    rows, valid, vidx, rset = _columns(e)
    _, seal_row, src, _, _ = SH.stage(L, t, rows, rset)
    p = e["parsed"]
    verdicts = [SC.B.recover_address(p[j].proposal_hash, p[j].committed_seal) == p[j].sender for j in src]
    assert SH.combine(L, e["bits"], seal_row, verdicts) == e["seal"]
    if name == "s" and not recode:
        (j,) = [k for k, kind in enumerate(c.kinds) if kind == "sig_flip"]
        assert verdicts[src.index(j)] and not e["seal"][j]              # a perfect seal under a bad envelope
    # every seal verdict set: exactly the valid sealable rows; none set: nothing
    assert SH.combine(L, e["bits"], seal_row, [True] * len(src)) == [bool(e["bits"][j]) and j in set(src) for j in range(len(rows))]
    assert not any(SH.combine(L, e["bits"], seal_row, [False] * len(src)))
    assert not any(SH.combine(L, [0] * len(rows), seal_row, [True] * len(src)))


@pytest.mark.parametrize("name,big,recode", CASES)
def test_records(dev, oracle, name, big, recode):
    L, LV = dev
    c, cap, e = _case(name, big, recode)
    t = H.Tables(LV, c.model_sets(), 4 if big else 1, VC.proposers(c))
    rows, valid, vidx, rset = _columns(e)
    n = len(rows)
    floor = LV.wvh_table_slots(n, 1)
    for slots, salt in ((LV.wvh_table_slots(n, 0), 12345), (floor, 0), (floor, 0xDEADBEEF), (4 * floor, 999)):
        view, stored, n_views, recs = SH.run(L, t, rows, valid, vidx, rset, e["seal"], cap, slots, salt)
        assert (view, stored, n_views) == (e["view"], e["stored"], e["n_views"])
        assert recs == [SH.model_record(w) for w in e["records"]]
    # against the plain views stage: only pad[0] and tally of COMMIT records differ
    plain = H.run(LV, t, rows, valid, vidx, rset, cap, floor, 7)[3]
    assert len(plain) == len(recs) and plain == [SH.model_record(w) for w in e["views_records"]]
    for a, b in zip(plain, recs):
        if a["type"] == SM.COMMIT:
            assert b["pad"] == bytes([1, 0, 0, 0, 0]) and {k: v for k, v in a.items() if k not in ("pad", "tally")} == {
                k: v for k, v in b.items() if k not in ("pad", "tally")}
            assert b["tally"]["valid_rows"] <= b["stored_rows"]
        else:
            assert a == b


def test_caps_and_random_seal_masks(dev, oracle):
    """corpus S at small caps and under random seal masks: whatever the seal bits are, the records follow the model"""
    L, LV = dev
    c = SC.corpus_s()
    n = len(c.msgs)
    e = SC.expected(c, WS.MAP_A, False, n)
    t = H.Tables(LV, c.model_sets(), 1, VC.proposers(c))
    rows, valid, vidx, rset = _columns(e)
    rng = random.Random(31)
    for cap in (1, e["n_views"] - 1, n + 5):
        seal = [bool(e["bits"][j]) and rng.random() < 0.6 for j in range(n)]
        view, stored, n_views, want = SM.views(e["rows"], seal, cap, c.model_sets(), VC.proposers(c))
        got = SH.run(L, t, rows, valid, vidx, rset, seal, cap, LV.wvh_table_slots(n, 0), cap)
        assert got[:3] == (view, stored, n_views) and got[3] == [SH.model_record(w) for w in want]
