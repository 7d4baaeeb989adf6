"""The corpora of tests/test_gpu_wire_views.py hold every case they claim (tests/wire_views_cases.py), checked on the CPU with
the oracle's walk and the plain model; and for every GPU input the longest probe run of both tables — at the default slot
count and at the hooked floor, under several salts — stays below the slot count, so no GPU test can reach the table-exhausted
error."""
import numpy as np
import pytest

import wire_sets_cases as WS
import wire_views_cases as VC
import wire_views_harness as H
import wire_views_model as VM


@pytest.fixture(scope="module")
def dev():
    return H.load()


def _rows_of(c, e, kind):
    return [j for j, k in enumerate(c.kinds) if k == kind]


def test_corpus_a_holds_its_cases(oracle):
    c = VC.corpus_a()
    n = len(c.msgs)
    assert 330 <= n <= 390
    e = VC.expected(c, WS.MAP_A, False, n)
    recs = {(r["height"], r["round"], r["type"], r["hash"]): r for r in e["records"]}
    parsed, bits, stored, view = e["parsed"], e["bits"], e["stored"], e["view"]
    valid = [j for j in range(n) if bits[j]]
    assert {parsed[j].round for j in valid} == {0, 1, 2} and {parsed[j].type for j in valid} == {VM.PREPARE, VM.COMMIT}
    assert {e["set"][j] for j in valid} == {0, 1, 2}
    # two proposal hashes in one view
    assert (100, 0, VM.PREPARE, VC.HA) in recs and (100, 0, VM.PREPARE, VC.HB) in recs
    # a sender twice under one key: the earlier row is superseded, the record counts the sender once
    (tw,) = _rows_of(c, e, "twice")
    first = next(j for j in valid if c.senders[j] == VC.TWICE and view[j] == view[tw])
    assert first < tw and not stored[first] and stored[tw]
    r = recs[(100, 0, VM.PREPARE, VC.HA)]
    assert r["rows"] == r["stored_rows"] + 2                     # … and the changer's HA row
    # hash A then B: two records change
    (ch,) = _rows_of(c, e, "changer")
    early = next(j for j in valid if c.senders[j] == VC.CHANGER and parsed[j].round == 0 and parsed[j].type == VM.PREPARE and j < ch)
    assert view[early] != view[ch] and not stored[early] and stored[ch]
    assert recs[(100, 0, VM.PREPARE, VC.HB)]["stored_rows"] == 4 and c.pool.addrs[VC.CHANGER].tobytes() in recs[(100, 0, VM.PREPARE, VC.HB)]["senders"]
    # the same sender in two rounds: nothing is superseded
    js = [j for j in valid if c.senders[j] == VC.CROSS_ROUND and parsed[j].type == VM.COMMIT and parsed[j].height == 100]
    assert len(js) == 3 and all(stored[j] for j in js) and len({view[j] for j in js}) == 3
    # the proposer's PREPARE voids the quorum; another PREPARE view gains it only through the seat
    assert r["prepare_rule"] == 1 and r["tally"]["proposer_rows"] == 1 and r["tally"]["has_quorum"] == 0
    assert r["tally"]["power"] >= c.model_sets()[0].quorum       # (by power alone it would have one)
    seat = recs[(100, 1, VM.PREPARE, VC.HA)]
    assert seat["prepare_rule"] == 1 and seat["tally"]["distinct_senders"] == seat["stored_rows"] + 1 and seat["tally"]["has_quorum"] == 1
    assert VM.tally(c.model_sets()[0], seat["senders"])["has_quorum"] == 0
    own = recs[(100, 1, VM.PREPARE, VC.HB)]
    assert own["tally"]["proposer_rows"] == 1 and own["stored_rows"] == 1
    # a PREPARE view outside the table and one at another height
    assert recs[(100, 2, VM.PREPARE, VC.HA)]["prepare_rule"] == 0 and recs[(101, 0, VM.PREPARE, VC.HA)]["prepare_rule"] == 0
    # hash_len 31 and 0 are keys of their own, and their senders' earlier HA rows are superseded
    assert recs[(101, 1, VM.COMMIT, VC.H31)]["stored_rows"] == 3 and recs[(101, 1, VM.PREPARE, VC.H0)]["stored_rows"] == 3
    assert recs[(101, 1, VM.COMMIT, VC.HA)]["rows"] == recs[(101, 1, VM.COMMIT, VC.HA)]["stored_rows"] + 3
    # a key whose only row is superseded keeps its record, with S_v empty
    lone = recs[(100, 1, VM.COMMIT, VC.HB)]
    assert lone["rows"] == 1 and lone["stored_rows"] == 0 and lone["tally"]["power"] == 0
    # every invalid kind stands BEHIND a valid stored row of the same sender and view and supersedes nothing
    for kind in (k for k in WS.KINDS if k != "good"):
        (j,) = _rows_of(c, e, kind)
        assert not bits[j] and view[j] == VM.VIEW_NONE and not stored[j], kind
        if kind not in ("not_in_set",):                           # (that sender never has a valid row in the set)
            before = [i for i in valid if i < j and c.senders[i] == c.senders[j] and parsed[i].type == VM.COMMIT and parsed[i].round == 2]
            assert before and all(stored[i] for i in before), kind
    assert all((h, r_, t, VC.HB) not in recs for h in (100, 101) for r_ in (2,) for t in (VM.COMMIT,))
    # the empty View: no set under map A, a valid row of set 2 at height 0 under map B
    ev = _rows_of(c, e, "empty_view_valid")
    assert len(ev) == 2 and not any(bits[j] for j in ev)
    eb = VC.expected(c, WS.MAP_B, False, n)
    assert all(eb["bits"][j] and eb["set"][j] == 2 and eb["parsed"][j].height == 0 for j in ev)
    assert eb["n_views"] == e["n_views"] + 1
    # the recodable row: NEEDS_HOST without the flag, a valid row of height 228 (set 1) with it
    (pj,) = _rows_of(c, e, "padded_height")
    er = VC.expected(c, WS.MAP_A, True, n)
    assert parsed[pj].status != 0 and er["bits"][pj] and er["parsed"][pj].height == WS.RECODE_HEIGHT and er["set"][pj] == 1
    assert er["n_views"] == e["n_views"] + 1
    # the u256 twin: the same rows, powers beyond 2^128
    big = VC.corpus_a(True)
    assert big.msgs == c.msgs and big.big and min(min(p) for p in big.powers) > 2**128


def test_corpus_b_spans_three_workgroups(oracle):
    c = VC.corpus_b()
    n = len(c.msgs)
    assert n > 2 * 256 and n % 256 and n % 64                     # two full workgroups of the row kernels and a partial one
    e = VC.expected(c, WS.MAP_A, False, n)
    assert all(e["bits"])
    everywhere = {e["view"][j] for j, k in enumerate(c.kinds) if k == "everywhere"}
    assert len(everywhere) == 1
    (v,) = everywhere
    assert {j // 256 for j in range(n) if e["view"][j] == v} == {0, 1, 2}
    # a sender whose earlier (superseded) and later (stored) row of one view lie in different workgroups
    pairs = [(i, j) for j in range(n) if e["stored"][j] for i in range(j) if not e["stored"][i] and e["view"][i] == e["view"][j]
             and c.senders[i] == c.senders[j] and i // 256 != j // 256]
    assert pairs


def test_corpus_c_is_a_view_per_row(oracle):
    c = VC.corpus_c()
    n = len(c.msgs)
    assert n == VC.C_VIEWS + VC.C_REPEATS and n % 64
    e = VC.expected(c, WS.MAP_A, False, VC.C_VIEWS)
    assert all(e["bits"]) and e["n_views"] == VC.C_VIEWS
    assert e["view"][:VC.C_VIEWS] == list(range(VC.C_VIEWS))      # more than 64 views in every wavefront
    e100 = VC.expected(c, WS.MAP_A, False, 100)
    assert e100["n_views"] == VC.C_VIEWS and len(e100["records"]) == 100
    over = [j for j in range(n) if e100["view"][j] == VM.VIEW_OVER]
    assert len(over) == n - 100 and sum(1 for j in over if not e100["stored"][j]) == VC.C_REPEATS
    assert e100["stored"] == e["stored"]


@pytest.mark.parametrize("name,hmap,recode", [("a", WS.MAP_A, False), ("a", WS.MAP_B, False), ("a", WS.MAP_A, True), ("a", WS.MAP_B, True),
                                               ("b", WS.MAP_A, False), ("c", WS.MAP_A, False)])
def test_probe_runs_stay_below_the_slot_count(oracle, dev, name, hmap, recode):
    c = {"a": VC.corpus_a, "b": VC.corpus_b, "c": VC.corpus_c}[name]()
    n = len(c.msgs)
    cols = VC.device_columns(c, hmap, recode)
    t = H.Tables(dev, c.model_sets(), 1, VC.proposers(c))
    e = VC.expected(c, hmap, recode, n)
    for hook in (0, 1):
        slots = dev.wvh_table_slots(n, hook)
        assert slots > n
        for salt in (0, 1, 0x9E3779B9, 0xFFFFFFFF):
            got = H.run(dev, t, *cols, n, slots, salt)
            assert got is not None
            assert got[:3] == (e["view"], e["stored"], e["n_views"])
            tab = got[4]
            assert H.longest_run(tab[:slots]) < slots and H.longest_run(tab[slots:]) < slots
            assert int((tab[:slots] != H.EMPTY).sum()) == e["n_views"] and int((tab[slots:] != H.EMPTY).sum()) == sum(e["stored"])
