"""The corpora of tests/wire_view_seals_cases.py hold every case they claim, and the models answer each the way
ibft_verify_messages_wire_views documents it — checked on the CPU, so that the GPU test's inputs are known to be what its name
says before a device sees them."""
import pytest

import wire_sets_cases as WS
import wire_view_seals_cases as SC
import wire_view_seals_model as SM


def _rows_of(c, kind):
    return [j for j, k in enumerate(c.kinds) if k == kind]


def _record(e, height, round_, typ, h, which="records"):
    got = [r for r in e[which] if (r["height"], r["round"], r["type"], r["hash"]) == (height, round_, typ, h)]
    assert len(got) == 1
    return got[0]


def test_corpus_s_holds_every_kind(oracle):
    c = SC.corpus_s()
    n = len(c.msgs)
    assert 128 < n < 192 and n % 64 != 0
    e = SC.expected(c, WS.MAP_A, False, n)
    p = e["parsed"]
    assert {p[j].height for j in range(n) if e["bits"][j]} == {100, 101, 105}
    types = [p[j].type for j in range(n)]
    assert sum(1 for a, b in zip(types, types[1:]) if a != b) > n // 2          # PREPAREs and COMMITs interleaved
    for kind in SC.SEAL_KINDS + SC.ENVELOPE_KINDS + SC.SUPERSEDING + ("edge_full", "edge_short", "edge_short_bad"):
        assert _rows_of(c, kind), kind
    # bad seals under a fine envelope: the sender bit stands, the seal bit does not
    for kind in SC.SEAL_KINDS[1:]:
        for j in _rows_of(c, kind):
            assert e["bits"][j] and not e["seal"][j], kind
    for kind in ("seal_64", "hash31", "hash0"):                                   # no arithmetic: not even sealable
        assert all(j not in e["dense"] for j in _rows_of(c, kind))
    for kind in ("seal_flip", "seal_other_hash", "seal_other_member", "seal_outsider", "seal_recid"):
        assert all(j in e["dense"] for j in _rows_of(c, kind))
    j = _rows_of(c, "seal_other_member")[0]                                       # a VALID seal by another member of the set
    who = SC.B.recover_address(p[j].proposal_hash, p[j].committed_seal)
    assert who != p[j].sender and who in c.model_sets()[e["set"][j]].power
    assert all(e["seal"][j] for j in _rows_of(c, "good")) and all(not e["seal"][j] for j in _rows_of(c, "prepare"))
    # bad envelopes around a perfect seal
    for kind in SC.ENVELOPE_KINDS:
        (j,) = _rows_of(c, kind)
        assert not e["bits"][j] and not e["seal"][j], kind
        digest = SM.seal_digest(p[j].proposal_hash, None, SC.B.keccak256) if p[j].status == 0 else None
        if digest:
            assert SC.B.recover_address(digest, p[j].committed_seal) == p[j].sender, kind     # the seal itself is perfect
    (flip,) = _rows_of(c, "sig_flip")
    assert flip in e["dense"]                                                     # a member's row: its seal is checked, its bit stays 0
    for kind in ("not_in_set", "outsider", "future", "padded_height"):            # no seal check spent
        assert _rows_of(c, kind)[0] not in e["dense"], kind
    assert e["set"][_rows_of(c, "future")[0]] == -1 and e["set"][_rows_of(c, "not_in_set")[0]] == 0
    assert e["commit_rows"] == sum(1 for j in range(n) if SM.is_commit(p[j], e["set"][j])) > e["seal_rows"] == len(e["dense"])
    assert e["dense"] == sorted(e["dense"])
    # the recode flag: the padded row becomes a valid, sealed COMMIT of set 1
    er = SC.expected(c, WS.MAP_A, True, n)
    (j,) = _rows_of(c, "padded_height")
    assert er["bits"][j] and er["seal"][j] and er["set"][j] == 1 and er["seal_rows"] == e["seal_rows"] + 1


def test_corpus_s_superseding(oracle):
    c = SC.corpus_s()
    e = SC.expected(c, WS.MAP_A, False, len(c.msgs))
    senders = {kind: e["parsed"][_rows_of(c, kind)[0]].sender for kind in SC.SUPERSEDING}
    ha = _record(e, 101, 1, SM.COMMIT, SC.HA)
    hb = _record(e, 101, 1, SM.COMMIT, SC.HB)
    first, last = _rows_of(c, "good_then_bad")
    assert e["seal"][first] and not e["stored"][first] and e["stored"][last] and not e["seal"][last]
    assert senders["good_then_bad"] not in ha["sealed_senders"]                  # the earlier good seal does not count
    first, last = _rows_of(c, "bad_then_good")
    assert not e["seal"][first] and e["stored"][last] and e["seal"][last] and senders["bad_then_good"] in ha["sealed_senders"]
    first, last = _rows_of(c, "ha_then_hb")
    assert e["seal"][first] and e["seal"][last] and not e["stored"][first] and e["stored"][last]
    assert senders["ha_then_hb"] not in ha["sealed_senders"] and hb["sealed_senders"] == [senders["ha_then_hb"]]
    assert ha["pad"] == hb["pad"] == bytes([1, 0, 0, 0, 0]) and ha["tally"]["valid_rows"] == ha["stored_rows"] - 1
    # PREPARE records are the views model's
    for r, w in zip(e["records"], e["views_records"]):
        if r["type"] == SM.PREPARE:
            assert r == dict(w, pad=bytes(5))
        else:
            assert all(r[k] == w[k] for k in w if k != "tally") and r["pad"][SM.SEAL_RULE] == 1


@pytest.mark.parametrize("big", [False, True], ids=["u64", "u256"])
def test_quorum_edge_differs_between_the_two_models(oracle, big):
    c = SC.corpus_s(big)
    e = SC.expected(c, WS.MAP_A, False, len(c.msgs))
    st = c.model_sets()[2]
    powers = sorted(st.power.values())
    assert len(powers) == 5 and sum(powers[:3]) + powers[-1] >= st.quorum > sum(powers[-3:])     # any four reach it, no three do
    for round_, sealed, quorum in ((SC.EDGE_FULL_ROUND, 4, 1), (SC.EDGE_SHORT_ROUND, 3, 0)):
        plain = _record(e, SC.EDGE_HEIGHT, round_, SM.COMMIT, SC.HA, "views_records")
        seals = _record(e, SC.EDGE_HEIGHT, round_, SM.COMMIT, SC.HA)
        assert plain["stored_rows"] == seals["stored_rows"] == 4 and plain["tally"]["has_quorum"] == 1
        assert seals["tally"]["valid_rows"] == seals["tally"]["distinct_senders"] == sealed and seals["tally"]["has_quorum"] == quorum
    (j,) = _rows_of(c, "edge_short_bad")
    assert e["bits"][j] and e["stored"][j] and not e["seal"][j]


def test_corpus_s_under_the_suffix_convention(oracle):
    c = SC.corpus_s(suffix=SC.SUFFIX)
    plain = SC.corpus_s()
    assert c.kinds == plain.kinds and c.msgs != plain.msgs
    n = len(c.msgs)
    e = SC.expected(c, WS.MAP_A, False, n)
    assert e["seal"] == SC.expected(plain, WS.MAP_A, False, n)["seal"]            # signed for the convention: the same answer
    # the identity-signed corpus on a context with the suffix convention: no seal verifies, no COMMIT record has a quorum
    x = SC.expected(plain, WS.MAP_A, False, n, suffix=SC.SUFFIX)
    assert not any(x["seal"]) and x["seal_rows"] == e["seal_rows"]
    assert not any(r["tally"]["has_quorum"] for r in x["records"] if r["type"] == SM.COMMIT)
    assert any(r["tally"]["has_quorum"] for r in e["records"] if r["type"] == SM.COMMIT)


def test_small_sizes(oracle):
    t = SC.corpus_t()
    assert len(t.msgs) == 65
    for n in (1, 64, 65):
        c = SC.corpus_t(n)
        e = SC.expected(c, WS.MAP_A, False, n)
        assert e["dense"] == list(range(n)) and e["seal_rows"] == e["commit_rows"] == n      # (n = 65: seal row 64 is in the second seal word)
        assert e["seal"] == [j not in SC.T_BAD for j in range(n)] and all(e["bits"])


def test_corpus_b_and_c(oracle):
    b = SC.corpus_b()
    n = len(b.msgs)
    assert n == 601
    e = SC.expected(b, WS.MAP_A, False, n)
    view = e["view"][0]
    rows = [j for j in range(n) if e["view"][j] == view]
    assert {j // 256 for j in rows} == {0, 1, 2} and all(b.kinds[j].startswith("everywhere") for j in rows)
    commits = [j for j in range(n) if e["parsed"][j].type == SM.COMMIT]
    bad = [j for j in commits if not e["seal"][j]]
    assert abs(len(bad) * 5 - len(commits)) <= 5 and any(b.kinds[j] == "everywhere_bad" for j in bad)
    superseded = [j for j in rows if not e["stored"][j]]
    assert any(k // 256 != j // 256 for j in superseded for k in rows if k > j and b.senders[k] == b.senders[j])
    rec = e["records"][view]
    assert 0 < rec["tally"]["valid_rows"] < rec["stored_rows"]
    c = SC.corpus_c()
    n = len(c.msgs)
    assert n == SC.C_ROWS == 200
    e = SC.expected(c, WS.MAP_A, False, SC.C_CAP)
    assert e["n_views"] == n > SC.C_CAP == len(e["records"]) and e["view"][:SC.C_CAP] == list(range(SC.C_CAP))
    assert e["seal"] == [j % 3 != 2 for j in range(n)]                            # defined for rows beyond the cap as well
    assert [r["tally"]["valid_rows"] for r in e["records"]] == [int(j % 3 != 2) for j in range(SC.C_CAP)]
