"""The recode class on the CPU (IBFT_FLAG_WIRE_RECODE): the plain model (wire_recode_model.py) against the protobuf runtime,
against the claim that a canonical re-encoding is never longer than its source, and against the canonical walk's oracle —
over every named case and 3 000 random compositions of the scramblers (wire_recode_cases.corpus)."""
import importlib.util
import os

import pytest

import wire_recode_cases as RC
import wire_recode_model as RM
from oracle import wire_parse as WP


@pytest.fixture(scope="module")
def rows():
    return RC.corpus()[1]


def test_corpus_covers_both_sides(rows):
    inside = sum(RM.canonical(m)[0] for _, m, _ in rows)
    assert inside > 3000 and len(rows) - inside > 300
    assert sum(label == "random" for label, _, _ in rows) == 3000
    for name, m in RC.named_out_of_class(RC.signed_parts(RC.corpus()[0])[0]):
        assert RM.canonical(m) == (False, m), name
    r = RC.corpus()[0]
    for p in RC.signed_parts(r)[:2]:
        for name, m in RC.named_in_class(p):
            assert RM.canonical(m)[0], name


def test_scrambled_rows_decode_to_the_signed_message(rows):
    """meaning-preserving: the canonical re-encoding of a scrambled row is the row that was signed"""
    seen = set()
    for label, m, p in rows:
        if p is not None:
            assert RM.canonical(m) == (True, p.canonical), (label, m.hex())
            seen.add(label)
    assert {"reorder", "pad2", "pad5", "pad10", "split view", "garbage first", "zero first", "other member first", "member twice",
            "member split", "random", "canonical"} <= seen


def test_model_against_the_protobuf_runtime(rows):
    """in the class ⇒ the runtime parses the row and serialises it to the model's bytes"""
    pytest.importorskip("google.protobuf")
    from google.protobuf.message import DecodeError
    spec = importlib.util.spec_from_file_location("make_wire_fixtures", os.path.join(os.path.dirname(__file__), "golden", "make_wire_fixtures.py"))
    mwf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mwf)
    cls = mwf.build_messages()["IbftMessage"]
    checked = 0
    for label, m, _ in rows:
        inside, canon = RM.canonical(m)
        if not inside:
            continue
        g = cls()
        try:
            g.ParseFromString(m)
        except DecodeError:
            pytest.fail(f"the runtime refuses a row of the class: {label} {m.hex()}")
        assert g.SerializeToString(deterministic=True) == canon, (label, m.hex())
        checked += 1
    assert checked > 3000


def test_canonical_length_never_exceeds_the_input(rows):
    for label, m, _ in rows:
        inside, canon = RM.canonical(m)
        assert len(canon) <= len(m), (label, m.hex())


def test_canonical_walk_judges_exactly_the_class(rows):
    """the contract: a row of the class is judged as its canonical re-encoding — which the canonical walk accepts; a row the
    canonical walk accepts already is its own re-encoding; any other row stays NEEDS_HOST"""
    for label, m, _ in rows:
        inside, canon = RM.canonical(m)
        assert (WP.expected(canon).status == WP.OK) == inside, (label, m.hex())
        if WP.expected(m).status == WP.OK:
            assert inside and canon == m, (label, m.hex())
