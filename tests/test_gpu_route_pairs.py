"""GPU: every verifying entry point behind every other on ONE context.  For each ordered pair of routes (A, B), A = B included:
A's dirtier batch, then B's probe twice; both probe answers must be B's expectation exactly — verdict words, per-row indices,
every tally field, records.  The expectation is the CPU oracle's or the route's Python model's (tests/route_pair_cases.py, whose
claims about the batches tests/test_route_pair_inputs.py checks without a GPU); everything compared is a bit, an integer or a
byte string.

What a route may leave behind for the next: verdict bits in the work mask beyond what its tally consumed, a wrong "dirty words"
record, bits in the distinct-sender bitmap, sums and the ticket, columns of a longer batch, a proposer noted and not used, and
the tables of the wire and certificate routes that are documented as zero again when the call returns.  The dirtier sets as
much of that as its route can; the probe is shorter (its words a strict prefix of the dirtier's), Byzantine and weighted, so a
stale 1 bit, bitmap bit or sum changes its answer.

Two regimes: a context of 300 rows, whose 256-byte mask buffer is never reallocated (300 rows, then 133 = 2·64 + 5 = 33·4 + 1:
ragged for every kernel form; a message set's seal half begins at word 3) and one of 8 192 rows (5 000 rows through the row
forms and the multi-workgroup tally, then 700 through the one-wavefront forms and the one-workgroup tally).  On one context the
pairs of a dirtier follow each other, so from the second pair on the dirtier itself is a long batch behind a short one: its
answer is checked as well.

Three arrangements where the order matters in another way: the dirtier SMALLER than the probe (100 rows, then 260) for the pairs
with a message set on either side; the probe as the context's FIRST message set, under which the verdict rows double; and a
long probe behind a short one behind the hash pass, whose ballot words no tally consumes — only the record of dirty words keeps
the long probe from ORing into them."""
import numpy as np
import pytest

import route_pair_cases as RP

pytestmark = pytest.mark.gpu

DIRTIERS = [r.name for r in RP.ROUTES if r.dirtier]
SET_ROUTES = [r.name for r in RP.ROUTES if r.sets_route]


def _V():
    import go_ibft_amd.verifier as V
    return V


@pytest.fixture(scope="module", autouse=True)
def dirty_allocator(oracle):
    """fresh device memory is zero and hides stale scratch: contexts that ran batches full of valid rows free theirs first"""
    V = _V()
    for regime in sorted(RP.REGIMES):
        cap, nd, _ = RP.REGIMES[regime]
        junk = V.BatchVerifier(max_rows=cap)
        try:
            RP.install(junk)
            for name in ("verify_messages[commit]", "is_valid_proposal_hash"):
                r = RP.route(name)
                r.run(junk, r.batch("dirty", nd))
        finally:
            junk.close()


def _probe(bv, a, b, batch, what):
    """B's probe twice behind whatever ran before; the message names A, B, the run and the first difference"""
    for run in ("first", "second"):
        d = RP.first_difference(batch.want, b.run(bv, batch))
        assert d is None, f"{b.name} behind {a} ({what}): the {run} probe run differs at {d}"


PROBES = [r for r in RP.ROUTES if r.probe]


@pytest.mark.parametrize("a", DIRTIERS)
@pytest.mark.parametrize("regime", sorted(RP.REGIMES))
def test_probe_behind_dirtier(oracle, regime, a):
    cap, nd, npr = RP.REGIMES[regime]
    ra = RP.route(a)
    dirt = ra.batch("dirty", nd)
    bv = _V().BatchVerifier(max_rows=cap)
    try:
        RP.install(bv)
        for rb in PROBES:
            # the dirtier's own answer is the oracle's too: from the second pair on it is a long batch behind a short one
            d = RP.first_difference(dirt.want, ra.run(bv, dirt))
            assert d is None, f"{a} (the dirtier in front of {rb.name}, {regime}) differs at {d}"
            _probe(bv, a, rb, rb.batch("probe", npr), f"{regime}: {nd} rows, then {npr}")
    finally:
        bv.close()


@pytest.mark.parametrize("a", DIRTIERS)
def test_probe_reaches_beyond_a_smaller_dirtier(oracle, a):
    """the pairs with a message set on either side, the dirtier SMALLER than the probe: the probe's words [2, 5) — for a set:
    its seal half — were never written by the call in front"""
    cap, nd, npr = RP.SMALLER_FIRST
    ra = RP.route(a)
    others = [r for r in RP.ROUTES if r.probe and (ra.sets_route or r.sets_route)]
    dirt = ra.batch("dirty", nd)
    bv = _V().BatchVerifier(max_rows=cap)
    try:
        RP.install(bv)
        for rb in others:
            ra.run(bv, dirt)
            _probe(bv, a, rb, rb.batch("probe", npr), f"{nd} rows, then {npr}")
    finally:
        bv.close()


@pytest.mark.parametrize("b", [r.name for r in PROBES])
def test_long_probe_behind_a_short_one_behind_the_hash_pass(oracle, b):
    """the hash pass leaves ballot words and no tally behind it (300 rows: five words); B's short probe consumes three of
    them; C's probe of 260 rows then reaches words 3 and 4, which only the record of dirty words protects — every C behind
    this B"""
    cap, _, npr = RP.SMALLER_FIRST
    short = RP.REGIMES["small"][2]
    hashes, rb = RP.route("is_valid_proposal_hash"), RP.route(b)
    bv = _V().BatchVerifier(max_rows=cap)
    try:
        RP.install(bv)
        for rc in PROBES:
            d = RP.first_difference(hashes.batch("dirty", cap).want, hashes.run(bv, hashes.batch("dirty", cap)))
            assert d is None, f"is_valid_proposal_hash in front of {b} differs at {d}"
            d = RP.first_difference(rb.batch("probe", short).want, rb.run(bv, rb.batch("probe", short)))
            assert d is None, f"{b} behind the hash pass differs at {d}"
            _probe(bv, f"{b} ({short} rows) behind the hash pass", rc, rc.batch("probe", npr), f"{npr} rows")
    finally:
        bv.close()


@pytest.mark.parametrize("b", SET_ROUTES)
def test_first_message_set_of_the_context_is_the_probe(oracle, b):
    """the verdict rows double under the first message set of a context: here that set is the probe, behind a dirtier of
    another kind — a fresh context per dirtier"""
    cap, nd, npr = RP.REGIMES["small"]
    rb = RP.route(b)
    for a in DIRTIERS:
        if a in SET_ROUTES:
            continue
        ra = RP.route(a)
        bv = _V().BatchVerifier(max_rows=cap)
        try:
            RP.install(bv)
            ra.run(bv, ra.batch("dirty", nd))
            _probe(bv, a, rb, rb.batch("probe", npr), "the context's first message set")
        finally:
            bv.close()
