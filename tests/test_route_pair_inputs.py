"""CPU: the inputs of the cross-route GPU tests (tests/route_pair_cases.py) hold what they claim — the dirtiers leave all-ones
words behind, the probes have both verdicts in every word, the two tallies differ where stale state would show, and the
directed sequence's last step carries its forged seals beyond the split.  Conditions on the inputs: no GPU, no library call."""
import numpy as np
import pytest

import route_pair_cases as RP

REGIMES = sorted(RP.REGIMES)
NAMES = [r.name for r in RP.ROUTES]


def _words(bits):
    pad = (-len(bits)) % 64
    return np.concatenate([bits, np.zeros(pad, bool)]).reshape(-1, 64), len(bits)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", NAMES)
def test_the_dirtier_leaves_ones_beyond_the_probe(oracle, name, regime):
    r = RP.route(name)
    _, nd, npr = RP.REGIMES[regime]
    d = r.batch("dirty", nd)
    last = (min(npr, d.n) + 63) // 64                # the probe's words are [0, last)
    w, n = _words(np.asarray(d.bits, bool))
    assert len(w) > last, (name, "the dirtier has no word beyond the probe's")
    full = w[last:n // 64]
    assert len(full) and full.all(), (name, "a full word of the dirtier beyond the probe's last is not all ones")
    assert w[-1][:n - 64 * (len(w) - 1)].all()


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", [r.name for r in RP.ROUTES if r.probe])
def test_the_probe_has_both_verdicts_in_every_word(oracle, name, regime):
    r = RP.route(name)
    p = r.batch("probe", RP.REGIMES[regime][2])
    for f, bits in [("main", p.bits)] + [(f, v) for f, v in p.want.items() if f in RP.VERDICT_FIELDS]:
        bits = np.asarray(bits, bool)
        w, n = _words(bits)
        for k in range(len(w)):
            assert not w[k][:min(64, n - 64 * k)].all(), (name, f, "word", k, "has no 0 bit")
        assert bits.mean() >= 0.2 and (~bits).mean() >= 0.2, (name, f, float(bits.mean()))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", [r.name for r in RP.ROUTES if r.probe and r.has_tally])
def test_the_two_tallies_differ(oracle, name, regime):
    r = RP.route(name)
    _, nd, npr = RP.REGIMES[regime]
    d, p = r.batch("dirty", nd), r.batch("probe", npr)
    for f in ("power", "distinct_senders", "has_quorum"):
        assert d.tally[f] != p.tally[f], (name, f, d.tally[f])
    assert d.tally["has_quorum"] == 1 and d.tally["distinct_senders"] > 2 * p.tally["distinct_senders"]


def test_smaller_first_variant_reaches_new_words(oracle):
    _, nd, npr = RP.SMALLER_FIRST
    assert (nd + 63) // 64 < (npr + 63) // 64
    for r in RP.ROUTES:
        if r.sets_route:
            assert r.batch("dirty", nd).bits.all() and not r.batch("probe", npr).bits[nd:].all()
    # the long probe behind a short one: its rows beyond the short probe's words hold rejected rows, the hash pass in front of
    # both left ones there
    short = RP.REGIMES["small"][2]
    assert RP.route("is_valid_proposal_hash").batch("dirty", RP.SMALLER_FIRST[0]).bits.all()
    for r in RP.ROUTES:
        if r.probe:
            bits = np.asarray(r.batch("probe", npr).bits, bool)
            beyond = bits[(short + 63) // 64 * 64:]
            assert len(beyond) > 60 and (~beyond).mean() >= 0.2, r.name


def test_the_sequence_forges_seals_beyond_the_split(oracle):
    s = RP.sequence()
    b = s.seal_step()
    tail = slice(RP.SEQ_SPLIT_AT, None)
    assert b.n == RP.SEQ_SEAL_ROWS and RP.SEQ_SPLIT_AT < b.n <= RP.SEQ_MAX_ROWS
    assert not b.forged[:RP.SEQ_SPLIT_AT].any() and b.forged[tail].mean() > 0.33
    assert not b.bits[b.forged].any()                        # a stolen seal is never accepted
    assert (~b.bits[tail]).mean() >= 0.25                    # the share of rejected rows beyond the split
    assert b.bits[tail].mean() >= 0.25
    # step 3 is a Byzantine set with both verdicts, large enough for the lane kernel, small enough to leave words beyond it
    m = s.set_step()
    assert 2 * ((m.n + 63) // 64 * 64) < RP.SEQ_SPLIT_AT and (m.n + 63) // 64 * 64 + m.n > 32768
    for bits in (m.valid, m.w_valid, m.sender, m.w_sender):
        assert bits.mean() > 0.5
    assert (~m.valid).mean() > 0.1 and (~m.w_valid).mean() > 0.1 and (m.w_sender == m.sender).all()
    # (a 64-byte seal is pre-flagged among the columns and travels as 65 bytes on the wire: the two legs may differ in such rows)
    assert (m.w_valid != m.valid).mean() < 0.05
    assert m.tally["has_quorum"] == 1 and m.w_tally["has_quorum"] == 1 and b.tally["has_quorum"] == 1
