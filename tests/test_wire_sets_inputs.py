"""The GPU corpus of tests/test_gpu_wire_sets.py (tests/wire_sets_cases.py) really holds what that test claims to cover —
checked here on the CPU, with the oracle's walk and signature check and the plain model: every kind of row with the fate the
row rule gives it, rows of three sets inside one verdict word, one address at two indices, repeated senders, a set without
rows, power sums past 2^64, both outcomes of has_quorum, and a padded height whose low byte names another range."""
import wire_sets_cases as WS
import wire_sets_model as M
from oracle import wire_parse as WP


def test_every_kind_is_there_with_its_fate(oracle):
    c = WS.corpus()
    n = len(c.msgs)
    assert n == 300 and set(c.kinds) == set(WS.KINDS)
    assert set(c.kinds[:63]) == set(WS.KINDS)                       # … already in the smallest multi-row size
    bits, sets, vidx, tallies, rows = WS.expected(c, n, WS.MAP_A, False)
    bits_b, sets_b, _, tallies_b, _ = WS.expected(c, n, WS.MAP_B, False)
    bits_r, sets_r, vidx_r, _, rows_r = WS.expected(c, n, WS.MAP_A, True)
    union = {c.pool.addrs[i].tobytes() for ix in WS.MEMBERS for i in ix}
    model = c.model_sets()
    for j, k in enumerate(c.kinds):
        e, s = rows[j], j % 3
        if k == "good":
            assert bits[j] and sets[j] == s and vidx[j] == WS.MEMBERS[s].index(c.senders[j])
        elif k == "sig_flip":
            assert e.status == WP.OK and sets[j] == s and not bits[j] and e.sender in model[s].index
        elif k == "outsider":
            assert e.status == WP.OK and sets[j] == s and not bits[j] and e.sender not in union
        elif k == "not_in_set":
            assert sets[j] == s and not bits[j] and vidx[j] == -1 and e.sender in union and e.sender not in model[s].index
            assert WS.B.recover_address(e.digest, e.signature) == e.sender          # a good signature: only the set says no
        elif k == "needs_host":
            assert e.status != WP.OK and sets[j] == -1 and not bits[j]
        elif k == "no_view":
            assert e.status == WP.OK and not e.has_view and sets[j] == -1 and sets_b[j] == -1 and not bits_b[j]
        elif k == "empty_view":
            assert e.status == WP.OK and e.has_view and e.height == 0
            assert sets[j] == -1 and not bits[j] and sets_b[j] == 2 and bits_b[j]   # range 0 not mapped / mapped
        elif k == "future":
            assert e.status == WP.OK and e.height == WS.FUTURE_HEIGHT and sets[j] == -1 and sets_b[j] == -1
        elif k == "max_height":
            assert e.status == WP.OK and e.height == 2**64 - 1 and sets[j] == -1 and sets_b[j] == -1
        elif k == "below":
            assert e.height == 99 and sets[j] == -1 and sets_b[j] == 2 and bits_b[j]
        elif k == "padded_height":
            assert e.status != WP.OK and sets[j] == -1 and not bits[j]               # the canonical walk refuses it
            assert rows_r[j].status == WP.OK and rows_r[j].height == WS.RECODE_HEIGHT
            low = M.set_of_height(*WS.MAP_A, WS.RECODE_HEIGHT & 0x7F)
            assert low == 0 and sets_r[j] == 1 and bits_r[j] and vidx_r[j] == 3     # another range than its low byte's
    assert [sets_r[j] == sets[j] for j in range(n)].count(False) == 1               # the flag changes that one row only
    assert {0, 1, 2} <= set(sets[:63]) and sets[62:65].count(-1) == 0               # three sets in one verdict word, and at the seam
    assert tallies[3]["valid_rows"] == 0 and tallies[3]["has_quorum"] == 0 and tallies[3]["quorum"] > 0
    assert all(t["valid_rows"] > t["distinct_senders"] > 0 for t in tallies[:3])    # senders repeated inside every set
    assert all(t["power"] >= 2**64 for t in tallies[:3])                            # u64 sums that carry
    assert [t["has_quorum"] for t in tallies[:3]] == [1, 1, 1]
    small = WS.expected(c, 63, WS.MAP_A, False)[3]
    assert small[0]["has_quorum"] == 0 and small[2]["has_quorum"] == 1              # both outcomes
    assert tallies_b[2]["valid_rows"] == tallies[2]["valid_rows"] + 2


def test_one_address_two_indices_and_senders_across_sets(oracle):
    c = WS.corpus()
    model = c.model_sets()
    a = c.pool.addrs[30].tobytes()
    assert model[0].index[a] == 30 and model[1].index[a] == 0
    bits, sets, vidx, _, _ = WS.expected(c, 300, WS.MAP_A, False)
    per_sender = {}
    for j in range(300):
        if bits[j]:
            per_sender.setdefault(c.senders[j], set()).add((sets[j], vidx[j]))
    across = [v for v in per_sender.values() if len({s for s, _ in v}) > 1]
    assert across and any(len({i for _, i in v}) > 1 for v in across)   # one signer, valid in two sets, at different indices


def test_u256_corpus_goes_beyond_128_bits(oracle):
    c = WS.corpus(big=True)
    t = WS.expected(c, 300, WS.MAP_A, False)[3]
    assert all(x["power"] >= 2**200 for x in t[:3]) and t[0]["quorum"] >= 2**200
