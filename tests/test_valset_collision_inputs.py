"""The colliding validator sets (tests/valset_collision_cases.py) hold what they claim — under the plain model alone: chain
lengths, wraps, decoys one word (one bit) from the signer in its bucket and ahead of it, outsiders that walk the stated run,
64 and 128 slots.  A change of the table's sizing rule or of the hash fails HERE instead of quietly emptying the corpora the
device tests rely on.  The model's hash and table are checked against the host-compiled device source in
test_dev_valset_collision_host.py."""
import pytest

import valset_collision_cases as VC


def _chain(c):
    """the table and, per distinct member, (index, occupied slots passed, wrapped)"""
    slots, table = VC.build_table(c.addrs)
    return slots, table, [VC.probe(table, a) for a in VC.distinct(c.addrs)]


def test_sizing_rule_and_slot_counts(oracle):
    assert [VC.slots_for(n) for n in (0, 1, 31, 32, 63, 64)] == [64, 64, 64, 128, 128, 256]
    assert VC.chain64().slots == 64 and len(VC.chain64().addrs) == 31 and 2 * 31 + 2 == 64
    assert VC.chain128().slots == 128 and len(VC.chain128().addrs) == 32
    assert VC.decoys().slots == 64
    for make in VC.CORPORA.values():
        c = make()
        # the single-set builders size by the LISTED count, the union builder by the distinct one: the same table either way
        assert VC.slots_for(len(c.addrs)) == VC.slots_for(len(VC.distinct(c.addrs))) == c.slots
        assert len(c.addrs) <= 62 and c.powers == [1 << i for i in range(len(c.addrs))]
        assert sum(c.powers) < 1 << 64


def test_chain64_is_one_bucket_that_wraps(oracle):
    c = VC.chain64()
    slots, table, runs = _chain(c)
    buckets = {VC.bucket(a, slots) for a in c.addrs}
    assert len(buckets) == 1 and len(set(c.addrs)) == 31
    b = buckets.pop()
    assert slots - 24 < b < slots - 2                                        # near the end, and the chain passes slot 63
    assert [r[0] for r in runs] == list(range(31)) and [r[1] for r in runs] == list(range(31))
    assert runs[-1][1] == 30 and runs[-1][2]                                 # the member listed last: 30 probes away, wrapped
    assert sum(r[2] for r in runs) == 31 - (slots - b) > 0
    occupied = [s for s in range(slots) if table[s] is not None]
    assert sorted(occupied) == sorted((b + i) & (slots - 1) for i in range(31)) and table[0] is not None and table[slots - 1] is not None


def test_chain128_is_two_buckets_that_wrap(oracle):
    c = VC.chain128()
    slots, table, runs = _chain(c)
    bs = [VC.bucket(a, slots) for a in c.addrs]
    assert sorted(set(bs)) == [126, 127] and bs.count(126) == bs.count(127) == 16 and len(set(c.addrs)) == 32
    assert [r[0] for r in runs] == list(range(32))
    assert {s for s in range(slots) if table[s] is not None} == {126, 127, *range(30)}
    assert sum(r[2] for r in runs) == 30 and max(r[1] for r in runs) >= 30


def test_decoys_surround_the_signer(oracle):
    c = VC.decoys()
    slots, table, runs = _chain(c)
    A = c.A
    bA = VC.bucket(A, slots)
    ia, walked_a, _ = VC.probe(table, A)
    assert len(c.decoys) == len(c.bit_decoys) == 5 and A in c.keys
    for w in range(5):
        d, b = c.decoys[w], c.bit_decoys[w]
        assert VC.differing_words(d, A) == [w] and VC.differing_words(b, A) == [w]
        assert bin(VC.words(b)[w] ^ VC.words(A)[w]).count("1") == 1
        assert bin(VC.words(d)[w] ^ VC.words(A)[w]).count("1") > 1
        for x in (d, b):
            ix, walked, _ = VC.probe(table, x)
            assert VC.bucket(x, slots) == bA and 0 <= ix < ia and walked < walked_a       # A's bucket, ahead of A in the chain
            assert c.addrs.index(x) < c.addrs.index(A)
    assert walked_a == 11 and len(set(c.decoys + c.bit_decoys)) == 10
    # the zero address is a member; C is a real key in A's bucket, listed on both sides of A with two powers
    assert VC.ZERO in c.addrs and VC.probe(table, VC.ZERO)[0] == c.addrs.index(VC.ZERO) == 10
    assert c.addrs.count(c.twice) == 2 and c.twice in c.keys and VC.bucket(c.twice, slots) == bA
    first, last = c.addrs.index(c.twice), len(c.addrs) - 1
    assert first < c.addrs.index(A) < last and c.addrs[last] == c.twice
    assert VC.list_index(c.addrs, c.twice) == first and VC.final_powers(c.addrs, c.powers)[c.twice] == 1 << last
    assert VC.list_index(c.addrs, A) == ia == 12 and len(VC.distinct(c.addrs)) == 13


@pytest.mark.parametrize("name", sorted(VC.CORPORA))
def test_outsiders_walk_the_cluster(oracle, name):
    c = VC.CORPORA[name]()
    slots, table, runs = _chain(c)
    members = set(c.addrs)
    head = VC.bucket(c.A if c.A else c.addrs[-1 if name == "chain64" else 1], slots)
    cluster = len(VC.distinct(c.addrs)) - (1 if VC.ZERO in members else 0)      # (the zero address sits alone in slot 0)
    kinds = set()
    for o in c.outsiders:
        assert o.addr not in members
        ix, walked, _ = VC.probe(table, o.addr)
        assert ix == -1 and walked == o.walk
        start = VC.bucket(o.addr, slots)
        if o.where == "head":
            assert start == head and walked == cluster                       # the WHOLE cluster, then the empty slot
        else:
            assert start != head and walked == cluster - ((start - head) & (slots - 1)) >= 5
        if o.sk is None:
            assert len(VC.differing_words(o.addr, o.near)) == 1 and o.near in members
        kinds.add((o.where, o.sk is not None))
    assert kinds == {("head", True), ("head", False), ("middle", True), ("middle", False)}
    if c.A:                                                                   # one non-member neighbour of A per word
        assert sorted(VC.differing_words(o.addr, c.A)[0] for o in c.outsiders if o.near == c.A and o.where == "head") == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("name", sorted(VC.CORPORA))
def test_rows_hold_every_kind_and_the_oracle_agrees_with_the_model(oracle, name):
    """every member and every outsider has a row; the oracle's own set (sorted, bsearch) names the same members as the model's
    table, and recovers the signer each row was made with"""
    c = VC.CORPORA[name]()
    rws = VC.rows(name)
    assert len(rws) <= 80
    _, table = VC.build_table(c.addrs)
    vs = oracle.ValSet(VC.addr_column(c.addrs), c.powers)
    for a in list(c.addrs) + [o.addr for o in c.outsiders]:
        assert (vs.index(a) >= 0) == (VC.probe(table, a)[0] >= 0) == (a in c.addrs)
    claimed = {r.claimed for r in rws}
    assert set(c.keys) <= claimed and {o.addr for o in c.outsiders} <= claimed and set(c.decoys + c.bit_decoys) <= claimed
    assert {r.what for r in rws} == {"member", "outsider", "keyless", "swap", "nothing"}
    for r in rws:
        rec = oracle.recover_address(r.hash, r.sig)
        if r.what in ("member", "outsider"):
            assert rec == r.claimed
        elif r.what == "nothing":
            assert rec is None and r.claimed == VC.ZERO
        else:
            assert rec is not None and rec != r.claimed and rec in c.keys
