"""The row bodies of the wire_views_*_kernel launches (csrc/wire_views_dev.h), compiled for the host
(csrc/host_wire_views_harness.hip), against the plain model of tests/wire_views_model.py: rows inserted in several orders
give identical tables and outputs, tiny tables with wrap-around, two salts, the cap at 1, n_views − 1 and beyond, u64 and u256
pieces, the PREPARE rule, and the one error a table can raise — more keys than slots, which the library's sizing rules out."""
import random

import numpy as np
import pytest

import wire_sets_cases as WS
import wire_sets_model as M
import wire_views_cases as VC
import wire_views_harness as H
import wire_views_model as VM


@pytest.fixture(scope="module")
def dev():
    return H.load()


def _addr(i):
    return bytes([i & 0xFF, i >> 8]) + b"\xCD" * 18


def _small(pw, rng, n, n_rounds=3, hashes=(b"\x11" * 32, b"\x22" * 32, b"\x11" * 31, b"")):
    """a family of two sets over a dozen addresses and n random rows of heights 7 (set 0) and 8 (set 1)"""
    power = (lambda k, i: (1 << 62) + 7 * k + i) if pw == 1 else (lambda k, i: (1 << 250) + (k << 130) + (i << 64) + 5)
    sets = [M.Set([(_addr(i), power(0, i)) for i in range(8)]), M.Set([(_addr(i), power(1, i)) for i in (9, 3, 5, 10, 2)])]
    rows = []
    for _ in range(n):
        s = rng.randrange(2)
        sender = rng.choice(sets[s].order + [_addr(50)])
        valid = sender in sets[s].power and rng.random() < 0.85
        rows.append((valid, rng.choice((VM.PREPARE, VM.COMMIT)), 7 + s, rng.randrange(n_rounds), rng.choice(hashes), s, sender))
    return sets, rows


def _columns(sets, rows):
    n = len(rows)
    col = np.zeros(n, VC.WS_WIRE_ROW)
    for j, (valid, typ, height, round_, h, s, sender) in enumerate(rows):
        col[j]["height"], col[j]["round"], col[j]["type"], col[j]["hash_len"] = height, round_, typ, len(h)
        col[j]["proposal_hash"][:len(h)] = np.frombuffer(h, np.uint8)
        col[j]["proposal_hash"][len(h):] = 0xEE          # bytes past hash_len are no part of the key and never reach a record
    valid = np.array([1 if r[0] else 0 for r in rows], np.uint8)
    vidx = np.array([sets[r[5]].index[r[6]] if r[0] else -1 for r in rows], np.int32)
    rset = np.array([r[5] for r in rows], np.int32)
    return col, valid, vidx, rset


def _against_model(dev, sets, rows, pw, cap, slots, salt, proposers=None, order=None):
    t = H.Tables(dev, sets, pw, proposers)
    got = H.run(dev, t, *_columns(sets, rows), cap, slots, salt, order)
    assert got is not None
    view, stored, n_views, recs, tab = got
    wv, ws, wn, wr = VM.views(rows, cap, sets, proposers)
    assert (view, stored, n_views) == (wv, ws, wn)
    assert recs == [H.model_record(w) for w in wr]
    return got


@pytest.mark.parametrize("pw", [1, 4], ids=["u64", "u256"])
def test_random_batches_against_the_model(dev, pw):
    rng = random.Random(40 + pw)
    for trial in range(25):
        n = rng.randrange(1, 150)
        sets, rows = _small(pw, rng, n)
        prop = VM.Proposers(7, 1, [_addr(3), _addr(77)]) if trial % 2 else None     # a member of set 0; an outsider
        slots = dev.wvh_table_slots(n, 0)
        first = _against_model(dev, sets, rows, pw, n, slots, 12345, prop)
        n_views = first[2]
        for cap in {1, max(n_views - 1, 1), n_views + 3}:
            _against_model(dev, sets, rows, pw, cap, slots, 999, prop)


def test_row_order_table_size_and_salt_do_not_show(dev):
    rng = random.Random(7)
    sets, rows = _small(1, rng, 120)
    n = len(rows)
    prop = VM.Proposers(7, 0, [_addr(1), _addr(2), _addr(3)])
    base = _against_model(dev, sets, rows, 1, n, 256, 1, prop)
    orders = [np.arange(n)[::-1], np.array(rng.sample(range(n), n)), np.array(rng.sample(range(n), n))]
    for order in orders:
        got = _against_model(dev, sets, rows, 1, n, 256, 1, prop, order)
        # the TABLES hold the same rows — the lowest of every key, the highest of every (view, sender) —; WHERE two keys that
        # collide come to lie depends on which arrived first, which is why no output may depend on a slot number
        assert sorted(got[4][:256].tolist()) == sorted(base[4][:256].tolist())
        assert sorted(got[4][256:].tolist()) == sorted(base[4][256:].tolist())
        assert got[:4] == base[:4]
    floor = dev.wvh_table_slots(n, 1)
    assert floor == 128                                       # the smallest power of two above 120
    for slots in (floor, 256, 1024):
        for salt in (0, 0xDEADBEEF):
            assert _against_model(dev, sets, rows, 1, n, slots, salt, prop, orders[1])[:4] == base[:4]


def test_table_slots_rule(dev):
    assert [dev.wvh_table_slots(n, 0) for n in (0, 1, 32, 33, 64, 65, 1500, 4096)] == [64, 64, 64, 128, 128, 256, 4096, 8192]
    assert [dev.wvh_table_slots(n, 1) for n in (0, 1, 63, 64, 65, 1500, 4096)] == [1, 2, 64, 128, 128, 2048, 8192]
    assert dev.wvh_table_slots(1500, 3000) == 2048 and dev.wvh_table_slots(1500, 4095) == 2048 and dev.wvh_table_slots(1500, 4096) == 4096
    assert dev.wvh_table_slots(1500, 1 << 20) == 4096         # the hook only lowers


def test_tiny_tables_wrap_around_and_fill_up(dev):
    """as many keys as slots: every probe run wraps; one key more exhausts the table, which is an error and never a spin"""
    sets = [M.Set([(_addr(i), 10 + i) for i in range(8)])]
    rows = [(True, VM.PREPARE, 7, r, b"\x33" * 32, 0, _addr(r % 8)) for r in range(8)]      # 8 keys, 8 (view, sender) pairs
    for salt in (1, 2, 3):
        got = _against_model(dev, sets, rows, 1, 8, 8, salt)
        assert got[2] == 8 and (got[4] != H.EMPTY).all()
        assert H.longest_run(got[4][:8]) == 8
    t = H.Tables(dev, sets, 1)
    more = rows + [(True, VM.PREPARE, 7, 8, b"\x33" * 32, 0, _addr(0))]
    assert H.run(dev, t, *_columns(sets, more), 9, 8, 1) is None
    assert H.run(dev, t, *_columns(sets, more), 9, 16, 1) is not None


def test_prepare_rule_cases(dev):
    """the proposer's seat, the proposer's own PREPARE, a proposer outside the set, a view outside the table, a COMMIT"""
    sets = [M.Set([(_addr(i), 10) for i in range(4)])]       # quorum 27: three members
    h = b"\x44" * 32
    rows = [(True, VM.PREPARE, 7, 0, h, 0, _addr(0)), (True, VM.PREPARE, 7, 0, h, 0, _addr(1)),            # round 0: two + the seat
            (True, VM.PREPARE, 7, 1, h, 0, _addr(0)), (True, VM.PREPARE, 7, 1, h, 0, _addr(1)), (True, VM.PREPARE, 7, 1, h, 0, _addr(2)),
            (True, VM.PREPARE, 7, 2, h, 0, _addr(0)), (True, VM.PREPARE, 7, 2, h, 0, _addr(1)),            # round 2: an outsider proposes
            (True, VM.PREPARE, 7, 3, h, 0, _addr(0)), (True, VM.PREPARE, 7, 3, h, 0, _addr(1)),            # round 3: outside the table
            (True, VM.COMMIT, 7, 0, h, 0, _addr(0)), (True, VM.COMMIT, 7, 0, h, 0, _addr(1)),
            (True, VM.PREPARE, 8, 0, h, 0, _addr(0)), (True, VM.PREPARE, 8, 0, h, 0, _addr(1)),            # another height
            (True, VM.PREPARE, 7, 0, b"\x55" * 32, 0, _addr(3))]                                            # proposer 3 of round 0 names another hash
    prop = VM.Proposers(7, 0, [_addr(3), _addr(2), _addr(99)])
    recs = _against_model(dev, sets, rows, 1, len(rows), 64, 5, prop)[3]
    by = {(r["height"], r["round"], r["type"], r["hash"][:1]): r for r in recs}
    seat = by[(7, 0, VM.PREPARE, b"\x44")]
    assert seat["prepare_rule"] == 1 and seat["tally"]["distinct_senders"] == 3 and seat["tally"]["has_quorum"] == 1 and seat["stored_rows"] == 2
    void = by[(7, 1, VM.PREPARE, b"\x44")]
    assert void["prepare_rule"] == 1 and void["tally"]["proposer_rows"] == 1 and void["tally"]["has_quorum"] == 0 and void["tally"]["power"] == 30
    out = by[(7, 2, VM.PREPARE, b"\x44")]
    assert out["prepare_rule"] == 1 and out["tally"]["distinct_senders"] == 2 and out["tally"]["has_quorum"] == 0
    for k in ((7, 3, VM.PREPARE, b"\x44"), (7, 0, VM.COMMIT, b"\x44"), (8, 0, VM.PREPARE, b"\x44")):
        assert by[k]["prepare_rule"] == 0 and by[k]["tally"]["distinct_senders"] == 2 and by[k]["tally"]["has_quorum"] == 0
    own = by[(7, 0, VM.PREPARE, b"\x55")]
    assert own["tally"]["proposer_rows"] == 1 and own["tally"]["distinct_senders"] == 1


def test_corpus_a_through_the_device_source(dev):
    """the GPU corpus' columns as the model gives them, through the device's row bodies: what the GPU test expects of the kernels"""
    c = VC.corpus_a()
    for hmap, recode in ((WS.MAP_A, False), (WS.MAP_B, False), (WS.MAP_A, True)):
        e = VC.expected(c, hmap, recode, len(c.msgs))
        t = H.Tables(dev, c.model_sets(), 1, VC.proposers(c))
        n = len(c.msgs)
        view, stored, n_views, recs, _ = H.run(dev, t, *VC.device_columns(c, hmap, recode), n, dev.wvh_table_slots(n, 0), 77)
        assert (view, stored, n_views) == (e["view"], e["stored"], e["n_views"])
        assert recs == [H.model_record(w) for w in e["records"]]
