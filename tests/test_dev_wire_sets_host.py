"""The row bodies of wire_row_set_kernel and wire_sets_tally_kernel (csrc/wire_sets_dev.h), compiled for the host
(csrc/host_wire_sets_harness.hip), against the plain model of tests/wire_sets_model.py: the height map at every edge of a
range, the row rule, and the per-set tally over interleaved rows — a union member outside the row's set, one address at
different indices in two sets, senders repeated inside one set and across two, u64 power sums that carry past 2^64 and u256
powers; and tally_record (csrc/tally_dev.h), the one place that turns sums into a record, against Python integers at the
quorum's edges, with every carry, and under the proposer rule.  The tables the harness reads (union order, setidx, set_meta, packed power pieces, quorum words) are built here the
way ibft_set_validator_sets documents them."""
import ctypes as C
import random

import numpy as np
import pytest

import wire_sets_model as M

WIRE_ROW = np.dtype([("height", "<u8"), ("round", "<u8"), ("status", "u1"), ("type", "u1"), ("payload_kind", "u1"),
                     ("has_view", "u1"), ("hash_len", "u1"), ("seal_len", "u1"), ("from_len", "u1"), ("sig_len", "u1"),
                     ("from", "u1", 20), ("proposal_hash", "u1", 32), ("pad", "u1", 4)])
U64_MAX = 2**64 - 1


@pytest.fixture(scope="module")
def dev():
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_wire_sets_harness())
    vp, u32 = C.c_void_p, C.c_uint32
    L.wsh_heights.argtypes = [vp, vp, u32, vp, u32, vp]
    L.wsh_row_sets.argtypes = [vp, u32, vp, vp, u32, vp, vp]
    L.wsh_tally.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp, u32, vp, u32, vp]
    L.wsh_tally_record.argtypes = [vp, u32, C.c_uint64, vp, C.c_uint64, vp, vp]
    for f in (L.wsh_heights, L.wsh_row_sets, L.wsh_tally, L.wsh_tally_record):
        f.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _heights(dev, first, range_set, heights):
    f = np.array(first if len(range_set) else [0], np.uint64)
    s = np.array(range_set if len(range_set) else [0], np.uint32)
    h = np.array(heights, np.uint64)
    out = np.full(len(h), 99, np.int32)
    dev.wsh_heights(_p(f), _p(s), len(range_set), _p(h), len(h), _p(out))
    return out.tolist()


MAPS = [
    ([100, 101, 102, 110, 111, 229], [0, 1, 2, 3, 1]),
    ([7, 9], [4]),                                   # one range
    ([0, 5, 10, 20], [2, 2, 0]),                     # 0 mapped; adjacent ranges naming the same set
    ([U64_MAX - 3, U64_MAX - 1, U64_MAX], [1, 0]),   # the last height a map can hold is 2^64 − 2
    (list(range(50, 50 + 4097)), [k % 7 for k in range(4096)]),
]


@pytest.mark.parametrize("first,range_set", MAPS)
def test_height_map_at_the_edges(dev, first, range_set):
    hs = {0, 1, U64_MAX, U64_MAX - 1, first[0] - 1 if first[0] else 0, first[-1], min(first[-1] + 1, U64_MAX)}
    for k in range(len(range_set)):
        hs |= {first[k], first[k + 1] - 1}
    hs = sorted(hs)
    want = [M.set_of_height(first, range_set, h) for h in hs]
    assert _heights(dev, first, range_set, hs) == want
    assert want[hs.index(first[-1])] == -1 and want[hs.index(U64_MAX)] == -1      # the end is exclusive; 2^64 − 1 is never mapped
    assert want[hs.index(first[0])] == range_set[0] and want[hs.index(first[-1] - 1)] == range_set[-1]
    if first[0]:
        assert want[hs.index(first[0] - 1)] == -1


def test_no_ranges_map_nothing(dev):
    assert _heights(dev, [], [], [0, 1, 100, U64_MAX]) == [-1] * 4


def test_row_rule(dev):
    first, range_set = MAPS[2]
    rows = np.zeros(8, WIRE_ROW)
    spec = [(0, 1, 0), (0, 1, 4), (0, 1, 19), (0, 1, 20), (1, 1, 4), (0, 0, 4), (0, 0, 0), (1, 0, 4)]   # status, has_view, height
    for r, (st, hv, h) in zip(rows, spec):
        r["status"], r["has_view"], r["height"] = st, hv, h
    out = np.full(8, 99, np.int32)
    pre = np.array([0, 1, 0, 0, 0, 0, 0, 1], np.uint8)   # the walks' own pre-flags stay
    f, s = np.array(first, np.uint64), np.array(range_set, np.uint32)
    dev.wsh_row_sets(_p(rows), 8, _p(f), _p(s), len(range_set), _p(out), _p(pre))
    want = [M.row_set(st, hv, h, first, range_set) for st, hv, h in spec]
    assert out.tolist() == want == [2, 2, 0, -1, -1, -1, -1, -1]
    assert pre.tolist() == [0, 1, 0, 1, 1, 1, 1, 1]


def _tables(sets, pw):
    """[M.Set] → union list, setidx (n_sets × n_union), set_meta (n_sets × 2), vpower32 (entries × 2·pw), quorum (n_sets × 5)"""
    union = []
    for st in sets:
        for a in st.order:
            if a not in union:
                union.append(a)
    setidx = np.full((len(sets), max(len(union), 1)), -1, np.int32)
    meta, pieces, quorum = [], [], []
    for k, st in enumerate(sets):
        meta.append((len(pieces), len(st.order)))
        for i, a in enumerate(st.order):
            setidx[k, union.index(a)] = i
            pieces.append([(st.power[a] >> (32 * j)) & 0xFFFFFFFF for j in range(2 * pw)])
        quorum.append([(st.quorum >> (64 * j)) & U64_MAX for j in range(5)])
    return (union, setidx, np.array(meta, np.uint32).reshape(-1, 2), np.array(pieces, np.uint32).reshape(-1, 2 * pw),
            np.array(quorum, np.uint64).reshape(-1, 5))


def _run(dev, sets, pw, rows):
    """rows: [(set, sender, union verdict)] → the harness against the model"""
    union, setidx, meta, vp32, quorum = _tables(sets, pw)
    n = len(rows)
    bit = np.array([1 if ok else 0 for _, _, ok in rows], np.uint8)
    # the verdict kernel leaves the union index where the bit is set; anything may stand where it is not
    vidx = np.array([union.index(a) if (ok and a in union) else (-1 if i % 2 else 12345) for i, (_, a, ok) in enumerate(rows)], np.int32)
    for i, (_, a, ok) in enumerate(rows):
        if ok and a not in union:
            bit[i] = 0          # a sender outside every set: the verdict kernel itself answers 0
    rset = np.array([s for s, _, _ in rows], np.int32)
    rec = np.zeros((len(sets), 4), np.uint64)
    dev.wsh_tally(_p(bit), _p(vidx), _p(rset), n, _p(setidx), len(union), _p(meta), _p(vp32), 2 * pw, _p(quorum), len(sets), _p(rec))
    wb, wv, wt = M.judge(sets, rows)
    assert bit.astype(bool).tolist() == wb
    assert vidx.tolist() == wv
    for k, t in enumerate(wt):
        got = dict(power=int(rec[k, 0]) | (int(rec[k, 1]) << 64), valid_rows=int(rec[k, 2]) & 0xFFFFFFFF,
                   distinct_senders=int(rec[k, 2]) >> 32, has_quorum=int(rec[k, 3]))
        want = dict(power=t["power"] & (2**128 - 1), valid_rows=t["valid_rows"], distinct_senders=t["distinct_senders"],
                    has_quorum=t["has_quorum"])
        assert got == want, (k, got, want)
    return wb, wv, wt


def _addr(i):
    return bytes([i & 0xFF, i >> 8]) + b"\xAB" * 18


def _family(power_of):
    """three interleavable sets and one that gets no rows: 3 is in sets 0 and 1 at DIFFERENT indices, 9 only in set 2"""
    return [M.Set([(_addr(i), power_of(0, i)) for i in (0, 1, 2, 3, 4)]),
            M.Set([(_addr(i), power_of(1, i)) for i in (3, 5, 1, 6, 3)]),          # 3 repeated: first position, last power
            M.Set([(_addr(i), power_of(2, i)) for i in (7, 8, 9)]),
            M.Set([(_addr(i), power_of(3, i)) for i in (10, 11)])]


@pytest.mark.parametrize("pw,power_of", [
    (1, lambda k, i: 10 + 3 * k + i),
    (1, lambda k, i: (1 << 63) + 1000 * k + i),            # three members carry past 2^64
    (4, lambda k, i: (1 << 250) + (k << 130) + (i << 64) + 5),   # u256: sums beyond 2^128 (low words and has_quorum compared)
])
def test_interleaved_sets_against_the_model(dev, pw, power_of):
    sets = _family(power_of)
    assert sets[0].index[_addr(3)] == 3 and sets[1].index[_addr(3)] == 0
    rows = [
        (0, _addr(0), True), (1, _addr(3), True), (2, _addr(7), True),
        (0, _addr(3), True), (1, _addr(5), True), (2, _addr(8), False),            # a failed signature
        (0, _addr(0), True), (1, _addr(3), True), (2, _addr(9), True),             # repeated inside a set
        (0, _addr(9), True), (1, _addr(0), True), (2, _addr(3), True),             # union members outside the row's set
        (-1, _addr(1), False), (0, _addr(77), True), (1, _addr(1), True),          # no set; an outsider; 1 is in sets 0 and 1
        (0, _addr(1), True), (0, _addr(2), True), (1, _addr(6), True), (0, _addr(4), True),
    ]
    wb, wv, wt = _run(dev, sets, pw, rows)
    assert wv[1] == 0 and wv[3] == 3                       # one address, two indices
    assert wb[9:12] == [False] * 3 and wv[9:12] == [-1] * 3
    assert wt[3]["valid_rows"] == 0 and wt[3]["has_quorum"] == 0 and wt[3]["quorum"] > 0   # a set without rows
    assert wt[0]["has_quorum"] == 1 and wt[0]["distinct_senders"] == 5 and wt[0]["valid_rows"] == 6
    assert wt[2]["has_quorum"] == 0                       # two of three near-equal powers
    if pw == 1 and power_of(0, 0) > 2**62:
        assert wt[0]["power"] >= 2**64                      # the carry really happens


def test_random_rows_against_the_model(dev):
    rng = random.Random(5)
    for trial in range(30):
        pw = rng.choice([1, 4])
        n_sets = rng.randrange(1, 6)
        pool = [_addr(i) for i in range(rng.randrange(1, 14))]
        sets = [M.Set([(rng.choice(pool), rng.randrange(1, 1 << (64 * pw - 1))) for _ in range(rng.randrange(1, 12))]) for _ in range(n_sets)]
        rows = [(rng.randrange(-1, n_sets), rng.choice(pool + [_addr(500)]), rng.random() < 0.8) for _ in range(rng.randrange(0, 200))]
        rows = [(s, a, ok and s >= 0) for s, a, ok in rows]   # rows without a set are pre-flagged: no verdict bit
        _run(dev, sets, pw, rows)


# ---- tally_record: piece sums → {power_lo, power_hi, counts, has_quorum} and the power in full ---------------------------------
PIECE_MAX = (2**32 - 1) << 20      # a piece is a sum of 32-bit values over at most 2^20 rows


def _record(dev, pieces, counts, quorum, proposer_rows):
    """the harness's record and full-width power against Python integers; returns has_quorum"""
    p = np.array(pieces, np.uint64)
    q = np.array([(quorum >> (64 * j)) & U64_MAX for j in range(5)], np.uint64)
    out, wide = np.full(4, 0xA5A5, np.uint64), np.full(5, 0xA5A5, np.uint64)
    dev.wsh_tally_record(_p(p), len(pieces), counts, _p(q), proposer_rows, _p(out), _p(wide))
    total = sum(int(v) << (32 * k) for k, v in enumerate(pieces))
    assert total < 2**320 and quorum < 2**320
    assert sum(int(w) << (64 * j) for j, w in enumerate(wide)) == total, (pieces, wide)
    want = [total & U64_MAX, (total >> 64) & U64_MAX, counts, 1 if (total >= quorum and proposer_rows == 0) else 0]
    assert [int(x) for x in out] == want, (pieces, quorum, proposer_rows, out, want)
    return int(out[3])


def _piece_sets(n_pieces):
    rng = random.Random(40 + n_pieces)
    return [[PIECE_MAX] * n_pieces,                                        # every carry of pieces_to_words propagates
            [rng.randrange(1, PIECE_MAX + 1) for _ in range(n_pieces)],
            [rng.randrange(1, 2**32) for _ in range(n_pieces)],            # no piece carries
            [0] * (n_pieces - 1) + [PIECE_MAX],
            [1] + [0] * (n_pieces - 1)]


@pytest.mark.parametrize("n_pieces", [2, 8])
def test_tally_record_at_the_quorum_edges(dev, n_pieces):
    counts = 7 | (5 << 32)
    for pieces in _piece_sets(n_pieces):
        total = sum(v << (32 * k) for k, v in enumerate(pieces))
        assert _record(dev, pieces, counts, total, 0) == 1          # sum == quorum
        assert _record(dev, pieces, counts, total + 1, 0) == 0      # sum == quorum − 1
        assert _record(dev, pieces, counts, total - 1, 0) == 1      # sum == quorum + 1
        # the proposer rule on a sum that has the quorum: one valid PREPARE of the proposer voids it
        assert _record(dev, pieces, counts, total - 1, 1) == 0
        assert _record(dev, pieces, counts, total, 1) == 0
    if n_pieces == 8:
        assert sum(PIECE_MAX << (32 * k) for k in range(8)) >> 256                  # the fifth word is in use
        assert sum(PIECE_MAX << (32 * k) for k in range(8)) < 2**312


@pytest.mark.parametrize("n_pieces", [2, 8])
def test_tally_record_word_that_decides(dev, n_pieces):
    pieces = [PIECE_MAX] * n_pieces
    total = sum(v << (32 * k) for k, v in enumerate(pieces))
    top = (total.bit_length() - 1) // 64                  # the sum's highest word in use: 1 for two pieces, 4 for eight
    assert top == (1 if n_pieces == 2 else 4)
    low = (1 << (64 * top)) - 1
    hi = total >> (64 * top)
    # the top word decides, against what every lower word says
    assert _record(dev, pieces, 1, ((hi - 1) << (64 * top)) | low, 0) == 1
    assert _record(dev, pieces, 1, (hi + 1) << (64 * top), 0) == 0
    if top < 4:                                           # a quorum word above everything the sum has
        assert _record(dev, pieces, 1, 1 << 256, 0) == 0
    # every word above equal: the lowest word decides
    w0 = total & U64_MAX
    assert 0 < w0 < U64_MAX
    assert _record(dev, pieces, 1, total - w0, 0) == 1                     # quorum's low word 0
    assert _record(dev, pieces, 1, total - w0 + U64_MAX, 0) == 0           # quorum's low word all ones
    assert _record(dev, pieces, 1, total - 1, 0) == 1
    assert _record(dev, pieces, 1, total + 1, 0) == 0
