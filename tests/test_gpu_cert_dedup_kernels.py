"""GPU: the certificate dedup's kernels (csrc/cert_dedup_kernels.h) on key columns of their own, through the test library
(devtest_cert_dedup: the product's kernels and the product's launch geometry — table clear, insert, mark, tile sums, offsets,
apply; scatter; count), each against plain numpy over the key bytes (cert_dedup_model.np_reference), compared exactly:

    rep[r]          the lowest row without a pre-flag that carries row r's 117 key bytes
    dense batch     the representatives in ascending order, their columns gathered behind the tree's rows
    bit[r]          its representative's bit (the test library judges a dense row by its GATHERED bytes); 0 with a pre-flag
    counts          the zero bytes of the two pre-flag columns, twice in a row, the accumulators zero after each launch

The sizes reach 262 145 rows (257 tiles of the apply kernel, the count kernel's loop in its second pass and beyond), the key
patterns put up to n lanes on one table word.  Exact results are demanded where no row can give up
(tests/test_dev_cert_dedup_host.py checks the table of every such input without a GPU); under a slot cap, which keys get a
slot depends on the order of the lanes, and only what holds in every order is asserted.  The buffers carry sentinel cells
around everything the kernels may write."""
import ctypes as C

import numpy as np
import pytest

import cert_dedup_model as M

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5
SLOT_UNPLACED, SLOT_SKIP = 0xFFFFFFFF, 0xFFFFFFFE


@pytest.fixture(scope="module")
def dt():
    import go_ibft_amd.build as B
    L = C.CDLL(B.build_devtest())
    vp, u32 = C.c_void_p, C.c_uint32
    L.devtest_cert_dedup_max_probes.restype = u32
    L.devtest_cert_dedup_table_slots.restype = u32
    L.devtest_cert_dedup_table_slots.argtypes = [u32, u32]
    L.devtest_cert_dedup.argtypes = [u32, vp, vp, vp, vp, u32, u32, vp] + [vp] * 11
    L.devtest_cert_dedup_count.argtypes = [u32, vp, u32, vp, vp, vp]
    assert L.devtest_cert_dedup_max_probes() == M.MAX_PROBES
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Answer:
    pass


def run(dt, keys, pre, pre_b, cap=0):
    n = len(keys)
    d, s, f = (np.ascontiguousarray(keys[:, a:b]) for a, b in ((0, 32), (32, 97), (97, 117)))
    pre, pre_b = np.ascontiguousarray(pre, dtype=np.uint8), np.ascontiguousarray(pre_b, dtype=np.uint8)
    a = Answer()
    a.rep, a.slot_of, a.dense_pos = (np.zeros(n, np.uint32) for _ in range(3))
    a.g = [np.full((n, w), 0x5A, np.uint8) for w in (32, 65, 20, 1)]
    a.mask = np.zeros((n + 63) // 64, np.uint64)
    a.stat, a.count, changed = np.zeros(4, np.uint32), np.zeros(14, np.uint32), np.full(1, 0xFFFFFFFF, np.uint32)
    rc = dt.devtest_cert_dedup(n, _p(d), _p(s), _p(f), _p(pre), cap, len(pre_b), _p(pre_b), _p(a.rep), _p(a.slot_of), _p(a.dense_pos),
                               *[_p(x) for x in a.g], _p(a.mask), _p(a.stat), _p(a.count), _p(changed))
    assert rc == 0, ("status", rc)
    a.changed = int(changed[0])
    a.dense = int(a.stat[0])
    a.bits = np.unpackbits(a.mask.view(np.uint8), bitorder="little").astype(bool)
    a.gathered = np.concatenate([x[:a.dense] for x in a.g[:3]], axis=1)
    a.gathered_pre = a.g[3][:a.dense, 0]
    return a


def flags_b(n):
    """the second pre-flag column of a run: about 3/7 of n bytes, a quarter of them flags"""
    rng = np.random.default_rng(n)
    return rng.choice(np.array([0, 0, 0, 2], np.uint8), 3 * n // 7 + 5)


def check_counts(where, count, pre, pre_b):
    want = [int((pre == 0).sum()), int((pre_b == 0).sum())]
    for launch in range(2):
        got = count[7 * launch:7 * launch + 7].tolist()
        assert got == want + want + [0, 0, 0], (where, "count launch", launch, got, want)


def check_exact(where, a, keys, pre, pre_b, cap=0):
    n = len(keys)
    rep, dense_rows, bit = M.np_reference(keys, pre)
    judged = pre == 0
    assert a.changed == 0, (where, "sentinel cells changed", bin(a.changed))
    assert a.stat.tolist() == [len(dense_rows), 0] * 2, (where, "dense, unplaced (device, host)", a.stat.tolist(), len(dense_rows))
    bad = np.nonzero(a.rep.astype(np.int64) != rep)[0]
    assert bad.size == 0, (where, "rep", int(bad[0]), int(a.rep[bad[0]]), int(rep[bad[0]]))
    assert (a.slot_of[~judged] == SLOT_SKIP).all() and (a.slot_of[judged] < M.table_slots(n, cap)).all(), (where, "slot_of")
    assert (a.slot_of[judged] == a.slot_of[rep[judged]]).all(), (where, "rows of one key at different slots")
    want_pos = np.full(n, FILL, np.int64)
    want_pos[dense_rows] = np.arange(len(dense_rows))
    assert (a.dense_pos == want_pos).all(), (where, "dense_pos")
    assert (a.gathered == keys[dense_rows]).all() and (a.gathered_pre == 0).all(), (where, "gathered rows")
    assert all((x[a.dense:] == 0x5A).all() for x in a.g), (where, "rows behind the dense batch handed out")
    bad = np.nonzero(a.bits[:n] != bit)[0]
    assert bad.size == 0, (where, "bit", int(bad[0]))
    assert not a.bits[n:].any(), (where, "bits of the last word at and beyond n")
    check_counts(where, a.count, pre, pre_b)


def same_answer(where, a, b):
    """two runs of one roomy input (the slots themselves may differ: two keys that start at one slot take it in either order)"""
    for name in ("rep", "dense_pos", "gathered", "gathered_pre", "mask", "stat", "count"):
        assert (getattr(a, name) == getattr(b, name)).all(), (where, "the second run differs in", name)


@pytest.mark.parametrize("kind", M.KERNEL_KINDS)
@pytest.mark.parametrize("klass", list(M.KERNEL_SIZES))
def test_roomy_table(dt, klass, kind):
    for n in M.KERNEL_SIZES[klass]:
        keys, pre = M.kernel_input(kind, n)
        pre_b = flags_b(n)
        assert dt.devtest_cert_dedup_table_slots(n, 0) == M.table_slots(n)
        first = run(dt, keys, pre, pre_b)
        check_exact((kind, n), first, keys, pre, pre_b)
        same_answer((kind, n), first, run(dt, keys, pre, pre_b))


@pytest.mark.parametrize("kind", ["all_distinct", "mod16"])
@pytest.mark.parametrize("cap", [64, 1])
@pytest.mark.parametrize("n", [1025, 16385])
def test_capped_table(dt, n, cap, kind):
    """more keys than slots (cap 1: the slot mask is 0): rows give up and are their own representatives — what holds in
    whatever order the lanes insert.  16 keys in 64 slots all find one (no run of occupied slots can reach MAX_PROBES, as
    tests/test_dev_cert_dedup_host.py checks): nothing gives up there and the results are exact."""
    keys, pre = M.kernel_input(kind, n)
    pre_b = flags_b(n)
    where = (kind, n, cap)
    assert dt.devtest_cert_dedup_table_slots(n, cap) == cap
    a = run(dt, keys, pre, pre_b, cap)
    _, _, bit = M.np_reference(keys, pre)
    distinct = len(M.np_distinct(keys)[0])
    if distinct <= cap:
        assert (kind, cap) == ("mod16", 64)
        return check_exact(where, a, keys, pre, pre_b, cap)
    assert a.changed == 0, (where, "sentinel cells changed", bin(a.changed))
    assert (a.bits[:n] == bit).all() and not a.bits[n:].any(), (where, "every row's bit is its own")
    rep = a.rep.astype(np.int64)
    assert (rep <= np.arange(n)).all() and (keys[rep] == keys).all(), (where, "rep")
    dense_rows = np.nonzero(rep == np.arange(n))[0]                         # ascending by construction
    assert a.dense == len(dense_rows) and (a.dense_pos[dense_rows] == np.arange(a.dense)).all(), (where, "the dense rows ascend")
    assert (np.delete(a.dense_pos, dense_rows) == FILL).all(), where
    assert (a.gathered == keys[dense_rows]).all() and (a.gathered_pre == 0).all(), (where, "gathered rows")
    assert distinct <= a.dense <= n, (where, a.dense)
    gave_up = int((a.slot_of == SLOT_UNPLACED).sum())
    assert a.stat.tolist() == [a.dense, gave_up] * 2 and gave_up > 0, (where, a.stat.tolist(), gave_up)
    assert (a.slot_of[a.slot_of != SLOT_UNPLACED] < cap).all(), where
    check_counts(where, a.count, pre, pre_b)


def count_alone(dt, pre_a, pre_b):
    out, changed = np.zeros(14, np.uint32), np.full(1, 0xFFFFFFFF, np.uint32)
    pre_a, pre_b = np.ascontiguousarray(pre_a, dtype=np.uint8), np.ascontiguousarray(pre_b, dtype=np.uint8)
    rc = dt.devtest_cert_dedup_count(len(pre_a), _p(pre_a), len(pre_b), _p(pre_b), _p(out), _p(changed))
    assert rc == 0 and changed[0] == 0, ("status", rc, bin(int(changed[0])))
    return out


def test_count_kernel_alone(dt):
    """the boundary between the two columns inside a wavefront (1 000 + 700) and in the second pass of the loop (16 000 + 1 000);
    either column empty; all flags set; a column of 70 000: five passes"""
    rng = np.random.default_rng(5)
    column = lambda n: rng.choice(np.array([0, 0, 1, 2, 3], np.uint8), n)
    empty = np.zeros(0, np.uint8)
    for label, a, b in (("1000 + 700", column(1000), column(700)), ("16000 + 1000", column(16000), column(1000)),
                        ("b empty", column(1000), empty), ("a empty", empty, column(700)), ("a empty, second pass", empty, column(16385)),
                        ("b empty, second pass", column(16385), empty), ("all flags set", np.full(1000, 1, np.uint8), np.full(700, 2, np.uint8)),
                        ("all flags set, second pass", np.full(16000, 3, np.uint8), np.full(1000, 1, np.uint8)),
                        ("no flag set", np.zeros(16000, np.uint8), np.zeros(1000, np.uint8)), ("one byte", np.zeros(1, np.uint8), empty),
                        ("70000 + 1", column(70000), np.zeros(1, np.uint8))):
        check_counts(label, count_alone(dt, a, b), a, b)
