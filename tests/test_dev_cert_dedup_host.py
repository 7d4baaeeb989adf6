"""cert_dedup_dev.h on the CPU (host_cert_dedup_harness.hip, hipcc's host pass — the exact source the cert_dedup_*_kernels run):
table insert in several orders, representatives, the dense batch and the scattered bits against tests/cert_dedup_model.py; and
the model's check that the table of every GPU-test input is roomy enough for exact counts."""
import ctypes as C
import random

import numpy as np
import pytest

import go_ibft_amd.build as build

import cert_dedup_model as M

NO_REP = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(build.build_cert_dedup_harness())
    vp = C.c_void_p
    L.cdh_max_probes.restype = C.c_uint32
    L.cdh_table_slots.restype = C.c_uint32
    L.cdh_table_slots.argtypes = [C.c_uint32, C.c_uint32]
    L.cdh_key_hash.restype = C.c_uint32
    L.cdh_key_hash.argtypes = [vp, vp, C.c_uint32]
    L.cdh_run.restype = None
    L.cdh_run.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def orders(n):
    shuffled = list(range(n))
    random.Random(77).shuffle(shuffled)
    return {"ascending": list(range(n)), "descending": list(range(n - 1, -1, -1)), "shuffled": shuffled}


def run(lib, keys, pre, row_bit, order, cap=0):
    n = len(keys)
    d, s, f, p = M.columns(keys, pre)
    rep, dense_row = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    bit, counts = np.zeros(n, np.uint8), np.zeros(4, np.uint32)
    lib.cdh_run(_p(d), _p(s), _p(f), _p(p), n, cap, _p(np.asarray(order, np.uint32)), _p(np.asarray(row_bit, np.uint8)), _p(rep), _p(dense_row),
                _p(bit), _p(counts))
    dense = int(counts[0])
    gathered = [d[n + k].tobytes() + s[n + k].tobytes() + f[n + k].tobytes() for k in range(dense)]
    return rep, dense_row[:dense], bit, [int(x) for x in counts], gathered


def test_constants_and_hash_agree_with_the_model(lib):
    assert lib.cdh_max_probes() == M.MAX_PROBES
    for rows in (0, 1, 31, 32, 33, 1000, 4096, 4097, 467172):
        for cap in (0, 1, 64, 100, 1 << 20):
            assert lib.cdh_table_slots(rows, cap) == M.table_slots(rows, cap), (rows, cap)
    slots = M.table_slots(1000)
    assert slots >= 2000 and slots & (slots - 1) == 0
    rng = random.Random(3)
    keys = [M.random_key(rng) for _ in range(200)]
    d, s, _, _ = M.columns(keys, [0] * len(keys))
    for r, k in enumerate(keys):
        assert lib.cdh_key_hash(_p(d), _p(s), r) == M.key_hash(k)
    # the signature is mixed in: equal digests, different signatures start at different slots (almost always)
    same_digest = [keys[0][:32] + M.random_key(rng)[32:] for _ in range(64)]
    assert len({M.key_hash(k) & 0xFFFF for k in same_digest}) > 56


@pytest.mark.parametrize("kind", M.KEY_SET_KINDS)
def test_key_sets_in_every_order(lib, kind):
    for n in M.KEY_SET_SIZES:
        keys, pre, row_bit = M.key_set(kind, n)
        want_rep, want_dense = M.representatives(keys, pre)
        want_bits = M.scattered_bits(keys, pre, row_bit)
        assert want_bits == [bool(b) for b in row_bit], "a row's bit is a function of its key"
        for label, order in orders(n).items():
            rep, dense_row, bit, counts, gathered = run(lib, keys, pre, row_bit, order)
            where = (kind, n, label)
            assert [None if x == NO_REP else int(x) for x in rep] == want_rep, where
            assert [int(x) for x in dense_row] == want_dense and sorted(want_dense) == want_dense, where   # ascending
            assert gathered == [keys[r] for r in want_dense], where
            assert [bool(b) for b in bit] == want_bits, where
            assert counts[:3] == [len(want_dense), 0, sum(1 for p in pre if not p)], where
            assert all(not pre[r] for r in want_dense), where                                  # a pre-flagged row is no representative


def test_shapes_of_the_key_sets():
    """what the kinds are there for"""
    keys, pre, _ = M.key_set("v_only", 65)
    assert len({k[:96] + k[97:] for k in keys}) == 1 and len(set(keys)) == 4
    keys, _, _ = M.key_set("digest_byte", 65)
    assert len({k[32:] for k in keys}) == 1 and len(set(keys)) > 32
    keys, _, _ = M.key_set("from_byte", 65)
    assert len({k[:97] for k in keys}) == 1 and len(set(keys)) == 20       # one key per From byte
    keys, pre, bits = M.key_set("pre_among_duplicates", 65)
    rep, _ = M.representatives(keys, pre)
    assert pre[0] and rep[0] is None and any(keys[r] == keys[0] and not pre[r] for r in range(1, 65))
    keys, pre, bits = M.key_set("duplicates", 1000)
    assert any(not b for b in bits) and len(set(keys)) < 200          # copies of a bad signature: they all read 0 above


def test_a_table_too_small_gives_up_and_stays_exact(lib):
    """1 000 distinct keys, 64 slots: most rows give up, become their own representatives, and every bit is still the row's"""
    keys, pre, row_bit = M.key_set("all_distinct", 1000)
    more = M.key_set("duplicates", 1000)
    for keys, pre, row_bit in ((keys, pre, row_bit), more):
        for label, order in orders(1000).items():
            rep, dense_row, bit, counts, gathered = run(lib, keys, pre, row_bit, order, cap=64)
            assert counts[3] == 64 and counts[1] > 0, label
            assert counts[0] <= counts[2] == 1000 and counts[0] >= len(set(keys)), label
            assert [bool(b) for b in bit] == [bool(b) for b in row_bit], label
            assert list(dense_row) == sorted(dense_row) and gathered == [keys[r] for r in dense_row], label
            for r in range(1000):
                assert keys[int(rep[r])] == keys[r] and int(rep[r]) <= r, (label, r)
    # all-distinct keys: exactly 64 find a slot
    rep, dense_row, bit, counts, _ = run(lib, *M.key_set("all_distinct", 1000), list(range(1000)), cap=64)
    assert counts[0] == 1000 and counts[1] == 1000 - 64


def test_gpu_test_inputs_have_roomy_tables():
    """No row of a GPU-test input can give up, in whatever order the lanes insert: the longest run of occupied slots in the
    table the default slot count gives is shorter than MAX_PROBES.  Under this condition tests/test_gpu_cert_dedup.py demands
    exact counts; a seed that breaks it has to be changed (cert_dedup_model.COUNT_SEEDS, EDGE_SEED)."""
    for label, tree in M.gpu_input_trees():
        run_len, bound = M.table_is_roomy(tree)
        assert run_len < bound, (label, run_len)


def test_counts_the_gpu_test_demands():
    """the model's own numbers for the count inputs: at 40 validators fewer than a quarter of the judged rows are distinct"""
    for n in M.COUNT_SEEDS:
        r, d = M.count_inputs(n)
        for label, msgs in d.items():
            tree = M.WC.expected_tree(msgs, r.addrs)
            for two in (False, True):
                rows, judged, verdict = M.expected_stats(tree, two)
                assert rows == tree.n_rows == judged and verdict <= judged
                if n == 40:
                    assert verdict < judged / 4, (label, two, verdict, judged)
    msgs, ordinal = M.flipped_inputs()
    tree = M.WC.expected_tree(msgs, M.edge_round().addrs)
    bad = [r for r in range(tree.n_rows) if not tree.sender_ok[r]]
    assert bad == [3 + 42 * c + ordinal for c in range(3)] and tree.n_rows == 129
