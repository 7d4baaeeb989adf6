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


def test_numpy_hash_and_run_length_agree_with_the_model():
    """cert_dedup_model.np_key_hash / np_longest_run (what the inputs of tests/test_gpu_cert_dedup_kernels.py are measured with)
    against key_hash / longest_run, the run lengths also in tables so full that runs go around the end"""
    rng = np.random.default_rng(17)
    keys = rng.integers(0, 256, (300, 117), dtype=np.uint8)
    keys[:40, :97] = keys[0, :97]                                          # equal digest and signature: one home slot for 40 keys
    as_bytes = [k.tobytes() for k in keys]
    assert M.np_key_hash(keys).tolist() == [M.key_hash(k) for k in as_bytes]
    distinct, inv = M.np_distinct(np.concatenate([keys, keys[::-1]]))
    assert len(distinct) == 300 and sorted(d.tobytes() for d in distinct) == sorted(as_bytes)
    assert (distinct[inv] == np.concatenate([keys, keys[::-1]])).all()
    for count, slots in ((1, 64), (63, 64), (64, 64), (40, 64), (200, 256), (255, 256), (300, 512), (300, 1024), (300, 65536)):
        for shift in range(4):
            sub = keys[shift:shift + count]
            want = M.longest_run({k.tobytes() for k in sub}, slots)
            assert M.np_longest_run(sub, slots) == want, (count, slots, shift)
            assert count + 1 != slots or want == count          # one free slot: the run goes around the end unless that slot is the last
    assert M.np_longest_run(keys[:0], 64) == 0


def test_reference_of_the_kernel_inputs_agrees_with_the_model():
    """np_reference against representatives / scattered_bits on every kind at small sizes"""
    for kind in M.KERNEL_KINDS:
        for n in (1, 17, 65, 130, 300):
            keys, pre = M.kernel_input(kind, n)
            as_bytes = [k.tobytes() for k in keys]
            rep, dense_rows, bit = M.np_reference(keys, pre)
            want_rep, want_dense = M.representatives(as_bytes, pre.tolist())
            assert [None if x == M.NP_NO_REP else int(x) for x in rep] == want_rep, (kind, n)
            assert dense_rows.tolist() == want_dense, (kind, n)
            row_bit = [int(p == 0 and k[0] & 1) for k, p in zip(as_bytes, pre)]
            assert bit.tolist() == M.scattered_bits(as_bytes, pre.tolist(), row_bit), (kind, n)


def test_shapes_of_the_kernel_inputs():
    """what the kinds of cert_dedup_model.kernel_input are there for"""
    n = 2049
    count = lambda kind: len(M.np_distinct(M.kernel_input(kind, n)[0])[0])
    assert count("one_key") == 1 and count("mod16") == 16 and count("mirror") == 1025 and count("all_distinct") == n
    assert count("v_only") == 4 and count("from_byte") == 20 and count("digest_byte") == 96
    for kind, what in (("v_only", slice(96, 97)), ("from_byte", slice(97, 117)), ("digest_byte", slice(0, 32))):
        keys, _ = M.kernel_input(kind, n)
        rest = np.delete(keys, np.arange(117)[what], axis=1)
        assert (rest == rest[0]).all(), kind
    assert M.kernel_input("one_key", n)[0][0, 0] & 1 == 1 and M.kernel_input("one_key_bit0", n)[0][0, 0] & 1 == 0
    keys, pre = M.kernel_input("mirror", n)
    assert (keys == keys[::-1]).all()
    rep, dense_rows, bit = M.np_reference(keys, pre)
    assert (rep[1025:] == np.arange(1023, -1, -1)).all() and not bit.all() and bit.any()      # copies of keys whose bit is 0
    keys, pre = M.kernel_input("pre_lowest", n)
    rep, dense_rows, _ = M.np_reference(keys, pre)
    assert pre[:16].all() and dense_rows.tolist() == list(range(16, 32)) and (rep[:16] == M.NP_NO_REP).all()
    keys, pre = M.kernel_input("pre_wavefront", n)
    rep, dense_rows, _ = M.np_reference(keys, pre)
    assert pre[64:128].all() and pre.sum() == 128 and (rep[n - 128:n - 64] == np.arange(n - 128, n - 64)).all()
    keys, pre = M.kernel_input("pre_all", n)
    assert pre.all() and len(M.np_reference(keys, pre)[1]) == 0


@pytest.mark.parametrize("klass", list(M.KERNEL_SIZES))
def test_gpu_kernel_test_inputs_have_roomy_tables(klass):
    """the same condition for the key columns of tests/test_gpu_cert_dedup_kernels.py under the default slot count: no row can
    give up, so that test demands exact results; a seed that breaks it has to be changed (cert_dedup_model.KERNEL_SEED)"""
    for n in M.KERNEL_SIZES[klass]:
        for kind in M.KERNEL_KINDS:
            run_len, bound = M.kernel_input_run(*M.kernel_input(kind, n))
            assert run_len < bound, (kind, n, run_len)
            assert M.table_slots(n) >= 2 * n
    # the one capped input of that test with no more keys than slots: nothing gives up there either
    for n in (1025, 16385):
        run_len, bound = M.kernel_input_run(*M.kernel_input("mod16", n), cap=64)
        assert run_len <= 16 < bound and M.table_slots(n, 64) == 64


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
