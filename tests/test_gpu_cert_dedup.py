"""IBFT_FLAG_CERT_DEDUP on the GPU: with the flag on, ibft_verify_certificates_wire and ibft_judge_certificates_wire give, byte for
byte, what they give with it off (which is also the oracle's tree), while ibft_cert_stats shows the verdict launch shrunk to the
distinct (digest, signature, From) that tests/cert_dedup_model.py counts.  Every input signs with the oracle's deterministic
nonce, so a message nested twice is the same bytes twice."""
import numpy as np
import pytest

import cert_cases as CC
import cert_dedup_model as M
import cert_verdict_cases as K
from oracle import wire_cert as WC

pytestmark = pytest.mark.gpu
CAP = 4096
_trees = {}


def tree_of(label, msgs, addrs):
    """the oracle's tree of a batch, computed once for all tests"""
    if label not in _trees:
        _trees[label] = WC.expected_tree(msgs, addrs)
    return _trees[label]


def make_bv(r, powers, dedup, cache=False):
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=(V.FLAG_CERT_DEDUP if dedup else 0) | (V.FLAG_PUBKEY_CACHE if cache else 0), max_rows=CAP)
    bv.set_validators(K.H, r.addrs, np.asarray(powers, dtype=np.uint64))
    return bv


def answers(bv, msgs):
    """every output of both calls, as bytes, and the stats behind the second"""
    buf, off = CC.pack(msgs)
    n, nodes, rows, cls, sender, hb, sb = bv.verify_certificates_wire(buf, off)
    certs, n2, (nodes2, rows2, cls2, sender2, hb2, sb2) = bv.judge_certificates_wire(buf, off, per_row=True)
    as_bytes = [x.tobytes() for x in (nodes, rows, cls, sender, hb, sb, certs, nodes2, rows2, cls2, sender2, hb2, sb2)]
    return (n, n2, as_bytes), (n, nodes, rows, cls, sender, hb, sb), bv.cert_stats()


def check_pair(label, off_bv, on_bv, msgs, tree):
    a, per_row, stats_off = answers(off_bv, msgs)
    b, _, stats_on = answers(on_bv, msgs)
    assert a[:2] == b[:2], label
    for k, (x, y) in enumerate(zip(a[2], b[2])):
        assert x == y, (label, "output", k)
    CC.compare(label, tree, *per_row)                       # the pair cannot agree on a wrong answer
    assert stats_off[0] == stats_on[0] == tree.n_rows and stats_off[1] == stats_on[1] == stats_off[2] and stats_off[3] == 0, (label, stats_off, stats_on)
    assert stats_on[2] <= stats_on[1], (label, stats_on)
    return stats_off, stats_on


@pytest.mark.parametrize("cache", [False, True], ids=["cold", "key cache"])
@pytest.mark.parametrize("overlap", ["0", "1"], ids=["one stream", "overlap"])
def test_parity_on_every_existing_case(monkeypatch, overlap, cache):
    monkeypatch.setenv("IBFT_CERT_OVERLAP", overlap)
    r, cases = K.all_cases()
    batches = [(c.label, c.msgs) for c in cases] + [(f"fuzz {i}", m) for i, m in enumerate(CC.fuzz_batches(r, 60, 4243))]
    off_bv, on_bv = make_bv(r, K.POWERS, False, cache), make_bv(r, K.POWERS, True, cache)
    try:
        for label, msgs in batches:
            tree = tree_of(label, msgs, r.addrs)
            for call in range(2 if cache else 1):            # the second call of a key-cache context is warm: two launches
                check_pair((label, overlap, cache, call), off_bv, on_bv, msgs, tree)
        if cache:
            assert on_bv.cache_stats()[0] > 0 and on_bv.cache_stats()[1] > 0
    finally:
        off_bv.close()
        on_bv.close()


@pytest.mark.parametrize("n", sorted(M.COUNT_SEEDS))
def test_counts(n):
    r, inputs = M.count_inputs(n)
    powers = [1] * n
    off_bv, on_bv, warm_bv = make_bv(r, powers, False), make_bv(r, powers, True), make_bv(r, powers, True, cache=True)
    try:
        for label, msgs in inputs.items():
            tree = tree_of(f"count {n} {label}", msgs, r.addrs)
            rows, judged, verdict = M.expected_stats(tree, two_launches=False)     # cold and under 4 096 rows: one launch
            stats_off, stats_on = check_pair((n, label), off_bv, on_bv, msgs, tree)
            assert stats_off == (rows, judged, judged, 0)
            assert stats_on == (rows, judged, verdict, 0)
            if n == 40:
                assert stats_on[2] < stats_on[1] / 4
            # a key-cache context: its first call is cold (one launch) unless an earlier input taught the device the keys; from
            # the second call on the kernels are warm and the deferred rows get a launch of their own
            check_pair((n, label, "warm, first"), off_bv, warm_bv, msgs, tree)
            _, stats_warm = check_pair((n, label, "warm, second"), off_bv, warm_bv, msgs, tree)
            assert warm_bv.cache_stats()[0] > 0
            assert stats_warm == M.expected_stats(tree, two_launches=True) + (0,)
            if n == 40:
                assert stats_warm[2] < stats_warm[1] / 4
    finally:
        for bv in (off_bv, on_bv, warm_bv):
            bv.close()


def test_wavefront_edges():
    r = M.edge_round()
    powers = [1] * r.n
    off_bv, on_bv = make_bv(r, powers, False), make_bv(r, powers, True)
    try:
        for judged, msgs in M.edge_inputs().items():
            tree = tree_of(f"edge {judged}", msgs, r.addrs)
            stats_off, stats_on = check_pair(("edge", judged), off_bv, on_bv, msgs, tree)
            assert stats_off[1] == judged and all(tree.sender_ok)
            assert stats_on == M.expected_stats(tree, False) + (0,)
        # one PREPARE with a flipped signature byte, nested in three certificates: its three copies read 0 (rows in three
        # different verdict words), their honest neighbours 1
        msgs, ordinal = M.flipped_inputs()
        tree = tree_of("flipped", msgs, r.addrs)
        buf, off = CC.pack(msgs)
        check_pair("flipped", off_bv, on_bv, msgs, tree)
        _, _, _, _, sender, _, _ = on_bv.verify_certificates_wire(buf, off)
        bad = [3 + 42 * c + ordinal for c in range(3)]
        assert len({b // 64 for b in bad}) == 3
        assert [i for i in range(129) if not sender[i]] == bad
        assert on_bv.cert_stats() == M.expected_stats(tree, False) + (0,)
    finally:
        off_bv.close()
        on_bv.close()


def test_a_capped_table_gives_up_and_stays_exact(monkeypatch):
    monkeypatch.setenv("IBFT_CERT_DEDUP_SLOTS", "64")
    r, inputs = M.count_inputs(40)
    powers = [1] * r.n
    off_bv, on_bv = make_bv(r, powers, False), make_bv(r, powers, True)
    try:
        for label, msgs in inputs.items():
            tree = tree_of(f"count 40 {label}", msgs, r.addrs)
            _, stats_on = check_pair(("capped", label), off_bv, on_bv, msgs, tree)
            assert stats_on[1] > 300 and stats_on[3] > 0 and stats_on[2] <= stats_on[1], stats_on
    finally:
        off_bv.close()
        on_bv.close()


def test_the_environment_overrides_the_flag(monkeypatch):
    r, inputs = M.count_inputs(7)
    msgs = inputs["roots"]
    tree = tree_of("count 7 roots", msgs, r.addrs)
    rows, judged, verdict = M.expected_stats(tree, False)
    assert verdict < judged
    buf, off = CC.pack(msgs)
    for env, flag, want in (("1", False, verdict), ("0", True, judged)):
        monkeypatch.setenv("IBFT_CERT_DEDUP", env)
        bv = make_bv(r, [1] * r.n, flag)
        try:
            assert bv.cert_stats() == (0, 0, 0, 0)             # nothing before the first certificate call
            bv.verify_certificates_wire(buf, off)
            assert bv.cert_stats() == (rows, judged, want, 0), (env, flag)
        finally:
            bv.close()
