"""IBFT_FLAG_CERT_DEDUP and ibft_judge_certificates_wire on trees of about 26 650 rows (cert_cases.long_tree: flat and nested, T
and T + 1 draws, T = CERT_SCAN_ONE_GROUP_MAX — the trees tests/test_gpu_cert.py judges, built once per process): about
1 600 rows contend on each word of the dedup's table, its count kernel is in the second pass of its loop, the deferred batch
of the two-launch form has more than 8 192 rows, and the record kernels see 8 192 / 8 193 records in one level.  With the flag
on every output of both calls equals, byte for byte, what the flag-off context gives and the oracle's tree
(test_gpu_cert_dedup.check_pair); ibft_cert_stats equals cert_dedup_model.expected_stats; the records equal
cert_verdict_model over the context's own per-row outputs (test_gpu_judge_certificates.judged)."""
import pytest

from oracle import binding as B
from oracle import wire
from oracle import wire_cert as WC

import cert_cases as CC
import cert_dedup_model as M
import cert_verdict_cases as K
import cert_verdict_model as VM
import test_gpu_cert_dedup as D
import test_gpu_judge_certificates as J

pytestmark = pytest.mark.gpu
CAP = CC.LONG_LEVEL_MAX_ROWS
SHAPES = ["flat", "nested"]


@pytest.fixture(scope="module")
def scan_threshold():
    import ctypes as C
    import go_ibft_amd.build as B
    L = C.CDLL(B.build_devtest())
    L.devtest_cert_scan_threshold.restype = C.c_uint32
    return int(L.devtest_cert_scan_threshold())


def make_bv(r, dedup, cache=False, max_rows=CAP):
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=(V.FLAG_CERT_DEDUP if dedup else 0) | (V.FLAG_PUBKEY_CACHE if cache else 0), max_rows=max_rows)
    bv.set_validators(5, r.addrs, r.power)
    return bv


def two_launches(overlap, tree, warm=False):
    """certificates_wire_impl's rule: the deferred rows get a verdict launch of their own when the overlap is not switched off
    (IBFT_CERT_OVERLAP=0), there are any, and the tree has 4 096 rows or the context verifies against learnt keys"""
    carriers = sum(M.tree_keys(tree)[1])
    return overlap != "0" and carriers != 0 and (tree.n_rows >= 4096 or warm)


def set_overlap(monkeypatch, overlap):
    if overlap is None:
        monkeypatch.delenv("IBFT_CERT_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("IBFT_CERT_OVERLAP", overlap)


def test_the_long_trees_are_what_this_file_takes_them_for(scan_threshold):
    """all counts beyond the count kernel's first pass, the deferred batch beyond 8 192 rows, no row can give up (the condition of
    tests/test_dev_cert_dedup_host.py for exact counts), and far fewer keys than rows"""
    for shape in SHAPES:
        for dk in (0, 1):
            tree = CC.long_tree(shape, scan_threshold + dk)[2]
            run_len, bound = M.table_is_roomy(tree)
            assert run_len < bound, (shape, dk, run_len)
            rows, judged, verdict = M.expected_stats(tree, False)
            rows2, judged2, verdict2 = M.expected_stats(tree, True)
            assert 16384 < judged == judged2 <= rows == rows2 <= CAP and verdict <= 32 and 8192 < verdict2 < judged / 2
            assert two_launches(None, tree) and not two_launches("0", tree)


@pytest.mark.parametrize("overlap", [None, "0"], ids=["overlap", "one stream"])
@pytest.mark.parametrize("dk", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_and_counts_cold(shape, dk, overlap, scan_threshold, monkeypatch):
    set_overlap(monkeypatch, overlap)
    r, msgs, tree, _ = CC.long_tree(shape, scan_threshold + dk)
    off_bv, on_bv = make_bv(r, False), make_bv(r, True)
    try:
        stats_off, stats_on = D.check_pair((shape, dk, overlap), off_bv, on_bv, msgs, tree)
        want = M.expected_stats(tree, two_launches(overlap, tree))
        assert stats_off == (want[0], want[1], want[1], 0), (stats_off, want)
        assert stats_on == want + (0,), (stats_on, want)
    finally:
        off_bv.close()
        on_bv.close()


@pytest.mark.parametrize("dk", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_and_counts_in_a_key_cache_context(shape, dk, scan_threshold, monkeypatch):
    """the second call verifies against the learnt keys' tables: both verdict launches, over the dense batch and over the
    deferred batch, are the known-key kernels"""
    set_overlap(monkeypatch, None)
    r, msgs, tree, _ = CC.long_tree(shape, scan_threshold + dk)
    off_bv, warm_bv = make_bv(r, False), make_bv(r, True, cache=True)
    try:
        D.check_pair((shape, dk, "first call"), off_bv, warm_bv, msgs, tree)
        assert warm_bv.cache_stats()[0] > 0
        _, stats_warm = D.check_pair((shape, dk, "second call"), off_bv, warm_bv, msgs, tree)
        assert warm_bv.cache_stats()[1] > 0
        assert stats_warm == M.expected_stats(tree, two_launches(None, tree, warm=True)) + (0,)
    finally:
        off_bv.close()
        warm_bv.close()


@pytest.mark.parametrize("dk", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_records(shape, dk, scan_threshold, monkeypatch):
    """flat: 8 192 / 8 193 root records (cert_record_scan_kernel sums 8 / 9 roots per thread, its last threads none); nested: 4
    roots and 8 192 / 8 193 level-1 records under ONE root, which cert_judge_kernel walks 128 children per lane"""
    set_overlap(monkeypatch, None)
    T = scan_threshold + dk
    r, msgs, tree, _ = CC.long_tree(shape, T)
    addrs = [a.tobytes() for a in r.addrs]
    powers = [int(p) for p in r.power]
    off_bv, on_bv = make_bv(r, False), make_bv(r, True)
    try:
        certs, cv = J.judged(on_bv, (shape, dk, "flag on"), msgs, addrs, powers, False, VM.proposers_for(addrs), rows_cap=CAP)
        buf, off = CC.pack(msgs)
        plain, n_rows, _ = off_bv.judge_certificates_wire(buf, off)
        assert n_rows == cv.n_rows == tree.n_rows and plain.tobytes() == certs.tobytes()
        assert len(certs) == (T if shape == "flat" else 4 + T)
        if shape == "nested":
            assert int(certs[2]["n_children"]) == T and int(certs[2]["first_child_cert"]) == 4
            assert [int(c["row"]) for c in certs[4:]] == list(range(4, 4 + T))
        assert {int(c["pc"]) for c in certs} <= {-1, 0, 2}         # (what these trees yield: tests/test_gpu_judge_many_roots.py has the rest)
    finally:
        off_bv.close()
        on_bv.close()


def test_eight_slots_for_sixteen_keys(scan_threshold, monkeypatch):
    """IBFT_CERT_DEDUP_SLOTS=8 on the flat tree of T + 1 draws: whole keys give up, thousands of rows are judged on their own"""
    set_overlap(monkeypatch, None)
    monkeypatch.setenv("IBFT_CERT_DEDUP_SLOTS", "8")
    r, msgs, tree, _ = CC.long_tree("flat", scan_threshold + 1)
    off_bv, on_bv = make_bv(r, False), make_bv(r, True)
    try:
        stats_off, stats_on = D.check_pair("8 slots", off_bv, on_bv, msgs, tree)
        assert stats_on[3] > 0 and stats_on[2] <= stats_on[1] == stats_off[1], stats_on
        assert stats_on[2] > M.expected_stats(tree, True)[2]
    finally:
        off_bv.close()
        on_bv.close()


@pytest.mark.parametrize("slots", [None, "8"], ids=["default table", "8 slots"])
def test_a_full_context(slots, scan_threshold, monkeypatch):
    """max_rows == rows_cap == the tree's rows (26 652: no multiple of 64), two verdict launches: the tree's rows, the deferred
    batch and the dense batch lie one behind the other in the columns the library sized for this context; one row fewer in
    rows_cap is IBFT_E_TOOBIG, as without the flag"""
    set_overlap(monkeypatch, None)
    if slots:
        monkeypatch.setenv("IBFT_CERT_DEDUP_SLOTS", slots)
    r, msgs, tree, _ = CC.long_tree("flat", scan_threshold + 1)
    assert tree.n_rows % 64 != 0 and two_launches(None, tree)
    off_bv, on_bv = make_bv(r, False, max_rows=tree.n_rows), make_bv(r, True, max_rows=tree.n_rows)
    try:
        _, stats_on = D.check_pair(("full", slots), off_bv, on_bv, msgs, tree)
        if slots is None:
            assert stats_on == M.expected_stats(tree, True) + (0,)
        else:
            assert stats_on[3] > 0
        buf, off = CC.pack(msgs)
        for bv in (off_bv, on_bv):
            with pytest.raises(RuntimeError, match="-7"):
                bv.verify_certificates_wire(buf, off, rows_cap=tree.n_rows - 1)
            with pytest.raises(RuntimeError, match="-7"):
                bv.judge_certificates_wire(buf, off, rows_cap=tree.n_rows - 1)
        D.check_pair(("full, after the refusals", slots), off_bv, on_bv, msgs, tree)
    finally:
        off_bv.close()
        on_bv.close()


def test_a_full_context_of_129_rows():
    """the 129-row edge input of cert_dedup_model.edge_inputs in a context of exactly 129 rows"""
    r = M.edge_round()
    msgs = M.edge_inputs()[129]
    tree = WC.expected_tree(msgs, r.addrs)
    assert tree.n_rows == 129
    off_bv, on_bv = D.make_bv(r, [1] * r.n, False), D.make_bv(r, [1] * r.n, True)
    import go_ibft_amd.verifier as V
    full_off, full_on = (J.make_bv([1] * r.n, r.addrs, flags=f, max_rows=129) for f in (0, V.FLAG_CERT_DEDUP))
    try:
        _, roomy = D.check_pair("129 rows, a roomy context", off_bv, on_bv, msgs, tree)
        _, stats_on = D.check_pair("129 rows, a full context", full_off, full_on, msgs, tree)
        assert stats_on == roomy == M.expected_stats(tree, False) + (0,)
        buf, off = CC.pack(msgs)
        for bv in (full_off, full_on):
            with pytest.raises(RuntimeError, match="-7"):
                bv.verify_certificates_wire(buf, off, rows_cap=128)
    finally:
        for bv in (off_bv, on_bv, full_off, full_on):
            bv.close()


def all_flagged_batch():
    """three ROUND_CHANGE messages with a certificate of 12 messages each, every signature 64 bytes long: every row parses and
    every row carries a pre-flag"""
    r = M.edge_round()
    H, RND = M.H, M.RND

    def cut(m):
        m.signature = m.signature[:64]
        return m
    prop = K.proposer(r.n, H, 1)
    hsh = B.proposal_hash(r.raw, 1)
    pp = cut(CC.preprepare(r, prop, H, 1))
    prs = [cut(CC.prepare(r, i, H, 1, h=hsh)) for i in [i for i in range(r.n) if i != prop][:11]]
    pcb = wire.prepared_certificate(pp, prs)
    return r, [cut(CC.round_change(r, c, H, RND, wire.Proposal(r.raw, 1), pcb)).encode() for c in range(3)]


def test_every_row_carries_a_pre_flag():
    """the dense batch is empty: the verdict launch over it has nothing to do and every verdict word of the tree is stored as 0"""
    r, msgs = all_flagged_batch()
    tree = WC.expected_tree(msgs, r.addrs)
    assert tree.n_rows == 39 and not any(tree.sender_ok) and all(s == WC.OK for s in tree.status)
    assert M.expected_stats(tree, False) == (39, 0, 0)
    off_bv, on_bv = D.make_bv(r, [1] * r.n, False), D.make_bv(r, [1] * r.n, True)
    try:
        # an honest batch first: its verdict words are all ones where the flagged batch's must read 0
        honest = M.edge_inputs()[65]
        D.check_pair("honest", off_bv, on_bv, honest, WC.expected_tree(honest, r.addrs))
        stats_off, stats_on = D.check_pair("all flagged", off_bv, on_bv, msgs, tree)
        assert stats_off == stats_on == (39, 0, 0, 0)
    finally:
        off_bv.close()
        on_bv.close()
