"""§8f rank 2 from the transport's bytes, on the GPU: ibft_verify_certificates_wire — the certificate tree of PREPREPARE /
ROUND_CHANGE messages expanded level by level on the device, every nested message a row of ONE verdict launch — against
the independent oracle (oracle/wire_cert.py): tree shape, canonical / NEEDS_HOST classes, sender, hash and self bits."""
import numpy as np
import pytest

import cert_cases as CC
from oracle import wire
from oracle import wire_cert as WC
from oracle import workload as W

pytestmark = pytest.mark.gpu


def run(bv, r, label, msgs, cap=None, tree=None):
    """tree: the oracle's tree of msgs where it was made before (None under a rows_cap it does not fit, as expected_tree says)"""
    buf, off = CC.pack(msgs)
    limit = min(cap or bv.max_rows, bv.max_rows)
    exp = WC.expected_tree(msgs, r.addrs, rows_cap=limit) if tree is None else (tree if tree.n_rows <= limit else None)
    if exp is None:
        with pytest.raises(RuntimeError, match="-7"):
            bv.verify_certificates_wire(buf, off, rows_cap=cap)
        return None
    n, nodes, rows, cls, sender, hb, sb = bv.verify_certificates_wire(buf, off, rows_cap=cap)
    CC.compare(label, exp, n, nodes, rows, cls, sender, hb, sb)
    return exp


@pytest.mark.parametrize("cache", [False, True])
def test_handmade_and_fuzzed_trees(cache):
    import go_ibft_amd.verifier as V
    r = W.make_round(8, 811, height=5, round_=1)
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if cache else 0, max_rows=4096)
    try:
        bv.set_validators(5, r.addrs, r.power)
        for _ in range(2 if cache else 1):  # second pass on the warm kernels
            for label, msgs in CC.handmade(r):
                run(bv, r, label, msgs)
        for i, msgs in enumerate(CC.fuzz_batches(r, 150, 4242)):
            run(bv, r, f"fuzz {i}", msgs)
        msgs = [m.encode() for m in CC.honest_round_change_set(r)]
        assert run(bv, r, "cap exactly", msgs, cap=56) is not None
        assert run(bv, r, "cap one short", msgs, cap=55) is None
        assert run(bv, r, "cap below the call's messages", msgs, cap=7) is None
    finally:
        bv.close()


def test_longer_than_the_device_hashes(gpu_verifier):
    r = W.make_round(4, 812, height=5, round_=1, raw_len=(1 << 20) + 5)
    gpu_verifier.set_validators(5, r.addrs, r.power)
    rc = CC.round_change(r, 0, 5, 2, wire.Proposal(r.raw, 1), CC.pc_bytes(r, 5, 1, 1, [2, 3]))
    exp = run(gpu_verifier, r, "1 MiB proposal", [rc.encode(), CC.prepare(r, 1, 5, 2).encode()])
    both = WC.CLASS_DIGEST_BY_HOST | WC.CLASS_PROPOSAL_BY_HOST
    assert exp.cls[0] == both and exp.cls[2] == both and exp.cls[1] == 0 and exp.sender_ok[3]


def test_round_change_certificate_n256(gpu_verifier):
    """BASELINE-style worst case at N = 256: a PREPREPARE whose RoundChangeCertificate holds 171 ROUND_CHANGE messages, each
    with a PreparedCertificate of 1 + 170 messages — 29 412 nested signatures from one 4.1 MB message, one call; then the
    same with a fifth of the nested PREPAREs corrupted.  What it covers: parsing, walking and judging a tree of that size.  What
    it does not: the tiled scan's output.  Its only level of more than CERT_SCAN_ONE_GROUP_MAX rows is the leaf level (171²
    messages, none deferred, no children), where first_child is not compared and both totals are 0; the levels with children have
    1 and 171 rows.  The long levels WITH children are test_long_level* below and tests/test_gpu_cert_scan.py."""
    n = 256
    r = W.make_round(n, 815, height=5, round_=1, raw_len=256)
    gpu_verifier.set_validators(5, r.addrs, r.power)
    q = (2 * n) // 3 + 1
    proposer = 1
    h1 = r.proposal_hash
    pm = CC.preprepare(r, proposer, 5, 1)
    prepares = [CC.prepare(r, j, 5, 1, h=h1) for j in range(n) if j != proposer][: q - 1]
    pcb = wire.prepared_certificate(pm, prepares)
    rcs = [CC.round_change(r, i, 5, 2, wire.Proposal(r.raw, 1), pcb) for i in range(q)]
    top = CC.preprepare(r, 2, 5, 2, rcc=wire.round_change_certificate(rcs))
    exp = run(gpu_verifier, r, "rcc n=256", [top.encode()])
    assert exp.n_rows == 1 + q + q * q and all(exp.sender_ok[1:]) and all(exp.hash_bit[1 + q:]) and exp.self_bit[0]
    assert exp.cls[0] == WC.CLASS_DIGEST_BY_HOST and not any(exp.cls[1:])  # the 4 MB envelope itself: its digest is the host's
    # Byzantine: every fifth nested PREPARE of every certificate is forged, for another proposal, or from a stranger
    outsider = b"\x07" * 32
    bad = []
    for k, m in enumerate(prepares):
        if k % 5 == 0:
            m = CC.prepare(r, (k + 3) % n, 5, 1, h=h1, sk=outsider)
        elif k % 5 == 1 and k % 2:
            m = CC.prepare(r, (k + 3) % n, 5, 1, h=b"\x00" * 32)
        bad.append(m)
    pcb2 = wire.prepared_certificate(pm, bad)
    rcs2 = [CC.round_change(r, i, 5, 2, wire.Proposal(r.raw, 1), pcb2 if i % 2 else pcb) for i in range(q)]
    top2 = CC.preprepare(r, 2, 5, 2, rcc=wire.round_change_certificate(rcs2))
    exp = run(gpu_verifier, r, "rcc n=256 byzantine", [top2.encode()])
    assert 1000 < sum(1 for x in exp.sender_ok if not x) < exp.n_rows // 4


def test_certificate_longer_than_the_walk_window(gpu_verifier):
    """children on either side of the 16 KiB LDS windows of cert_walk_kernel, more than 64 per window, a batch of containers"""
    r = W.make_round(600, 816, height=5, round_=1, raw_len=40)
    gpu_verifier.set_validators(5, r.addrs, r.power)
    msgs = []
    for k, cnt in enumerate((599, 130, 64, 65, 1, 0, 257)):
        pc = CC.pc_bytes(r, 5, 1, 1, [i for i in range(600) if i != 1][:cnt])
        msgs.append(CC.round_change(r, k, 5, 2, wire.Proposal(r.raw, 1), pc).encode())
    exp = run(gpu_verifier, r, "long certificates", msgs)
    assert exp.n_rows == 7 + 7 + 599 + 130 + 64 + 65 + 1 + 257 and all(exp.sender_ok)


def test_golden_trees(gpu_verifier):
    """tests/golden/cert_trees.json: 2 000 batches (hand-made cases, then byte-level fuzz), one digest per batch over tree shape,
    classes, sender / hash / self bits and parsed fields; the expectation was cross-checked against the google.protobuf runtime when
    the fixture was made (tests/golden/make_cert_golden.py)"""
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cert_trees.json")))
    r, batches = CC.golden_batches(gold["count"])
    gpu_verifier.set_validators(5, r.addrs, r.power)
    bad = []
    for bi, msgs in enumerate(batches):
        buf, off = CC.pack(msgs)
        n, nodes, rows, cls, sender, hb, sb = gpu_verifier.verify_certificates_wire(buf, off, rows_cap=4096)
        if CC.digest_actual(n, nodes, rows, cls, sender, hb, sb) != gold["digests"][bi]:
            bad.append(bi)
    assert not bad, bad[:20]


def test_certificate_calls_feed_the_key_cache():
    """The certificate path has no tally kernel to carry the "keys learned" counter to the host: a key-caching context must
    still notice what its certificate calls taught the device, build the tables and serve the next call warm (a regression
    of round 3's device-wide key cache showed up as warm = cold in the bench line's certificates leg)."""
    import go_ibft_amd.verifier as V
    n = 64
    r = W.make_round(n, 871, height=5, round_=1, raw_len=64)
    q = (2 * n) // 3 + 1
    pm = CC.preprepare(r, 1, 5, 1)
    pcb = wire.prepared_certificate(pm, [CC.prepare(r, j, 5, 1) for j in range(n) if j != 1][: q - 1])
    msgs = [CC.round_change(r, i, 5, 2, wire.Proposal(r.raw, 1), pcb).encode() for i in range(q)]
    buf, off = CC.pack(msgs)
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=4096)
    try:
        bv.set_validators(5, r.addrs, r.power)
        for _ in range(3):
            k, _, _, cls, snd, _, _ = bv.verify_certificates_wire(buf, off, rows_cap=4096, want_rows=False)
            assert k == q * (q + 1) and snd.all() and not cls.any()
        tables, warm, cold = bv.cache_stats()
        assert tables >= q and warm >= 1, (tables, warm, cold)       # every signer of the tree has a table; a warm pass ran
    finally:
        bv.close()


@pytest.mark.parametrize("world", [2, 3, 5])
def test_certificates_sharded_by_carrier_equal_one_call(world):
    """ibft_group_verify_certificates_wire: the trees of a batch split by carrier over `world` contexts (here all on device 0,
    each with its own stream), judged at once, and renumbered — n_rows, every node field (offsets into the WHOLE wire, parents,
    first children, ordinals), the parsed rows, classes and the three masks equal those of ONE call over the whole batch;
    and the oracle's tree.  Batches with fewer carriers than contexts, deep trees (PREPREPARE → ROUND_CHANGE → PREPARE) and
    non-canonical messages included."""
    import go_ibft_amd.verifier as V
    r = W.make_round(8, 811, height=5, round_=1)
    bv = V.BatchVerifier(max_rows=4096)
    g = V.DeviceGroup([0] * world, max_rows_total=4096 * world)
    try:
        bv.set_validators(5, r.addrs, r.power)
        g.set_validators(5, r.addrs, r.power)
        batches = [msgs for _, msgs in CC.handmade(r)] + list(CC.fuzz_batches(r, 60, 77))
        honest = [m.encode() for m in CC.honest_round_change_set(r)]
        batches += [honest, honest[:1], honest + [CC.preprepare_with_rcc(r).encode()] + honest[:3]]
        checked = 0
        for k, msgs in enumerate(batches):
            buf, off = CC.pack(msgs)
            if WC.expected_tree(msgs, r.addrs, rows_cap=4096) is None:
                continue
            one = bv.verify_certificates_wire(buf, off, rows_cap=4096)
            many = g.verify_certificates_wire(buf, off, rows_cap=4096)
            assert one[0] == many[0], k
            for name in one[1].dtype.names:
                if name == "first_child":       # means nothing for a leaf (include/ibftgpu.h): compared where there are children
                    has = one[1]["n_children"] > 0
                    assert (one[1][name][has] == many[1][name][has]).all(), (k, name)
                    assert (many[1][name][~has] < max(many[0], 1)).all(), (k, "a leaf's first_child must stay inside the tree")
                elif name != "pad":
                    assert (one[1][name] == many[1][name]).all(), (k, name)
            assert one[2].tobytes() == many[2].tobytes(), k
            for a, b in zip(one[3:], many[3:]):
                assert (a == b).all(), k
            CC.compare(f"sharded {k}", WC.expected_tree(msgs, r.addrs, rows_cap=4096), *many)
            checked += 1
        assert checked > 40
        with pytest.raises(RuntimeError, match="-7"):              # the merged tree must fit rows_cap
            g.verify_certificates_wire(*CC.pack(honest), rows_cap=55)
    finally:
        g.close()
        bv.close()


# ---- long levels: more rows with children in one level than the single-workgroup scan takes --------------------------
# tests/cert_cases.py: long_tree (what these trees are is checked without a device in tests/test_cert_long_cases.py).
LONG_SHAPES = ["flat", "nested"]


@pytest.fixture(scope="module")
def scan_threshold():
    import ctypes as C
    import go_ibft_amd.build as B
    L = C.CDLL(B.build_devtest())
    L.devtest_cert_scan_threshold.restype = C.c_uint32
    return int(L.devtest_cert_scan_threshold())


def run_long(bv, label, shape, K, cap=None):
    r, msgs, tree, _ = CC.long_tree(shape, K)
    bv.set_validators(5, r.addrs, r.power)
    buf, off = CC.pack(msgs)
    if cap is None or cap >= tree.n_rows:
        # first, the scan's own output where it means something, so that a failure names the scan
        n, nodes = bv.verify_certificates_wire(buf, off, rows_cap=cap, want_rows=False)[:2]
        assert n == tree.n_rows, (label, "rows", n, tree.n_rows)
        want = np.array([nd["first_child"] for nd in tree.nodes], dtype=np.int64)
        has = np.array([nd["n_children"] > 0 for nd in tree.nodes])
        kids = np.array([nd["n_children"] for nd in tree.nodes], dtype=np.int64)
        assert (nodes["n_children"] == kids).all(), (label, "n_children", int(np.nonzero(nodes["n_children"] != kids)[0][0]))
        bad = np.nonzero(has & (nodes["first_child"] != want))[0]
        assert bad.size == 0, (label, "first_child (the level's scan)", int(bad[0]), int(nodes["first_child"][bad[0]]), int(want[bad[0]]))
    return run(bv, r, label, msgs, cap=cap, tree=tree)


@pytest.mark.parametrize("overlap", [None, "0"])
@pytest.mark.parametrize("dk", [0, 1])
@pytest.mark.parametrize("shape", LONG_SHAPES)
def test_long_level(shape, dk, overlap, scan_threshold, monkeypatch):
    """A level of T and of T + 1 rows with children (T = CERT_SCAN_ONE_GROUP_MAX: the single workgroup's last size, and the tiled
    form with one row in its last tile), at row 0 of the tree and at lo = 4 / slot_base = 2, and a longer level below it; more
    than 8 192 deferred rows, so with IBFT_CERT_OVERLAP unset their second verdict launch is a group kernel at a row base
    (cert_carrier_stage_kernel, cert_scatter_kernel), with =0 there is one launch.  Every node field, row, class and mask
    against the oracle."""
    import go_ibft_amd.verifier as V
    if overlap is None:
        monkeypatch.delenv("IBFT_CERT_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("IBFT_CERT_OVERLAP", overlap)
    bv = V.BatchVerifier(max_rows=CC.LONG_LEVEL_MAX_ROWS)
    try:
        assert run_long(bv, f"long {shape} K=T+{dk} overlap={overlap}", shape, scan_threshold + dk) is not None
    finally:
        bv.close()


@pytest.mark.parametrize("dk", [0, 1])
@pytest.mark.parametrize("shape", LONG_SHAPES)
def test_long_level_on_the_warm_kernels(shape, dk, scan_threshold, monkeypatch):
    """the same trees in a key-caching context, twice: the second call judges both launches with the known-key kernels"""
    import go_ibft_amd.verifier as V
    monkeypatch.delenv("IBFT_CERT_OVERLAP", raising=False)
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=CC.LONG_LEVEL_MAX_ROWS)
    try:
        for call in range(2):
            assert run_long(bv, f"long {shape} K=T+{dk} cached, call {call}", shape, scan_threshold + dk) is not None
        tables, warm, cold = bv.cache_stats()
        assert tables >= 7 and warm >= 1, (tables, warm, cold)   # validators 0 … 6 sign in these trees
    finally:
        bv.close()


@pytest.mark.parametrize("dk", [0, 1])
def test_long_level_sharded_equals_one_call(dk, scan_threshold, monkeypatch):
    """The flat tree over three contexts: every shard's levels are short (the single-workgroup scan on each), the library
    renumbers — field by field the answer of ONE call, whose long levels went through the tiled scan; and the oracle's tree."""
    import go_ibft_amd.verifier as V
    monkeypatch.delenv("IBFT_CERT_OVERLAP", raising=False)
    r, msgs, tree, _ = CC.long_tree("flat", scan_threshold + dk)
    cap = CC.LONG_LEVEL_MAX_ROWS
    per = (len(msgs) + 2) // 3                                      # a shard's messages, and the rows of its level 1
    below = [sum(tree.nodes[k]["n_children"] for k in range(lo, min(lo + per, len(msgs)))) for lo in range(0, len(msgs), per)]
    assert len(below) == 3 and per <= scan_threshold and max(below) <= scan_threshold < sum(below)   # short on every shard, long in one call
    bv = V.BatchVerifier(max_rows=cap)
    g = V.DeviceGroup([0] * 3, max_rows_total=3 * cap)
    try:
        bv.set_validators(5, r.addrs, r.power)
        g.set_validators(5, r.addrs, r.power)
        buf, off = CC.pack(msgs)
        one = bv.verify_certificates_wire(buf, off, rows_cap=cap)
        many = g.verify_certificates_wire(buf, off, rows_cap=cap)
        assert one[0] == many[0] == tree.n_rows
        for name in one[1].dtype.names:
            if name == "first_child":       # means nothing for a leaf (include/ibftgpu.h): compared where there are children
                has = one[1]["n_children"] > 0
                assert (one[1][name][has] == many[1][name][has]).all(), name
                assert (many[1][name][~has] < many[0]).all(), "a leaf's first_child must stay inside the tree"
            elif name != "pad":
                assert (one[1][name] == many[1][name]).all(), name
        assert one[2].tobytes() == many[2].tobytes()
        for a, b in zip(one[3:], many[3:]):
            assert (a == b).all()
        CC.compare(f"long flat K=T+{dk} sharded", tree, *many)
        CC.compare(f"long flat K=T+{dk} one call", tree, *one)
    finally:
        g.close()
        bv.close()


def test_long_level_rows_cap_edge(scan_threshold, monkeypatch):
    """hi + total > cap with the total from cert_scan_offsets_kernel: exactly n_rows passes, one less is IBFT_E_TOOBIG"""
    import go_ibft_amd.verifier as V
    monkeypatch.delenv("IBFT_CERT_OVERLAP", raising=False)
    tree = CC.long_tree("flat", scan_threshold + 1)[2]
    bv = V.BatchVerifier(max_rows=CC.LONG_LEVEL_MAX_ROWS)
    try:
        assert run_long(bv, "long flat cap exactly", "flat", scan_threshold + 1, cap=tree.n_rows) is not None
        assert run_long(bv, "long flat cap one short", "flat", scan_threshold + 1, cap=tree.n_rows - 1) is None
    finally:
        bv.close()
