"""GPU: ibft_verify_messages_wire_views — the views call with the committed seals of the COMMIT rows judged in the same verdict
launch and the COMMIT records tallied over stored ∧ sealed.  Oracles: (1) ibft_verify_senders_wire_views on the same context
and batch: every shared output byte for byte, the records equal but for pad[0] and tally of COMMIT records; (2) the plain model
of tests/wire_view_seals_model.py over the CPU oracle's walk, signature check and seal check (tests/wire_view_seals_cases.py:
expected) for out_seal and every record; (3) the device's own single-set calls on a second context: ibft_set_validators(set) +
ibft_verify_seals over the valid COMMIT rows of each set for out_seal, ibft_tally(S_v, seal bits) for each COMMIT record.
Everything compared is a bit, an integer or a byte string: equality is exact.  The corpora and what they hold:
tests/wire_view_seals_cases.py, tests/test_wire_view_seals_inputs.py."""
import numpy as np
import pytest

import wire_sets_cases as WS
import wire_view_seals_cases as SC
import wire_view_seals_harness as SH
import wire_view_seals_model as SM
import wire_views_child as K
import wire_views_harness as H

pytestmark = pytest.mark.gpu


def _V():
    import go_ibft_amd.verifier as V
    return V


def _tally_fields(t):
    return (t.quorum_lo, t.quorum_hi, t.power_lo, t.power_hi, t.valid_rows, t.distinct_senders, t.has_quorum, t.shard_overlap,
            t.proposer_rows, t.reserved)


def _pad(b: bytes, k: int) -> bytes:
    return b.ljust(k, b"\0")[:k]


def _install_set(ref, c, s):
    h, a, p = c.sets()[s]
    (ref.set_validators_u256 if c.big else ref.set_validators)(h, a, p)


def _check(bv, ref, c, hmap, recode, cap, suffix="corpus", sample=None):
    """one batch on bv against the three oracles, then a second call (all scratch is zero again); ref: a second context with
    the same seal-digest convention.  sample: the COMMIT records oracle (3) tallies (default: all)"""
    n = len(c.msgs)
    wire, off = WS.pack(c.msgs)
    plain = bv.verify_senders_wire_views(wire, off, cap)
    out = bv.verify_messages_wire_views(wire, off, cap)
    got, rows, rset, vidx, tl, view, stored, views, n_views, seal = out
    e = SC.expected(c, hmap, recode, cap, suffix)
    # (1) the views call: every shared output, and every record field but pad[0] and tally of COMMIT records
    blank = [views.copy(), plain[7].copy()]
    for recs in blank:
        commit = recs["type"] == SM.COMMIT
        recs["pad"][commit, SM.SEAL_RULE] = 0
        recs["tally"][commit] = np.zeros((), recs["tally"].dtype)
    assert SH.output_bytes(out[:7] + (blank[0], n_views)) == SH.output_bytes(plain[:7] + (blank[1], plain[8]))
    assert (views["pad"][views["type"] == SM.COMMIT, SM.SEAL_RULE] == 1).all() and not plain[7]["pad"].any()
    assert views[views["type"] != SM.COMMIT].tobytes() == plain[7][plain[7]["type"] != SM.COMMIT].tobytes()
    # (2) the model
    K.check_model(plain, dict(e, records=[]), cap, n)
    assert [H.record_dict(r) for r in plain[7]] == [SH.model_record(w) for w in e["views_records"]]
    assert seal.tolist() == e["seal"], np.nonzero(seal != np.array(e["seal"]))[0][:10]
    assert [H.record_dict(r) for r in views] == [SH.model_record(w) for w in e["records"]]
    assert bv.wire_seal_stats() == (e["commit_rows"], e["seal_rows"])
    # (3) the single-set calls: ibft_verify_seals over the valid COMMIT rows of each set, rows that are not sealable pre-flagged
    p = e["parsed"]
    sets = c.model_sets()
    for s in sorted({x for x in e["set"] if x >= 0}):
        idx = [j for j in range(n) if got[j] and e["set"][j] == s and p[j].type == SM.COMMIT]
        if not idx:
            continue
        _install_set(ref, c, s)
        h = np.frombuffer(b"".join(_pad(p[j].proposal_hash, 32) for j in idx), np.uint8).reshape(-1, 32)
        sg = np.frombuffer(b"".join(_pad(p[j].committed_seal, 65) for j in idx), np.uint8).reshape(-1, 65)
        fr = np.frombuffer(b"".join(_pad(p[j].sender, 20) for j in idx), np.uint8).reshape(-1, 20)
        pre = np.array([0 if SM.is_sealable(p[j], s, sets) else 1 for j in idx], np.uint8)
        bits, _ = ref.is_valid_committed_seal(h, sg, fr, pre)
        assert bits.tolist() == [bool(seal[j]) for j in idx], s
    # … and ibft_tally(S_v, the seal bits of S_v) for the COMMIT records
    senders = np.array([np.frombuffer(_pad(x.sender, 20), np.uint8) for x in p], np.uint8).reshape(n, 20)
    installed = None
    for v, r in enumerate(views):
        if int(r["type"]) != SM.COMMIT or (sample is not None and v not in sample):
            continue
        s = int(r["set"])
        if s != installed:
            _install_set(ref, c, s)
            installed = s
        sv = (view == v) & stored
        assert sv.sum() == int(r["stored_rows"]) >= int(r["tally"]["valid_rows"])
        t = ref.has_quorum(senders[sv], seal[sv])
        assert _tally_fields(t) == tuple(int(r["tally"][f]) for f in r["tally"].dtype.names), v
    # afterwards: what the views call leaves
    assert bv.seals_rows()[0] == 0 and bv.wire_stats()[0] == n
    # a second identical call returns the same bytes
    assert SH.output_bytes(bv.verify_messages_wire_views(wire, off, cap)) == SH.output_bytes(out)
    return out, plain


@pytest.mark.parametrize("big", [False, True], ids=["u64", "u256"])
@pytest.mark.parametrize("cache", [False, True], ids=["cold", "warm"])
def test_corpus_s_defining_property(oracle, big, cache):
    V = _V()
    c = SC.corpus_s(big)
    n = len(c.msgs)
    flags = V.FLAG_PUBKEY_CACHE if cache else 0
    bv, ref = V.BatchVerifier(flags=flags, max_rows=1024), V.BatchVerifier(flags=flags, max_rows=1024)
    try:
        K.install(bv, c)
        out, plain = _check(bv, ref, c, WS.MAP_A, False, n)          # (with the cache flag its second and later calls run warm)
        if cache:
            assert bv.cache_stats()[1] > 0
            _check(bv, ref, c, WS.MAP_A, False, n)                   # warm from the first launch on
        # the quorum edge: the views call sees a quorum in both views of height 105, this call in the one whose seals all verify
        for round_, want in ((SC.EDGE_FULL_ROUND, 1), (SC.EDGE_SHORT_ROUND, 0)):
            pick = lambda recs: [r for r in recs if (int(r["height"]), int(r["round"]), int(r["type"])) == (SC.EDGE_HEIGHT, round_, SM.COMMIT)]
            (a,), (b,) = pick(plain[7]), pick(out[7])
            assert int(a["tally"]["has_quorum"]) == 1 and int(b["tally"]["has_quorum"]) == want and int(b["stored_rows"]) == 4
        for cap in (1, out[8] - 1):
            _check(bv, ref, c, WS.MAP_A, False, cap)
    finally:
        bv.close()
        ref.close()


def test_corpus_s_suffix_convention(oracle):
    V = _V()
    signed, identity = SC.corpus_s(suffix=SC.SUFFIX), SC.corpus_s()
    n = len(signed.msgs)
    bv, ref = V.BatchVerifier(max_rows=1024), V.BatchVerifier(max_rows=1024)
    try:
        K.install(bv, signed)
        bv.set_seal_digest(SC.SUFFIX)
        ref.set_seal_digest(SC.SUFFIX)
        out, _ = _check(bv, ref, signed, WS.MAP_A, False, n)
        assert out[9].any() and any(int(r["tally"]["has_quorum"]) for r in out[7] if int(r["type"]) == SM.COMMIT)
        # the identity-signed corpus on this context: no seal verifies, no COMMIT record has a quorum
        out, plain = _check(bv, ref, identity, WS.MAP_A, False, n, suffix=SC.SUFFIX)
        assert not out[9].any() and not any(int(r["tally"]["has_quorum"]) for r in out[7] if int(r["type"]) == SM.COMMIT)
        assert any(int(r["tally"]["has_quorum"]) for r in plain[7] if int(r["type"]) == SM.COMMIT)
    finally:
        bv.close()
        ref.close()


def test_corpus_s_with_the_recode_flag(oracle):
    V = _V()
    c = SC.corpus_s()
    bv, ref = V.BatchVerifier(flags=V.FLAG_WIRE_RECODE, max_rows=1024), V.BatchVerifier(flags=V.FLAG_WIRE_RECODE, max_rows=1024)
    try:
        K.install(bv, c)
        out, _ = _check(bv, ref, c, WS.MAP_A, True, len(c.msgs))
        j = c.kinds.index("padded_height")
        assert out[0][j] and out[9][j] and bv.wire_stats()[1] == 1          # the recoded COMMIT is valid and its seal verifies
    finally:
        bv.close()
        ref.close()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_small_sizes(oracle, n):
    V = _V()
    c = SC.corpus_t(n)
    bv, ref = V.BatchVerifier(max_rows=128), V.BatchVerifier(max_rows=128)
    try:
        K.install(bv, c)
        out, _ = _check(bv, ref, c, WS.MAP_A, False, n)
        assert out[9].tolist() == [j not in SC.T_BAD for j in range(n)] and bv.wire_seal_stats() == (n, n)
    finally:
        bv.close()
        ref.close()


def test_corpus_b_across_workgroups(oracle):
    V = _V()
    c = SC.corpus_b()
    bv, ref = V.BatchVerifier(max_rows=1024), V.BatchVerifier(max_rows=1024)
    try:
        K.install(bv, c)
        _check(bv, ref, c, WS.MAP_A, False, len(c.msgs))
    finally:
        bv.close()
        ref.close()


def test_more_rows_than_scan_threads(oracle):
    """1 029 rows: wire_seals_scan_kernel (and the views' rank kernel) give two rows to a thread, the last thread that has any
    a single one; sealable rows, PREPAREs and bad seals interleaved, so the dense seal rows depend on every thread's offset"""
    V = _V()
    c = SC.corpus_b(1029)
    bv, ref = V.BatchVerifier(max_rows=2048), V.BatchVerifier(max_rows=2048)
    try:
        K.install(bv, c)
        out, _ = _check(bv, ref, c, WS.MAP_A, False, len(c.msgs))
        assert 0 < bv.wire_seal_stats()[1] < 1029 and 0 < out[9].sum() < bv.wire_seal_stats()[1]
    finally:
        bv.close()
        ref.close()


def test_corpus_c_a_view_per_row(oracle):
    """64 views in every wavefront: the tally's per-lane fallback; views_cap below the number of views"""
    V = _V()
    c = SC.corpus_c()
    bv, ref = V.BatchVerifier(max_rows=1024), V.BatchVerifier(max_rows=1024)
    try:
        K.install(bv, c)
        out, _ = _check(bv, ref, c, WS.MAP_A, False, SC.C_CAP, sample=(0, 1, 2, 63, 64, 65, SC.C_CAP - 1))
        assert out[8] == SC.C_ROWS and len(out[7]) == SC.C_CAP
        assert out[9].tolist() == [j % 3 != 2 for j in range(SC.C_ROWS)]     # the bit is defined beyond the cap as well
    finally:
        bv.close()
        ref.close()


def test_alternating_calls_and_a_clean_work_mask(oracle):
    V = _V()
    c = SC.corpus_s()
    n = len(c.msgs)
    wire, off = WS.pack(c.msgs)
    bv = V.BatchVerifier(max_rows=1024)
    try:
        K.install(bv, c)
        # views call → this call → views call: the views call's bytes unchanged; stats are this call's alone
        first = SH.output_bytes(bv.verify_senders_wire_views(wire, off, n))
        assert bv.wire_seal_stats() == (0, 0)
        out = bv.verify_messages_wire_views(wire, off, n)
        e = SC.expected(c, WS.MAP_A, False, n)
        assert bv.wire_seal_stats() == (e["commit_rows"], e["seal_rows"]) and e["seal_rows"] > 0
        assert SH.output_bytes(bv.verify_senders_wire_views(wire, off, n)) == first
        assert bv.wire_seal_stats() == (0, 0)                                # 0 / 0 after any other wire call
        assert SH.output_bytes(bv.verify_messages_wire_views(wire, off, n)) == SH.output_bytes(out)
        bv.verify_senders_wire_sets(wire, off)
        assert bv.wire_seal_stats() == (0, 0)
        bv.verify_messages_wire_views(wire, off, n)
        # a clean work mask: ibft_verify_seals over more than half + n rows on the same context, against the oracle — seal
        # words left behind in the work mask would show as bits of rows that have none
        half = (n + 63) // 64 * 64
        m = half + n + 70
        assert m <= 1024
        pool = c.pool
        members = WS.MEMBERS[0]
        _install_set(bv, c, 0)
        h = np.frombuffer(SC.HA * m, np.uint8).reshape(m, 32)
        seals, froms, want = [], [], []
        for j in range(m):
            i = members[j % 40]
            good = j % 3 != 1
            seals.append(SC.seal_of(pool.sks[i], SC.HA if good else SC.HB, None))
            froms.append(pool.addrs[i].tobytes())
            want.append(good)
        bits, _ = bv.is_valid_committed_seal(h, np.frombuffer(b"".join(seals), np.uint8).reshape(m, 65),
                                             np.frombuffer(b"".join(froms), np.uint8).reshape(m, 20))
        assert want == [oracle.recover_address(SC.HA, s) == f for s, f in zip(seals, froms)]
        assert bits.tolist() == want
    finally:
        bv.close()


def test_edge_batches(oracle):
    V = _V()
    c = SC.corpus_s()
    bv = V.BatchVerifier(max_rows=1024)
    try:
        K.install(bv, c)
        # n = 0
        out = bv.verify_messages_wire_views(b"", np.zeros(1, np.uint32), 8)
        assert len(out[0]) == 0 and len(out[5]) == 0 and len(out[7]) == 0 and out[8] == 0 and len(out[9]) == 0
        assert [bytes(t) for t in out[4]] == [bytes(t) for t in bv.verify_senders_wire_sets(b"", np.zeros(1, np.uint32))[4]]
        assert bv.wire_seal_stats() == (0, 0)
        # a batch without COMMITs: seal mask zero, stats 0 / 0, records equal the views call's
        prepares = [m for m, k in zip(c.msgs, c.kinds) if k == "prepare"]
        wire, off = WS.pack(prepares)
        out = bv.verify_messages_wire_views(wire, off, len(prepares))
        assert out[0].any() and not out[9].any() and bv.wire_seal_stats() == (0, 0) and len(out[7]) > 0
        assert SH.output_bytes(out[:9]) == SH.output_bytes(bv.verify_senders_wire_views(wire, off, len(prepares)))
        # views_cap = 0 with rows is refused and writes nothing
        mask, seal, nv = np.full(1, 7, np.uint64), np.full(1, 5, np.uint64), np.full(1, 9, np.uint32)
        assert bv._L.ibft_verify_messages_wire_views(bv._h, V._p(np.frombuffer(wire, np.uint8)), V._p(off), len(prepares), 0, V._p(mask), None,
                                                     None, None, None, None, None, None, nv.ctypes.data_as(V.C.POINTER(V.C.c_uint32)),
                                                     V._p(seal)) == SM.E_INVAL
        assert mask[0] == 7 and seal[0] == 5 and nv[0] == 9
    finally:
        bv.close()
