"""GPU: ibft_verify_senders_wire_views — the sets call plus one quorum record per (height, round, type, proposal hash).
Oracles: (1) ibft_verify_senders_wire_sets on the same context and batch for the five shared outputs, byte for byte; (2) the
plain model of tests/wire_views_model.py over the CPU oracle's walk and signature check (tests/wire_views_cases.py: expected)
for out_view, out_stored, n_views and every record field; (3) the device's own ibft_set_validators(set) + ibft_tally /
ibft_tally_prepare over S_v on a second context for every record's tally, field for field.  Everything compared is a bit, an
integer or a byte string: equality is exact.  The corpora and what they hold: tests/wire_views_cases.py,
tests/test_wire_views_inputs.py."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import wire_sets_cases as WS
import wire_views_cases as VC
import wire_views_child as K
import wire_views_harness as H
import wire_views_model as VM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _V():
    import go_ibft_amd.verifier as V
    return V


def _tally_fields(t):
    return (t.quorum_lo, t.quorum_hi, t.power_lo, t.power_hi, t.valid_rows, t.distinct_senders, t.has_quorum, t.shard_overlap,
            t.proposer_rows, t.reserved)


def _check(bv, ref, c, hmap, recode, cap, with_proposers=True):
    """one batch on bv against the three oracles, then a second call (the scratch is zero again); ref: a second context"""
    n = len(c.msgs)
    wire, off = WS.pack(c.msgs)
    sets_out = bv.verify_senders_wire_sets(wire, off)
    out = bv.verify_senders_wire_views(wire, off, cap)
    got, rows, rset, vidx, tl, view, stored, views, n_views = out
    # (1) the five shared outputs
    assert got.tolist() == sets_out[0].tolist() and rows.tobytes() == sets_out[1].tobytes()
    assert rset.tobytes() == sets_out[2].tobytes() and vidx.tobytes() == sets_out[3].tobytes()
    assert [bytes(t) for t in tl] == [bytes(t) for t in sets_out[4]]
    # (2) the model
    e = VC.expected(c, hmap, recode, cap, with_proposers)
    K.check_model(out, e, cap, n)
    # (3) every record's tally: the single-set calls over S_v
    sets = c.sets()
    senders = np.array([np.frombuffer(p.sender.ljust(20, b"\0")[:20], np.uint8) for p in e["parsed"]], np.uint8).reshape(n, 20)
    installed = None
    for v, r in enumerate(views):
        s = int(r["set"])
        if s != installed:
            h, a, p = sets[s]
            (ref.set_validators_u256 if c.big else ref.set_validators)(h, a, p)
            installed = s
        sv = senders[(view == v) & stored]
        assert len(sv) == int(r["stored_rows"])
        prop = e["records"][v]["proposer"]
        assert (prop is not None) == bool(r["prepare_rule"])
        t = ref.has_quorum(sv, np.ones(len(sv), bool)) if prop is None else ref.has_prepare_quorum(sv, np.ones(len(sv), bool), prop)
        rt = r["tally"]
        assert _tally_fields(t) == tuple(int(rt[f]) for f in rt.dtype.names), v
    # afterwards: what the sets call leaves — no resident batch, the walks' statistics of this call
    assert bv.seals_rows()[0] == 0 and bv._L.ibft_wire_stage_seals(bv._h) == VM.E_INVAL
    assert bv.wire_stats()[0] == n
    # a second call returns the same bytes: all scratch was left zero
    assert K.output_bytes(bv.verify_senders_wire_views(wire, off, cap)) == K.output_bytes(out)
    return out


@pytest.mark.parametrize("big", [False, True], ids=["u64", "u256"])
@pytest.mark.parametrize("cache", [False, True], ids=["cold", "warm"])
def test_corpus_a_defining_property(oracle, big, cache):
    V = _V()
    c = VC.corpus_a(big)
    n = len(c.msgs)
    flags = V.FLAG_PUBKEY_CACHE if cache else 0
    bv, ref = V.BatchVerifier(flags=flags, max_rows=4096), V.BatchVerifier(flags=flags, max_rows=4096)
    try:
        K.install(bv, c)
        out = _check(bv, ref, c, WS.MAP_A, False, n)       # (with the cache flag its second and later calls run warm)
        n_views = out[8]
        if cache:
            assert bv.cache_stats()[1] > 0
        recs = [H.record_dict(r) for r in out[7]]
        assert any(r["prepare_rule"] and r["tally"]["proposer_rows"] for r in recs) and any(r["tally"]["has_quorum"] for r in recs)
        for cap in (1, n_views - 1, n + 5):
            _check(bv, ref, c, WS.MAP_A, False, cap)
        # no proposer table: every record under the plain rule
        K.install(bv, c, with_proposers=False)
        out = _check(bv, ref, c, WS.MAP_A, False, n, with_proposers=False)
        assert not out[7]["prepare_rule"].any()
    finally:
        bv.close()
        ref.close()


@pytest.mark.parametrize("hmap", [WS.MAP_A, WS.MAP_B], ids=["map_a", "map_b"])
def test_corpus_a_with_the_recode_flag(oracle, hmap):
    V = _V()
    c = VC.corpus_a()
    bv, ref = V.BatchVerifier(flags=V.FLAG_WIRE_RECODE, max_rows=1024), V.BatchVerifier(flags=V.FLAG_WIRE_RECODE, max_rows=1024)
    try:
        K.install(bv, c, hmap)
        out = _check(bv, ref, c, hmap, True, len(c.msgs))
        j = c.kinds.index("padded_height")
        assert out[0][j] and out[5][j] >= 0 and bv.wire_stats()[1] == 1        # the recoded row is valid and has a view
        if hmap is WS.MAP_B:
            assert all(out[0][i] for i, k in enumerate(c.kinds) if k == "empty_view_valid")
            assert any(int(r["height"]) == 0 and int(r["set"]) == 2 for r in out[7])
    finally:
        bv.close()
        ref.close()


def test_corpus_b_across_workgroups(oracle):
    V = _V()
    c = VC.corpus_b()
    bv, ref = V.BatchVerifier(max_rows=4096), V.BatchVerifier(max_rows=4096)
    try:
        K.install(bv, c)
        _check(bv, ref, c, WS.MAP_A, False, len(c.msgs))
    finally:
        bv.close()
        ref.close()


@pytest.mark.parametrize("cap", [VC.C_VIEWS, 100])
def test_corpus_c_a_view_per_row(oracle, cap):
    V = _V()
    c = VC.corpus_c()
    bv, ref = V.BatchVerifier(max_rows=4096), V.BatchVerifier(max_rows=4096)
    try:
        K.install(bv, c)
        wire, off = WS.pack(c.msgs)
        out = bv.verify_senders_wire_views(wire, off, cap)
        e = VC.expected(c, WS.MAP_A, False, cap)
        K.check_model(out, e, cap, len(c.msgs))
        assert out[8] == VC.C_VIEWS and len(out[7]) == cap
        if cap == 100:                                         # the −2 rows still clear earlier stored bits
            over = out[5] == VM.VIEW_OVER
            assert over.sum() == len(c.msgs) - 100 and (~out[6][over]).sum() == VC.C_REPEATS
        assert K.output_bytes(bv.verify_senders_wire_views(wire, off, cap)) == K.output_bytes(out)
        # the tallies of a sample of records against the single-set calls (all 1 500 would be 1 500 launches)
        h, a, p = c.sets()[0]
        ref.set_validators(h, a, p)
        for v in (0, 1, 2, 63, 64, cap - 1):
            r = out[7][v]
            sv = np.frombuffer(e["parsed"][int(r["first_row"])].sender, np.uint8).reshape(1, 20)
            prop = e["records"][v]["proposer"]
            t = ref.has_quorum(sv, [True]) if prop is None else ref.has_prepare_quorum(sv, [True], prop)
            assert _tally_fields(t) == tuple(int(r["tally"][f]) for f in r["tally"].dtype.names), v
    finally:
        bv.close()
        ref.close()


@pytest.mark.parametrize("name,cap", [("a", 10**6), ("c", VC.C_VIEWS), ("c", 100)])
def test_table_size_hook_at_its_floor(oracle, name, cap):
    """IBFT_WIRE_VIEWS_SLOTS=1: the smallest table the library allows (the first power of two above n) — long probe runs and
    wrap-around — in a fresh child process; its outputs are the default run's, byte for byte"""
    V = _V()
    c = K.CORPORA[name]()
    bv = V.BatchVerifier(max_rows=4096)
    try:
        K.install(bv, c)
        want = hashlib.sha256(K.output_bytes(bv.verify_senders_wire_views(*WS.pack(c.msgs), cap))).hexdigest()
    finally:
        bv.close()
    env = dict(os.environ, IBFT_WIRE_VIEWS_SLOTS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wire_views_child.py"), ROOT, name, str(cap)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and f"WIRE_VIEWS_{name.upper()}_OK {want}" in p.stdout, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"


def test_edge_batches(oracle):
    V = _V()
    c = VC.corpus_a()
    bv = V.BatchVerifier(max_rows=1024)
    try:
        K.install(bv, c)
        # n = 0
        got, rows, rset, vidx, tl, view, stored, views, n_views = bv.verify_senders_wire_views(b"", np.zeros(1, np.uint32), 8)
        assert len(got) == 0 and len(view) == 0 and len(views) == 0 and n_views == 0
        assert [bytes(t) for t in tl] == [bytes(t) for t in bv.verify_senders_wire_sets(b"", np.zeros(1, np.uint32))[4]]
        # no valid row: only the invalid kinds
        bad = [m for m, k in zip(c.msgs, c.kinds) if k in WS.KINDS and k != "good"]
        assert len(bad) == len(WS.KINDS) - 1
        got, _, _, _, _, view, stored, views, n_views = bv.verify_senders_wire_views(*WS.pack(bad), 4)
        assert not got.any() and (view == VM.VIEW_NONE).all() and not stored.any() and n_views == 0 and len(views) == 0
        # views_cap = 0 with rows is refused and writes nothing
        wire, off = WS.pack(bad)
        mask, nv = np.full(1, 7, np.uint64), np.full(1, 9, np.uint32)
        assert bv._L.ibft_verify_senders_wire_views(bv._h, V._p(np.frombuffer(wire, np.uint8)), V._p(off), len(bad), 0, V._p(mask), None, None,
                                                    None, None, None, None, None, nv.ctypes.data_as(V.C.POINTER(V.C.c_uint32))) == VM.E_INVAL
        assert mask[0] == 7 and nv[0] == 9
        # only the mask is required
        assert bv._L.ibft_verify_senders_wire_views(bv._h, V._p(np.frombuffer(wire, np.uint8)), V._p(off), len(bad), 3, V._p(mask), None, None,
                                                    None, None, None, None, None, None) == VM.E_OK
        assert mask[0] == 0
    finally:
        bv.close()
