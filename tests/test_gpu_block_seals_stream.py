"""GPU: streamed chain sync — ibft_block_seals_submit / _collect / _pending keep block batches in flight.  Every collect
must be, bit for bit, what ibft_verify_block_seals returns for the same batch: expected values come from the CPU oracle (as
tests/test_gpu_block_seals.py builds them) and from the synchronous call on a second context, never from the streamed path."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import block_stream_cases as S

pytestmark = pytest.mark.gpu

E_INVAL, E_NOVALSET, E_TOOBIG = -1, -5, -7


def _V():
    import go_ibft_amd.verifier as V
    return V


def _raw_submit(bv, bh, off, sig, signer, pre=None, nb=None):
    V = _V()
    o = np.ascontiguousarray(off, np.uint32)
    return V.load_library().ibft_block_seals_submit(bv._h, V._p(bh), V._p(o), len(o) - 1 if nb is None else nb, V._p(sig),
                                                    V._p(signer), V._p(pre))


@pytest.fixture(scope="module")
def seq():
    return S.stream()


@pytest.fixture(scope="module")
def sync(seq):
    return S.sync_results(seq)


def test_stream_of_differing_shapes_one_in_flight(seq, sync):
    assert len(seq) >= 8 and seq[4].n == 65536 and seq[5].n == 4 and seq[2].n == 0 and len(seq[2].bh) == 3
    bv = _V().BatchVerifier(max_rows=65536)
    try:
        got = S.run_stream(bv, seq, 1)
    finally:
        bv.close()
    for b, g, s in zip(seq, got, sync):
        S.compare(b, g, s)
    # the fixtures have what they claim: quorums on both sides, invalid rows
    for k in (0, 3, 6):
        hq = [t.has_quorum for t in got[k][1]]
        assert 0 < sum(hq) < len(hq) and not got[k][0].all(), seq[k].name
    assert got[5][0].tolist() == [True, False, True, True]   # 4 rows behind 65 536: nothing stale, tail bits clear


def test_stream_with_the_key_cache_goes_warm(seq, sync):
    V = _V()
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=65536)
    seen = {}

    def on_collect(k):
        seen[k] = (bv.cache_stats(), bv.last_dispatch())

    try:
        # three 100-validator batches first: 0 and 1 are submitted cold, the collect of 0 builds the tables (draining 1)
        lead = [seq[0], seq[6], seq[1], seq[0]]
        got = S.run_stream(bv, lead, 1, on_collect)
        for b, g in zip(lead, got):
            S.compare(b, g)
        (tab0, warm0, cold0), _ = seen[0]
        assert tab0 > 0 and warm0 == 0 and cold0 == 2            # both first batches went out cold; tables exist after collect 0
        (tab3, warm3, cold3), (cold_lanes, warm_lanes) = seen[3]
        assert warm3 >= 2 and warm_lanes > 0                     # batches 2 and 3 took the warm kernel
        assert (got[0][0] == got[3][0]).all() and [S.fields(t) for t in got[0][1]] == [S.fields(t) for t in got[3][1]]
        # and the whole stream, validator-set changes included, on the same (now warm) context
        got = S.run_stream(bv, seq, 1)
        for b, g, s in zip(seq, got, sync):
            S.compare(b, g, s)
    finally:
        bv.close()


def test_third_submit_is_refused_and_both_batches_collect(seq, sync):
    V = _V()
    a, b = seq[0], seq[1]
    bv = V.BatchVerifier(max_rows=65536)
    small = V.BatchVerifier(max_rows=64)
    try:
        L = V.load_library()
        mask = np.full(4, 0xA5A5A5A5A5A5A5A5, np.uint64)
        assert L.ibft_block_seals_collect(bv._h, V._p(mask), None) == E_INVAL and (mask == 0xA5A5A5A5A5A5A5A5).all()
        assert b"without a submitted batch" in L.ibft_last_error(bv._h)
        # refused submits take no slot: no validator set, offsets not from 0 / going down, too many rows / blocks
        assert _raw_submit(bv, *a.cols()) == E_NOVALSET
        bv.set_validators(a.r.height, a.r.addrs, a.r.power)
        small.set_validators(a.r.height, a.r.addrs, a.r.power)
        bad = a.off.copy(); bad[0] = 1
        assert _raw_submit(bv, a.bh, bad, a.sig, a.signer) == E_INVAL
        bad = a.off.copy(); bad[2] = bad[1] - 1
        assert _raw_submit(bv, a.bh, bad, a.sig, a.signer) == E_INVAL
        assert _raw_submit(bv, a.bh, a.off, None, a.signer) == E_INVAL
        assert _raw_submit(small, *a.cols()) == E_TOOBIG
        assert _raw_submit(small, a.bh, np.zeros(66, np.uint32), a.sig, a.signer) == E_TOOBIG
        assert bv.block_seals_pending() == (0, 0, 0) and small.block_seals_pending() == (0, 0, 0)
        bv.block_seals_submit(*a.cols())
        bv.block_seals_submit(*b.cols())
        assert _raw_submit(bv, *a.cols()) == E_INVAL
        assert b"two block batches already in flight" in L.ibft_last_error(bv._h)
        bad = a.off.copy(); bad[0] = 1
        assert _raw_submit(bv, a.bh, bad, a.sig, a.signer) == E_INVAL    # (a refused call while two are in flight)
        assert bv.block_seals_pending() == (2, a.n, len(a.bh))
        # a batch with rows cannot be collected without a verdict buffer — and stays collectable
        assert L.ibft_block_seals_collect(bv._h, None, None) == E_INVAL and bv.block_seals_pending()[0] == 2
        S.compare(a, bv.block_seals_collect(), sync[0])
        S.compare(b, bv.block_seals_collect(), sync[1])
        with pytest.raises(RuntimeError):
            bv.block_seals_collect()
        # a batch without rows may be collected with no buffers at all
        bv.block_seals_submit(*seq[2].cols())
        assert L.ibft_block_seals_collect(bv._h, None, None) == 0 and bv.block_seals_pending() == (0, 0, 0)
    finally:
        bv.close()
        small.close()


def test_pinned_and_pageable_sources_agree(seq, sync):
    idx = [0, 6, 1, 2, 3]
    bv = _V().BatchVerifier(max_rows=65536)
    try:
        page = S.run_stream(bv, [seq[i] for i in idx], 1)
        pin = S.run_stream(bv, [S.pinned(seq[i]) for i in idx], 1)
        mixed = S.run_stream(bv, [S.pinned(seq[i]) if k % 2 else seq[i] for k, i in enumerate(idx)], 1)
    finally:
        bv.close()
    for k, i in enumerate(idx):
        for got in (page, pin, mixed):
            S.compare(seq[i], got[k], sync[i])


@pytest.mark.parametrize("entry", ["seals", "block", "senders"])
def test_another_entry_point_between_submit_and_collect(seq, sync, entry):
    from oracle import binding as B, workload as W
    import test_gpu_block_seals as BS
    a, b = seq[0], seq[6]
    rx = W.make_round(100, S.SEED, byzantine=True, with_envelopes=True)
    assert rx.addrs.tobytes() == a.r.addrs.tobytes()
    vs = B.ValSet(a.r.addrs, a.r.power)
    bv = _V().BatchVerifier(max_rows=65536)
    try:
        bv.set_validators(a.r.height, a.r.addrs, a.r.power)
        bv.block_seals_submit(*a.cols())
        bv.block_seals_submit(*b.cols())
        if entry == "seals":
            m, t = bv.is_valid_committed_seal(rx.hash32, rx.seal65, rx.signer20, rx.pre_flags)
            e = B.verify_seals(vs, rx.hash32, rx.seal65, rx.signer20, rx.pre_flags).astype(bool)
            assert (m == e).all() and S.fields(t) == S.fields(B.tally(vs, rx.signer20, e))
        elif entry == "block":
            c = seq[1]
            S.compare(c, bv.verify_block_seals(*c.cols()), sync[1])
        else:
            m, t = bv.is_valid_validator(rx.payload, rx.off, rx.msg_sig65, rx.signer20)
            e = B.verify_senders(vs, rx.payload, rx.off, rx.msg_sig65, rx.signer20).astype(bool)
            assert (m == e).all() and S.fields(t) == S.fields(B.tally(vs, rx.signer20, e))
        assert bv.block_seals_pending() == (2, a.n, len(a.bh))
        S.compare(a, bv.block_seals_collect(), sync[0])
        S.compare(b, bv.block_seals_collect(), sync[6])
        # afterwards the context behaves like a fresh one (the checks of test_following_calls_see_a_clean_context)
        r2 = W.make_round(100, 82, byzantine=True)
        bv.set_validators(r2.height, r2.addrs, r2.power)
        vs2 = B.ValSet(r2.addrs, r2.power)
        for n in (100, 37, 1000):
            idx = np.arange(n) % r2.n
            m, t = bv.is_valid_committed_seal(r2.hash32[idx], r2.seal65[idx], r2.signer20[idx], r2.pre_flags[idx])
            e = B.verify_seals(vs2, r2.hash32[idx], r2.seal65[idx], r2.signer20[idx], r2.pre_flags[idx]).astype(bool)
            te = B.tally(vs2, r2.signer20[idx], e)
            assert (m == e).all() and S.fields(t) == S.fields(te)
            assert S.fields(bv.has_quorum(r2.signer20[idx], e)) == S.fields(te)
        # and the staged batch is the last submitted batch's rows, as after ibft_verify_block_seals
        bv.set_validators(a.r.height, a.r.addrs, a.r.power)
        bv.block_seals_submit(*a.cols())
        got, _ = bv.block_seals_collect()
        m, t = bv.seals_run()
        assert len(m) == len(got) and (m == got).all()
        S.compare(b, S.run_stream(bv, [b], 1)[0], sync[6])
    finally:
        bv.close()


def test_the_two_pipelines_are_not_mixed(seq, sync):
    from oracle import binding as B, workload as W
    V = _V()
    L = V.load_library()
    a = seq[0]
    rx = W.make_round(100, S.SEED, byzantine=True)
    vs = B.ValSet(a.r.addrs, a.r.power)
    ex = B.verify_seals(vs, rx.hash32, rx.seal65, rx.signer20, rx.pre_flags).astype(bool)
    bv = V.BatchVerifier(max_rows=65536)
    try:
        bv.set_validators(a.r.height, a.r.addrs, a.r.power)
        bv.seals_stage(rx.hash32, rx.seal65, rx.signer20, rx.pre_flags)
        bv.block_seals_submit(*a.cols())
        assert L.ibft_seals_submit(bv._h) == E_INVAL and b"block batches in flight" in L.ibft_last_error(bv._h)
        S.compare(a, bv.block_seals_collect(), sync[0])
        bv.seals_stage(rx.hash32, rx.seal65, rx.signer20, rx.pre_flags)
        bv.seals_submit()                                            # works again
        assert _raw_submit(bv, *a.cols()) == E_INVAL and b"seal passes in flight" in L.ibft_last_error(bv._h)
        assert bv.block_seals_pending() == (0, 0, 0)
        m, t = bv.seals_collect()
        assert (m == ex).all() and S.fields(t) == S.fields(B.tally(vs, rx.signer20, ex))
        S.compare(a, S.run_stream(bv, [a], 1)[0], sync[0])           # works again
    finally:
        bv.close()


def test_u256_powers_quorum_exact_at_the_boundary():
    """powers w, w + 1, w (w ≈ 2^200): quorum = 2w + 1 exactly — {A, B} is a quorum, {A, C} one short of it"""
    from oracle import binding as B
    from oracle.semantics import ValidatorManager
    import test_gpu_block_seals as BS
    r = S.round_of(3, 51)
    w = 2**200 + 7
    powers = [w, w + 1, w]
    vm = ValidatorManager()
    assert vm.init({bytes(a): p for a, p in zip(r.addrs, powers)}) and vm.quorum == 2 * w + 1
    subsets = [(0, 1), (0, 2), (1, 2), (0, 1, 2), (0,), (), (0, 0, 2)]
    bh = BS._block_hashes(len(subsets), 51)
    rows, off = [], [0]
    for b, s in enumerate(subsets):
        rows += [(i, b) for i in s]
        off.append(len(rows))
    sig = np.array([np.frombuffer(B.sign(r.sks[i], bytes(bh[b])), np.uint8) for i, b in rows], np.uint8).reshape(-1, 65)
    signer = np.array([r.addrs[i] for i, _ in rows], np.uint8).reshape(-1, 20)
    bv = _V().BatchVerifier(max_rows=1024)
    ref = _V().BatchVerifier(max_rows=1024)
    try:
        bv.set_validators_u256(r.height, r.addrs, powers)
        ref.set_validators_u256(r.height, r.addrs, powers)
        bv.block_seals_submit(bh, off, sig, signer)
        bv.block_seals_submit(bh[:0], [0], sig[:0], signer[:0])
        got, tl = bv.block_seals_collect()
        g2, t2 = bv.block_seals_collect()
        assert len(g2) == 0 and t2 == []
        gs, ts = ref.verify_block_seals(bh, off, sig, signer)
        assert got.all() and (got == gs).all() and [S.fields(t) for t in tl] == [S.fields(t) for t in ts]
        for b, s in enumerate(subsets):
            exact = sum(powers[i] for i in set(s))
            assert bool(tl[b].has_quorum) == vm.has_quorum([bytes(r.addrs[i]) for i in s]), (s, tl[b].has_quorum)
            assert tl[b].power == exact & (2**128 - 1) and tl[b].quorum == vm.quorum & (2**128 - 1)
        assert [bool(t.has_quorum) for t in tl] == [True, False, True, True, False, False, False]
    finally:
        bv.close()
        ref.close()


def test_keccak_suffix_seal_digest_and_a_change_between_submits():
    """batch 0 is submitted under keccak256(hash ‖ 0x02), batch 1 — the same rows — under the identity convention: each is
    judged under the convention current at its submit"""
    from oracle import binding as B
    import test_gpu_block_seals as BS
    r = S.round_of(100, 71)
    vs = B.ValSet(r.addrs, r.power)
    nb = 12
    bh = BS._block_hashes(nb, 71)
    off = (np.arange(nb + 1) * 70).astype(np.uint32)
    digest = lambda h: B.keccak256(h + b"\x02")
    who = np.arange(70 * nb) % 100
    rh = BS._rows_hash(bh, off)
    sig = np.array([np.frombuffer(B.sign(r.sks[i], digest(bytes(h)) if k % 7 else bytes(h)), np.uint8)
                    for k, (i, h) in enumerate(zip(who, rh))], np.uint8).reshape(-1, 65)   # every 7th signs the bare hash
    signer = r.addrs[who].copy()
    bv = _V().BatchVerifier(max_rows=4096)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        bv.set_seal_digest(b"\x02")
        bv.block_seals_submit(bh, off, sig, signer)
        bv.set_seal_digest(None)
        bv.block_seals_submit(bh, off, sig, signer)
        for dg in (digest, None):
            got, tl = bv.block_seals_collect()
            exp, te = BS._expect(vs, bh, off, sig, signer, None, dg)
            assert (got == exp).all() and [S.fields(t) for t in tl] == [S.fields(t) for t in te]
            assert 0 < (~got).sum() < len(got)
    finally:
        bv.close()


def test_each_batch_is_judged_under_the_validator_set_of_its_submit():
    """the same rows submitted under three sets: all 100 validators, the first 50 (the others' seals stop counting, the
    quorum moves), all 100 weighted — with the set changed while the batch before is still in flight"""
    from oracle import binding as B
    import test_gpu_block_seals as BS
    r = S.round_of(100, 73)
    rw = S.round_of(100, 73, weighted=True)
    assert r.addrs.tobytes() == rw.addrs.tobytes() and (r.power != rw.power).any()
    nb = 24
    bh = BS._block_hashes(nb, 73)
    rng = np.random.default_rng(73)
    counts = rng.integers(30, 101, nb)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    who = np.concatenate([rng.permutation(100)[:c] for c in counts])
    rh = BS._rows_hash(bh, off)
    sig = np.array([np.frombuffer(B.sign(r.sks[i], bytes(h)), np.uint8) for i, h in zip(who, rh)], np.uint8).reshape(-1, 65)
    signer = r.addrs[who].copy()
    sets = [(r.addrs, r.power), (r.addrs[:50], r.power[:50]), (rw.addrs, rw.power)]
    for flags in (0, _V().FLAG_PUBKEY_CACHE):
        bv = _V().BatchVerifier(flags=flags, max_rows=4096)
        try:
            got = []
            for k, (ad, pw) in enumerate(sets):
                bv.set_validators(r.height + k, ad, pw)
                bv.block_seals_submit(bh, off, sig, signer)
                if k:
                    got.append(bv.block_seals_collect())
            got.append(bv.block_seals_collect())
            quorums = set()
            for (ad, pw), (m, tl) in zip(sets, got):
                exp, te = BS._expect(B.ValSet(ad, pw), bh, off, sig, signer)
                assert (m == exp).all() and [S.fields(t) for t in tl] == [S.fields(t) for t in te]
                quorums.add(tl[0].quorum)
            assert len(quorums) == 3 and got[0][0].all()
        finally:
            bv.close()


def test_seal_replayed_into_the_next_batch_is_invalid():
    from oracle import binding as B
    import test_gpu_block_seals as BS
    r = S.round_of(4, 21)
    bh = BS._block_hashes(4, 21)
    seals = [[B.sign(r.sks[i], bytes(bh[b])) for i in range(4)] for b in range(4)]
    col = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 65)
    # batch 0: blocks 0, 1 honest.  batch 1: block 2 holds validator 0's seal of block 1 (the LAST block of the batch before)
    # in place of its own, block 3 is honest
    sig0, signer0 = col(seals[0] + seals[1]), np.concatenate([r.addrs, r.addrs])
    sig1, signer1 = col([seals[1][0]] + seals[2][1:] + seals[3]), np.concatenate([r.addrs, r.addrs])
    bv = _V().BatchVerifier(max_rows=1024)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        bv.block_seals_submit(bh[:2], [0, 4, 8], sig0, signer0)
        bv.block_seals_submit(bh[2:], [0, 4, 8], sig1, signer1)
        g0, t0 = bv.block_seals_collect()
        g1, t1 = bv.block_seals_collect()
        assert g0.all() and [t.has_quorum for t in t0] == [1, 1]
        assert g1.tolist() == [False] + [True] * 7
        assert (t1[0].valid_rows, t1[0].has_quorum, t1[1].valid_rows, t1[1].has_quorum) == (3, 1, 4, 1)
        vs = B.ValSet(r.addrs, r.power)
        exp, te = BS._expect(vs, bh[2:], np.array([0, 4, 8], np.uint32), sig1, signer1)
        assert (g1 == exp).all() and [S.fields(t) for t in t1] == [S.fields(t) for t in te]
    finally:
        bv.close()


def test_no_host_direct_child_process():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, IBFT_NO_HOST_DIRECT="1")
    code = ("import sys; sys.path[:0] = [%r, %r]; import block_stream_cases as S; sys.exit(S.main())"
            % (root, os.path.join(root, "tests")))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert p.returncode == 0 and "BLOCK_STREAM_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_two_threads_stream_at_once(seq, sync):
    V = _V()
    idx = [0, 6, 1, 2, 8, 0]
    for i in idx:
        S.expected(seq[i])     # (the oracle's answers, computed once, before the threads start)
    errors = []

    def worker(k):
        try:
            bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if k else 0, max_rows=65536)
            try:
                for _ in range(3):
                    batches = [S.pinned(seq[i]) if k else seq[i] for i in idx]
                    got = S.run_stream(bv, batches, 1)
                    for i, g in zip(idx, got):
                        S.compare(seq[i], g, sync[i])
            finally:
                bv.close()
        except Exception as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
