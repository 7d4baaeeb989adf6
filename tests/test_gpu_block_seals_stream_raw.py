"""GPU: the streamed submits that take proposals or bare seals — ibft_block_seals_submit_raw, ibft_recover_block_seals_submit,
ibft_recover_block_seals_submit_raw, collected with ibft_block_seals_collect_ex.  Defining property: every collect is, bit
for bit and in every output, what the synchronous sibling (ibft_verify_block_seals_raw, ibft_recover_block_seals,
ibft_recover_block_seals_raw) returns for the same arguments on a second context; one case per kind is compared with the CPU
oracle directly.  Shapes and generators: tests/block_stream_raw_cases.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import block_stream_raw_cases as S

pytestmark = pytest.mark.gpu

E_INVAL, E_NOVALSET, E_TOOBIG = -1, -5, -7
HERE = os.path.dirname(os.path.abspath(__file__))


def _V():
    import go_ibft_amd.verifier as V
    return V


_SYNC: dict = {}


def sync_results(kind, suffix=None, flags=0, u256=False):
    """the synchronous sibling over the cases on a context of its own — computed once per configuration and shared"""
    key = (kind, suffix, flags, u256)
    if key not in _SYNC:
        bv = _V().BatchVerifier(flags=flags, max_rows=S.MAX_ROWS)
        try:
            bv.set_seal_digest(suffix)
            _SYNC[key] = run(bv, kind, S.cases(suffix), u256, streamed=False)
        finally:
            bv.close()
    return _SYNC[key]


def set_vals(bv, r, u256):
    if u256:   # powers beyond 64 bits: (2^200 + i), the quorum is decided over the full width
        bv.set_validators_u256(r.height, r.addrs, [(1 << 200) + i for i in range(len(r.addrs))])
    else:
        bv.set_validators(r.height, r.addrs, r.power)


def run(bv, kind, seq, u256=False, streamed=True, in_flight=1):
    if not u256:
        return S.run_streamed(bv, kind, seq, in_flight) if streamed else S.run_sync(bv, kind, seq)
    out, cur, pend = [], None, 0
    for c in seq:
        if cur is not c.r:
            set_vals(bv, c.r, True)
            cur = c.r
        if not streamed:
            out.append(S.sibling(bv, kind, c))
            continue
        S.submit(bv, kind, c)
        pend += 1
        if pend > in_flight:
            out.append(bv.block_seals_collect_ex())
            pend -= 1
    while pend:
        out.append(bv.block_seals_collect_ex())
        pend -= 1
    return out


CONFIGS = {
    "cold": dict(),
    "suffix": dict(suffix=S.SUFFIX),
    "strict_low_s": dict(flags=1),
    "u256": dict(u256=True),
    "warm": dict(flags=2),
    "warm_suffix_strict": dict(flags=3, suffix=S.SUFFIX),
}


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_streamed_equals_the_synchronous_sibling(kind, config):
    cfg = CONFIGS[config]
    suffix, flags, u256 = cfg.get("suffix"), cfg.get("flags", 0), cfg.get("u256", False)
    seq = S.cases(suffix)
    want = sync_results(kind, suffix, flags, u256)
    V = _V()
    bv = V.BatchVerifier(flags=flags, max_rows=S.MAX_ROWS)
    try:
        bv.set_seal_digest(suffix)
        got = run(bv, kind, seq, u256)
        if flags & V.FLAG_PUBKEY_CACHE and kind == "verify_raw":
            got += run(bv, kind, seq, u256)      # the keys are known by now: these batches are warm
            want = want + want
            assert bv.cache_stats()[1] > 0, "no warm pass"
        assert bv.block_seals_pending() == (0, 0, 0)
    finally:
        bv.close()
    for c, g, w in zip(seq + seq, got, want):
        S.same(g, w, f"{kind}/{config}/{c.name}")
    # the fixtures have what they claim: invalid rows, quorums on both sides, hashes that are the oracle's
    big = got[7]
    assert not big["verdict"].all() and big["verdict"].any()
    hq = [t.has_quorum for t in big["tallies"]]
    assert 0 < sum(hq) < len(hq)
    if "block_hash32" in big:
        assert (big["block_hash32"] == seq[7].bh).all()


def test_strict_low_s_changes_verdicts():
    """(the high-s rows of the fixtures are what the strict flag is about)"""
    a = sync_results("recover", None, 0)[7]["verdict"]
    b = sync_results("recover", None, 1)[7]["verdict"]
    assert (a != b).any() and not (b & ~a).any()


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("suffix", [None, S.SUFFIX], ids=["identity", "suffix"])
def test_streamed_equals_the_oracle(kind, suffix):
    from oracle import binding as B
    import test_gpu_block_seals as BS
    import test_gpu_recover_seals as RS
    c = S.cases(suffix)[5]
    vs = B.ValSet(c.r.addrs, c.r.power)
    bv = _V().BatchVerifier(max_rows=S.MAX_ROWS)
    try:
        bv.set_seal_digest(suffix)
        bv.set_validators(c.r.height, c.r.addrs, c.r.power)
        S.submit(bv, kind, c)
        got = bv.block_seals_collect_ex()
    finally:
        bv.close()
    digest = lambda h: S.seal_digest(h, suffix)
    if kind == "verify_raw":
        exp, te = BS._expect(vs, c.bh, c.off, c.sig, c.signer, c.pre, digest)
        assert (got["verdict"] == exp).all()
        assert [S.fields(t)[:5] for t in got["tallies"]] == [BS._fields(t) for t in te]
    else:
        for b in range(len(c.bh)):
            lo, hi = int(c.off[b]), int(c.off[b + 1])
            if lo == hi:   # an empty block: power 0 below the quorum
                assert S.fields(got["tallies"][b])[:5] == (0, vs.quorum, 0, 0, 0), f"block {b}"
                continue
            d = np.frombuffer(digest(bytes(c.bh[b])), np.uint8)
            rows = np.repeat(d[None, :], hi - lo, axis=0)
            ea, ev, em, et = RS.expect(B, vs, c.r.addrs, rows, c.sig[lo:hi], None if c.pre is None else c.pre[lo:hi])
            assert (got["signer20"][lo:hi] == ea).all() and (got["vidx"][lo:hi] == ev).all(), f"block {b}"
            assert (got["verdict"][lo:hi] == em).all(), f"block {b}"
            assert S.fields(got["tallies"][b])[:5] == RS.fields(et), f"block {b}"
    if kind != "recover":
        assert (got["block_hash32"] == c.bh).all()   # the hashes BEFORE the convention
    assert not got["verdict"].all() and got["verdict"].any()


def test_two_batches_of_different_kinds_in_flight():
    seq = S.cases(None)
    plan = [("verify", seq[5]), ("recover_raw", seq[6]), ("verify_raw", seq[1]), ("recover", seq[5]), ("verify", seq[4]),
            ("recover_raw", seq[4])]
    V = _V()
    bv, ref = V.BatchVerifier(max_rows=S.MAX_ROWS), V.BatchVerifier(max_rows=S.MAX_ROWS)
    try:
        for x in (bv, ref):
            x.set_validators(seq[5].r.height, seq[5].r.addrs, seq[5].r.power)
        want = [S.sibling(ref, k, c) for k, c in plan]
        got, inflight = [], []
        for k, c in plan:
            S.submit(bv, k, c)
            inflight.append((k, c))
            if len(inflight) == 2:
                # a third submit of any kind is refused and takes no slot
                for k3 in S.KINDS + ("verify",):
                    with pytest.raises(RuntimeError, match="two block batches already in flight"):
                        S.submit(bv, k3, seq[0])
                o = inflight[0]
                assert bv.block_seals_pending_ex() == (2, o[1].n, len(o[1].bh), S.kind_bits(o[0]))
                assert bv.block_seals_pending() == (2, o[1].n, len(o[1].bh))
                got.append(bv.block_seals_collect_ex())
                inflight.pop(0)
                o = inflight[0]
                assert bv.block_seals_pending_ex() == (1, o[1].n, len(o[1].bh), S.kind_bits(o[0]))
        got.append(bv.block_seals_collect_ex())
        assert bv.block_seals_pending_ex() == (0, 0, 0, 0)
    finally:
        bv.close()
        ref.close()
    for (k, c), g, w in zip(plan, got, want):
        S.same(g, w, f"{k}/{c.name}")


def _nine_rows(suffix):
    """4 validators, blocks of 4, 0 and 5 rows: one seal with r = 0, one by a signer outside the set, one signer twice"""
    from oracle import binding as B, workload as W
    r = S.round_of(4)
    outsider = W.make_round(1, S.SEED + 99, raw_len=64)
    raws, rounds = [b"nine rows, block %d" % b for b in range(3)], [0, 3, 2**40 + 3]
    bh = np.frombuffer(b"".join(B.proposal_hash(x, q) for x, q in zip(raws, rounds)), np.uint8).reshape(3, 32).copy()
    off = np.array([0, 4, 4, 9], np.uint32)
    sig, signer = np.zeros((9, 65), np.uint8), np.zeros((9, 20), np.uint8)
    for row, (b, i) in enumerate([(0, 0), (0, 1), (0, 2), (0, 3), (2, 0), (2, 1), (2, None), (2, 3), (2, 0)]):
        sk, a = (outsider.sks[0], outsider.addrs[0]) if i is None else (r.sks[i], r.addrs[i])
        s = bytearray(B.sign(sk, S.seal_digest(bytes(bh[b]), suffix)))
        if row == 2:
            s[:32] = bytes(32)
        sig[row] = np.frombuffer(bytes(s), np.uint8)
        signer[row] = np.frombuffer(bytes(a), np.uint8)
    return S.Case("v4_nine_rows", r, raws, rounds, bh, off, sig, signer, None)


@pytest.mark.parametrize("suffix", [None, S.SUFFIX], ids=["identity", "suffix"])
def test_a_hashes_given_batch_in_flight_with_a_raw_or_a_recover_batch(suffix):
    """ibft_block_seals_submit shares slots, streams and kernels with the three newer submits: a batch of it in flight together
    with a raw / a recover batch, the first collected with ibft_block_seals_collect and the second with _collect_ex, is what
    the synchronous siblings return"""
    c = _nine_rows(suffix)
    V = _V()
    bv, ref = V.BatchVerifier(max_rows=S.MAX_ROWS), V.BatchVerifier(max_rows=S.MAX_ROWS)
    try:
        for x in (bv, ref):
            x.set_seal_digest(suffix)
            x.set_validators(c.r.height, c.r.addrs, c.r.power)
        want = {k: S.sibling(ref, k, c) for k in ("verify", "recover_raw", "verify_raw", "recover")}
        for second in ("recover_raw", "verify_raw", "recover"):
            assert S.submit(bv, "verify", c) == 9 and S.submit(bv, second, c) == 9
            assert bv.block_seals_pending_ex() == (2, 9, 3, 0)
            m, tl = bv.block_seals_collect()
            assert bv.block_seals_pending_ex() == (1, 9, 3, S.kind_bits(second))
            S.same({"kind": 0, "verdict": m, "tallies": tl}, want["verify"], f"verify in front of {second}")
            S.same(bv.block_seals_collect_ex(), want[second], f"{second} behind verify")
        assert bv.block_seals_pending_ex() == (0, 0, 0, 0)
    finally:
        bv.close()
        ref.close()
    v = want["verify"]["verdict"]
    assert v.tolist() == [True, True, False, True, True, True, False, True, True]
    assert [t.valid_rows for t in want["verify"]["tallies"]] == [3, 0, 4]
    assert [t.distinct_senders for t in want["verify"]["tallies"]] == [3, 0, 3]
    assert (want["recover"]["vidx"] == [0, 1, -1, 3, 0, 1, -1, 3, 0]).all()


@pytest.mark.parametrize("kind", S.KINDS)
def test_pinned_and_pageable_sources_give_the_same(kind):
    seq = [S.cases(None)[i] for i in (5, 7, 4)]
    want = [sync_results(kind)[i] for i in (5, 7, 4)]
    bv = _V().BatchVerifier(max_rows=S.MAX_ROWS)
    try:
        cur = None
        pend = []
        got = []
        for c in seq:
            if cur is not c.r:
                bv.set_validators(c.r.height, c.r.addrs, c.r.power)
                cur = c.r
            raws, pc = S.pinned(c)
            S.submit(bv, kind, pc, raws)
            pend.append(pc)
            if len(pend) > 1:
                got.append(bv.block_seals_collect_ex())
                pend.pop(0)
        got.append(bv.block_seals_collect_ex())
    finally:
        bv.close()
    for c, g, w in zip(seq, got, want):
        S.same(g, w, f"{kind}/{c.name}/pinned")


def test_refusals_take_no_slot():
    V = _V()
    L = V.load_library()
    p = V._p
    c = S.cases(None)[5]
    raw, roff, rnd = V.proposal_columns(c.raws, c.rounds)
    nb = len(c.bh)

    def calls(bv, off=c.off, n_blocks=nb, sig=c.sig, signer=c.signer, raw_=raw, roff_=roff, rnd_=rnd, bh=c.bh, raw_only=False):
        """the three submits with the same arguments → their codes; raw_only: the two that take proposals (a bad proposal
        argument is nothing the hashes-given submit sees: it would be accepted and take a slot)"""
        o = np.ascontiguousarray(off, np.uint32)
        r0 = L.ibft_block_seals_submit_raw(bv._h, p(raw_), p(roff_), p(rnd_), p(o), n_blocks, p(sig), p(signer), p(c.pre))
        r1 = None if raw_only else L.ibft_recover_block_seals_submit(bv._h, p(bh), p(o), n_blocks, p(sig), p(c.pre))
        r2 = L.ibft_recover_block_seals_submit_raw(bv._h, p(raw_), p(roff_), p(rnd_), p(o), n_blocks, p(sig), p(c.pre))
        return (r0, r1, r2)

    bv = V.BatchVerifier(max_rows=256)
    try:
        # the sibling's order: the offsets, the sizes, the columns — all before the validator set is asked for
        bad0 = c.off.copy(); bad0[0] = 1
        assert calls(bv, off=bad0) == (E_INVAL,) * 3
        assert calls(bv, off=np.zeros(300, np.uint32), n_blocks=299) == (E_TOOBIG,) * 3          # n_blocks > max_rows
        dec = c.off.copy(); dec[-2] = dec[-1] + 1
        assert calls(bv, off=dec) == (E_INVAL,) * 3
        big = c.off.copy(); big[-1] = 257
        assert calls(bv, off=big) == (E_TOOBIG,) * 3                                             # rows > max_rows
        assert calls(bv, sig=None) == (E_INVAL,) * 3
        assert calls(bv, signer=None)[0] == E_INVAL
        assert calls(bv, bh=None)[1] == E_INVAL
        assert calls(bv) == (E_NOVALSET,) * 3                                                    # … then the validator set
        bv.set_validators(c.r.height, c.r.addrs, c.r.power)
        # … then the proposals, in ibft_proposal_hashes' order
        r = calls(bv, roff_=None, raw_only=True); assert (r[0], r[2]) == (E_INVAL, E_INVAL)
        r = calls(bv, rnd_=None, raw_only=True); assert (r[0], r[2]) == (E_INVAL, E_INVAL)
        b = roff.copy(); b[0] = 1
        r = calls(bv, roff_=b, raw_only=True); assert (r[0], r[2]) == (E_INVAL, E_INVAL)
        b = roff.copy(); assert b[1] > 0; b[2] = b[1] - 1
        r = calls(bv, roff_=b, raw_only=True); assert (r[0], r[2]) == (E_INVAL, E_INVAL)
        r = calls(bv, raw_=None, raw_only=True); assert (r[0], r[2]) == (E_INVAL, E_INVAL)
        assert bv.block_seals_pending_ex() == (0, 0, 0, 0)

        # collecting a recover batch the wrong way: refused, nothing written, the batch stays and is delivered intact
        ref = V.BatchVerifier(max_rows=256)
        try:
            ref.set_validators(c.r.height, c.r.addrs, c.r.power)
            want = S.sibling(ref, "recover_raw", c)
        finally:
            ref.close()
        S.submit(bv, "recover_raw", c)
        mask = np.full((c.n + 63) // 64, 0x5A5A, np.uint64)
        tal = (V.Tally * nb)()
        tal[0].power_lo = 0x1234
        assert L.ibft_block_seals_collect(bv._h, p(mask), tal) == E_INVAL
        assert b"ibft_block_seals_collect_ex" in L.ibft_last_error(bv._h)
        hashes = np.full((nb, 32), 0x77, np.uint8)
        vidx = np.full(c.n, 99, np.int32)
        assert L.ibft_block_seals_collect_ex(bv._h, p(hashes), None, p(vidx), p(mask), tal) == E_INVAL
        assert (mask == 0x5A5A).all() and tal[0].power_lo == 0x1234 and (hashes == 0x77).all() and (vidx == 99).all()
        assert bv.block_seals_pending_ex() == (1, c.n, nb, 3)
        S.same(bv.block_seals_collect_ex(), want, "after two refused collects")
        with pytest.raises(RuntimeError):
            bv.block_seals_collect_ex()     # nothing in flight

        # the old collect takes a verify batch submitted raw (its hashes are dropped)
        S.submit(bv, "verify_raw", c)
        m, tl = bv.block_seals_collect()
        w = sync_results("verify_raw")[5]
        assert (m == w["verdict"]).all() and [S.fields(t) for t in tl] == [S.fields(t) for t in w["tallies"]]
    finally:
        bv.close()


@pytest.mark.parametrize("kind", S.KINDS)
def test_other_calls_between_submit_and_collect(kind):
    import proposal_hash_cases as P
    seq = S.cases(None)
    c, other = seq[5], seq[6]
    want = sync_results(kind)[5]
    bv = _V().BatchVerifier(max_rows=S.MAX_ROWS)
    try:
        bv.set_validators(c.r.height, c.r.addrs, c.r.power)
        S.submit(bv, kind, c)
        raws, rounds = P.short_batch(65)
        assert (bv.proposal_hashes(raws, rounds) == P.expected(raws, rounds)).all()
        rh = np.repeat(other.bh, np.diff(other.off).astype(np.int64), axis=0)
        m1, _ = bv.is_valid_committed_seal(rh, other.sig, other.signer)
        a2, v2, m2, _ = bv.recover_seals(rh, other.sig)
        w = sync_results("recover")[6]
        assert (a2 == w["signer20"]).all() and (v2 == w["vidx"]).all() and (m2 == w["verdict"]).all()
        assert (m1 == sync_results("verify_raw")[6]["verdict"]).all()
        S.same(bv.block_seals_collect_ex(), want, f"{kind}: other calls in between")
    finally:
        bv.close()


@pytest.mark.parametrize("kind", S.KINDS)
def test_a_batch_is_judged_under_the_state_at_its_submit(kind):
    c = S.cases(S.SUFFIX)[5]
    want = sync_results(kind, S.SUFFIX)[5]
    r4 = S.round_of(4)
    bv = _V().BatchVerifier(max_rows=S.MAX_ROWS)
    try:
        bv.set_seal_digest(S.SUFFIX)
        bv.set_validators(c.r.height, c.r.addrs, c.r.power)
        S.submit(bv, kind, c)
        bv.set_seal_digest(None)
        bv.set_validators(r4.height, r4.addrs, r4.power)
        bv.is_valid_proposal_hash(b"another proposal", 3, np.zeros((1, 32), np.uint8), np.full(1, 32, np.uint8))
        S.same(bv.block_seals_collect_ex(), want, f"{kind}: state changed in flight")
    finally:
        bv.close()


def test_a_streamed_recover_batch_teaches_keys():
    """keys of a validator set no other test uses: the device-wide key cache cannot know them yet"""
    from oracle import binding as B, workload as W
    V = _V()
    r = W.make_round(7, 77031, raw_len=64)
    nb = 9
    bh = np.frombuffer(b"".join(B.keccak256(b"teach" + bytes([b])) for b in range(nb)), np.uint8).reshape(nb, 32).copy()
    off = (np.arange(nb + 1) * 7).astype(np.uint32)
    sig = np.array([np.frombuffer(B.sign(r.sks[i % 7], bytes(bh[i // 7])), np.uint8) for i in range(nb * 7)], np.uint8)
    signer = np.array([r.addrs[i % 7] for i in range(nb * 7)], np.uint8)
    sig[5, 64] = 2
    ref = V.BatchVerifier(max_rows=S.MAX_ROWS)
    try:
        ref.set_validators(r.height, r.addrs, r.power)
        a, v, m, tl = ref.recover_block_seals(bh, off, sig)
        want = {"kind": 1, "verdict": m, "tallies": tl, "signer20": a, "vidx": v}
        wm, wt = ref.verify_block_seals(bh, off, sig, signer)
    finally:
        ref.close()
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=S.MAX_ROWS)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        assert bv.cache_stats() == (0, 0, 0)
        assert bv.recover_block_seals_submit(bh, off, sig) == nb * 7
        S.same(bv.block_seals_collect_ex(), want, "recover, cache on")
        assert bv.cache_stats() == (7, 0, 1)     # every validator's table, built at the collect
        m, tl = bv.verify_block_seals(bh, off, sig, signer)
        assert bv.cache_stats() == (7, 1, 1) and bv.last_dispatch()[0] == 0   # … and the verify call that follows is warm
        assert (m == wm).all() and [S.fields(t) for t in tl] == [S.fields(t) for t in wt]
        assert not m[5] and m.sum() == nb * 7 - 1
    finally:
        bv.close()


@pytest.mark.parametrize("lanes", ["1", "64"])
@pytest.mark.parametrize("placement", ["copy", "main"])
def test_digest_placement_and_form_give_the_same_bits(placement, lanes):
    """IBFT_STREAM_DIGEST and IBFT_PROPOSAL_LANES are read at ibft_ctx_create: a fresh child process per setting, compared
    with the synchronous siblings of THIS process (default form)"""
    env = dict(os.environ, IBFT_STREAM_DIGEST=placement, IBFT_PROPOSAL_LANES=lanes,
               PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, os.path.join(HERE, "block_stream_raw_cases.py")], env=env, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and "STREAM_RAW_CHILD_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    got = {tuple(l.split()[1:3]): l.split()[3] for l in out.stdout.splitlines() if l.startswith("FP ")}
    seq = S.cases(None)
    for kind in ("verify_raw", "recover_raw"):
        for c, w in zip(seq, sync_results(kind)):
            assert got[(kind, c.name)] == S.fingerprint(w), f"{placement}/{lanes}/{kind}/{c.name}"
