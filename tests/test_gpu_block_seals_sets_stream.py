"""GPU: chain sync across validator-set changes FROM THE PROPOSALS and STREAMED — ibft_verify_block_seals_sets_raw,
ibft_recover_block_seals_sets_raw and the four _sets submits (ibft_block_seals_submit_sets[_raw],
ibft_recover_block_seals_submit_sets[_raw]) collected with ibft_block_seals_collect_ex.  Defining properties, all of them exact
equality of bits and integers: the _sets_raw calls equal ibft_proposal_hashes + the hashes-given _sets call and the CPU oracle
block by block; every submit delivers what its synchronous sibling returns under the family installed AT THE SUBMIT, whatever
is installed before the collect.  Shapes, generators and the oracle's answer: tests/block_sets_stream_cases.py (whose inputs
tests/test_block_seals_sets_stream_inputs.py checks without a GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import block_sets_stream_cases as SC
import block_stream_raw_cases as S

pytestmark = pytest.mark.gpu

E_INVAL, E_NOVALSET = -1, -5
HERE = os.path.dirname(os.path.abspath(__file__))


def _V():
    import go_ibft_amd.verifier as V
    return V


def _ctx(flags=0, suffix=None, fam=None):
    bv = _V().BatchVerifier(flags=flags, max_rows=SC.MAX_ROWS)
    bv.set_seal_digest(suffix)
    if fam is not None:
        fam.install(bv)
    return bv


_SYNC: dict = {}


def sync_results(kind, case_fn, suffix=None, flags=0, big=False):
    """the synchronous sibling on a cold context of its own — computed once per configuration and shared"""
    key = (kind, case_fn.__name__, suffix, flags, big)
    if key not in _SYNC:
        c = case_fn(suffix, big) if case_fn is SC.main_case else case_fn()
        bv = _ctx(flags & ~2, suffix, c.f)
        try:
            _SYNC[key] = SC.sibling(bv, kind, c)
        finally:
            bv.close()
    return _SYNC[key]


def _against_cpu(res, c, suffix, flags):
    bits, tallies, who, vidx = SC.expect_cpu(c, suffix, flags & 1, bare="signer20" in res)
    bad = np.nonzero(res["verdict"] != bits)[0]
    assert len(bad) == 0, f"verdicts differ from the CPU oracle at rows {bad[:10].tolist()} of {len(bits)}"
    low = (1 << 128) - 1
    assert [S.fields(t)[:5] for t in res["tallies"]] == [(t[0] & low, t[1] & low) + tuple(t[2:]) for t in tallies]
    assert (res["block_hash32"] == c.bh).all()            # the hashes BEFORE the seal-digest convention
    if "signer20" in res:
        assert (res["signer20"] == who).all() and (res["vidx"] == vidx).all()


CONFIGS = {
    "cold": dict(),
    "u256": dict(big=True),
    "suffix": dict(suffix=SC.SUFFIX),
    "strict_low_s": dict(flags=1),
    "warm": dict(flags=2),
    "warm_suffix_strict": dict(flags=3, suffix=SC.SUFFIX),
}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_sets_raw_equals_proposal_hashes_plus_sets_and_the_oracle(config):
    cfg = CONFIGS[config]
    suffix, flags, big = cfg.get("suffix"), cfg.get("flags", 0), cfg.get("big", False)
    V = _V()
    c = SC.main_case(suffix, big)
    ref, bv = _ctx(flags & 1, suffix, c.f), _ctx(flags, suffix, c.f)
    wants = {}
    try:
        for kind in ("verify_raw", "recover_raw"):
            want = wants[kind] = SC.hashes_route(ref, kind, c)
            _against_cpu(want, c, suffix, flags)
            SC.same(SC.sibling(bv, kind, c), want, f"{config}/{kind}/first")
            assert bv.seals_rows()[0] == 0                 # not a resident staged batch
            SC.same(SC.sibling(bv, kind, c), want, f"{config}/{kind}/again")
        if flags & V.FLAG_PUBKEY_CACHE:                    # the verify call taught the keys: its repeat ran warm
            assert bv.cache_stats()[1] > 0, "no warm pass"
        # no seal rows at all: the proposals are hashed only if the caller asks for the hashes
        e = SC.empty_case() if not big and suffix is None else None
        if e is not None:
            m, tl, bh = bv.verify_block_seals_sets_raw(e.raws, e.rounds, e.off, e.bset, e.sig, e.signer)
            assert len(m) == 0 and (bh == e.bh).all() and [S.fields(t)[:5] for t in tl] == SC.expect_cpu(e)[1]
            assert bv.verify_block_seals_sets_raw(e.raws, e.rounds, e.off, e.bset, e.sig, e.signer, want_hashes=False)[2] is None
    finally:
        ref.close(); bv.close()
    if config == "strict_low_s":   # the flag changes verdicts of this batch
        assert wants["verify_raw"]["verdict"].sum() < sync_results("verify_raw", SC.main_case)["verdict"].sum()


def test_sets_raw_over_rows_that_span_verdict_words():
    c = SC.wide_case()
    ref, bv = _ctx(fam=c.f), _ctx(fam=c.f)
    try:
        for kind in ("verify_raw", "recover_raw"):
            want = SC.hashes_route(ref, kind, c)
            _against_cpu(want, c, None, 0)
            SC.same(SC.sibling(bv, kind, c), want, kind)
    finally:
        ref.close(); bv.close()


def test_sets_raw_error_order_and_buffers_untouched():
    """first the errors of the hashes-given _sets call in its order (minus the NULL block_hash32), then those of
    ibft_proposal_hashes' arguments; a refused call writes nothing"""
    V = _V()
    L, p = V.load_library(), V._p
    c = SC.main_case()
    raw, roff, rnd = V.proposal_columns(c.raws, c.rounds)
    nb, n = len(c.bh), c.n
    CAN = 0xA5A5A5A5A5A5A5A5

    def call(bv, recover, off=c.off, bset=c.bset, sig=c.sig, roff_=roff, raw_=raw, rnd_=rnd):
        mask = np.full((n + 63) // 64, CAN, np.uint64)
        who, vidx, bh = np.full((n, 20), 0x5A, np.uint8), np.full(n, 77, np.int32), np.full((nb, 32), 0x3C, np.uint8)
        tal = (V.Tally * nb)()
        for t in tal:
            t.power_lo = 0x1234
        if recover:
            rc = L.ibft_recover_block_seals_sets_raw(bv._h, p(raw_), p(roff_), p(rnd_), p(off), p(bset), nb, p(sig), None, p(bh), p(who),
                                                     p(vidx), p(mask), tal)
        else:
            rc = L.ibft_verify_block_seals_sets_raw(bv._h, p(raw_), p(roff_), p(rnd_), p(off), p(bset), nb, p(sig), p(c.signer), None,
                                                    p(bh), p(mask), tal)
        assert (mask == CAN).all() and (who == 0x5A).all() and (vidx == 77).all() and (bh == 0x3C).all()
        assert all(t.power_lo == 0x1234 for t in tal)
        return rc

    bv = V.BatchVerifier(max_rows=SC.MAX_ROWS)
    try:
        bad_roff = roff.copy(); bad_roff[0] = 1
        for rec in (False, True):
            assert call(bv, rec, roff_=bad_roff) == E_NOVALSET          # no family: before the proposals are looked at
        bv.set_validators(1, c.f.addrs(0), c.f.power[0])
        assert call(bv, False) == E_NOVALSET                            # a single set does not count
        c.f.install(bv)
        for rec in (False, True):
            bad = c.off.copy(); bad[0] = 1
            assert call(bv, rec, off=bad, roff_=bad_roff) == E_INVAL
            assert call(bv, rec, sig=None) == E_INVAL
            assert call(bv, rec, bset=None) == E_INVAL
            oob = c.bset.copy(); oob[5] = 3
            assert call(bv, rec, bset=oob, roff_=bad_roff) == E_INVAL    # an entry = n_sets, decided on the host
            assert call(bv, rec, roff_=None) == E_INVAL and call(bv, rec, rnd_=None) == E_INVAL
            assert call(bv, rec, roff_=bad_roff) == E_INVAL
            dec = roff.copy(); dec[3] = dec[2] - 1
            assert call(bv, rec, roff_=dec) == E_INVAL
            assert call(bv, rec, raw_=None) == E_INVAL
        SC.same(SC.sibling(bv, "verify_raw", c), sync_results("verify_raw", SC.main_case), "after the refusals")
    finally:
        bv.close()


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("in_flight", [1, 2])
def test_streamed_equals_the_synchronous_sibling(kind, in_flight):
    """one and two batches in flight; an empty batch between batches with rows; pinned and pageable sources"""
    c, e = SC.main_case(), SC.empty_case()
    seq = [c, e, SC.pinned(c), SC.pinned(e), c]
    want = [sync_results(kind, SC.main_case), sync_results(kind, SC.empty_case)]
    want = [want[0], want[1], want[0], want[1], want[0]]
    bv = _ctx(fam=c.f)
    try:
        got = SC.run_streamed(bv, kind, seq, in_flight)
        assert bv.seals_rows()[0] == 0 and bv.block_seals_pending() == (0, 0, 0)
    finally:
        bv.close()
    for k, (g, w) in enumerate(zip(got, want)):
        SC.same(g, w, f"{kind}/{in_flight} in flight/batch {k} ({seq[k].name})")
    assert got[0]["kind"] == SC.kind_bits(kind) and got[0]["kind"] & _V().BatchVerifier.BATCH_SETS
    hq = [t.has_quorum for t in got[0]["tallies"]]
    assert 0 < sum(hq) < len(hq) and got[0]["verdict"].any() and not got[0]["verdict"].all()


@pytest.mark.parametrize("kind", ["verify_raw", "recover"])
@pytest.mark.parametrize("config", ["u256", "warm_suffix_strict", "wide"])
def test_streamed_under_other_configurations(kind, config):
    cfg = CONFIGS.get(config, {})
    suffix, flags, big = cfg.get("suffix"), cfg.get("flags", 0), cfg.get("big", False)
    if config == "wide":
        c, want = SC.wide_case(), sync_results(kind, SC.wide_case)
    else:
        c, want = SC.main_case(suffix, big), sync_results(kind, SC.main_case, suffix, flags, big)
    bv = _ctx(flags, suffix, c.f)
    try:
        got = SC.run_streamed(bv, kind, [c, SC.pinned(c), c], 2)
        if flags & 2 and kind == "verify_raw":
            assert bv.cache_stats()[1] > 0, "no warm pass"
    finally:
        bv.close()
    for k, g in enumerate(got):
        SC.same(g, want, f"{kind}/{config}/batch {k}")


@pytest.mark.parametrize("order", ["single first", "sets first"])
def test_a_single_set_batch_and_a_sets_batch_in_flight_together(order):
    """each is judged under its own kind of set; pending_ex reports the oldest batch's kind bits"""
    V = _V()
    c = SC.main_case()
    one = S._case("v7_middle_empty", 7, [7, 0, 6], None, True, True, 2)   # three blocks under a single set of 7
    ref = V.BatchVerifier(max_rows=SC.MAX_ROWS)
    try:
        ref.set_validators(one.r.height, one.r.addrs, one.r.power)
        want_one = S.sibling(ref, "verify_raw", one)
    finally:
        ref.close()
    want_sets = sync_results("recover_raw", SC.main_case)
    bv = _ctx(fam=c.f)
    try:
        assert bv.try_set_validators(one.r.height, one.r.addrs, one.r.power) == 0
        steps = [("single", one), ("sets", c)] if order == "single first" else [("sets", c), ("single", one)]
        for what, x in steps:
            assert (S.submit(bv, "verify_raw", x) if what == "single" else SC.submit(bv, "recover_raw", x)) == x.n
        for k, (what, x) in enumerate(steps):
            bits = 2 if what == "single" else SC.kind_bits("recover_raw")
            assert bv.block_seals_pending_ex() == (2 - k, x.n, len(x.bh), bits)
            got = bv.block_seals_collect_ex()
            S.same(got, want_one if what == "single" else want_sets, f"{order}/{what}")
        # a single-set batch BETWEEN two sets batches: three batches through the two slots
        SC.submit(bv, "verify", c)
        S.submit(bv, "verify_raw", one)
        SC.same(bv.block_seals_collect_ex(), sync_results("verify", SC.main_case), "sets, single behind it")
        SC.submit(bv, "verify_raw", c)
        S.same(bv.block_seals_collect_ex(), want_one, "single between two sets batches")
        SC.same(bv.block_seals_collect_ex(), sync_results("verify_raw", SC.main_case), "sets behind a single")
        # the old collect: a sets verify batch like any verify batch, a sets recover batch with rows refused and left in flight
        SC.submit(bv, "verify", c)
        m, tl = bv.block_seals_collect()
        w = sync_results("verify", SC.main_case)
        assert (m == w["verdict"]).all() and [S.fields(t) for t in tl] == [S.fields(t) for t in w["tallies"]]
        SC.submit(bv, "recover", c)
        mask = np.zeros((c.n + 63) // 64, np.uint64)
        assert bv._L.ibft_block_seals_collect(bv._h, V._p(mask), (V.Tally * len(c.bh))()) == E_INVAL
        assert bv.block_seals_pending_ex()[0] == 1 and not mask.any()
        SC.same(bv.block_seals_collect_ex(), sync_results("recover", SC.main_case), "recover after the refused old collect")
    finally:
        bv.close()


@pytest.mark.parametrize("flags,in_flight", [(0, 1), (2, 2)])
def test_a_batch_is_judged_under_the_family_of_its_submit(flags, in_flight):
    """submit under F, install F′ — other members, other powers, fewer sets: the old block_set entries are out of range there —,
    collect: every bit, vidx and quorum_* is F's.  Then a synchronous call under F′ is correct, and a second identical cycle
    leaves ibft_cache_memory where it was."""
    c, o = SC.main_case(), SC.other_case()
    kinds = ["recover_raw", "verify"][:in_flight]
    want = {k: sync_results(k, SC.main_case) for k in kinds}
    obits, otallies, owho, ovidx = SC.expect_cpu(o)
    rbits, rtallies, _, _ = SC.expect_cpu(o, bare=True)
    bv = _ctx(flags)
    try:
        memory = []
        for cycle in range(2):
            c.f.install(bv)
            for k in kinds:
                assert SC.submit(bv, k, c) == c.n
            o.f.install(bv)                                  # legal with batches in flight; waits for their kernels
            assert bv.validator_sets_info()[:2] == (2, 11) and bv.block_seals_pending_ex()[0] == in_flight
            for k in kinds:
                SC.same(bv.block_seals_collect_ex(), want[k], f"cycle {cycle}: {k} submitted under F, collected under F′")
            a, v, m, tl, bh = bv.recover_block_seals_sets_raw(o.raws, o.rounds, o.off, o.bset, o.sig, o.pre)
            assert (m == rbits).all() and (a == owho).all() and (v == ovidx).all() and (bh == o.bh).all()
            assert [S.fields(t)[:5] for t in tl] == rtallies
            # a refused install (a set without power) leaves F′ and a batch in flight untouched
            assert SC.submit(bv, "verify_raw", o) == o.n
            assert bv.try_set_validator_sets([(c.f.addrs(0), [0] * 7)]) == -6
            assert bv.validator_sets_info()[:2] == (2, 11)
            got = bv.block_seals_collect_ex()
            assert (got["verdict"] == obits).all() and [S.fields(t)[:5] for t in got["tallies"]] == otallies
            memory.append(bv.cache_memory())
        assert memory[0] == memory[1], "a cycle of install / submit / install / collect leaks key-cache slots or bytes"
        if flags & 2:
            assert memory[0][1] > 0                          # the union installed last holds its slots
    finally:
        bv.close()


def test_refusals_take_no_slot():
    V = _V()
    L, p = V.load_library(), V._p
    c = SC.main_case()
    raw, roff, rnd = V.proposal_columns(c.raws, c.rounds)
    nb = len(c.bh)

    def raw_submit(bv, bset):
        return L.ibft_block_seals_submit_sets_raw(bv._h, p(raw), p(roff), p(rnd), p(c.off), p(bset), nb, p(c.sig), p(c.signer), p(c.pre))

    def hash_submits(bv, bset):
        return (L.ibft_block_seals_submit_sets(bv._h, p(c.bh), p(c.off), p(bset), nb, p(c.sig), p(c.signer), p(c.pre)),
                L.ibft_recover_block_seals_submit_sets(bv._h, p(c.bh), p(c.off), p(bset), nb, p(c.sig), p(c.pre)),
                L.ibft_recover_block_seals_submit_sets_raw(bv._h, p(raw), p(roff), p(rnd), p(c.off), p(bset), nb, p(c.sig), p(c.pre)))

    bv = V.BatchVerifier(max_rows=SC.MAX_ROWS)
    try:
        bv.set_validators(1, c.f.addrs(0), c.f.power[0])
        assert raw_submit(bv, c.bset) == E_NOVALSET and hash_submits(bv, c.bset) == (E_NOVALSET,) * 3   # a single set is no family
        assert bv.block_seals_pending_ex() == (0, 0, 0, 0)
        c.f.install(bv)
        assert SC.submit(bv, "verify_raw", c) == c.n
        state = bv.block_seals_pending_ex()
        assert state == (1, c.n, nb, SC.kind_bits("verify_raw"))
        oob = c.bset.copy(); oob[nb - 1] = 3                                       # = n_sets
        assert raw_submit(bv, oob) == E_INVAL and hash_submits(bv, oob) == (E_INVAL,) * 3
        assert bv.block_seals_pending_ex() == state
        assert raw_submit(bv, None) == E_INVAL and hash_submits(bv, None) == (E_INVAL,) * 3
        assert bv.block_seals_pending_ex() == state
        bad_roff = roff.copy(); bad_roff[0] = 1                                    # the sibling's checks, then the proposals'
        assert L.ibft_block_seals_submit_sets_raw(bv._h, p(raw), p(bad_roff), p(rnd), p(c.off), p(c.bset), nb, p(c.sig), p(c.signer),
                                                  p(c.pre)) == E_INVAL
        assert bv.block_seals_pending_ex() == state
        assert SC.submit(bv, "recover", c) == c.n
        state = bv.block_seals_pending_ex()
        assert state[0] == 2
        assert raw_submit(bv, c.bset) == E_INVAL and hash_submits(bv, c.bset) == (E_INVAL,) * 3      # a third submit
        assert b"two block batches" in L.ibft_last_error(bv._h)
        assert bv.block_seals_pending_ex() == state
        SC.same(bv.block_seals_collect_ex(), sync_results("verify_raw", SC.main_case), "first in flight")
        SC.same(bv.block_seals_collect_ex(), sync_results("recover", SC.main_case), "second in flight")
        # a family alone: the single-set submits keep answering IBFT_E_NOVALSET
        only = V.BatchVerifier(max_rows=SC.MAX_ROWS)
        try:
            c.f.install(only)
            assert L.ibft_block_seals_submit(only._h, p(c.bh), p(c.off), nb, p(c.sig), p(c.signer), p(c.pre)) == E_NOVALSET
            assert only.block_seals_pending_ex() == (0, 0, 0, 0)
        finally:
            only.close()
    finally:
        bv.close()


def test_digest_placement_and_form_give_the_same_bits():
    """IBFT_STREAM_DIGEST and IBFT_PROPOSAL_LANES are read at ibft_ctx_create: a fresh child process per setting, each under
    its own time limit, compared with the synchronous siblings of THIS process (default form).  The first child that fails
    ends the test: nothing more is started on the device behind it."""
    seq = [SC.main_case(), SC.empty_case()]
    want = {(kind, c.name): SC.fingerprint(sync_results(kind, fn))
            for kind in ("verify_raw", "recover_raw") for c, fn in zip(seq, (SC.main_case, SC.empty_case))}
    for placement in ("copy", "main"):
        for lanes in ("1", "64"):
            env = dict(os.environ, IBFT_STREAM_DIGEST=placement, IBFT_PROPOSAL_LANES=lanes,
                       PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
            out = subprocess.run([sys.executable, os.path.join(HERE, "block_sets_stream_cases.py")], env=env, capture_output=True,
                                 text=True, timeout=120)
            assert out.returncode == 0 and "SETS_STREAM_CHILD_OK" in out.stdout, \
                f"{placement}/{lanes}: exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
            got = {tuple(l.split()[1:3]): l.split()[3] for l in out.stdout.splitlines() if l.startswith("FP ")}
            assert got == want, f"{placement}/{lanes}"


def test_a_streamed_sets_recover_batch_teaches_keys():
    """keys no other test uses: the device-wide key cache cannot know them yet"""
    from oracle import binding as B
    import test_gpu_block_seals_sets as T
    V = _V()
    f = T.Fam(11, 7, 2, 3, 77411)
    bset = np.array([b % 3 for b in range(6)], np.uint32)
    raws, rounds, bh = SC.proposals(6, 77412)
    who = [(i, b) for b in range(6) for i in f.idx[bset[b]]]          # every member of the block's set signs, every row valid
    sig = np.array([np.frombuffer(B.sign(f.r.sks[i], bytes(bh[b])), np.uint8) for i, b in who], np.uint8)
    signer = np.array([f.r.addrs[i] for i, _ in who], np.uint8)
    c = SC.Case("teach", f, bset, raws, rounds, bh, (np.arange(7) * 7).astype(np.uint32), sig, signer, None, [-1] * 6)
    ref = _ctx(fam=f)
    try:
        want_r, want_v = SC.sibling(ref, "recover", c), SC.sibling(ref, "verify", c)
    finally:
        ref.close()
    bv = _ctx(V.FLAG_PUBKEY_CACHE, fam=f)
    try:
        assert bv.cache_stats()[1:] == (0, 0)
        assert SC.submit(bv, "recover", c) == c.n
        SC.same(bv.block_seals_collect_ex(), want_r, "recover, cache on")
        assert bv.cache_stats()[1:] == (0, 1)                # one cold pass; the tables were built at the collect
        assert SC.submit(bv, "verify", c) == c.n
        SC.same(bv.block_seals_collect_ex(), want_v, "the sets verify pass that follows")
        assert bv.cache_stats()[1:] == (1, 1) and bv.last_dispatch()[0] == 0   # … and it ran warm, no cold stage behind it
        assert want_v["verdict"].all() and all(t.has_quorum for t in want_v["tallies"])
    finally:
        bv.close()
