"""GPU: consecutive pipelined passes (ibft_seals_submit / ibft_seals_collect) put their verdict launch alternately on two streams
(round 21; IBFT_ALT_VERDICT=0|1 pins it, ibft_pipeline_stats_ex counts the passes that took the second one).
Pass k+1 may then run NEXT TO pass k, so everything the two would share has to exist twice or be ordered: every pass's verdict
words and tally are held to the by-construction expectation of its own batch (go-ibft_amd/simulate.py: every validator signs
once, crafted rows carry another validator's seal, a zero r, a zero s) — IsValidCommittedSeal and HasQuorum of the reference
(core/backend.go:53-55, core/validator_manager.go:77-96 there) row for row.

Shapes: 2 049 and 4 096 rows are the smallest and largest batch of the row form with a helper wavefront, 4 097 takes the plain
row form, 1 and 64 the two-wavefront form, 0 launches no verdict kernel at all.  Crafted rows sit at row 0, row n − 1 and on both
sides of a 64-row word boundary of every one of these sizes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_MAX = 4097
SIZES = [0, 1, 64, 2049, 4096, 4097]
BAD_ROWS = [0, 63, 64, 2048, 4095, 4096]       # row 0, row n − 1 of every size above, both sides of the word boundary 63 | 64


class Expect:
    def __init__(self, verdict, power, total):
        self.verdict = verdict
        self.valid_rows = int(verdict.sum())
        self.power = int(power[: len(verdict)][verdict].sum())       # every row is another validator: nothing counts twice
        self.quorum = 2 * total // 3 + 1
        self.has_quorum = int(self.power >= self.quorum)


def _check(got, want, what=""):
    verdict, t = got
    assert len(verdict) == len(want.verdict) and (verdict == want.verdict).all(), (what, np.flatnonzero(verdict != want.verdict)[:8])
    assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum, t.quorum) == \
           (want.power, want.valid_rows, want.valid_rows, want.has_quorum, want.quorum), what


@pytest.fixture(scope="module")
def rnd():
    """One validator set of 4 097 with a seal each (signed on the device, all valid by construction), the crafted rows, and the
    expectation of every prefix the tests use: computed once, never written again."""
    import go_ibft_amd.verifier as V
    import go_ibft_amd.simulate as SIM
    bv = V.BatchVerifier(max_rows=N_MAX)
    try:
        r = SIM.make_round(bv, N_MAX, 1501, weighted=True)
    finally:
        bv.close()
    assert r.expect.all()
    seal = r.seal65.copy()
    for j, i in enumerate(BAD_ROWS):
        if j % 3 == 0:
            seal[i] = r.seal65[(i + 7) % N_MAX]     # a valid seal — of another validator
        elif j % 3 == 1:
            seal[i, :32] = 0                        # r = 0
        else:
            seal[i, 32:64] = 0                      # s = 0
    good = np.ones(N_MAX, dtype=bool)
    bad = good.copy()
    bad[BAD_ROWS] = False
    total = int(r.power.sum())
    r.cols_valid = lambda n: (r.hash32[:n], r.seal65[:n], r.signer20[:n], None)
    r.cols = lambda n: (r.hash32[:n], seal[:n], r.signer20[:n], None)
    r.want_valid = {n: Expect(good[:n], r.power, total) for n in SIZES}
    r.want = {n: Expect(bad[:n], r.power, total) for n in SIZES}
    for a in (r.hash32, r.seal65, r.signer20, r.power, seal):
        a.setflags(write=False)
    return r


def _verifier(r, monkeypatch, pin, **kw):
    import go_ibft_amd.verifier as V
    if pin is None:
        monkeypatch.delenv("IBFT_ALT_VERDICT", raising=False)
    else:
        monkeypatch.setenv("IBFT_ALT_VERDICT", pin)
    bv = V.BatchVerifier(max_rows=8192, **kw)            # (the pin is read when the context is created)
    bv.set_validators(1, r.addrs, r.power)
    return bv


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pin", ["1", "0"])
def test_eight_pipelined_passes_equal_the_synchronous_pass(rnd, monkeypatch, n, pin):
    """Eight passes with one kept in flight: each one's verdict words and tally are the expectation's and those of a synchronous
    ibft_seals_run on the same context.  Pinned on, every pass behind the first that finds its predecessor in flight takes the
    other stream than that one — passes 2, 4, 6, 8; pinned off (and for the empty batch) none does."""
    bv = _verifier(rnd, monkeypatch, pin)
    try:
        bv.seals_stage(*rnd.cols(n))
        sync = bv.seals_run()
        _check(sync, rnd.want[n], "synchronous")
        bv.seals_submit()
        for k in range(7):
            bv.seals_submit()
            got = bv.seals_collect()
            _check(got, rnd.want[n], k)
            assert (got[0] == sync[0]).all() and got[1].power == sync[1].power
        _check(bv.seals_collect(), rnd.want[n], 7)
        assert bv.alt_verdict_passes() == (4 if pin == "1" and n else 0)
        _check(bv.seals_run(), rnd.want[n], "synchronous, after")
    finally:
        bv.close()


@pytest.mark.parametrize("pin", ["1", None])
def test_each_collect_delivers_its_own_batch(rnd, monkeypatch, pin):
    """The batch changes under the pipeline: two passes over A (all valid), a restage to B (crafted rows), two passes over B — and
    the same with the batch travelling through the spare column set while the passes before it are in flight (ibft_seals_stage_next
    / ibft_seals_swap: the second verdict stream is a reader of the old columns and of the new ones)."""
    import go_ibft_amd.verifier as V
    n = 4096
    A, B = rnd.cols_valid(n), rnd.cols(n)
    bv = _verifier(rnd, monkeypatch, pin)
    try:
        bv.seals_stage(*A)
        bv.seals_submit(); bv.seals_submit()
        _check(bv.seals_collect(), rnd.want_valid[n], "A1"); _check(bv.seals_collect(), rnd.want_valid[n], "A2")
        bv.seals_stage(*B)
        bv.seals_submit(); bv.seals_submit()
        _check(bv.seals_collect(), rnd.want[n], "B1"); _check(bv.seals_collect(), rnd.want[n], "B2")
        assert bv.alt_verdict_passes() == 2              # (the row form with a helper wavefront takes it by default)
        # submit(k) → stage_next(k+1) → collect(k−1) → swap, the batches alternating B, A, B, A, B, A
        pa, pb = (tuple(None if c is None else V.pinned_copy(c) for c in x) for x in (A, B))
        in_flight = []
        for k in range(6):
            bv.seals_submit()
            in_flight.append("BA"[k & 1])
            bv.seals_stage_next(*(pa if k & 1 == 0 else pb))
            if len(in_flight) == 2:
                which = in_flight.pop(0)
                _check(bv.seals_collect(), (rnd.want_valid if which == "A" else rnd.want)[n], (k, which))
            bv.seals_swap()
        which = in_flight.pop(0)
        _check(bv.seals_collect(), (rnd.want_valid if which == "A" else rnd.want)[n], which)
        assert bv.alt_verdict_passes() == 2 + 3
    finally:
        bv.close()


@pytest.mark.parametrize("pin", ["1", None])
def test_calls_outside_the_pipeline_between_a_submit_and_its_collect(rnd, monkeypatch, pin):
    """A synchronous pass, a one-shot ibft_verify_seals over OTHER rows and a plain ibft_tally while two pipelined passes are in
    flight on two streams: each returns its own result, and the passes still deliver theirs."""
    n, m = 4096, 2049
    bv = _verifier(rnd, monkeypatch, pin)
    try:
        bv.seals_stage(*rnd.cols(n))
        for step in range(3):
            bv.seals_submit(); bv.seals_submit()
            if step == 0:
                _check(bv.seals_run(), rnd.want[n], "seals_run in between")
            elif step == 1:
                _check(bv.is_valid_committed_seal(*rnd.cols_valid(m)), rnd.want_valid[m], "one-shot in between")
                bv.seals_stage(*rnd.cols(n))
            else:
                t = bv.has_quorum(rnd.signer20[:m], rnd.want[m].verdict)
                assert (t.power, t.distinct_senders, t.has_quorum) == (rnd.want[m].power, rnd.want[m].valid_rows, rnd.want[m].has_quorum)
            _check(bv.seals_collect(), rnd.want[n], (step, 0)); _check(bv.seals_collect(), rnd.want[n], (step, 1))
        assert bv.alt_verdict_passes() == 3
    finally:
        bv.close()


@pytest.mark.parametrize("pin", ["1", None])
def test_sizes_and_kernel_forms_changing_from_pass_to_pass(rnd, monkeypatch, pin):
    """4 096 → 2 049 → 4 097 → 64 → 0 → 4 096 through the spare column set, one pass in flight: the kernel form changes from pass
    to pass, an empty pass sits between two full ones; every pass is its own batch's, and ibft_seals_rows reports its rows."""
    import go_ibft_amd.verifier as V
    sizes = [4096, 2049, 4097, 64, 0, 4096]
    host = {n: tuple(None if c is None else V.pinned_copy(c) for c in rnd.cols(n)) for n in set(sizes)}
    bv = _verifier(rnd, monkeypatch, pin)
    try:
        bv.seals_stage(*rnd.cols(sizes[0]))
        in_flight = []
        for k, n in enumerate(sizes):
            bv.seals_submit()
            in_flight.append(n)
            assert bv.seals_rows() == (n, in_flight[0])
            if k + 1 < len(sizes):
                bv.seals_stage_next(*host[sizes[k + 1]])
            if len(in_flight) == 2:
                done = in_flight.pop(0)
                _check(bv.seals_collect(), rnd.want[done], (k, done))
            if k + 1 < len(sizes):
                bv.seals_swap()
        _check(bv.seals_collect(), rnd.want[in_flight.pop(0)], "last")
        assert bv.seals_rows() == (4096, 0)
        # passes 2, 4 and 6 found their predecessor in flight on the main stream (the empty pass 5 never leaves it)
        assert bv.alt_verdict_passes() == 3
    finally:
        bv.close()


def test_a_learning_key_cache_and_a_rank_of_a_local_group_keep_one_verdict_stream(rnd, monkeypatch):
    """Pinned ON all the same: a context whose key cache is still learning (the passes teach it keys through one device-wide
    counter) and a rank of a group on one device (its exchange follows the tally on the main stream) never take the second
    stream, and their passes are correct."""
    import go_ibft_amd.verifier as V
    n = 2049
    bv = _verifier(rnd, monkeypatch, "1", flags=V.FLAG_PUBKEY_CACHE)
    try:
        bv.seals_stage(*rnd.cols(n))
        bv.seals_submit(); bv.seals_submit()             # both enqueued before the first collect could build a table
        assert bv.alt_verdict_passes() == 0
        _check(bv.seals_collect(), rnd.want[n], "learning 1"); _check(bv.seals_collect(), rnd.want[n], "learning 2")
    finally:
        bv.close()
    g = V.DeviceGroup([0, 0], max_rows_total=16384)
    rank = object.__new__(V.BatchVerifier)               # rank 0's context, borrowed: the group owns it
    try:
        g.set_validators(1, rnd.addrs, rnd.power)
        rank._L, rank._h, rank.max_rows = g._L, C.c_void_p(g._L.ibft_group_ctx(g._g, 0)), 4096
        rank.seals_stage(*rnd.cols(n))
        rank.seals_submit(); rank.seals_submit()
        for k in range(2):
            verdict, t = rank.seals_collect()
            assert (verdict == rnd.want[n].verdict).all() and (t.valid_rows, t.power) == (rnd.want[n].valid_rows, rnd.want[n].power), k
        assert rank.alt_verdict_passes() == 0
    finally:
        rank._h = C.c_void_p()
        g.close()


@pytest.mark.parametrize("pin", ["1", "0"])
def test_an_empty_pass_between_two_timed_passes(rnd, monkeypatch, pin):
    """ibft_set_kernel_timing(1): a timed pass's stop event is what its tally waits for.  An EMPTY pass records none — it used to
    pick up the stop event of the pass before it; with two verdict streams that would order its tally, and through the shared
    tally stream the next pass's, behind the wrong stream.  The empty pass reports nothing valid, the pass behind it its own
    batch, and the event time read afterwards covers the two timed launches."""
    n = 4096
    bv = _verifier(rnd, monkeypatch, pin)
    try:
        bv.set_kernel_timing(1)
        bv.last_kernel_ms()
        bv.seals_stage(*rnd.cols(n))
        bv.seals_submit()
        bv.seals_stage(*rnd.cols(0))
        bv.seals_submit()
        _check(bv.seals_collect(), rnd.want[n], "timed, before")
        bv.seals_stage(*rnd.cols_valid(n))
        bv.seals_submit()
        _check(bv.seals_collect(), rnd.want[0], "empty")
        bv.seals_submit()
        _check(bv.seals_collect(), rnd.want_valid[n], "timed, after")
        _check(bv.seals_collect(), rnd.want_valid[n], "timed, last")
        ms, launches = bv.last_kernel_ms()
        assert launches == 3 and ms > 0.0
    finally:
        bv.close()
