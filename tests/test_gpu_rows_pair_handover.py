"""GPU: the hand-over that ends a rows pair (ecrecover_rows_pair_kernel, wave_fe_dev.h: rows_pair_shared).  A helper wavefront
publishes u1·G into LDS and ENDS; only the main wavefronts stand at the workgroup's second barrier, which opens once every
helper has ended — whichever side got there first.

1. The hand-over alone (devtest_handover: one workgroup, helpers publish a pattern through the policy object of the devtest
   pair kernel): in both orders the pattern arrives, and the s_memrealtime stamps say which order it was.
2. The pair form, pinned (IBFT_COLD_LANES=16, IBFT_ROWS_PAIR=1; IBFT_PAIR_LEAVE=1: as shipped the helpers of so small a launch
   stay at barrier 2), against the oracle at the sizes where workgroups mix working and idle pairs or end in a ragged
   wavefront — committed seals, senders and bare-seal recovery: the kernel's three modes.
3. Eight pipelined passes, one in flight, over two batches that differ in one forged seal: every collect is its own batch's.
   At 4 096 rows the chip is full, and pass k + 1's workgroups land beside pass k's live main wavefronts."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the hand-over alone -------------------------------------------------------------------------------------------
# A delay round is one s_sleep of about 1 000 clocks (≈ 0.45 µs): 256 rounds are ≈ 100 µs, against the few µs a wavefront
# without delay needs from barrier 1 to its next stamp.
DELAY = 256


def _handover(helper_delay, main_delay, salt):
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_devtest())
    L.devtest_handover.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    out = np.zeros(1024, np.uint32)
    stamps = np.zeros(64, np.uint64)
    assert L.devtest_handover(helper_delay, main_delay, salt, out.ctypes.data, stamps.ctypes.data) == 0
    slot, field, lane = np.meshgrid(np.arange(4, dtype=np.uint32), np.arange(4, dtype=np.uint32), np.arange(64, dtype=np.uint32),
                                    indexing="ij")
    want = np.uint32((salt * 0x9E3779B1) & 0xFFFFFFFF) ^ (slot << 16 | field << 8 | lane)
    st = stamps.reshape(8, 8).astype(np.int64)
    print(f"helper_delay {helper_delay} main_delay {main_delay}: ticks (100 MHz) since the first start, per wavefront\n"
          f"{np.where(st > 0, st - st[:, 0].min(), 0)}")
    return out.reshape(4, 4, 64), want, st[:4], st[4:]


def _common(out, want, main, helper):
    assert (out == want).all(), "the main wavefronts did not read what the helpers published"
    assert (main[:, 1:6] > 0).all() and (helper[:, [1, 2, 3, 5]] > 0).all()
    assert (helper[:, 4] == 0).all(), "a helper never stands at barrier 2"
    # barrier 1 held all eight: nobody left it before the last one had reached it
    assert min(main[:, 2].min(), helper[:, 2].min()) >= max(main[:, 1].max(), helper[:, 1].max())
    # barrier 2 opened behind the last helper's publish (its end stamp is taken behind the wait for its LDS stores)
    assert main[:, 4].min() >= helper[:, 5].max()


def test_helpers_that_ended_before_the_main_wavefronts_arrive():
    out, want, main, helper = _handover(0, DELAY, 0x5EED0001)
    _common(out, want, main, helper)
    assert helper[:, 5].max() < main[:, 3].min(), "meant: every helper gone before the first main wavefront reaches barrier 2"


def test_main_wavefronts_that_wait_for_the_helpers_to_end():
    out, want, main, helper = _handover(DELAY, 0, 0x5EED0002)
    _common(out, want, main, helper)
    assert main[:, 3].max() < helper[:, 3].min(), "meant: every main wavefront at barrier 2 before the first helper publishes"


# ---- 2. the pair form against the oracle ------------------------------------------------------------------------------
SIZES = [1, 4, 5, 16, 17, 33, 64, 65]


@pytest.fixture(scope="module")
def pair_bv():
    """one context with the pair form pinned (the pins are read when the context is created)"""
    import go_ibft_amd.verifier as V
    mp = pytest.MonkeyPatch()
    mp.setenv("IBFT_COLD_LANES", "16")
    mp.setenv("IBFT_ROWS_PAIR", "1")
    mp.setenv("IBFT_PAIR_LEAVE", "1")      # (as shipped only a launch that fills the device lets its helpers leave)
    bv = V.BatchVerifier(max_rows=4096)
    mp.undo()
    yield bv
    bv.close()


_ROUNDS = {}


def _round(n):
    from oracle import workload as W
    if n not in _ROUNDS:
        _ROUNDS[n] = W.make_round(n, 8800 + n, byzantine=True, with_envelopes=True)
    return _ROUNDS[n]


def _tally_fields(t):
    return (t.power, t.quorum, t.has_quorum, t.valid_rows, t.distinct_senders)


def _check_seals(bv, oracle, r, pre):
    vs = oracle.ValSet(r.addrs, r.power)
    bv.set_validators(r.height, r.addrs, r.power)
    got, t = bv.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, pre)
    exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, pre)
    assert (got == exp.astype(bool)).all(), np.nonzero(got != exp.astype(bool))[0][:10]
    assert _tally_fields(t) == _tally_fields(oracle.tally(vs, r.signer20, exp))
    assert bv.last_dispatch() == (16, 0)
    return exp


@pytest.mark.parametrize("n", SIZES)
def test_pair_form_seals(pair_bv, oracle, n):
    r = _round(n)
    _check_seals(pair_bv, oracle, r, r.pre_flags)


def test_an_idle_pair_between_working_ones(pair_bv, oracle):
    """16 rows, one workgroup; rows 4..7 pre-flagged: pair 1 only synchronises, pairs 0, 2 and 3 work"""
    r = _round(16)
    pre = np.zeros(16, np.uint8)
    pre[4:8] = 1
    exp = _check_seals(pair_bv, oracle, r, pre)
    assert not exp[4:8].any() and exp[:4].any() and exp[8:].any()
    from test_gpu_recover_seals import check, expect
    vs = oracle.ValSet(r.addrs, r.power)
    check(pair_bv.recover_seals(r.hash32, r.seal65, pre), expect(oracle, vs, r.addrs, r.hash32, r.seal65, pre), "idle pair")


@pytest.mark.parametrize("n", SIZES)
def test_pair_form_senders(pair_bv, oracle, n):
    r = _round(n)
    vs = oracle.ValSet(r.addrs, r.power)
    pair_bv.set_validators(r.height, r.addrs, r.power)
    got, t = pair_bv.is_valid_validator(r.payload, r.off, r.msg_sig65, r.signer20, r.pre_flags)
    exp = oracle.verify_senders(vs, r.payload, r.off, r.msg_sig65, r.signer20, r.pre_flags)
    assert (got == exp.astype(bool)).all(), np.nonzero(got != exp.astype(bool))[0][:10]
    assert _tally_fields(t) == _tally_fields(oracle.tally(vs, r.signer20, exp))
    assert pair_bv.last_dispatch() == (16, 0)


@pytest.mark.parametrize("n", SIZES)
def test_pair_form_recover_seals(pair_bv, oracle, n):
    from test_gpu_recover_seals import check, expect
    r = _round(n)
    vs = oracle.ValSet(r.addrs, r.power)
    pair_bv.set_validators(r.height, r.addrs, r.power)
    check(pair_bv.recover_seals(r.hash32, r.seal65, r.pre_flags), expect(oracle, vs, r.addrs, r.hash32, r.seal65, r.pre_flags), f"n = {n}")
    assert pair_bv.last_dispatch() == (16, 0)


# ---- 3. the pipeline --------------------------------------------------------------------------------------------------
def _eight_passes(bv, oracle, addrs, power, A, B):
    """A, B: (hash32, seal65, signer20).  Passes alternate A, B, A, … through the spare column set, one kept in flight."""
    import go_ibft_amd.verifier as V
    vs = oracle.ValSet(addrs, power)
    want = {}
    for name, (h, s, f) in (("A", A), ("B", B)):
        e = oracle.verify_seals(vs, h, s, f, nthreads=8)
        want[name] = (e.astype(bool), _tally_fields(oracle.tally(vs, f, e)))
    assert (want["A"][0] != want["B"][0]).sum() == 1      # the forged seal, and nothing else
    host = {name: tuple(V.pinned_copy(c) for c in cols) + (None,) for name, cols in (("A", A), ("B", B))}

    def collected(which, k):
        verdict, t = bv.seals_collect()
        assert (verdict == want[which][0]).all(), (k, which, np.nonzero(verdict != want[which][0])[0][:8])
        assert _tally_fields(t) == want[which][1], (k, which)

    bv.set_validators(1, addrs, power)
    bv.seals_stage(*A, None)
    in_flight = []
    for k in range(8):
        bv.seals_submit()
        in_flight.append("AB"[k & 1])
        if k < 7:
            bv.seals_stage_next(*host["BA"[k & 1]])
        if len(in_flight) == 2:
            collected(in_flight.pop(0), k)
        if k < 7:
            bv.seals_swap()
    collected(in_flight.pop(0), 8)
    # passes 2, 4, 6 and 8 found their predecessor in flight on the main stream and took the second one
    assert bv.alt_verdict_passes() == 4


def _forge(seal65, i, j):
    """row i carries row j's seal: a valid seal — of another validator"""
    s = seal65.copy()
    s[i] = seal65[j]
    return s


def test_pipeline_n17(oracle, monkeypatch):
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    r = W.make_round(17, 8901)
    monkeypatch.setenv("IBFT_COLD_LANES", "16")
    monkeypatch.setenv("IBFT_ROWS_PAIR", "1")
    monkeypatch.setenv("IBFT_PAIR_LEAVE", "1")
    bv = V.BatchVerifier(max_rows=4096)
    try:
        _eight_passes(bv, oracle, r.addrs, r.power, (r.hash32, r.seal65, r.signer20), (r.hash32, _forge(r.seal65, 16, 3), r.signer20))
        assert bv.last_dispatch() == (16, 0)
    finally:
        bv.close()


@pytest.fixture(scope="module")
def bench_round():
    with np.load(os.path.join(ROOT, "tests", "golden", "bench_round_n4096.npz")) as z:
        g = {k: z[k] for k in ("addrs", "power", "hash32", "seal65", "signer20")}
    for a in g.values():
        a.setflags(write=False)
    return g


@pytest.mark.parametrize("n, leave", [(2049, "1"), (2049, None), (4096, None)])
def test_pipeline_on_the_bench_round(oracle, bench_round, monkeypatch, n, leave):
    """These sizes take the pair form and the second verdict stream as shipped.  As shipped, too, the helpers of 4 096 rows (as
    many workgroups as the device has compute units) leave and those of 2 049 stay; pinned, those of 2 049 leave as well, and
    the next pass's workgroups may land beside this one's on a half-empty device."""
    import go_ibft_amd.verifier as V
    if leave is None:
        monkeypatch.delenv("IBFT_PAIR_LEAVE", raising=False)
    else:
        monkeypatch.setenv("IBFT_PAIR_LEAVE", leave)
    g = bench_round
    h, s, f = g["hash32"][:n], g["seal65"][:n], g["signer20"][:n]
    bv = V.BatchVerifier(max_rows=4096)
    try:
        _eight_passes(bv, oracle, g["addrs"], g["power"], (h, s, f), (h, _forge(s, n - 1, 7), f))
        assert bv.last_dispatch() == (16, 0)
    finally:
        bv.close()
