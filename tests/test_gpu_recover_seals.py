"""GPU: ibft_recover_seals / ibft_recover_block_seals — bare committed seals, the signer is what ecrecover returns.  Every
expectation comes from the oracle (recover_address row by row, ValSet.index for membership, tally) or from the verify sibling
(ibft_verify_seals / ibft_verify_block_seals fed with the recovered addresses), never from the call under test.

The oracle numbers validators in its own sorted order; the library in the caller's order.  Membership is therefore taken from
ValSet.index and the expected index from the caller's list (rounds of oracle.workload have distinct addresses)."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = 16
# every AUTO branch and its ragged edges: two wavefronts per signature (≤ 512), one (≤ 2 048), a DPP row per signature with
# helper wavefronts (≤ 4 096) and without (≤ 8 192), four lanes (≤ 16 384), two lanes (≤ 32 768), one lane with its tables in
# LDS (≤ 65 536), the split batch (65 536 rows through that kernel + the rest through what AUTO picks for the rest)
SIZES = [1, 3, 64, 65, 512, 513, 2048, 2049, 4096, 4097, 8192, 8193, 16385, 65536, 70001]


def _V():
    import go_ibft_amd.verifier as V
    return V


def auto_lanes(n):
    return 128 if n <= 512 else 64 if n <= 2048 else 16 if n <= 8192 else 4 if n <= 16384 else 2 if n <= 32768 else 1


def fields(t):
    return (t.power, t.quorum, t.valid_rows, t.distinct_senders, t.has_quorum)


def oracle_recover(B, digest32, sig65, pre=None, flags=0):
    """orc_recover_address row by row → (address (n, 20) uint8 — zeros where there is none or the row is pre-flagged)"""
    n = len(sig65)
    out = np.zeros((n, 20), np.uint8)
    d = np.ascontiguousarray(digest32, np.uint8)
    s = np.ascontiguousarray(sig65, np.uint8)

    def part(k):
        for i in range(k, n, THREADS):
            if pre is not None and pre[i]:
                continue
            a = B.recover_address(d[i].tobytes(), s[i].tobytes(), flags)
            if a is not None:
                out[i] = np.frombuffer(a, np.uint8)

    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(part, range(THREADS)))
    return out


def expect(B, vs, addrs, digest32, sig65, pre=None, flags=0):
    """(address column, validator index in the caller's order, verdict bool, oracle tally) from the oracle alone"""
    n = len(sig65)
    a = oracle_recover(B, digest32, sig65, pre, flags)
    place = {}
    for i, x in enumerate(addrs):
        place.setdefault(x.tobytes(), len(place))
    vidx = np.full(n, -1, np.int32)
    for i in range(n):
        if a[i].any() and vs.index(a[i].tobytes()) >= 0:
            vidx[i] = place[a[i].tobytes()]
    bit = vidx >= 0
    return a, vidx, bit, B.tally(vs, a, bit.astype(np.uint8))


def check(got, exp, what=""):
    ga, gv, gm, gt = got
    ea, ev, em, et = exp
    assert ga.shape == ea.shape and ga.dtype == np.uint8 and gv.dtype == np.int32 and gm.dtype == bool
    bad = np.nonzero((ga != ea).any(axis=1))[0]
    assert not len(bad), f"{what}: addresses differ from the oracle at rows {bad[:10]}"
    assert (gv == ev).all(), f"{what}: validator indices differ at rows {np.nonzero(gv != ev)[0][:10]}"
    assert (gm == em).all(), f"{what}: verdicts differ at rows {np.nonzero(gm != em)[0][:10]}"
    assert fields(gt) == fields(et), f"{what}: tally {fields(gt)} != {fields(et)}"


_ROUNDS = {}


def round_of(n, byz):
    from oracle import workload as W
    if (n, byz) not in _ROUNDS:
        _ROUNDS[(n, byz)] = W.make_round(n, 9100 + n + (1 if byz else 0), raw_len=64, byzantine=byz, weighted=byz)
    return _ROUNDS[(n, byz)]


@pytest.fixture(scope="module")
def bv_big():
    bv = _V().BatchVerifier(max_rows=98304)
    yield bv
    bv.close()


@pytest.mark.parametrize("byz", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_rounds_match_the_oracle_in_every_auto_branch(oracle, bv_big, n, byz):
    r = round_of(n, byz)
    vs = oracle.ValSet(r.addrs, r.power)
    pre = r.pre_flags if byz else None
    exp = expect(oracle, vs, r.addrs, r.hash32, r.seal65, pre)
    bv_big.set_validators(r.height, r.addrs, r.power)
    got = bv_big.recover_seals(r.hash32, r.seal65, pre)
    check(got, exp, f"n = {n}")
    assert bv_big.last_dispatch()[0] == auto_lanes(n)
    if not byz:      # honest rows: the address is the signer the workload names
        assert (got[0] == r.signer20).all() and (got[1] == np.arange(n)).all() and got[2].all() and got[3].has_quorum == 1
    else:
        assert 0 < got[2].sum() < n or n < 8
    # round trip: the recovered addresses as claimed signers → the same mask words and the same tally
    m, t = bv_big.is_valid_committed_seal(r.hash32, r.seal65, got[0], pre)
    assert (m == got[2]).all() and fields(t) == fields(got[3])


def test_split_batch_is_split(oracle):
    V = _V()
    r = round_of(70001, True)
    bv = V.BatchVerifier(max_rows=98304)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        before = bv.pipeline_stats()[1]
        got = bv.recover_seals(r.hash32, r.seal65, r.pre_flags)
        assert bv.pipeline_stats()[1] == before + 1 and bv.last_dispatch()[0] == 1
        # a dirty work mask in front of the split (the second part ORs its bits in): a round of other rows first
        r2 = round_of(65, True)
        bv.set_validators(r2.height, r2.addrs, r2.power)
        bv.recover_seals(r2.hash32, r2.seal65, r2.pre_flags)
        bv.set_validators(r.height, r.addrs, r.power)
        again = bv.recover_seals(r.hash32, r.seal65, r.pre_flags)
        for x, y in zip(got[:3], again[:3]):
            assert (x == y).all()
        assert fields(got[3]) == fields(again[3])
    finally:
        bv.close()


# ---- every cold variant pinned, each in a fresh child process (the pins are read when the context is created) ---------
VARIANTS = [{"IBFT_COLD_LANES": "1"}, {"IBFT_COLD_LANES": "2"}, {"IBFT_COLD_LANES": "4"}, {"IBFT_COLD_LANES": "8"},
            {"IBFT_COLD_LANES": "16", "IBFT_ROWS_PAIR": "0"}, {"IBFT_COLD_LANES": "16", "IBFT_ROWS_PAIR": "1"},
            {"IBFT_COLD_LANES": "64"}, {"IBFT_COLD_LANES": "128"},
            {"IBFT_COLD_LANES": "1", "IBFT_COLD_TABLE": "private"}, {"IBFT_COLD_LANES": "1", "IBFT_COLD_TABLE": "private2"},
            {"IBFT_COLD_LANES": "4", "IBFT_COLD_TABLE": "private"}, {"IBFT_COLD_LANES": "4", "IBFT_COLD_TABLE": "private2"}]
PINNED_N = 333   # ragged for every form: 333 = 5·64 + 13 = 83·4 + 1, odd


def child_main(path):
    """run in the child: the round stored at `path` through recover_seals and recover_block_seals (three blocks) → npz"""
    V = _V()
    z = np.load(path + ".in.npz")
    bv = V.BatchVerifier(max_rows=4096)
    try:
        bv.set_validators(1, z["addrs"], z["power"])
        a, v, m, t = bv.recover_seals(z["hash32"], z["sig"], z["pre"])
        lanes = bv.last_dispatch()[0]
        table = bv.last_cold_table()
        ba, bvx, bm, bt = bv.recover_block_seals(z["bh"], z["off"], z["sig"], z["pre"])
    finally:
        bv.close()
    np.savez(path + ".out.npz", a=a, v=v, m=m, t=np.array(fields(t), object).astype(str), ba=ba, bv=bvx, bm=bm,
             bt=np.array([fields(x) for x in bt], object).astype(str), lanes=lanes, table=table)
    print("RECOVER_CHILD_OK")
    return 0


def test_every_pinned_cold_variant_gives_the_same_bytes(oracle, tmp_path):
    r = round_of(PINNED_N, True)
    n = r.n
    vs = oracle.ValSet(r.addrs, r.power)
    exp = expect(oracle, vs, r.addrs, r.hash32, r.seal65, r.pre_flags)
    # the same rows as three blocks that all carry the round's hash (so the rows mean the same in the block form)
    off = np.array([0, 100, 100 + 64, n], np.uint32)
    bh = np.repeat(r.hash32[:1], 3, axis=0)
    bt_exp = [fields(oracle.tally(vs, exp[0][off[b]:off[b + 1]], exp[2][off[b]:off[b + 1]].astype(np.uint8))) for b in range(3)]
    path = str(tmp_path / "round")
    np.savez(path + ".in.npz", addrs=r.addrs, power=r.power, hash32=r.hash32, sig=r.seal65, pre=r.pre_flags, bh=bh, off=off)
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_recover_seals as T; sys.exit(T.child_main(%r))"
            % (ROOT, os.path.join(ROOT, "tests"), path))
    first = None
    for var in VARIANTS:
        env = {k: v for k, v in os.environ.items() if k not in ("IBFT_COLD_LANES", "IBFT_ROWS_PAIR", "IBFT_COLD_TABLE")}
        env.update(var)
        if os.path.exists(path + ".out.npz"):
            os.remove(path + ".out.npz")
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        # (a child that failed ends the test here: nothing more is started on the device by it)
        assert p.returncode == 0 and "RECOVER_CHILD_OK" in p.stdout, json.dumps(var) + p.stdout[-2000:] + p.stderr[-3000:]
        z = np.load(path + ".out.npz", allow_pickle=False)
        assert int(z["lanes"]) == int(var["IBFT_COLD_LANES"]), var
        if "IBFT_COLD_TABLE" in var:      # (the group kernels know LDS and private + prefetch only: private2 leaves them in LDS)
            lane = var["IBFT_COLD_LANES"] == "1"
            assert int(z["table"]) == {"private": 2, "private2": 3 if lane else 1}[var["IBFT_COLD_TABLE"]], var
        what = json.dumps(var)
        assert (z["a"] == exp[0]).all() and (z["v"] == exp[1]).all() and (z["m"] == exp[2]).all(), what
        assert tuple(z["t"]) == tuple(str(x) for x in fields(exp[3])), what
        assert [tuple(x) for x in z["bt"]] == [tuple(str(y) for y in f) for f in bt_exp], what
        out = {k: z[k].tobytes() for k in ("a", "v", "m", "t", "ba", "bv", "bm", "bt")}
        assert out["ba"] == out["a"] and out["bv"] == out["v"] and out["bm"] == out["m"], what
        if first is None:
            first = out
        assert out == first, f"{what}: bytes differ from the first variant"


# ---- round trip, cold and with the key cache -------------------------------------------------------------------------
@pytest.mark.parametrize("cache", [False, True])
def test_round_trip_through_the_verify_siblings(oracle, cache):
    V = _V()
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE if cache else 0, max_rows=16384)
    try:
        for n in (100, 3000, 9000):
            r = round_of(n, True) if (n, True) in _ROUNDS else None
            if r is None:
                from oracle import workload as W
                r = W.make_round(n, 9300 + n, raw_len=64, byzantine=True, weighted=True)
            bv.set_validators(r.height, r.addrs, r.power)
            for rep in range(2):      # with the cache: the second turn's verify call is warm
                a, v, m, t = bv.recover_seals(r.hash32, r.seal65, r.pre_flags)
                vm, vt = bv.is_valid_committed_seal(r.hash32, r.seal65, a, r.pre_flags)
                assert (vm == m).all() and fields(vt) == fields(t), (n, rep)
                # the block form, blocks of uneven size over the same rows
                off = np.array([0, n // 3, n // 3, n - 1, n], np.uint32)
                bh = np.repeat(r.hash32[:1], 4, axis=0)
                ba, bvx, bm, bt = bv.recover_block_seals(bh, off, r.seal65, r.pre_flags)
                assert (ba == a).all() and (bvx == v).all() and (bm == m).all()
                vbm, vbt = bv.verify_block_seals(bh, off, r.seal65, ba, r.pre_flags)
                assert (vbm == bm).all() and [fields(x) for x in vbt] == [fields(x) for x in bt], (n, rep)
        if cache:
            assert bv.cache_stats()[1] > 0      # (warm passes were among the verify calls)
    finally:
        bv.close()


def test_key_cache_learns_from_a_recover_call_and_recover_stays_cold(oracle):
    V = _V()
    from oracle import workload as W
    n = 200
    r = W.make_round(n, 9401, raw_len=64)
    vs = oracle.ValSet(r.addrs, r.power)
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=4096)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        assert bv.cache_stats() == (0, 0, 0)
        got = bv.recover_seals(r.hash32, r.seal65)
        check(got, expect(oracle, vs, r.addrs, r.hash32, r.seal65), "fresh cache")
        tables, warm, cold = bv.cache_stats()
        assert (tables, warm, cold) == (n, 0, 1)      # every validator's table, learned from the recover call
        m, t = bv.is_valid_committed_seal(r.hash32, r.seal65, r.signer20)
        assert m.all() and t.has_quorum == 1
        tables, warm, cold = bv.cache_stats()
        assert (tables, warm, cold) == (n, 1, 1) and bv.last_dispatch()[0] == 0     # a warm pass, no cold kernel
        # on the warm context a recover call still recovers: rows of a non-member, corrupted rows, a pre-flagged row
        sig = r.seal65.copy()
        pre = np.zeros(n, np.uint8)
        outsider = W.validator_key(9401 ^ 0x99, 1 << 42)
        for i in range(0, n, 9):
            sig[i] = np.frombuffer(oracle.sign(outsider, r.hash32[i].tobytes()), np.uint8)
        sig[1::9, 64] = 2
        sig[2::9, :32] = 0
        sig[3::9, 40] ^= 0x20          # another valid-looking s: some other address or none — whatever the oracle says
        sig[4::9] = sig[5::9][: len(sig[4::9])]     # a member's seal in another member's row: that member's address
        pre[6::9] = 1
        got = bv.recover_seals(r.hash32, sig, pre)
        exp = expect(oracle, vs, r.addrs, r.hash32, sig, pre)
        check(got, exp, "warm context")
        assert (exp[1] == -1).sum() > n // 3 and exp[0][0].any() and exp[1][0] == -1
        assert bv.cache_stats() == (n, 1, 2) and bv.last_dispatch()[0] == auto_lanes(n)
        vm, vt = bv.is_valid_committed_seal(r.hash32, sig, got[0], pre)     # (warm) round trip
        assert (vm == got[2]).all() and fields(vt) == fields(got[3])
    finally:
        bv.close()


# ---- flags and the seal-digest convention ----------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True])
def test_strict_low_s_both_ways(oracle, strict):
    V = _V()
    from oracle import pyref, workload as W
    n = 600
    r = W.make_round(n, 9501, raw_len=64)
    sig = r.seal65.copy()
    for i in range(n):               # even rows: the high-s form of the signature (s → n − s, v flipped: the same key), odd: the low one
        s = int.from_bytes(sig[i, 32:64].tobytes(), "big")
        if (s > pyref.N // 2) != (i % 2 == 0):
            sig[i, 32:64] = np.frombuffer((pyref.N - s).to_bytes(32, "big"), np.uint8)
            sig[i, 64] ^= 1
    high = np.array([int.from_bytes(x[32:64].tobytes(), "big") > pyref.N // 2 for x in sig])
    assert high[::2].all() and not high[1::2].any()
    flags = V.FLAG_STRICT_LOW_S if strict else 0
    vs = oracle.ValSet(r.addrs, r.power)
    exp = expect(oracle, vs, r.addrs, r.hash32, sig, None, flags)
    bv = V.BatchVerifier(flags=flags, max_rows=1024)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        got = bv.recover_seals(r.hash32, sig)
        check(got, exp, f"strict = {strict}")
        if strict:
            assert not got[2][high].any() and not got[0][high].any() and got[2][~high].all()
        else:
            assert got[2].all() and (got[0] == r.signer20).all()
    finally:
        bv.close()


def test_seal_digest_convention_on_and_off(oracle):
    V = _V()
    from oracle import workload as W
    n, suffix = 300, b"\x02"
    r = W.make_round(n, 9601, raw_len=64)
    dig = np.array([np.frombuffer(oracle.keccak256(h.tobytes() + suffix), np.uint8) for h in r.hash32])
    sig = np.array([np.frombuffer(oracle.sign(r.sks[i], dig[i].tobytes()), np.uint8) for i in range(n)])
    vs = oracle.ValSet(r.addrs, r.power)
    bh = r.hash32[:3].copy()
    off = np.array([0, 100, 250, n], np.uint32)
    bv = V.BatchVerifier(max_rows=1024)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        for on in (True, False, True):
            bv.set_seal_digest(suffix if on else None)
            exp = expect(oracle, vs, r.addrs, dig if on else r.hash32, sig)
            got = bv.recover_seals(r.hash32, sig)
            check(got, exp, f"suffix on = {on}")
            assert got[2].all() == on and (on or not got[2].any())     # off: the seals recover strangers' addresses
            assert on or got[0].any(axis=1).all()
            ba, bvx, bm, bt = bv.recover_block_seals(bh, off, sig)
            assert (ba == got[0]).all() and (bvx == got[1]).all() and (bm == got[2]).all()
    finally:
        bv.close()


# ---- the block form ---------------------------------------------------------------------------------------------------
def test_block_form_on_the_nine_batch_shapes(oracle):
    import block_stream_cases as S
    import test_gpu_block_seals as BS
    V = _V()
    seq = S.stream()
    bv = V.BatchVerifier(max_rows=65536)
    one = V.BatchVerifier(max_rows=65536)
    try:
        cur = None
        for b in seq:
            if cur is not b.r:
                bv.set_validators(b.r.height, b.r.addrs, b.r.power)
                one.set_validators(b.r.height, b.r.addrs, b.r.power)
                cur = b.r
            vs = oracle.ValSet(b.r.addrs, b.r.power)
            a, v, m, tl = bv.recover_block_seals(b.bh, b.off, b.sig, b.pre)
            assert len(a) == len(v) == len(m) == b.n and len(tl) == len(b.bh), b.name
            rh = BS._rows_hash(b.bh, b.off) if b.n else np.zeros((0, 32), np.uint8)
            ea, ev, em, _ = expect(oracle, vs, b.r.addrs, rh, b.sig, b.pre)
            assert (a == ea).all() and (v == ev).all() and (m == em).all(), b.name
            for k in range(len(b.bh)):
                lo, hi = int(b.off[k]), int(b.off[k + 1])
                te = oracle.tally(vs, ea[lo:hi], em[lo:hi].astype(np.uint8))
                assert fields(tl[k]) == fields(te), f"{b.name}: block {k}"
                assert tl[k].shard_overlap == 0 and tl[k].proposer_rows == 0
            # one recover_seals per block (every block of the small batches, a sample of the large ones)
            blocks = range(len(b.bh)) if len(b.bh) <= 64 else list(range(0, len(b.bh), max(1, len(b.bh) // 24)))
            for k in blocks:
                lo, hi = int(b.off[k]), int(b.off[k + 1])
                pa, pv, pm, pt = one.recover_seals(rh[lo:hi], b.sig[lo:hi], None if b.pre is None else b.pre[lo:hi])
                assert (pa == a[lo:hi]).all() and (pv == v[lo:hi]).all() and (pm == m[lo:hi]).all(), f"{b.name}: block {k}"
                assert fields(pt) == fields(tl[k]), f"{b.name}: block {k}"
            # round trip through the verify sibling
            vm, vt = one.verify_block_seals(b.bh, b.off, b.sig, a, b.pre)
            assert (vm == m).all() and [fields(x) for x in vt] == [fields(x) for x in tl], b.name
    finally:
        bv.close()
        one.close()


def test_block_form_duplicates_empty_blocks_and_moved_seals(oracle):
    V = _V()
    from oracle import workload as W
    r = W.make_round(7, 9701, raw_len=64)          # quorum: 5 of 7
    vs = oracle.ValSet(r.addrs, r.power)
    bh = np.frombuffer(b"".join(oracle.keccak256(b"blk" + bytes([k])) for k in range(5)), np.uint8).reshape(5, 32).copy()
    sg = lambda i, k: np.frombuffer(oracle.sign(r.sks[i], bh[k].tobytes()), np.uint8)
    blocks = [
        [sg(i, 0) for i in (0, 1, 2, 3, 4)],                       # 0: exactly a quorum
        [sg(i, 1) for i in (0, 0, 0, 1, 2, 3)],                    # 1: a duplicate signer counts once: four distinct, no quorum
        [],                                                        # 2: empty
        [sg(i, 3) for i in (0, 1, 2, 3)] + [sg(4, 0)],             # 3: the fifth seal was made for block 0: some other address
        [sg(i, 4) for i in (0, 1, 2, 3, 4, 5, 6)],                 # 4: signer 0 … 4 again: counts in this block too
    ]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.uint32)
    sig = np.array([s for b in blocks for s in b], np.uint8).reshape(-1, 65)
    rh = np.repeat(bh, np.diff(off).astype(np.int64), axis=0)
    ea, ev, em, _ = expect(oracle, vs, r.addrs, rh, sig)
    bv = V.BatchVerifier(max_rows=1024)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        a, v, m, tl = bv.recover_block_seals(bh, off, sig)
        assert (a == ea).all() and (v == ev).all() and (m == em).all()
        for k in range(5):
            lo, hi = int(off[k]), int(off[k + 1])
            assert fields(tl[k]) == fields(oracle.tally(vs, ea[lo:hi], em[lo:hi].astype(np.uint8))), k
        assert [t.has_quorum for t in tl] == [1, 0, 0, 0, 1]
        assert [t.distinct_senders for t in tl] == [5, 4, 0, 4, 7] and tl[1].valid_rows == 6
        moved = int(off[4]) - 1
        assert a[moved].any() and v[moved] == -1 and not m[moved]          # a stranger's address, no member: does not count
        assert tl[2].quorum == tl[0].quorum and tl[2].power == 0
    finally:
        bv.close()


def test_u256_powers_has_quorum_exact(oracle):
    V = _V()
    from oracle import workload as W
    from oracle.semantics import ValidatorManager
    r = W.make_round(3, 9801, raw_len=64)
    w = 2**200 + 7
    powers = [w, w + 1, w]
    vm = ValidatorManager()
    assert vm.init({bytes(a): p for a, p in zip(r.addrs, powers)}) and vm.quorum == 2 * w + 1
    subsets = [(0, 1), (0, 2), (1, 2), (0, 1, 2), (0,), (), (0, 0, 2)]
    bh = np.frombuffer(b"".join(oracle.keccak256(b"u256" + bytes([k])) for k in range(len(subsets))), np.uint8).reshape(-1, 32).copy()
    rows, off = [], [0]
    for b, s in enumerate(subsets):
        rows += [(i, b) for i in s]
        off.append(len(rows))
    sig = np.array([np.frombuffer(oracle.sign(r.sks[i], bytes(bh[b])), np.uint8) for i, b in rows], np.uint8).reshape(-1, 65)
    bv = V.BatchVerifier(max_rows=1024)
    try:
        bv.set_validators_u256(r.height, r.addrs, powers)
        a, v, m, tl = bv.recover_block_seals(bh, off, sig)
        assert m.all() and (v == np.array([i for i, _ in rows], np.int32)).all()
        for b, s in enumerate(subsets):
            want = vm.has_quorum([bytes(r.addrs[i]) for i in s])
            assert bool(tl[b].has_quorum) == want, (s, tl[b].has_quorum)
            assert tl[b].power == sum(powers[i] for i in set(s)) & (2**128 - 1) and tl[b].quorum == vm.quorum & (2**128 - 1)
            lo, hi = off[b], off[b + 1]
            pa, pv, pm, pt = bv.recover_seals(np.repeat(bh[b:b + 1], len(s), axis=0), sig[lo:hi])
            assert fields(pt) == fields(tl[b]) and bool(pt.has_quorum) == want
        assert [bool(t.has_quorum) for t in tl] == [True, False, True, True, False, False, False]
    finally:
        bv.close()


# ---- between a submit and its collect ----------------------------------------------------------------------------------
def test_recover_between_block_submit_and_collect(oracle):
    import block_stream_cases as S
    V = _V()
    seq = S.stream()
    b0, b6 = seq[0], seq[6]            # 64 × 100 with bad rows, 655 × 100: the same validator set
    assert b0.r is b6.r
    r = round_of(513, True)
    bv = V.BatchVerifier(max_rows=65536)
    try:
        bv.set_validators(b0.r.height, b0.r.addrs, b0.r.power)
        vs = oracle.ValSet(b0.r.addrs, b0.r.power)
        exp = expect(oracle, vs, b0.r.addrs, r.hash32, r.seal65, r.pre_flags)      # (strangers to this set: all -1)
        import test_gpu_block_seals as BS
        rh = BS._rows_hash(b0.bh, b0.off)
        exp0 = expect(oracle, vs, b0.r.addrs, rh, b0.sig, b0.pre)
        assert bv.block_seals_submit(*b6.cols()) == b6.n
        assert bv.block_seals_submit(*b0.cols()) == b0.n
        check(bv.recover_seals(r.hash32, r.seal65, r.pre_flags), exp, "two block batches in flight")
        a, v, m, tl = bv.recover_block_seals(b0.bh, b0.off, b0.sig, b0.pre)
        assert (a == exp0[0]).all() and (v == exp0[1]).all() and (m == exp0[2]).all() and m.any()
        assert bv.block_seals_pending()[0] == 2
        S.compare(b6, bv.block_seals_collect())
        S.compare(b0, bv.block_seals_collect())
    finally:
        bv.close()


def test_recover_between_seals_submit_and_collect(oracle):
    V = _V()
    r = round_of(4097, True)
    r2 = round_of(2049, True)
    vs = oracle.ValSet(r.addrs, r.power)
    expv = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=16).astype(bool)
    te = oracle.tally(vs, r.signer20, expv.astype(np.uint8))
    exp2 = expect(oracle, vs, r.addrs, r2.hash32, r2.seal65, r2.pre_flags)
    exp1 = expect(oracle, vs, r.addrs, r.hash32, r.seal65, r.pre_flags)
    bv = V.BatchVerifier(max_rows=8192)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        bv.seals_stage(r.hash32, r.seal65, r.signer20, r.pre_flags)
        bv.seals_submit()
        bv.seals_submit()
        check(bv.recover_seals(r2.hash32, r2.seal65, r2.pre_flags), exp2, "two seal passes in flight")
        check(bv.recover_seals(r.hash32, r.seal65, r.pre_flags), exp1, "two seal passes in flight, own rows")
        for _ in range(2):
            m, t = bv.seals_collect()
            assert (m == expv).all() and fields(t) == fields(te)
    finally:
        bv.close()


def test_arguments_and_timing(oracle):
    V = _V()
    import ctypes as C
    L = V.load_library()
    r = round_of(65, True)
    bv = V.BatchVerifier(max_rows=256)
    try:
        h, s = np.ascontiguousarray(r.hash32), np.ascontiguousarray(r.seal65)
        a = np.full((65, 20), 0xA5, np.uint8)
        v = np.full(65, 77, np.int32)
        m = np.full(2, 7, np.uint64)
        t = V.Tally()
        off = np.array([0, 65], np.uint32)
        untouched = lambda: (a == 0xA5).all() and (v == 77).all() and (m == 7).all() and t.quorum_lo == 0
        p = V._p
        assert L.ibft_recover_seals(bv._h, p(h), p(s), None, 65, p(a), p(v), p(m), C.byref(t)) == -5          # no validator set
        assert L.ibft_recover_block_seals(bv._h, p(h), p(off), 1, p(s), None, p(a), p(v), p(m), C.byref(t)) == -5
        bv.set_validators(r.height, r.addrs, r.power)
        for bad in ((bv._h, None, p(s), None, 65, p(a), p(v), p(m), C.byref(t)), (bv._h, p(h), None, None, 65, p(a), p(v), p(m), C.byref(t)),
                    (bv._h, p(h), p(s), None, 65, None, p(v), p(m), C.byref(t)), (bv._h, p(h), p(s), None, 65, p(a), p(v), None, C.byref(t))):
            assert L.ibft_recover_seals(*bad) == -1
        assert L.ibft_recover_seals(bv._h, p(h), p(s), None, 10**6, p(a), p(v), p(m), C.byref(t)) == -7
        bad_off = np.array([1, 65], np.uint32)
        assert L.ibft_recover_block_seals(bv._h, p(h), p(bad_off), 1, p(s), None, p(a), p(v), p(m), C.byref(t)) == -1
        assert L.ibft_recover_block_seals(bv._h, p(h), p(off), 1, p(s), None, None, p(v), p(m), C.byref(t)) == -1
        assert L.ibft_recover_block_seals(bv._h, p(h), p(np.array([0, 10**6], np.uint32)), 1, p(s), None, p(a), p(v), p(m), C.byref(t)) == -7
        assert untouched()
        assert L.ibft_recover_seals(bv._h, None, None, None, 0, None, None, None, None) == 0                   # n = 0 is legal
        assert untouched()
        # out_vidx and tally may be NULL; kernel timing sees the call as a cold verify pass
        bv.set_kernel_timing(1)
        bv.last_kernel_ms()
        assert L.ibft_recover_seals(bv._h, p(h), p(s), p(r.pre_flags), 65, p(a), None, p(m), None) == 0
        ms, launches = bv.last_kernel_ms()
        assert launches == 1 and 0.0 < ms < 50.0
        vs = oracle.ValSet(r.addrs, r.power)
        exp = expect(oracle, vs, r.addrs, r.hash32, r.seal65, r.pre_flags)
        assert (a == exp[0]).all() and (V.mask_to_bool(m, 65) == exp[2]).all() and (v == 77).all()
        bv.set_kernel_timing(0)
        bv.recover_seals(r.hash32, r.seal65, r.pre_flags)
        assert bv.last_kernel_ms()[1] == 0
    finally:
        bv.close()
