"""GPU: chain sync — the committed seals of many finalized blocks in one call (ibft_verify_block_seals), one HasQuorum per
block.  Oracles: the CPU oracle's verify_seals + tally block by block, and the device's own per-block
is_valid_committed_seal (the call must be bit for bit n_blocks separate ibft_verify_seals calls)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def _V():
    import go_ibft_amd.verifier as V
    return V


def _fields(t):
    return (t.power, t.quorum, t.valid_rows, t.distinct_senders, t.has_quorum)


def _block_hashes(nb: int, seed: int) -> np.ndarray:
    from oracle import binding as B
    return np.array([np.frombuffer(B.proposal_hash(seed.to_bytes(8, "little") + b.to_bytes(8, "little") * 3, b), np.uint8)
                     for b in range(nb)], dtype=np.uint8).reshape(nb, 32)


def _rows_hash(bh, off):
    return np.repeat(bh, np.diff(off).astype(np.int64), axis=0)


def _expect(vs, bh, off, sig, signer, pre=None, digest=None):
    """oracle verdicts and per-block tallies; digest(h) = what a seal over block hash h signs"""
    from oracle import binding as B
    rh = _rows_hash(bh, off)
    if digest is not None:
        rh = np.array([np.frombuffer(digest(bytes(h)), np.uint8) for h in rh], dtype=np.uint8).reshape(-1, 32)
    exp = B.verify_seals(vs, rh, sig, signer, pre, nthreads=16).astype(bool)
    tallies = [B.tally(vs, signer[off[b]:off[b + 1]], exp[off[b]:off[b + 1]]) for b in range(len(bh))]
    return exp, tallies


def _check(bv, vs, bh, off, sig, signer, pre=None, per_block=True, digest=None):
    got, tl = bv.verify_block_seals(bh, off, sig, signer, pre)
    exp, te = _expect(vs, bh, off, sig, signer, pre, digest)
    assert len(tl) == len(bh)
    assert (got == exp).all(), f"verdicts differ at rows {np.nonzero(got != exp)[0][:10]}"
    for b in range(len(bh)):
        assert _fields(tl[b]) == _fields(te[b]), f"block {b}"
        assert tl[b].shard_overlap == 0 and tl[b].proposer_rows == 0
    if per_block:
        rh = _rows_hash(bh, off)
        for b in range(len(bh)):
            lo, hi = int(off[b]), int(off[b + 1])
            m, t = bv.is_valid_committed_seal(rh[lo:hi], sig[lo:hi], signer[lo:hi], None if pre is None else pre[lo:hi])
            assert (m == got[lo:hi]).all(), f"block {b}: per-block call differs"
            assert _fields(t) == _fields(tl[b]) and (t.shard_overlap, t.proposer_rows) == (0, 0), f"block {b}"
    return got, tl


def _sync_fixture(V_: int, nb: int, seed: int, weighted: bool = False):
    """nb blocks signed by one key set, every kind of bad row: seal counts around quorum, corruptions, a stolen seal, a
    non-member, duplicate signers, NIL / BADLEN pre flags, and a seal of block b replayed in block b + 1"""
    from oracle import binding as B, workload as W
    r = W.make_round(V_, seed, raw_len=64, weighted=weighted)
    vs = B.ValSet(r.addrs, r.power)
    bh = _block_hashes(nb, seed)
    outsider = W.validator_key(seed ^ 0x77, 1 << 41)
    out_addr = np.frombuffer(B.address(B.pubkey(outsider)), np.uint8)
    q = int(2 * V_ // 3 + 1)
    rng = np.random.default_rng(seed)
    sigs, signers, pre, off = [], [], [], [0]
    prev = None
    for b in range(nb):
        H = bytes(bh[b])
        count = [q - 1, q, V_, q + 1][b % 4]
        who = rng.permutation(V_)[:count]
        rows = [(B.sign(r.sks[i], H), bytes(r.addrs[i]), 0) for i in who]
        k = b % 12
        if k == 0:   # r = 0
            s, a, _ = rows[0]; rows[0] = (bytes(32) + s[32:], a, 0)
        elif k == 1:  # s = 0
            s, a, _ = rows[0]; rows[0] = (s[:32] + bytes(32) + s[64:], a, 0)
        elif k == 2:  # r ≥ n
            s, a, _ = rows[0]; rows[0] = (N_ORDER.to_bytes(32, "big") + s[32:], a, 0)
        elif k == 3:  # s ≥ n
            s, a, _ = rows[0]; rows[0] = (s[:32] + (N_ORDER + 1).to_bytes(32, "big") + s[64:], a, 0)
        elif k == 4:  # v = 2
            s, a, _ = rows[0]; rows[0] = (s[:64] + b"\x02", a, 0)
        elif k == 5:  # random bytes
            rows[0] = (rng.integers(0, 256, 65, dtype=np.uint8).tobytes(), rows[0][1], 0)
        elif k == 6:  # BADLEN and NIL rows
            rows[0] = (rows[0][0], rows[0][1], _V().ROW_BADLEN)
            rows[1] = (rows[1][0], rows[1][1], _V().ROW_NIL)
        elif k == 7:  # a stolen seal: validator j's seal under From = i
            j = (int(who[0]) + 1) % V_
            rows[0] = (B.sign(r.sks[j], H), bytes(r.addrs[who[0]]), 0)
        elif k == 8:  # a non-member signer with a valid signature of its own
            rows.append((B.sign(outsider, H), bytes(out_addr), 0))
        elif k == 9:  # duplicate signer rows
            rows += [rows[0], rows[1], rows[0]]
        if prev is not None and b % 3 == 1:  # the previous block's seal replayed here: it signs another hash
            rows.insert(len(rows) // 2, prev)
        prev = rows[-1]
        for s, a, p in rows:
            sigs.append(np.frombuffer(s, np.uint8)); signers.append(np.frombuffer(a, np.uint8)); pre.append(p)
        off.append(off[-1] + len(rows))
    return (r, vs, bh, np.array(off, np.uint32), np.array(sigs, np.uint8).reshape(-1, 65),
            np.array(signers, np.uint8).reshape(-1, 20), np.array(pre, np.uint8))


def _device_signed(bv, r, bh, off, who_of_row):
    """seals of every row over its block's hash, signed on the device (ibft_sign_seals) — the large cases"""
    rh = _rows_hash(bh, off)
    sk = np.array([np.frombuffer(r.sks[i], np.uint8) for i in who_of_row], np.uint8).reshape(-1, 32)
    sig, signer, ok = bv.sign_seals(sk, rh)
    assert ok.all()
    return sig, signer


@pytest.mark.parametrize("weighted", [False, True])
def test_64_blocks_of_100_validators_with_every_bad_row(weighted):
    r, vs, bh, off, sig, signer, pre = _sync_fixture(100, 64, 11 + weighted, weighted=weighted)
    bv = _V().BatchVerifier(max_rows=65536)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        got, tl = _check(bv, vs, bh, off, sig, signer, pre)
        # the fixture has what it claims: blocks just short of and at quorum, invalid rows of every kind
        hq = [t.has_quorum for t in tl]
        assert 0 < sum(hq) < len(tl) and (~got).sum() >= 64
    finally:
        bv.close()


def test_replayed_seal_is_invalid_in_the_next_block():
    from oracle import binding as B, workload as W
    r = W.make_round(4, 21, raw_len=64)
    bh = _block_hashes(2, 21)
    s0 = [B.sign(r.sks[i], bytes(bh[0])) for i in range(4)]
    sig = np.frombuffer(b"".join(s0 + s0[:1]), np.uint8).reshape(-1, 65)   # block 1 = validator 0's seal of block 0
    signer = np.concatenate([r.addrs, r.addrs[:1]])
    bv = _V().BatchVerifier(max_rows=1024)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        got, tl = bv.verify_block_seals(bh, [0, 4, 5], sig, signer)
        assert got.tolist() == [True] * 4 + [False]
        assert (tl[0].has_quorum, tl[0].valid_rows, tl[1].has_quorum, tl[1].valid_rows) == (1, 4, 0, 0)
    finally:
        bv.close()


def test_ragged_layouts():
    """empty blocks, one-row blocks, boundaries off the 64-row verdict words; one block = the whole batch equals
    ibft_verify_seals exactly"""
    from oracle import binding as B, workload as W
    r = W.make_round(100, 31, raw_len=64, byzantine=True)
    vs = B.ValSet(r.addrs, r.power)
    sizes = [0, 1, 0, 0, 3, 63, 64, 65, 1, 0, 130, 7, 0, 200, 1, 1, 0]
    nb = len(sizes)
    bh = _block_hashes(nb, 31)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    rng = np.random.default_rng(31)
    who = rng.integers(0, 100, int(off[-1]))
    rh = _rows_hash(bh, off)
    sig = np.array([np.frombuffer(B.sign(r.sks[i], bytes(h)), np.uint8) for i, h in zip(who, rh)], np.uint8).reshape(-1, 65)
    signer = r.addrs[who].copy()
    bad = rng.random(len(who)) < 0.15
    sig[bad, 64] = 2
    bv = _V().BatchVerifier(max_rows=65536)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        _, tl = _check(bv, vs, bh, off, sig, signer)
        for b in np.nonzero(np.array(sizes) == 0)[0]:
            assert (tl[b].has_quorum, tl[b].valid_rows, tl[b].power) == (0, 0, 0)
        # one block holding every row: exactly ibft_verify_seals
        one_h = bh[:1]
        rh1 = np.repeat(one_h, len(who), axis=0)
        sig1 = np.array([np.frombuffer(B.sign(r.sks[i], bytes(one_h[0])), np.uint8) for i in who], np.uint8).reshape(-1, 65)
        got, t1 = bv.verify_block_seals(one_h, [0, len(who)], sig1, signer)
        m, t = bv.is_valid_committed_seal(rh1, sig1, signer)
        assert (got == m).all() and _fields(t1[0]) == _fields(t) and t.has_quorum == 1
        # no rows at all
        got, t0 = bv.verify_block_seals(bh[:3], [0, 0, 0, 0], np.zeros((0, 65), np.uint8), np.zeros((0, 20), np.uint8))
        assert len(got) == 0 and [x.has_quorum for x in t0] == [0, 0, 0] and t0[0].quorum == vs.quorum
    finally:
        bv.close()


def test_one_block_of_65536_rows():
    from oracle import binding as B, workload as W
    r = W.make_round(1024, 41, raw_len=64)
    vs = B.ValSet(r.addrs, r.power)
    bh = _block_hashes(1, 41)
    off = np.array([0, 65536], np.uint32)
    bv = _V().BatchVerifier(max_rows=65536)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        who = np.arange(65536) % 1024
        sig, signer = _device_signed(bv, r, bh, off, who)
        sig[::97, 0] ^= 0x55      # some rows invalid; every validator still has valid rows
        _check(bv, vs, bh, off, sig, signer, per_block=False)
        m, t = bv.is_valid_committed_seal(_rows_hash(bh, off), sig, signer)
        got, tl = bv.verify_block_seals(bh, off, sig, signer)
        assert (got == m).all() and _fields(tl[0]) == _fields(t)
    finally:
        bv.close()


def test_16384_blocks_of_4():
    from oracle import binding as B, workload as W
    r = W.make_round(4, 43, raw_len=64)
    vs = B.ValSet(r.addrs, r.power)
    nb = 16384
    bh = np.frombuffer(b"".join(B.keccak256(b"blk" + b.to_bytes(4, "little")) for b in range(nb)), np.uint8).reshape(nb, 32)
    off = (np.arange(nb + 1) * 4).astype(np.uint32)
    bv = _V().BatchVerifier(max_rows=65536)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        sig, signer = _device_signed(bv, r, bh, off, np.arange(nb * 4) % 4)
        rng = np.random.default_rng(43)
        drop = rng.integers(0, 4 * nb, 3000)
        sig[drop, 64] = 3          # some blocks fall below quorum (3 of 4)
        got, tl = _check(bv, vs, bh, off, sig, signer, per_block=False)
        assert 0 < sum(t.has_quorum for t in tl) < nb
        for b in rng.integers(0, nb, 16):   # a sample of blocks through the per-block call
            lo, hi = int(off[b]), int(off[b + 1])
            m, t = bv.is_valid_committed_seal(_rows_hash(bh, off)[lo:hi], sig[lo:hi], signer[lo:hi])
            assert (m == got[lo:hi]).all() and _fields(t) == _fields(tl[b])
    finally:
        bv.close()


def test_u256_powers_quorum_exact_at_the_boundary():
    """powers w, w + 1, w (w ≈ 2^200): quorum = 2w + 1 exactly — {A, B} is a quorum, {A, C} one short of it"""
    from oracle import binding as B, workload as W
    from oracle.semantics import ValidatorManager
    r = W.make_round(3, 51, raw_len=64)
    w = 2**200 + 7
    powers = [w, w + 1, w]
    vm = ValidatorManager()
    assert vm.init({bytes(a): p for a, p in zip(r.addrs, powers)}) and vm.quorum == 2 * w + 1
    subsets = [(0, 1), (0, 2), (1, 2), (0, 1, 2), (0,), (), (0, 0, 2)]
    bh = _block_hashes(len(subsets), 51)
    rows, off = [], [0]
    for b, s in enumerate(subsets):
        rows += [(i, b) for i in s]
        off.append(len(rows))
    sig = np.array([np.frombuffer(B.sign(r.sks[i], bytes(bh[b])), np.uint8) for i, b in rows], np.uint8).reshape(-1, 65)
    signer = np.array([r.addrs[i] for i, _ in rows], np.uint8).reshape(-1, 20)
    bv = _V().BatchVerifier(max_rows=1024)
    try:
        bv.set_validators_u256(r.height, r.addrs, powers)
        got, tl = bv.verify_block_seals(bh, off, sig, signer)
        assert got.all()
        for b, s in enumerate(subsets):
            want = vm.has_quorum([bytes(r.addrs[i]) for i in s])
            exact = sum(powers[i] for i in set(s))
            assert bool(tl[b].has_quorum) == want, (s, tl[b].has_quorum)
            assert tl[b].power == exact & (2**128 - 1) and tl[b].quorum == vm.quorum & (2**128 - 1)
            m, t = bv.is_valid_committed_seal(np.repeat(bh[b:b + 1], len(s), axis=0), sig[off[b]:off[b + 1]],
                                              signer[off[b]:off[b + 1]])
            assert _fields(t) == _fields(tl[b])
        assert [bool(t.has_quorum) for t in tl] == [True, False, True, True, False, False, False]
    finally:
        bv.close()


def test_pubkey_cache_second_call_is_warm():
    V = _V()
    r, vs, bh, off, sig, signer, pre = _sync_fixture(100, 16, 61)
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=65536)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        g1, t1 = _check(bv, vs, bh, off, sig, signer, pre, per_block=False)
        tables, warm0, _ = bv.cache_stats()
        assert tables > 0
        g2, t2 = bv.verify_block_seals(bh, off, sig, signer, pre)
        _, warm1, _ = bv.cache_stats()
        assert warm1 == warm0 + 1
        assert (g1 == g2).all() and [_fields(t) for t in t1] == [_fields(t) for t in t2]
    finally:
        bv.close()


def test_keccak_suffix_seal_digest():
    from oracle import binding as B, workload as W
    r = W.make_round(100, 71, raw_len=64)
    vs = B.ValSet(r.addrs, r.power)
    nb = 12
    bh = _block_hashes(nb, 71)
    off = (np.arange(nb + 1) * 70).astype(np.uint32)
    digest = lambda h: B.keccak256(h + b"\x02")
    who = np.arange(70 * nb) % 100
    rh = _rows_hash(bh, off)
    sig = np.array([np.frombuffer(B.sign(r.sks[i], digest(bytes(h)) if k % 7 else bytes(h)), np.uint8)
                    for k, (i, h) in enumerate(zip(who, rh))], np.uint8).reshape(-1, 65)   # every 7th signs the bare hash
    signer = r.addrs[who].copy()
    bv = _V().BatchVerifier(max_rows=4096)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        bv.set_seal_digest(b"\x02")
        got, _ = _check(bv, vs, bh, off, sig, signer, digest=digest)
        assert 0 < (~got).sum() < len(got)
    finally:
        bv.close()


def test_following_calls_see_a_clean_context():
    """after a block call: ibft_verify_seals and ibft_tally on other batches still equal the oracle (no stale work-mask bits)"""
    from oracle import binding as B, workload as W
    r2 = W.make_round(100, 82, byzantine=True)
    r, vs, bh, off, sig, signer, pre = _sync_fixture(100, 20, 81)
    bv = _V().BatchVerifier(max_rows=65536)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        _check(bv, vs, bh, off, sig, signer, pre, per_block=False)
        bv.set_validators(r2.height, r2.addrs, r2.power)
        vs2 = B.ValSet(r2.addrs, r2.power)
        for n in (100, 37, 1000):
            idx = np.arange(n) % r2.n
            m, t = bv.is_valid_committed_seal(r2.hash32[idx], r2.seal65[idx], r2.signer20[idx], r2.pre_flags[idx])
            e = B.verify_seals(vs2, r2.hash32[idx], r2.seal65[idx], r2.signer20[idx], r2.pre_flags[idx]).astype(bool)
            te = B.tally(vs2, r2.signer20[idx], e)
            assert (m == e).all() and _fields(t) == _fields(te)
            tq = bv.has_quorum(r2.signer20[idx], e)
            assert _fields(tq) == _fields(te)
        # and the staged batch is the block call's rows, as after ibft_verify_seals
        bv.set_validators(r.height, r.addrs, r.power)
        got, _ = bv.verify_block_seals(bh, off, sig, signer, pre)
        m, t = bv.seals_run()
        assert len(m) == len(got) and (m == got).all()
    finally:
        bv.close()


@pytest.mark.parametrize("entry", ["block", "seals"])
def test_pipelined_pass_in_flight(entry):
    """a submitted, uncollected pass survives the call and is collected intact — the same for ibft_verify_seals"""
    from oracle import binding as B, workload as W
    rx = W.make_round(200, 91, byzantine=True)
    r, vs, bh, off, sig, signer, pre = _sync_fixture(200, 8, 91)
    ex = B.verify_seals(vs, rx.hash32, rx.seal65, rx.signer20, rx.pre_flags).astype(bool)
    tx = B.tally(vs, rx.signer20, ex)
    bv = _V().BatchVerifier(max_rows=65536)
    try:
        assert r.addrs.tobytes() == rx.addrs.tobytes()   # one key set: one validator set for both
        bv.set_validators(r.height, r.addrs, r.power)
        bv.seals_stage(rx.hash32, rx.seal65, rx.signer20, rx.pre_flags)
        bv.seals_submit()
        if entry == "block":
            _check(bv, vs, bh, off, sig, signer, pre, per_block=False)
        else:
            rh = _rows_hash(bh, off)
            m, t = bv.is_valid_committed_seal(rh, sig, signer, pre)
            assert (m == B.verify_seals(vs, rh, sig, signer, pre).astype(bool)).all()
        mx, t = bv.seals_collect()
        assert (mx == ex).all() and _fields(t) == _fields(tx)
    finally:
        bv.close()


def test_one_verdict_launch_over_all_blocks():
    """655 blocks × 100 seals: the dispatch AUTO picks for 65 500 rows (one lane per signature), not the two-wavefront form
    a 100-row call gets"""
    from oracle import binding as B, workload as W
    r = W.make_round(100, 101, raw_len=64)
    nb = 655
    bh = np.frombuffer(b"".join(B.keccak256(b"h" + b.to_bytes(4, "little")) for b in range(nb)), np.uint8).reshape(nb, 32)
    off = (np.arange(nb + 1) * 100).astype(np.uint32)
    bv = _V().BatchVerifier(max_rows=65536)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        sig, signer = _device_signed(bv, r, bh, off, np.arange(nb * 100) % 100)
        bv.is_valid_committed_seal(_rows_hash(bh, off)[:100], sig[:100], signer[:100])
        assert bv.last_dispatch()[0] == 128
        got, tl = bv.verify_block_seals(bh, off, sig, signer)
        assert bv.last_dispatch()[0] == 1
        assert got.all() and all(t.has_quorum == 1 and t.distinct_senders == 100 for t in tl)
    finally:
        bv.close()


def test_error_codes_leave_buffers_untouched():
    from oracle import workload as W
    V = _V()
    L = V.load_library()
    r, vs, bh, off, sig, signer, pre = _sync_fixture(100, 4, 111)
    n = int(off[-1])

    def call(bv, off_, nb, n_rows=None):
        mask = np.full(max(1, ((n_rows or n) + 63) // 64), 0xA5A5A5A5A5A5A5A5, np.uint64)
        tal = (V.Tally * max(nb, 1))()
        for t in tal:
            t.power_lo = 0x1234
        o = np.ascontiguousarray(off_, np.uint32)
        rc = L.ibft_verify_block_seals(bv._h, V._p(bh), V._p(o), nb, V._p(sig), V._p(signer), None, V._p(mask), tal)
        assert (mask == 0xA5A5A5A5A5A5A5A5).all() and all(t.power_lo == 0x1234 for t in tal)
        return rc

    assert L.ibft_verify_block_seals(None, V._p(bh), V._p(off), 4, V._p(sig), V._p(signer), None, None, None) == -1
    fresh = V.BatchVerifier(max_rows=1024)
    small = V.BatchVerifier(max_rows=64)
    try:
        assert call(fresh, off, 4) == -5                                     # IBFT_E_NOVALSET
        fresh.set_validators(r.height, r.addrs, r.power)
        bad = off.copy(); bad[0] = 1
        assert call(fresh, bad, 4) == -1                                     # does not start at 0
        bad = off.copy(); bad[2] = bad[1] - 1
        assert call(fresh, bad, 4) == -1                                     # goes down
        small.set_validators(r.height, r.addrs, r.power)
        assert n > 64 and call(small, off, 4) == -7                          # IBFT_E_TOOBIG: rows
        assert call(small, np.zeros(66, np.uint32), 65, 1) == -7             # IBFT_E_TOOBIG: blocks
        got, _ = fresh.verify_block_seals(bh, off, sig, signer, pre)        # and the context still works
        assert (got == _expect(vs, bh, off, sig, signer, pre)[0]).all()
    finally:
        fresh.close()
        small.close()


@pytest.mark.parametrize("suffix", [None, b"\x02"])
@pytest.mark.parametrize("sizes", [[0, 5, 2, 0, 0, 3, 0], [40, 0, 30]])
def test_synchronous_spread_equals_one_call_per_block(sizes, suffix):
    """the four synchronous calls under one set — hashes and proposals, verify and recover — bit for bit one
    is_valid_committed_seal / recover_seals call per block: empty blocks in front, in the middle and at the end, a block
    boundary inside a verdict word and across one, under the identity convention and under keccak256(hash ‖ 0x02)"""
    from oracle import binding as B, workload as W
    r = W.make_round(7, 91, raw_len=64)
    nb = len(sizes)
    raws = [b"block %d of the spread test" % b * (b + 1) for b in range(nb)]
    rounds = list(range(3, 3 + nb))
    bh = np.array([np.frombuffer(B.proposal_hash(raw, rnd), np.uint8) for raw, rnd in zip(raws, rounds)], np.uint8).reshape(nb, 32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(off[-1])
    assert n <= 70
    digest = (lambda h: h) if suffix is None else (lambda h: B.keccak256(h + suffix))
    rh = _rows_hash(bh, off)
    who = np.arange(n) % 7
    # every 6th row signs something else than the convention says: invalid under its claimed signer, a stranger when recovered
    sig = np.array([np.frombuffer(B.sign(r.sks[i], digest(bytes(h)) if k % 6 != 5 else B.keccak256(bytes(h) + b"\x09")), np.uint8)
                    for k, (i, h) in enumerate(zip(who, rh))], np.uint8).reshape(-1, 65)
    signer = r.addrs[who].copy()
    bv = _V().BatchVerifier(max_rows=1024)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        bv.set_seal_digest(suffix)
        # the reference, once: one call per block
        ref_v, ref_r = [], []
        for b in range(nb):
            lo, hi = int(off[b]), int(off[b + 1])
            ref_v.append(bv.is_valid_committed_seal(rh[lo:hi], sig[lo:hi], signer[lo:hi]))
            ref_r.append(bv.recover_seals(rh[lo:hi], sig[lo:hi]) if hi > lo else None)
        v_hash = bv.verify_block_seals(bh, off, sig, signer)
        v_raw = bv.verify_block_seals_raw(raws, rounds, off, sig, signer)
        r_hash = bv.recover_block_seals(bh, off, sig)
        r_raw = bv.recover_block_seals_raw(raws, rounds, off, sig)
        assert (v_raw[2] == bh).all() and (r_raw[4] == bh).all()
        for name, (got, tl) in (("verify_block_seals", v_hash), ("verify_block_seals_raw", v_raw[:2])):
            assert len(got) == n and len(tl) == nb
            for b in range(nb):
                lo, hi = int(off[b]), int(off[b + 1])
                m, t = ref_v[b]
                assert (got[lo:hi] == m).all(), f"{name}: block {b}"
                assert _fields(tl[b]) == _fields(t) and (tl[b].shard_overlap, tl[b].proposer_rows) == (0, 0), f"{name}: block {b}"
        for name, (sg, vi, got, tl) in (("recover_block_seals", r_hash), ("recover_block_seals_raw", r_raw[:4])):
            assert len(got) == n and len(tl) == nb and sg.shape == (n, 20) and vi.shape == (n,)
            for b in range(nb):
                lo, hi = int(off[b]), int(off[b + 1])
                if hi == lo:   # no rows: the empty tally of the set
                    assert _fields(tl[b]) == _fields(ref_v[b][1]) and tl[b].has_quorum == 0, f"{name}: block {b}"
                    continue
                sg1, vi1, m1, t1 = ref_r[b]
                assert (sg[lo:hi] == sg1).all() and (vi[lo:hi] == vi1).all() and (got[lo:hi] == m1).all(), f"{name}: block {b}"
                assert _fields(tl[b]) == _fields(t1), f"{name}: block {b}"
        # the cases hold what they claim: valid and invalid rows, blocks with and without quorum
        assert 0 < v_hash[0].sum() < n and (v_hash[0] == r_hash[2]).all()
        assert {t.has_quorum for t in v_hash[1]} == {0, 1}
    finally:
        bv.close()
