"""GPU: chain sync across validator-set changes — a family of validator sets on the context (ibft_set_validator_sets) and the
block calls that judge block b under set block_set[b] (ibft_verify_block_seals_sets / ibft_recover_block_seals_sets).
Oracles: (1) the CPU oracle block by block, verify_seals + tally under ValSet(set of that block) (recover: recover_address
and the position in the set's list); (2) the device's own per-set route on a second context — set_validators(set k) +
verify_block_seals / recover_block_seals over the blocks of set k, for every k in turn.  Everything compared is a verdict bit
or an integer: equality is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
E_INVAL, E_NOVALSET, E_POWER, E_TOOBIG = -1, -5, -6, -7


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


class Fam:
    """a sliding family over one key pool: set k = validators k·step … k·step + V of the pool, every address with a power that
    DIFFERS from set to set"""

    def __init__(self, pool: int, V_: int, step: int, n_sets: int, seed: int, big: bool = False):
        from oracle import workload as W
        assert (n_sets - 1) * step + V_ <= pool
        self.r = W.make_round(pool, seed, raw_len=64, weighted=True)
        self.idx = [list(range(k * step, k * step + V_)) for k in range(n_sets)]
        base = (1 << 127) if big else 0    # big: sums of a set go beyond 2^128
        self.power = [[base + int(self.r.power[i]) + 3 * k + (i % 5) for i in ix] for k, ix in enumerate(self.idx)]
        self.big = big

    def addrs(self, k):
        return self.r.addrs[self.idx[k]].copy()

    def sets(self):
        return [(1000 + k, self.addrs(k), self.power[k]) for k in range(len(self.idx))]

    def install(self, bv):
        (bv.set_validator_sets_u256 if self.big else bv.set_validator_sets)(self.sets())

    def install_single(self, bv, k):
        if self.big:
            bv.set_validators_u256(1000 + k, self.addrs(k), self.power[k])
        else:
            bv.set_validators(1000 + k, self.addrs(k), self.power[k])

    def valset(self, k):
        from oracle import binding as B
        # (the oracle's powers are u64: under a `big` family it answers membership only, the sums are done in Python)
        return B.ValSet(self.addrs(k), np.ones(len(self.idx[k]), np.uint64) if self.big else np.array(self.power[k], np.uint64))

    def tally_big(self, k, signer, bits):
        """HasQuorum of one block under set k in exact integers (validator_manager.go:77-96, 128-136)"""
        mem = {bytes(a): p for a, p in zip(self.addrs(k), self.power[k])}
        seen = {bytes(a) for a, ok in zip(signer, bits) if ok and bytes(a) in mem}
        power, quorum = sum(mem[a] for a in seen), 2 * sum(self.power[k]) // 3 + 1
        return (power, quorum, int(np.sum(bits)), len(seen), int(power >= quorum))


def _fixture(f: Fam, bset, seed: int):
    """len(bset) blocks, block b signed by members of set bset[b] — every bad-row kind of the single-set block tests
    (corruptions, stolen seal, outsider, duplicates, pre flags, a replay into the next block) plus the family's own: a
    validator of ANOTHER set of the family signing this block correctly"""
    from oracle import binding as B, workload as W
    V = _V()
    r = f.r
    nb = len(bset)
    bh = _block_hashes(nb, seed)
    outsider = W.validator_key(seed ^ 0x77, 1 << 41)
    out_addr = B.address(B.pubkey(outsider))
    rng = np.random.default_rng(seed)
    sigs, signers, pre, off = [], [], [], [0]
    prev = None
    for b in range(nb):
        ix = f.idx[bset[b]]
        V_ = len(ix)
        q = int(2 * V_ // 3 + 1)
        H = bytes(bh[b])
        count = max(2, [q - 1, q, V_, min(V_, q + 1)][b % 4])
        who = [ix[j] for j in rng.permutation(V_)[:count]]
        rows = [(B.sign(r.sks[i], H), bytes(r.addrs[i]), 0) for i in who]
        k = b % 13
        s, a, _ = rows[0]
        if k == 0:
            rows[0] = (bytes(32) + s[32:], a, 0)                                   # r = 0
        elif k == 1:
            rows[0] = (s[:32] + bytes(32) + s[64:], a, 0)                           # s = 0
        elif k == 2:
            rows[0] = (N_ORDER.to_bytes(32, "big") + s[32:], a, 0)                  # r ≥ n
        elif k == 3:
            rows[0] = (s[:32] + (N_ORDER + 1).to_bytes(32, "big") + s[64:], a, 0)   # s ≥ n
        elif k == 4:
            rows[0] = (s[:64] + b"\x02", a, 0)                                      # v = 2
        elif k == 5:
            rows[0] = (rng.integers(0, 256, 65, dtype=np.uint8).tobytes(), a, 0)    # random bytes
        elif k == 6:
            rows[0] = (rows[0][0], rows[0][1], V.ROW_BADLEN)
            rows[1] = (rows[1][0], rows[1][1], V.ROW_NIL)
        elif k == 7:                                                                # a stolen seal
            j = ix[(ix.index(who[0]) + 1) % V_]
            rows[0] = (B.sign(r.sks[j], H), bytes(r.addrs[who[0]]), 0)
        elif k == 8:                                                                # a non-member of every set
            rows.append((B.sign(outsider, H), out_addr, 0))
        elif k == 9:                                                                # duplicate signer rows
            rows += [rows[0], rows[1], rows[0]]
        elif k in (10, 11):                                                         # in the family, not in this block's set
            others = [i for i in range(r.n) if i not in ix and any(i in o for o in f.idx)]
            for i in others[:1 + k % 2] + others[-1:]:
                rows.insert(1, (B.sign(r.sks[i], H), bytes(r.addrs[i]), 0))
        if prev is not None and b % 3 == 1:                                         # the previous block's seal replayed here
            rows.insert(len(rows) // 2, prev)
        prev = rows[-1]
        for s, a, p in rows:
            sigs.append(np.frombuffer(s, np.uint8)); signers.append(np.frombuffer(a, np.uint8)); pre.append(p)
        off.append(off[-1] + len(rows))
    return (bh, np.array(off, np.uint32), np.array(sigs, np.uint8).reshape(-1, 65), np.array(signers, np.uint8).reshape(-1, 20),
            np.array(pre, np.uint8))


def _rows_of(off, blocks):
    return np.concatenate([np.arange(off[b], off[b + 1]) for b in blocks] + [np.zeros(0, np.int64)]).astype(np.int64)


def _sub(off, blocks):
    return np.concatenate([[0], np.cumsum([int(off[b + 1] - off[b]) for b in blocks])]).astype(np.uint32)


def _expect_cpu(f, bset, bh, off, sig, signer, pre, digest=None, flags=0, recover=False):
    """oracle 1 → (bits, per-block tally fields, [recovered address column, index column])"""
    from oracle import binding as B
    n, nb = len(sig), len(bh)
    rh = _rows_hash(bh, off)
    if digest is not None:
        rh = np.array([np.frombuffer(digest(bytes(h)), np.uint8) for h in rh], np.uint8).reshape(-1, 32)
    bits = np.zeros(n, bool)
    tallies = [None] * nb
    for k in sorted(set(int(s) for s in bset)):
        vs = f.valset(k)
        blocks = [b for b in range(nb) if bset[b] == k]
        rows = _rows_of(off, blocks)
        if len(rows):
            bits[rows] = B.verify_seals(vs, rh[rows], sig[rows], signer[rows], None if pre is None else pre[rows], flags,
                                        nthreads=16).astype(bool)
        for b in blocks:
            sl = slice(int(off[b]), int(off[b + 1]))
            tallies[b] = f.tally_big(k, signer[sl], bits[sl]) if f.big else _fields(B.tally(vs, signer[sl], bits[sl]))
    if not recover:
        return bits, tallies
    who = np.zeros((n, 20), np.uint8)
    vidx = np.full(n, -1, np.int32)
    set_of_row = np.repeat(np.asarray(bset), np.diff(off).astype(np.int64))
    pos = [{bytes(f.r.addrs[i]): j for j, i in enumerate(ix)} for ix in f.idx]
    for i in range(n):
        a = None if (pre is not None and pre[i]) else B.recover_address(bytes(rh[i]), bytes(sig[i]), flags)
        if a is not None:
            who[i] = np.frombuffer(a, np.uint8)
            vidx[i] = pos[set_of_row[i]].get(a, -1)
    return bits, tallies, who, vidx


def _check(bv, ref, f, bset, bh, off, sig, signer, pre=None, cpu=True, digest=None, flags=0, recover=True):
    """the _sets calls on bv against both oracles; ref: a second context (same flags, same convention) for the per-set route"""
    bset = np.asarray(bset, np.uint32)
    nb = len(bh)
    got, tl = bv.verify_block_seals_sets(bh, off, bset, sig, signer, pre)
    assert bv.seals_rows()[0] == 0                        # no resident batch after a _sets call
    gt = [_fields(t) for t in tl]
    assert all(t.shard_overlap == 0 and t.proposer_rows == 0 for t in tl)
    if recover:
        who, vidx, rbits, rtl = bv.recover_block_seals_sets(bh, off, bset, sig, pre)
        assert bv.seals_rows()[0] == 0
        # out_signer20 fed back as signer20 gives the recover form's bits and tallies (the defining property of the bare calls)
        fb, ftl = bv.verify_block_seals_sets(bh, off, bset, sig, who, pre)
        assert (fb == rbits).all() and [_fields(t) for t in ftl] == [_fields(t) for t in rtl]
    if cpu:
        exp = _expect_cpu(f, bset, bh, off, sig, signer, pre, digest, flags, recover)
        bad = np.nonzero(got != exp[0])[0]
        assert len(bad) == 0, f"verdicts differ from the CPU oracle at rows {bad[:10]}"
        for b in range(nb):
            want = exp[1][b]
            if f.big:   # the oracle's tally is exact; the entry carries the low 128 bits
                want = (want[0] & (2**128 - 1), want[1] & (2**128 - 1)) + want[2:]
            assert gt[b] == want, f"block {b} (set {bset[b]})"
        if recover:
            assert (who == exp[2]).all() and (vidx == exp[3]).all()
    # oracle 2: the per-set route of the device itself
    for k in sorted(set(int(s) for s in bset)):
        blocks = [b for b in range(nb) if bset[b] == k]
        rows = _rows_of(off, blocks)
        f.install_single(ref, k)
        so = _sub(off, blocks)
        p = None if pre is None else pre[rows]
        m, t = ref.verify_block_seals(bh[blocks], so, sig[rows], signer[rows], p)
        assert (m == got[rows]).all(), f"set {k}: bits differ from the per-set call"
        assert [_fields(x) for x in t] == [gt[b] for b in blocks], f"set {k}: tallies differ from the per-set call"
        if recover:
            w2, v2, m2, t2 = ref.recover_block_seals(bh[blocks], so, sig[rows], p)
            assert (w2 == who[rows]).all() and (v2 == vidx[rows]).all() and (m2 == rbits[rows]).all(), f"set {k}: recover form"
            assert [_fields(x) for x in t2] == [_fields(rtl[b]) for b in blocks]
    return got, tl


def _pair(max_rows=65536, flags=0):
    V = _V()
    return V.BatchVerifier(max_rows=max_rows, flags=flags), V.BatchVerifier(max_rows=max_rows, flags=flags)


@pytest.mark.parametrize("V_,pool,n_sets", [(4, 40, 32), (100, 164, 64)])
@pytest.mark.parametrize("change", ["every block", "every 5 blocks", "never"])
def test_sliding_family_with_every_bad_row(V_, pool, n_sets, change):
    f = Fam(pool, V_, 1, n_sets, 300 + V_)
    nb = 64
    bset = {"every block": [b % n_sets for b in range(nb)], "every 5 blocks": [(b // 5) % n_sets for b in range(nb)],
            "never": [3] * nb}[change]
    bh, off, sig, signer, pre = _fixture(f, bset, 301 + V_)
    bv, ref = _pair()
    try:
        f.install(bv)
        assert bv.validator_sets_info()[:2] == (n_sets, n_sets - 1 + V_)
        got, tl = _check(bv, ref, f, bset, bh, off, sig, signer, pre)
        hq = [t.has_quorum for t in tl]
        assert 0 < sum(hq) < nb and (~got).sum() >= nb // 2   # the fixture has what it claims
        # the same address has another power in another set: the quorums of two sets differ
        assert len({t.quorum for t in tl}) > 1 or change == "never"
    finally:
        bv.close(); ref.close()


def test_validator_that_left_and_indices_that_moved():
    """what judging against the union alone would get wrong"""
    from oracle import binding as B, workload as W
    r = W.make_round(6, 410, raw_len=64)
    a = [r.addrs[i] for i in range(6)]
    sets = [(1, np.array([a[0], a[1], a[2], a[3]]), [1, 1, 1, 1]),        # quorum 3
            (2, np.array([a[3], a[2], a[1], a[4]]), [1, 1, 1, 1]),        # a[0] left; a[1], a[2], a[3] moved; a[4] joined
            (3, np.array([a[5], a[0], a[5]]), [7, 1, 9])]                 # a repeated address: first position, last power
    bh = _block_hashes(5, 410)
    plan = [(1, [0, 1, 2]),      # block of set 1 signed by a[0] (left), a[1], a[2]: only two members → no quorum
            (0, [0, 1, 2]),      # the same signers in a block of their own set: quorum
            (1, [0]),            # the one who left, alone
            (2, [5, 0, 3]),      # a[3] is in the family, not in set 2
            (0, [4, 3, 3])]      # a[4] not yet in set 0; a duplicate
    bset = [p[0] for p in plan]
    off = np.concatenate([[0], np.cumsum([len(p[1]) for p in plan])]).astype(np.uint32)
    who_rows = [(i, b) for b, p in enumerate(plan) for i in p[1]]
    sig = np.array([np.frombuffer(B.sign(r.sks[i], bytes(bh[b])), np.uint8) for i, b in who_rows], np.uint8).reshape(-1, 65)
    signer = np.array([a[i] for i, _ in who_rows], np.uint8).reshape(-1, 20)
    bv = _V().BatchVerifier(max_rows=1024)
    try:
        bv.set_validator_sets(sets)
        assert bv.validator_sets_info()[:2] == (3, 6)
        got, tl = bv.verify_block_seals_sets(bh, off, bset, sig, signer)
        who, vidx, rb, rtl = bv.recover_block_seals_sets(bh, off, bset, sig)
        assert got.tolist() == rb.tolist() == [False, True, True,  True, True, True,  False,  True, True, False,  False, True, True]
        assert (who == signer).all()                               # every address is delivered, a non-member's of the set too
        assert vidx.tolist() == [-1, 2, 1,  0, 1, 2,  -1,  0, 1, -1,  -1, 3, 3]
        for t in (tl, rtl):
            assert [_fields(x) for x in t] == [(2, 3, 2, 2, 0), (3, 3, 3, 3, 1), (0, 3, 0, 0, 0), (10, 7, 2, 2, 1), (1, 3, 2, 1, 0)]
    finally:
        bv.close()


def _ragged_offsets(total, seed, lo, hi, wide=0, empties=4):
    """block sizes in [lo, hi] (none of them a multiple of 64: boundaries fall inside verdict words), a few empty blocks, one
    block of `wide` rows, summing to exactly `total`"""
    rng = np.random.default_rng(seed)
    sizes = [wide] if wide else []
    while sum(sizes) < total:
        sizes.append(int(rng.integers(lo, hi + 1)) | 1)
    sizes[-1] -= sum(sizes) - total
    if sizes[-1] <= 0:
        sizes.pop()
        sizes[-1] += total - sum(sizes)
    for _ in range(empties):
        sizes.insert(int(rng.integers(0, len(sizes) + 1)), 0)
    assert sum(sizes) == total and min(s for s in sizes if s) > 0
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)


def _device_rows(bv, f, bset, bh, off, seed):
    """every row signed on the device by a member of its block's set — except every 7th row, signed by a validator of the
    family that is NOT in the block's set, and every 11th, corrupted"""
    rng = np.random.default_rng(seed)
    n = int(off[-1])
    set_of_row = np.repeat(np.asarray(bset), np.diff(off).astype(np.int64))
    V_ = len(f.idx[0])
    who = np.array([f.idx[s][j] for s, j in zip(set_of_row, rng.integers(0, V_, n))], np.int64)
    stray = np.arange(n) % 7 == 3
    who[stray] = (who[stray] + V_ + 1) % f.r.n        # pool = the union, step 1: V + 1 further on is outside the set or wraps into it
    sk = np.array([np.frombuffer(f.r.sks[i], np.uint8) for i in who], np.uint8).reshape(-1, 32)
    sig, signer, ok = bv.sign_seals(sk, _rows_hash(bh, off))
    assert ok.all()
    sig = sig.copy()
    sig[np.arange(n) % 11 == 5, 40] ^= 0x10
    return sig, signer


@pytest.mark.parametrize("total,lo,hi,wide,kernel", [(500, 3, 9, 0, 128), (2000, 3, 40, 0, 64), (8000, 50, 130, 1500, 16),
                                                      (65536, 60, 140, 0, 1)])
def test_row_counts_of_every_auto_form(total, lo, hi, wide, kernel):
    """the cold kernel AUTO picks for the TOTAL row count; ragged blocks, empty blocks; at 8 000 rows one block of 1 500 — more
    than the 256-thread tally covers in one step (256 × 4 rows), so the 1 024-thread form runs"""
    f = Fam(48, 16, 1, 32, 500 + total % 97)
    off = _ragged_offsets(total, total, lo, hi, wide)
    nb = len(off) - 1
    bset = [(b // 3) % 32 for b in range(nb)]
    bh = _block_hashes(nb, 600 + total % 89)
    bv, ref = _pair(max_rows=65536)
    try:
        f.install(bv)
        f.install_single(ref, 0)
        sig, signer = _device_rows(ref, f, bset, bh, off, total)
        got, tl = _check(bv, ref, f, bset, bh, off, sig, signer, cpu=total <= 8000, recover=total <= 8000)
        bv.verify_block_seals_sets(bh, off, bset, sig, signer)
        assert bv.last_dispatch()[0] == kernel
        assert 0 < got.sum() < total and any(t.valid_rows == 0 for t in tl)
        if total == 65536:   # the modest large case: the CPU oracle on every 16th block
            pick = list(range(0, nb, 16))
            rows = _rows_of(off, pick)
            e = _expect_cpu(f, [bset[b] for b in pick], bh[pick], _sub(off, pick), sig[rows], signer[rows], None)
            assert (e[0] == got[rows]).all() and e[1] == [_fields(tl[b]) for b in pick]
    finally:
        bv.close(); ref.close()


def test_largest_set_beyond_the_lds_bitmap():
    """block_tally_kernel (its sets form) keeps the distinct-signer bitmap of a block in LDS while ⌈largest set / 32⌉ words fit 49 152
    bytes (the bound of enqueue_block_tally / tally_kernel in csrc/ibftgpu.hip): 393 216 validators.  A set beyond it sends the
    whole launch through the one-workgroup form with the bitmap in HBM."""
    from oracle import binding as B, workload as W
    lds_validators = 49152 // 4 * 32
    r = W.make_round(12, 700, raw_len=64, weighted=True)
    filler = np.random.default_rng(700).integers(0, 256, (lds_validators + 40, 20), dtype=np.uint8)
    big_addrs = np.concatenate([filler[:1000], r.addrs[:8], filler[1000:], r.addrs[8:10]])
    big_power = (np.arange(len(big_addrs)) % 5 + 1).astype(np.uint64)
    small_addrs = r.addrs[[9, 3, 11, 0, 5]].copy()
    small_power = np.array([5, 4, 3, 2, 1], np.uint64)
    assert len(big_addrs) > lds_validators
    sets = [(1, big_addrs, big_power), (2, small_addrs, small_power)]
    vs = [B.ValSet(big_addrs, big_power), B.ValSet(small_addrs, small_power)]
    plan = [(0, [0, 1, 2, 9, 11, 0]), (1, [9, 3, 1, 11]), (0, []), (1, [0, 5, 5, 9, 3]), (0, [8, 9])]
    bh = _block_hashes(len(plan), 701)
    bset = [p[0] for p in plan]
    off = np.concatenate([[0], np.cumsum([len(p[1]) for p in plan])]).astype(np.uint32)
    wr = [(i, b) for b, p in enumerate(plan) for i in p[1]]
    sig = np.array([np.frombuffer(B.sign(r.sks[i], bytes(bh[b])), np.uint8) for i, b in wr], np.uint8).reshape(-1, 65)
    signer = np.array([r.addrs[i] for i, _ in wr], np.uint8).reshape(-1, 20)
    V = _V()
    bv = V.BatchVerifier(max_rows=lds_validators + 4096)
    try:
        bv.set_validator_sets(sets)
        assert bv.validator_sets_info()[:2] == (2, len(big_addrs) + 1)    # r.addrs[11] is in the small set only
        for _ in range(2):   # twice: the HBM bitmap is left zero for the next launch
            got, tl = bv.verify_block_seals_sets(bh, off, bset, sig, signer)
            who, vidx, rb, rtl = bv.recover_block_seals_sets(bh, off, bset, sig)
            for b, (k, members) in enumerate(plan):
                lo, hi = int(off[b]), int(off[b + 1])
                e = B.verify_seals(vs[k], _rows_hash(bh, off)[lo:hi], sig[lo:hi], signer[lo:hi]).astype(bool)
                assert (got[lo:hi] == e).all() and (rb[lo:hi] == e).all(), b
                assert _fields(tl[b]) == _fields(rtl[b]) == _fields(B.tally(vs[k], signer[lo:hi], e)), b
            assert vidx[0] == 1000 and vidx[3] == len(big_addrs) - 1 and vidx[4] == -1    # positions in the big set
            assert vidx[int(off[1]):int(off[2])].tolist() == [0, 1, -1, 2]
    finally:
        bv.close()


def test_warm_second_call_other_context_and_family_replacement():
    V = _V()
    f = Fam(40, 8, 2, 16, 800)
    nb = 32
    bset = [b % 16 for b in range(nb)]
    bh, off, sig, signer, pre = _fixture(f, bset, 801)
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=8192)
    other = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=8192)
    cold = V.BatchVerifier(max_rows=8192)
    try:
        f.install(bv)
        slots_family = bv.cache_memory()[1]
        assert slots_family >= 38                          # the union (sets 0…15 cover validators 0…37) holds its slots
        g1, t1 = _check(bv, cold, f, bset, bh, off, sig, signer, pre, recover=False)
        _, warm0, _ = bv.cache_stats()
        g2, t2 = bv.verify_block_seals_sets(bh, off, bset, sig, signer, pre)
        _, warm1, _ = bv.cache_stats()
        assert warm1 == warm0 + 1                          # the second call ran a warm kernel
        assert (g1 == g2).all() and [_fields(t) for t in t1] == [_fields(t) for t in t2]
        # a single-set call on ANOTHER context of the device is warm for addresses only the family taught
        f.install_single(other, 5)
        blocks = [b for b in range(nb) if bset[b] == 5]
        rows = _rows_of(off, blocks)
        tables, w0, _ = other.cache_stats()
        assert tables > 0
        m, t = other.verify_block_seals(bh[blocks], _sub(off, blocks), sig[rows], signer[rows], pre[rows])
        assert other.cache_stats()[1] == w0 + 1
        assert (m == g1[rows]).all() and [_fields(x) for x in t] == [_fields(t1[b]) for b in blocks]
        other.close(); other = None
        # a new family that keeps half of the union keeps those tables: still warm for the kept half at once
        half = Fam(40, 8, 2, 6, 800)                       # sets 0…5 of the same pool: validators 0…17
        half.install(bv)
        assert bv.cache_memory()[1] < slots_family         # the slots of the addresses that left are free again
        hb = [b for b in range(nb) if bset[b] < 6]
        rows = _rows_of(off, hb)
        _, w0, _ = bv.cache_stats()
        m, t = bv.verify_block_seals_sets(bh[hb], _sub(off, hb), [bset[b] for b in hb], sig[rows], signer[rows], pre[rows])
        # the FIRST call under the new family runs a warm kernel: it found tables built for its union.  (The table count of
        # cache_stats is the single set's, and this context has none.)
        assert bv.cache_stats()[1] == w0 + 1
        assert (m == g1[rows]).all() and [_fields(x) for x in t] == [_fields(t1[b]) for b in hb]
    finally:
        bv.close(); cold.close()
        if other is not None:
            other.close()


def test_u256_powers_beyond_128_bits():
    f = Fam(24, 6, 1, 12, 900, big=True)
    bset = [b % 12 for b in range(36)]
    bh, off, sig, signer, pre = _fixture(f, bset, 901)
    bv, ref = _pair(max_rows=4096)
    try:
        f.install(bv)
        got, tl = _check(bv, ref, f, bset, bh, off, sig, signer, pre)
        assert 0 < sum(t.has_quorum for t in tl) < len(tl)
        assert any(sum(f.power[k]) >> 128 for k in range(12))
    finally:
        bv.close(); ref.close()


def test_seal_digest_suffix_and_strict_low_s():
    from oracle import binding as B
    V = _V()
    f = Fam(24, 6, 1, 12, 910)
    nb = 24
    bset = [b % 12 for b in range(nb)]
    bh = _block_hashes(nb, 911)
    digest = lambda h: B.keccak256(h + b"\x02")
    rows = [(f.idx[bset[b]][j], b) for b in range(nb) for j in range(5)]
    off = (np.arange(nb + 1) * 5).astype(np.uint32)
    sigs = []
    for k, (i, b) in enumerate(rows):   # every 7th signs the bare hash; every 5th is flipped to its high-s twin
        s = B.sign(f.r.sks[i], digest(bytes(bh[b])) if k % 7 else bytes(bh[b]))
        if k % 5 == 2:
            s = s[:32] + (N_ORDER - int.from_bytes(s[32:64], "big")).to_bytes(32, "big") + bytes([s[64] ^ 1])
        sigs.append(np.frombuffer(s, np.uint8))
    sig = np.array(sigs, np.uint8).reshape(-1, 65)
    signer = np.array([f.r.addrs[i] for i, _ in rows], np.uint8).reshape(-1, 20)
    seen = []
    for flags in (0, V.FLAG_STRICT_LOW_S):
        bv, ref = _pair(max_rows=4096, flags=flags)
        try:
            f.install(bv)
            bv.set_seal_digest(b"\x02"); ref.set_seal_digest(b"\x02")
            got, _ = _check(bv, ref, f, bset, bh, off, sig, signer, digest=digest, flags=flags)
            seen.append(int(got.sum()))
        finally:
            bv.close(); ref.close()
    assert 0 < seen[1] < seen[0] < len(sig)     # the high-s rows pass only without the strict flag


def test_the_family_is_separate_state():
    """with a family installed the single-set entry points return what they return without one; a _sets call leaves no
    resident rows and leaves a streamed batch collectable"""
    from oracle import binding as B, workload as W
    V = _V()
    f = Fam(40, 8, 2, 16, 920)
    bset = [b % 16 for b in range(24)]
    bh, off, sig, signer, pre = _fixture(f, bset, 921)
    r2 = W.make_round(100, 922, byzantine=True)
    one = Fam(40, 8, 2, 16, 923)
    b1 = [4] * 12
    bh1, off1, sig1, signer1, pre1 = _fixture(one, b1, 924)
    bv, fresh = _pair()
    try:
        assert bv.try_set_validator_sets(f.sets()) == 0 and bv.validator_sets_info()[0] == 16
        for c in (bv, fresh):
            c.set_validators(r2.height, r2.addrs, r2.power)
        a = bv.is_valid_committed_seal(r2.hash32, r2.seal65, r2.signer20, r2.pre_flags)
        b = fresh.is_valid_committed_seal(r2.hash32, r2.seal65, r2.signer20, r2.pre_flags)
        assert (a[0] == b[0]).all() and _fields(a[1]) == _fields(b[1])
        bv.verify_block_seals_sets(bh, off, bset, sig, signer, pre)          # a _sets call in between changes nothing
        for c in (bv, fresh):
            one.install_single(c, 4)
        a = bv.verify_block_seals(bh1, off1, sig1, signer1, pre1)
        b = fresh.verify_block_seals(bh1, off1, sig1, signer1, pre1)
        assert (a[0] == b[0]).all() and [_fields(t) for t in a[1]] == [_fields(t) for t in b[1]]
        ra, rb = bv.seals_run(), fresh.seals_run()                             # the resident batch is the single-set call's
        assert (ra[0] == rb[0]).all() and _fields(ra[1]) == _fields(rb[1]) and (ra[0] == a[0]).all()
        assert bv.seals_rows()[0] == len(sig1)
        bv.verify_block_seals_sets(bh, off, bset, sig, signer, pre)
        assert bv.seals_rows()[0] == 0
        # between a streamed submit and its collect
        bv.block_seals_submit(bh1, off1, sig1, signer1, pre1)
        g, tl = bv.verify_block_seals_sets(bh, off, bset, sig, signer, pre)
        e = _expect_cpu(f, bset, bh, off, sig, signer, pre)
        assert (g == e[0]).all() and [_fields(t) for t in tl] == e[1]
        m, t = bv.block_seals_collect()
        assert (m == a[0]).all() and [_fields(x) for x in t] == [_fields(x) for x in a[1]]
        # and the family is still there after set_validators came and went
        assert bv.validator_sets_info()[0] == 16
    finally:
        bv.close(); fresh.close()


def test_error_codes_in_their_order_and_buffers_untouched():
    V = _V()
    L = V.load_library()
    p = V._p
    f = Fam(24, 6, 1, 12, 930)
    bset = np.array([b % 12 for b in range(6)], np.uint32)
    bh, off, sig, signer, pre = _fixture(f, bset, 931)
    n = int(off[-1])
    CAN = 0xA5A5A5A5A5A5A5A5

    def call(bv, off_=off, bset_=bset, nb=6, recover=False, sig_=sig, signer_=signer):
        mask = np.full(max(1, (n + 63) // 64), CAN, np.uint64)
        who = np.full((n, 20), 0x5A, np.uint8)
        vidx = np.full(n, 77, np.int32)
        tal = (V.Tally * max(nb, 1))()
        for t in tal:
            t.power_lo = 0x1234
        o = None if off_ is None else np.ascontiguousarray(off_, np.uint32)
        s = None if bset_ is None else np.ascontiguousarray(bset_, np.uint32)
        if recover:
            rc = L.ibft_recover_block_seals_sets(bv._h, p(bh), p(o), p(s), nb, p(sig_), None, p(who), p(vidx), p(mask), tal)
        else:
            rc = L.ibft_verify_block_seals_sets(bv._h, p(bh), p(o), p(s), nb, p(sig_), p(signer_), None, p(mask), tal)
        assert (mask == CAN).all() and (who == 0x5A).all() and (vidx == 77).all() and all(t.power_lo == 0x1234 for t in tal)
        return rc

    bv = V.BatchVerifier(max_rows=1024)
    small = V.BatchVerifier(max_rows=16)
    try:
        for rec in (False, True):
            assert call(bv, recover=rec) == E_NOVALSET                       # no family — a single set does not count
        bv.set_validators(1, f.addrs(0), f.power[0])
        assert call(bv) == E_NOVALSET
        # install: the documented order
        h = np.zeros(2, np.uint64)
        a = np.ascontiguousarray(np.concatenate([f.addrs(0), f.addrs(1)]))
        pw = np.ones(12, np.uint64)
        so = np.array([0, 6, 12], np.uint32)
        inst = L.ibft_set_validator_sets
        assert inst(bv._h, 0, p(h), p(so), p(a), p(pw)) == E_INVAL
        assert inst(bv._h, 2, p(h), None, p(a), p(pw)) == E_INVAL
        assert inst(bv._h, 2, p(h), p(np.array([1, 6, 12], np.uint32)), p(a), p(pw)) == E_INVAL
        assert inst(bv._h, 2, p(h), p(np.array([0, 7, 6], np.uint32)), p(a), p(pw)) == E_INVAL
        assert inst(bv._h, 2, p(h), p(so), None, p(pw)) == E_INVAL and inst(bv._h, 2, p(h), p(so), p(a), None) == E_INVAL
        assert inst(bv._h, 2, None, p(so), p(a), p(pw)) == 0                 # height is informational: NULL is fine
        assert bv.validator_sets_info()[:2] == (2, 7)
        # TOOBIG comes before POWER: a set beyond max_rows whose powers are all zero
        many = np.random.default_rng(1).integers(0, 256, (17, 20), dtype=np.uint8)
        assert small.try_set_validator_sets([(many, np.zeros(17, np.uint64))]) == E_TOOBIG
        assert small.try_set_validator_sets([(many[:9], np.ones(9, np.uint64)), (many[8:], np.ones(9, np.uint64))]) == E_TOOBIG  # the union
        # POWER: any set with total zero, an empty set included — and the family installed before stays usable
        f.install(bv)
        want = bv.verify_block_seals_sets(bh, off, bset, sig, signer, pre)
        assert bv.try_set_validator_sets([(f.addrs(0), f.power[0]), (f.addrs(1), [0] * 6)]) == E_POWER
        assert bv.try_set_validator_sets([(f.addrs(0), f.power[0]), (np.zeros((0, 20), np.uint8), [])]) == E_POWER
        assert bv.try_set_validator_sets([(f.addrs(0), [0] * 6)], u256=True) == E_POWER
        assert bv.validator_sets_info()[:2] == (12, 17)
        again = bv.verify_block_seals_sets(bh, off, bset, sig, signer, pre)
        assert (want[0] == again[0]).all() and [_fields(t) for t in want[1]] == [_fields(t) for t in again[1]]
        # calls: the order of ibft_verify_block_seals, then block_set
        for rec in (False, True):
            assert call(bv, off_=None, recover=rec) == E_INVAL
            bad = off.copy(); bad[0] = 1
            assert call(bv, off_=bad, recover=rec) == E_INVAL
            bad = off.copy(); bad[2] = bad[1] - 1
            assert call(bv, off_=bad, recover=rec) == E_INVAL
            assert call(bv, sig_=None, recover=rec) == E_INVAL
            assert call(bv, bset_=None, recover=rec) == E_INVAL
            out_of_range = bset.copy(); out_of_range[3] = 12
            assert call(bv, bset_=out_of_range, recover=rec) == E_INVAL     # refused on the host: nothing is launched
            out_of_range[3] = 0xFFFFFFFF
            assert call(bv, bset_=out_of_range, recover=rec) == E_INVAL
        assert call(bv, signer_=None) == E_INVAL
        small.set_validator_sets([(f.addrs(0), f.power[0])])
        assert n > 16 and call(small, bset_=np.zeros(6, np.uint32)) == E_TOOBIG
        assert call(small, off_=np.zeros(18, np.uint32), bset_=np.zeros(17, np.uint32), nb=17) == E_TOOBIG
        # no rows at all: every block empty, has_quorum 0, its set's quorum
        g, tl = bv.verify_block_seals_sets(bh[:3], [0, 0, 0, 0], [2, 5, 2], np.zeros((0, 65), np.uint8), np.zeros((0, 20), np.uint8))
        assert len(g) == 0 and [(t.has_quorum, t.power, t.valid_rows) for t in tl] == [(0, 0, 0)] * 3
        assert [t.quorum for t in tl] == [2 * sum(f.power[k]) // 3 + 1 for k in (2, 5, 2)]
        again = bv.verify_block_seals_sets(bh, off, bset, sig, signer, pre)
        assert (want[0] == again[0]).all()
    finally:
        bv.close(); small.close()


def test_byte_budget_from_the_environment():
    """IBFT_VALSETS_BYTES_MAX is read at ibft_ctx_create: a child process with a budget too small for the dense table"""
    code = r"""
import numpy as np
import go_ibft_amd.verifier as V
rng = np.random.default_rng(5)
addrs = rng.integers(0, 256, (200, 20), dtype=np.uint8)
sets = [(addrs[k:k + 100], np.ones(100, np.uint64)) for k in range(64)]      # 64 sets over a union of 163: 41 728 B dense
bv = V.BatchVerifier(max_rows=1024)
rc_small = bv.try_set_validator_sets(sets[:2])                              # 2 sets over a union of 101 fit
rc_big = bv.try_set_validator_sets(sets)
info = bv.validator_sets_info()
bv.close()
print("RESULT", rc_small, rc_big, info[0], info[1])
"""
    env = dict(os.environ, IBFT_VALSETS_BYTES_MAX="32768", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    assert [int(x) for x in line[1:]] == [0, E_TOOBIG, 2, 101]                # refused whole; the family before it stays
