"""The inputs of tests/test_gpu_block_seals_sets_stream.py against the CPU oracle alone (no GPU): the batches have what the GPU
comparisons rely on — both values of has_quorum, every bad-row kind of the fixture (each under two different sets), rows signed
by a member of the family that is not in its block's set, high-s twins, a block without rows, blocks that straddle 64-bit
verdict words, proposals on both sides of the Keccak rate.  Without this the GPU file could pass vacuously."""
import numpy as np
import pytest

import block_sets_stream_cases as SC

N_ORDER = SC.N_ORDER


@pytest.fixture(scope="module")
def main():
    c = SC.main_case()
    return c, SC.expect_cpu(c)


def _blocks_of_kind(c, k):
    return [b for b, kk in enumerate(c.kind_of_block) if kk == k]


def test_shapes():
    c, w, e = SC.main_case(), SC.wide_case(), SC.empty_case()
    assert len(c.f.idx) == 3 and all(len(ix) == 7 for ix in c.f.idx) and c.f.r.n == 11
    assert len(c.bh) == 28 and len(c.bset) == 28 and len(c.off) == 29 and len(c.raws) == 28
    assert sorted(set(len(x) for x in c.raws)) == [0, 135, 136, 137, 1000]
    assert len({bytes(h) for h in c.bh}) == 28 and max(c.rounds) > 2**63            # 28 different hashes; a round beyond int64
    assert sum(1 for b in range(27) if c.bset[b] != c.bset[b + 1]) >= 8          # the set changes inside the batch
    empties = [b for b in range(28) if c.off[b] == c.off[b + 1]]
    assert empties == [14] and c.kind_of_block[14] == -1
    for k in range(13):                                                            # every row kind under two different sets
        assert len({int(c.bset[b]) for b in _blocks_of_kind(c, k)}) >= 2, k
    assert len(w.f.idx) == 3 and all(len(ix) == 70 for ix in w.f.idx) and len(w.bh) == 5
    sizes = np.diff(w.off.astype(np.int64))
    assert (sizes > 64).any() and all(int(o) % 64 for o in w.off[1:])              # rows span verdict words, blocks straddle them
    assert e.n == 0 and len(e.bh) == 3
    o = SC.other_case()
    assert len(o.f.idx) == 2 < 3 and not {bytes(a) for a in o.f.r.addrs} & {bytes(a) for a in c.f.r.addrs}
    assert int(c.bset.max()) >= len(o.f.idx)                                       # out of range under the other family


def test_both_values_of_has_quorum(main):
    c, (bits, tallies, who, vidx) = main
    hq = [t[4] for t in tallies]
    assert 0 in hq and 1 in hq
    assert tallies[14] == (0, 2 * sum(c.f.power[1]) // 3 + 1, 0, 0, 0)             # the empty block: its set's quorum
    assert len({t[1] for t in tallies}) == 3                                       # the three sets' quorums differ
    assert bits.any() and not bits.all()
    wq = [t[4] for t in SC.expect_cpu(SC.wide_case())[1]]
    assert 0 in wq and 1 in wq


def test_every_bad_row_kind_of_the_fixture_occurs(main):
    import go_ibft_amd.verifier as V
    c, (bits, tallies, who, vidx) = main
    first = lambda b: int(c.off[b])
    r_of = lambda row: int.from_bytes(c.sig[row, :32].tobytes(), "big")
    s_of = lambda row: int.from_bytes(c.sig[row, 32:64].tobytes(), "big")
    union = {bytes(c.f.r.addrs[i]) for ix in c.f.idx for i in ix}
    for b in range(28):
        k = c.kind_of_block[b]
        row = first(b)
        members = {bytes(c.f.r.addrs[i]) for i in c.f.idx[int(c.bset[b])]}
        rows = range(int(c.off[b]), int(c.off[b + 1]))
        if k in (0, 1, 2, 3, 4, 5, 6, 7):
            assert not bits[row], (b, k)
        if k == 0:
            assert r_of(row) == 0
        elif k == 1:
            assert s_of(row) == 0
        elif k == 2:
            assert r_of(row) >= N_ORDER
        elif k == 3:
            assert s_of(row) >= N_ORDER
        elif k == 4:
            assert c.sig[row, 64] == 2
        elif k == 5:
            assert bytes(who[row]) != bytes(c.signer[row])                         # random bytes: whoever is recovered, not the claimed one
        elif k == 6:
            assert c.pre[row] == V.ROW_BADLEN and c.pre[row + 1] == V.ROW_NIL and not bits[row + 1]
        elif k == 7:                                                               # a stolen seal: a member's, under another member's name
            assert bytes(who[row]) in members and bytes(who[row]) != bytes(c.signer[row]) and bytes(c.signer[row]) in members
        elif k == 8:                                                               # validly signed by a non-member of every set
            out = [i for i in rows if bytes(c.signer[i]) not in union]
            assert out and all(bytes(who[i]) == bytes(c.signer[i]) and not bits[i] and vidx[i] == -1 for i in out)
        elif k == 9:
            assert tallies[b][2] > tallies[b][3] > 0                               # more valid rows than distinct signers
        elif k in (10, 11):                                                        # in the family, not in this block's set
            stray = [i for i in rows if bytes(c.signer[i]) in union - members and bytes(who[i]) == bytes(c.signer[i])]
            assert stray and all(not bits[i] and vidx[i] == -1 for i in stray), (b, k)
        if k in SC.HIGH_S_KINDS:                                                   # the high-s twin: valid here, refused under strict-low-s
            last = int(c.off[b + 1]) - 1
            assert s_of(last) > N_ORDER // 2 and bits[last]
    assert any(c.pre) and c.pre is not None
    # a seal of the previous block replayed: the same 65 bytes in two blocks, valid in one of them at most
    seen = {}
    replays = 0
    for i in range(c.n):
        key = c.sig[i].tobytes()
        b = int(np.searchsorted(c.off, i, side="right") - 1)
        if key in seen and seen[key] != b:
            replays += 1
        seen.setdefault(key, b)
    assert replays >= 1
    strict = SC.expect_cpu(c, flags=V.FLAG_STRICT_LOW_S)[0]
    assert 0 < strict.sum() < bits.sum()


def test_a_family_member_outside_its_blocks_set_signs_rows(main):
    c, (bits, tallies, who, vidx) = main
    union = {bytes(c.f.r.addrs[i]) for ix in c.f.idx for i in ix}
    set_of_row = np.repeat(c.bset, np.diff(c.off.astype(np.int64)))
    n_stray = 0
    for i in range(c.n):
        members = {bytes(c.f.r.addrs[j]) for j in c.f.idx[int(set_of_row[i])]}
        a = bytes(who[i])
        if a == bytes(c.signer[i]) and a in union and a not in members:
            assert not bits[i] and vidx[i] == -1
            n_stray += 1
    assert n_stray >= 2
    # … and members' indices differ from set to set (the sets slide): an index is the BLOCK's set's
    assert (vidx >= 0).sum() > c.n // 2


def test_the_suffix_and_u256_variants_are_as_meaningful(main):
    c, (bits, *_rest) = main
    s = SC.main_case(SC.SUFFIX)
    sb, st, _, _ = SC.expect_cpu(s, SC.SUFFIX)
    assert (sb == bits).all() and 0 < sum(t[4] for t in st) < 28                   # the same rows, signed under the convention
    assert not SC.expect_cpu(s, None)[0].any()                                     # … and worthless without it
    g = SC.main_case(big=True)
    gt = SC.expect_cpu(g)[1]
    assert 0 < sum(t[4] for t in gt) < 28 and any(t[1] >> 128 for t in gt)
