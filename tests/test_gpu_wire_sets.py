"""GPU: the wire route under a family of validator sets — ibft_set_height_sets + ibft_verify_senders_wire_sets, every message
judged under the set of ITS height.  Oracles: (1) the CPU oracle's walk and signature check with the plain model of
tests/wire_sets_model.py on top (tests/wire_sets_cases.py: expected); (2) the device's own per-set route on a second context —
set_validators(set s) + is_valid_validator_wire over the rows of set s, for every s in turn.  Everything compared is a verdict
bit or an integer: equality is exact.  The corpus and what it holds: tests/wire_sets_cases.py, tests/test_wire_sets_inputs.py."""
import numpy as np
import pytest

import wire_sets_cases as WS
import wire_sets_model as M

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 300)
MANY = 2100                       # > 2 × 1 024 rows: wire_sets_tally_kernel runs three workgroups
LOW128 = 2**128 - 1


def _V():
    import go_ibft_amd.verifier as V
    return V


def _fields(t):
    return (t.power, t.quorum, t.valid_rows, t.distinct_senders, t.has_quorum, t.shard_overlap, t.proposer_rows)


def _install_single(ref, sets, s, big):
    h, a, p = sets[s]
    (ref.set_validators_u256 if big else ref.set_validators)(h, a, p)


def _check(bv, ref, c, n, hmap, recode, sets=None, model=None):
    """the sets call on bv over the first n rows of the corpus against both oracles; ref: a second context with the same flags"""
    sets = sets if sets is not None else c.sets()
    wire, off = WS.pack(c.msgs[:n])
    got, rows, rset, vidx, tl = bv.verify_senders_wire_sets(wire, off)
    wb, ws, wv, wt, parsed = WS.expected(c, n, hmap, recode, model)
    assert got.tolist() == wb, np.nonzero(got != np.array(wb))[0][:10]
    assert rset.tolist() == ws and vidx.tolist() == wv
    assert len(tl) == len(sets)
    for k, (t, w) in enumerate(zip(tl, wt)):
        assert (t.power, t.quorum, t.valid_rows, t.distinct_senders, t.has_quorum) == \
            (w["power"] & LOW128, w["quorum"] & LOW128, w["valid_rows"], w["distinct_senders"], w["has_quorum"]), k
    # afterwards: no resident batch of either kind, and the walks' statistics are this call's
    V = _V()
    assert bv.seals_rows()[0] == 0
    assert bv._L.ibft_wire_stage_seals(bv._h) == M.E_INVAL
    assert bv.wire_stats() == (n, sum(int(r["pad"][0]) for r in rows), sum(1 for e in parsed if e.status != 0))
    assert [int(x) for x in rows["status"]] == [e.status for e in parsed]
    # oracle 2: the single-set call — its rows for the whole batch, its bits and its tally for the rows of each set
    _install_single(ref, sets, 0, c.big)
    _, ref_rows, _ = ref.is_valid_validator_wire(wire, off)
    assert rows.tobytes() == ref_rows.tobytes()
    for s in sorted(set(ws) - {-1}) + [k for k in range(len(sets)) if k not in ws][:1]:     # … and one set without rows
        idx = [j for j in range(n) if ws[j] == s]
        _install_single(ref, sets, s, c.big)
        rb, _, rt = ref.is_valid_validator_wire(*WS.pack([c.msgs[j] for j in idx]))
        assert rb.tolist() == [bool(got[j]) for j in idx], s
        assert _fields(rt) == _fields(tl[s]), s
        # the index ibft_set_validators(set s) gives a sender: its position among the set's distinct addresses
        pos = {bytes(a): i for i, a in reversed(list(enumerate(sets[s][1])))}
        assert [int(vidx[j]) for j in idx] == [pos[parsed[j].sender] if got[j] else -1 for j in idx]
    return got, tl


@pytest.mark.parametrize("big", [False, True], ids=["u64", "u256"])
@pytest.mark.parametrize("cache", [False, True], ids=["cold", "warm"])
def test_defining_property(oracle, big, cache):
    V = _V()
    c = WS.corpus(big=big)
    flags = V.FLAG_PUBKEY_CACHE if cache else 0
    bv, ref = V.BatchVerifier(flags=flags, max_rows=4096), V.BatchVerifier(flags=flags, max_rows=4096)
    try:
        (bv.set_validator_sets_u256 if big else bv.set_validator_sets)(c.sets())
        assert bv.height_sets_info() == (0, 0, 0)
        bv.set_height_sets(*WS.MAP_A)
        assert bv.height_sets_info() == (5, 100, 229)
        for n in SIZES:
            for _ in range(2 if cache else 1):      # cold, then the same batch again on the warm kernels
                _check(bv, ref, c, n, WS.MAP_A, False)
        if cache:
            assert bv.cache_stats()[1] > 0          # the repeated batches ran on the warm kernels
        # more rows than one workgroup of the tally takes (1 024): three workgroups, the ticket, the bitmap merge across them
        wide = WS.corpus(n=MANY, big=big)
        assert wide.msgs[:300] == c.msgs and wide.sets()[0][2] == c.sets()[0][2]
        for _ in range(2 if cache else 1):
            _check(bv, ref, wide, MANY, WS.MAP_A, False)
        got, tl = _check(bv, ref, c, 0, WS.MAP_A, False)
        assert len(got) == 0 and all(t.has_quorum == 0 and t.quorum > 0 for t in tl)
        bv.set_height_sets(*WS.MAP_B)               # range 0 mapped: the empty View and height 99 become rows of set 2
        _check(bv, ref, c, 300, WS.MAP_B, False)
        # the scratch is zero again and the context's own state was put back: the single-set call still matches the oracle
        sets = c.sets()
        _install_single(bv, sets, 1, big)
        for _ in range(2):
            sb, _, st = bv.is_valid_validator_wire(*WS.pack(c.msgs))
            parsed, _ = WS.parsed(c.msgs, False)
            wb, _, wt = M.judge(c.model_sets(), [(1 if not e.pre_flag else -1, e.sender, WS.B.recover_address(e.digest, e.signature) == e.sender
                                                  if not e.pre_flag else False) for e in parsed])
            assert sb.tolist() == wb
            assert (st.power, st.valid_rows, st.distinct_senders, st.has_quorum) == \
                (wt[1]["power"] & LOW128, wt[1]["valid_rows"], wt[1]["distinct_senders"], wt[1]["has_quorum"])
        _check(bv, ref, c, 300, WS.MAP_B, False)    # … and the sets call after it
        # a new family drops the map: its indices named the old family's sets
        (bv.set_validator_sets_u256 if big else bv.set_validator_sets)(sets[:2])
        assert bv.height_sets_info() == (0, 0, 0)
        wire, off = WS.pack(c.msgs[:5])
        mask = np.full(1, 7, np.uint64)
        assert bv._L.ibft_verify_senders_wire_sets(bv._h, V._p(np.frombuffer(wire, np.uint8)), V._p(off), 5, V._p(mask), None, None, None,
                                                   None) == M.E_NOVALSET
        assert mask[0] == 7
    finally:
        bv.close()
        ref.close()


def test_recode_flag_maps_the_decoded_height(oracle):
    """a padded-varint height: NEEDS_HOST and no set without the flag (test_defining_property), with it a row of the range its
    DECODED height lies in — not the one its low byte names"""
    V = _V()
    c = WS.corpus()
    j = c.kinds.index("padded_height")
    bv, ref = V.BatchVerifier(flags=V.FLAG_WIRE_RECODE, max_rows=1024), V.BatchVerifier(flags=V.FLAG_WIRE_RECODE, max_rows=1024)
    try:
        bv.set_validator_sets(c.sets())
        bv.set_height_sets(*WS.MAP_A)
        for n in (65, 300):
            got, _ = _check(bv, ref, c, n, WS.MAP_A, True)
            assert got[j]
            assert bv.wire_stats()[1] == 1
    finally:
        bv.close()
        ref.close()


@pytest.mark.parametrize("extra", [0, 1], ids=["lds_cap", "hbm"])
def test_bitmap_at_the_lds_cap_and_beyond(oracle, extra):
    """wire_sets_tally_kernel keeps the distinct-sender bitmap of a workgroup in 48 KiB of LDS — 393 216 (set, member) entries:
    six sets of 65 536 are the largest family of the LDS form (49 152 B of dynamic LDS); with ONE entry more — a seventh set of
    one — the kernel takes the form that sends every row's bit to HBM."""
    V = _V()
    c = WS.corpus()
    pool = c.pool.addrs
    rng = np.random.default_rng(11)
    filler = rng.integers(0, 256, (65536 - len(pool), 20), dtype=np.uint8)
    base = np.concatenate([pool, filler])
    sets, model = [], []
    for k in range(6):
        a = np.roll(base, -7 * k, axis=0)                    # the same addresses at other indices
        p = (np.arange(65536, dtype=np.uint64) % 5 + 1 + k).tolist()
        sets.append((1000 + k, a, p))
        model.append(M.Set(list(zip((x.tobytes() for x in a), p))))
    if extra:
        sets.append((1006, pool[:1].copy(), [9]))
        model.append(M.Set([(pool[0].tobytes(), 9)]))
    last = len(sets) - 1
    hmap = ([100, 101, 102, 110, 111, 229], [0, 1, 2, last, 3])
    bv, ref = V.BatchVerifier(max_rows=65536), V.BatchVerifier(max_rows=65536)
    try:
        bv.set_validator_sets(sets)
        assert bv.validator_sets_info()[:2] == (len(sets), 65536)
        assert sum(len(s[1]) for s in sets) == 48 * 1024 * 8 + extra
        bv.set_height_sets(*hmap)
        for _ in range(2):                                    # the second pass finds the bitmap zero again
            _, tl = _check(bv, ref, c, 300, hmap, False, sets, model)
        assert tl[0].valid_rows > tl[0].distinct_senders > 0 and tl[last].valid_rows == 0
    finally:
        bv.close()
        ref.close()
