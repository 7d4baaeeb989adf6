"""One scenario of tests/test_gpu_key_cache_lifecycle.py, run in a process of its own: only a fresh process has an empty
key-cache pool, so only here are capacity, growth and the free list the same on every run.

    python key_cache_child.py REPOSITORY_ROOT SCENARIO [WARM_LANES COLD_LANES]

Everything a scenario feeds the device is made, and checked against what the scenario needs of it, by a `*_inputs`
function that touches no GPU (the CPU tests of the parent module call them too); the expectations come from the CPU
oracle and from key_cache_model.KeyCacheModel, never from the library under test."""
import os
import sys
from types import SimpleNamespace

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
from key_cache_model import SLOT_BYTES, KeyCacheModel  # noqa: E402

KINDS = ("corrupt", "outsider", "claim", "pre")
N_OVER, N_KEPT = 1700, 1000          # scenario A: the set that overflows a 1 GB pool, and what is left of it afterwards
BUDGET_1GB = 1 << 30
NEVER = (610, 720, 830)              # … three of them with a corrupted seal in every round: no table before the kept set's first pass


def _oracle():
    from oracle import binding as B, workload as W
    B.build()
    return B, W


def columns(parts, round_, envelopes=False):
    """parts = [(n, seed, lo, hi), …]: the validators lo … hi − 1 of each make_round(n, seed), as ONE validator set in this
    order, every one with its honest seal over its proposal hash of round `round_` and claimed by itself"""
    _, W = _oracle()
    rs = [(W.make_round(n, seed, round_=round_, weighted=True, with_envelopes=envelopes), lo, hi) for n, seed, lo, hi in parts]
    cat = lambda f: np.concatenate([f(r)[lo:hi] for r, lo, hi in rs])  # noqa: E731
    c = SimpleNamespace(addrs=cat(lambda r: r.addrs), power=cat(lambda r: r.power), hash32=cat(lambda r: r.hash32).copy(),
                        seal65=cat(lambda r: r.seal65).copy(), signer20=cat(lambda r: r.signer20).copy())
    c.n = len(c.addrs)
    c.pre = np.zeros(c.n, np.uint8)
    c.bad = {}                       # row → kind, as placed by spoil()
    if envelopes:                    # (one part, taken whole)
        r = rs[0][0]
        c.payload, c.off, c.msg_sig65 = r.payload, r.off, r.msg_sig65.copy()
    return c


def spoil(c, plan):
    """plan: (kind, row, other) — "corrupt": a bit of s flipped; "outsider": a seal by a key outside every set; "claim": the
    row's honest seal claimed by member `other`; "pre": the row pre-flagged with `other` (its seal stays honest)"""
    B, W = _oracle()
    outsider = W.validator_key(0x5EED, 1 << 40)
    for kind, row, other in plan:
        assert row not in c.bad, (row, kind)
        c.bad[row] = kind
        if kind == "corrupt":
            c.seal65[row, 40] ^= 0x55
        elif kind == "outsider":
            c.seal65[row] = np.frombuffer(B.sign(outsider, c.hash32[row].tobytes()), np.uint8)
        elif kind == "claim":
            assert other != row
            c.signer20[row] = c.addrs[other]
        else:
            c.pre[row] = other
    return c


def plan_small(n, k, keep=()):
    """two rows of every kind among n ≥ 64 validators, at places that move with k; rows in `keep` are left honest"""
    rows = [(17 * k + 3 + 5 * t) % n for t in range(8)]
    other = [0, 0, 0, 0, (rows[4] + n // 2) % n, (rows[5] + n // 2 + 1) % n, 1 << (k % 3), 1 << ((k + 1) % 3)]
    return [(KINDS[t // 2], r, o) for t, (r, o) in enumerate(zip(rows, other)) if r not in keep]


def expect(c, placed=True):
    """the oracle's verdicts and tally for the rows of c against c's validator set.  placed: row i is validator i's, and the
    oracle must turn down exactly the rows spoil() touched (a condition on the input, checked before any GPU call)"""
    B, _ = _oracle()
    vs = B.ValSet(c.addrs, c.power)
    e = B.verify_seals(vs, c.hash32, c.seal65, c.signer20, c.pre, nthreads=8)
    exp = e.astype(bool)
    bad = np.zeros(len(exp), bool)
    bad[list(c.bad) if placed else []] = True
    assert not placed or (exp == ~bad).all(), np.flatnonzero(exp == bad)[:8]
    return exp, B.tally(vs, c.signer20, e)


def tally_fields(t):
    return (t.power, t.quorum, t.has_quorum, t.valid_rows, t.distinct_senders)


def claimed_valid(c, exp):
    """addresses with at least one accepted row in this batch: whose key a cold pass over it learns"""
    return {c.signer20[i].tobytes() for i in np.flatnonzero(exp)}


# ---- scenario A: more validators than the budget has slots -------------------------------------------------------------

def plan_overflow(k, n_slotted, n):
    """three rows of every kind on each side of the budget's edge, at places that move with the round; a "claim" row counts
    for the side of the member it CLAIMS to be (that member's slot, or lack of one, picks the kernel branch)"""
    n_un = n - n_slotted
    slotted_rows = [(97 * k + 5 + 7 * t) % n_slotted for t in range(12)]
    unslotted_rows = [n_slotted + (13 * k + t) % n_un for t in range(12)]
    plan = []
    for t in range(12):
        kind = KINDS[t // 3]
        o_s = {"claim": n_slotted + (13 * k + 20 + t) % n_un, "pre": 1 << (t % 3)}.get(kind, 0)    # slotted seal, unslotted claim
        o_u = {"claim": (97 * k + 500 + t) % n_slotted, "pre": 1 << (t % 3)}.get(kind, 0)          # unslotted seal, slotted claim
        plan += [(kind, slotted_rows[t], o_s), (kind, unslotted_rows[t], o_u)]
    return plan + [("corrupt", row, 0) for row in NEVER]


def overflow_inputs(seed=4100):
    """→ (rounds 0 … 3 of the 1 700 (spoiled; round 0 with envelopes, spoiled too), an honest and a spoiled round of the
    first 1 000, the model after both set_validators calls' predictions, the oracle's answers) — all checked here"""
    B, W = _oracle()
    model = KeyCacheModel(BUDGET_1GB)
    assert model.max_slots == BUDGET_1GB // SLOT_BYTES == 1638
    part = [(N_OVER, seed, 0, N_OVER)]
    rounds = [columns(part, k, envelopes=(k == 0)) for k in range(4)]
    unslotted, tables = model.set_validators("a", rounds[0].addrs)
    assert unslotted == list(range(1638, N_OVER)) and tables == 0 and model.slots_in_use == 1638
    un = {rounds[0].addrs[i].tobytes() for i in unslotted}
    for k, c in enumerate(rounds):
        assert (c.addrs == rounds[0].addrs).all()
        spoil(c, plan_overflow(k, 1638, N_OVER))
        c.exp, c.tally = expect(c)
        count = {(kind, side): 0 for kind in KINDS for side in (True, False)}
        for row, kind in c.bad.items():
            count[kind, c.signer20[row].tobytes() in un] += 1
        assert min(count.values()) >= 3, count                                   # every kind, three times, on each side
        assert len(claimed_valid(c, c.exp) & un) >= 50                           # … and the unslotted are mostly honest
    c = rounds[0]                                                                # senders mode: the envelopes of round 0
    outsider = W.validator_key(0x5EED, 1 << 40)
    for row, kind in c.bad.items():
        if kind == "corrupt":
            c.msg_sig65[row, 40] ^= 0x55
        elif kind == "outsider":
            c.msg_sig65[row] = np.frombuffer(B.sign(outsider, B.keccak256(c.payload[c.off[row]:c.off[row + 1]])), np.uint8)
    vs = B.ValSet(c.addrs, c.power)
    e = B.verify_senders(vs, c.payload, c.off, c.msg_sig65, c.signer20, c.pre, nthreads=8)
    c.senders_exp, c.senders_tally = e.astype(bool), B.tally(vs, c.signer20, e)
    bad = np.zeros(N_OVER, bool)
    bad[list(c.bad)] = True
    assert (c.senders_exp == ~bad).all()
    c = rounds[3]                                                                # recover mode: who signed round 3's seals
    c.rec_addr = np.zeros((N_OVER, 20), np.uint8)
    place = {a.tobytes(): i for i, a in enumerate(c.addrs)}
    c.rec_vidx = np.full(N_OVER, -1, np.int32)
    for i in range(N_OVER):
        a = None if c.pre[i] else B.recover_address(c.hash32[i].tobytes(), c.seal65[i].tobytes(), 0)
        if a is not None:
            c.rec_addr[i] = np.frombuffer(a, np.uint8)
            c.rec_vidx[i] = place.get(a, -1)
    c.rec_tally = B.tally(vs, c.rec_addr, (c.rec_vidx >= 0).astype(np.uint8))
    n_rec = int((c.rec_vidx >= 0).sum())
    assert n_rec == N_OVER - 3 * 6 - len(NEVER) and sum(c.rec_vidx[r] != r for r in c.bad) >= 18   # pre, corrupt, outsider: nobody's
    kept = [columns([(N_OVER, seed, 0, N_KEPT)], 4), spoil(columns([(N_OVER, seed, 0, N_KEPT)], 5), plan_small(N_KEPT, 5))]
    for c in kept:
        c.exp, c.tally = expect(c)
    assert kept[0].exp.all()
    return rounds, kept, model, un


def run_overflow(warm_lanes, cold_lanes):
    os.environ.update(IBFT_QTAB_BUDGET_GB="1", IBFT_WARM_LANES=str(warm_lanes), IBFT_COLD_LANES=str(cold_lanes))
    rounds, kept, model, un = overflow_inputs()
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=2048)
    try:
        bv.set_validators(1, rounds[0].addrs, rounds[0].power)
        seen = set()                                                 # slotted addresses with a valid signature so far

        def after_pass(k, c, exp):
            nonlocal seen
            seen |= claimed_valid(c, exp) - un
            by, used, cap, _ = bv.cache_memory()
            assert used == 1638 and cap <= 1638, (k, used, cap)
            model.check_capacity(used, cap, by)
            tables, warm, _ = bv.cache_stats()
            print(f"pass {k}: tables {tables} (valid so far {len(seen)}), dispatch {bv.last_dispatch()}, warm passes {warm}")
            return tables, warm

        warm_before = 0
        for k, c in enumerate(rounds):
            got, t = bv.is_valid_committed_seal(c.hash32, c.seal65, c.signer20, c.pre)
            assert (got == c.exp).all(), (k, np.flatnonzero(got != c.exp)[:8])
            assert tally_fields(t) == tally_fields(c.tally), (k, tally_fields(t), tally_fields(c.tally))
            tables, warm = after_pass(k, c, c.exp)
            if k >= 2:
                assert tables == len(seen) <= 1638, (k, tables, len(seen))
                # a member without a slot: never the all-warm exit, the cold kernel runs behind the warm one
                assert bv.last_dispatch() == (cold_lanes, warm_lanes) and warm == warm_before + 1, (k, bv.last_dispatch(), warm)
            warm_before = warm
        c = rounds[0]
        got, t = bv.is_valid_validator(c.payload, c.off, c.msg_sig65, c.signer20, c.pre)
        assert (got == c.senders_exp).all(), np.flatnonzero(got != c.senders_exp)[:8]
        assert tally_fields(t) == tally_fields(c.senders_tally)
        tables, warm = after_pass("senders", c, c.senders_exp)
        assert tables == len(seen) and bv.last_dispatch() == (cold_lanes, warm_lanes) and warm == warm_before + 1
        c = rounds[3]
        addr, vidx, bit, t = bv.recover_seals(c.hash32, c.seal65, c.pre)
        assert (addr == c.rec_addr).all() and (vidx == c.rec_vidx).all() and (bit == (c.rec_vidx >= 0)).all()
        assert tally_fields(t) == tally_fields(c.rec_tally)
        assert bv.cache_stats()[1] == warm                           # (always cold: no claimed key picks a table)
        # the first 1 000 alone fit: everybody keeps or gets a slot, one pass learns the rest, then nothing is cold
        model.learned(seen)
        unslotted, tables = model.set_validators("a", kept[0].addrs)
        assert unslotted == [] and model.slots_in_use == N_KEPT and tables == N_KEPT - len(NEVER)
        bv.set_validators(2, kept[0].addrs, kept[0].power)
        by, used, cap, _ = bv.cache_memory()
        model.check_capacity(used, cap, by)
        assert bv.cache_stats()[0] == tables, (bv.cache_stats()[0], tables)
        for k, c in enumerate(kept):
            got, t = bv.is_valid_committed_seal(c.hash32, c.seal65, c.signer20, c.pre)
            assert (got == c.exp).all(), (k, np.flatnonzero(got != c.exp)[:8])
            assert tally_fields(t) == tally_fields(c.tally)
            assert bv.cache_stats()[0] == N_KEPT
        assert bv.last_dispatch() == (0, warm_lanes), bv.last_dispatch()
    finally:
        bv.close()


# ---- scenario A0: no budget at all -------------------------------------------------------------------------------------

def budget0_inputs():
    B, W = _oracle()
    rounds = [W.make_round(64, 4200, round_=k, byzantine=True, weighted=True) for k in range(3)]
    vs = B.ValSet(rounds[0].addrs, rounds[0].power)
    for r in rounds:
        e = B.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags)
        r.exp, r.tally = e.astype(bool), B.tally(vs, r.signer20, e)
        assert r.exp.any() and not r.exp.all()
    model = KeyCacheModel(0)
    assert model.set_validators("a", rounds[0].addrs) == (list(range(64)), 0) and model.slots_in_use == 0
    return rounds, model


def run_budget0():
    os.environ["IBFT_QTAB_BUDGET_GB"] = "0"
    rounds, model = budget0_inputs()
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=1024)
    try:
        bv.set_validators(1, rounds[0].addrs, rounds[0].power)       # succeeds: the cache is off, not an error
        for k, r in enumerate(rounds):
            got, t = bv.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
            assert (got == r.exp).all(), (k, np.flatnonzero(got != r.exp)[:8])
            assert tally_fields(t) == tally_fields(r.tally)
            assert bv.cache_stats()[:2] == (0, 0) and bv.last_dispatch()[1] == 0 and bv.last_dispatch()[0] > 0
            by, used, cap, _ = bv.cache_memory()
            model.check_capacity(used, cap, by)
    finally:
        bv.close()


# ---- scenario B: the pool grows while other contexts hold built tables in it -------------------------------------------

SET_A = [(64, 4300, 0, 64)]
SET_B = [(64, 4300, 16, 32), (168, 4301, 0, 168), (64, 4300, 32, 48)]     # 200, 32 of them A's, on both sides of the new ones
SET_C = [(600, 4302, 0, 600)]


def growth_inputs():
    """→ (rounds by name, with the oracle's answers).  A's last validator — the last slot of the pool before it grows, the
    one a copy short by one entry loses — keeps an honest row in every round."""
    r = {"a0": columns(SET_A, 0), "a1": columns(SET_A, 1)}
    for k in (2, 3, 4):
        r[f"a{k}"] = spoil(columns(SET_A, k), plan_small(64, k, keep={63}))
    for k in range(4):
        r[f"b{k}"] = spoil(columns(SET_B, k), plan_small(200, k))
    r["c0"] = spoil(columns(SET_C, 0), plan_small(600, 0))
    for c in r.values():
        c.exp, c.tally = expect(c)
        assert 63 not in c.bad or c.n != 64
    a, b, c = (set(map(bytes, r[x].addrs)) for x in ("a0", "b0", "c0"))
    assert (len(a), len(b), len(c), len(a & b), len(a & c), len(b & c)) == (64, 200, 600, 32, 0, 0)
    assert r["a0"].exp.all() and r["a1"].exp.all()
    m = KeyCacheModel()                                              # the call sequence, on the model alone
    assert m.set_validators("a", r["a0"].addrs) == ([], 0)
    m.learned(r["a0"].addrs)
    assert m.set_validators("b", r["b0"].addrs) == ([], 32) and m.slots_in_use == 232
    assert m.set_validators("c", r["c0"].addrs) == ([], 0) and m.slots_in_use == 832
    m.close("c")
    assert m.slots_in_use == 232
    m.close("b")
    assert m.slots_in_use == 64 and m.tables("a") == 64
    return r


def run_growth():
    r = growth_inputs()
    import go_ibft_amd.verifier as V
    m = KeyCacheModel()
    ctx = {}

    def open_(who, name):
        ctx[who] = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=1024)
        unslotted, tables = m.set_validators(who, r[name].addrs)
        ctx[who].set_validators(1, r[name].addrs, r[name].power)
        by, used, cap, _ = ctx[who].cache_memory()
        m.check_capacity(used, cap, by)
        assert unslotted == [] and ctx[who].cache_stats()[0] == tables, (who, ctx[who].cache_stats()[0], tables)
        return cap

    def verify(who, name, all_warm=None, tables=True):
        c = r[name]
        got, t = ctx[who].is_valid_committed_seal(c.hash32, c.seal65, c.signer20, c.pre)
        assert (got == c.exp).all(), (name, np.flatnonzero(got != c.exp)[:8])
        assert tally_fields(t) == tally_fields(c.tally), (name, tally_fields(t), tally_fields(c.tally))
        m.learned(claimed_valid(c, c.exp))
        cold, warm = ctx[who].last_dispatch()
        print(f"{name}: dispatch {(cold, warm)}, tables {ctx[who].cache_stats()[0]}")
        if all_warm is not None:
            assert (cold == 0) == all_warm and warm > 0, (name, cold, warm)
        assert not tables or ctx[who].cache_stats()[0] == m.tables(who), (name, ctx[who].cache_stats()[0], m.tables(who))

    try:
        cap_a = open_("a", "a0")
        verify("a", "a0")
        verify("a", "a1")
        assert ctx["a"].cache_stats()[0] == 64
        cap_b = open_("b", "b0")                                     # 32 of A's tables are B's at once; the pool has moved
        assert ctx["b"].cache_stats()[0] == 32 and cap_b > cap_a, (cap_a, cap_b)
        verify("a", "a2", all_warm=True)                             # … and A's 64 tables came along, before B saw a seal
        verify("b", "b0", all_warm=False, tables=False)              # mixed: 32 warm, the others learned by the cold kernel
        verify("b", "b1", tables=False)
        verify("b", "b2")                                            # … and B ends with a table for everyone it saw sign
        cap_c = open_("c", "c0")
        assert cap_c > cap_b, (cap_b, cap_c)
        verify("a", "a3", all_warm=True)
        verify("b", "b3")
        verify("c", "c0", tables=False)
        for who in ("c", "b"):
            ctx.pop(who).close()
            m.close(who)
            by, used, cap, _ = ctx["a"].cache_memory()
            m.check_capacity(used, cap, by)
        verify("a", "a4", all_warm=True)
    finally:
        for bv in ctx.values():
            bv.close()


# ---- scenario C: what a recycled slot remembers ------------------------------------------------------------------------

SET_X, SET_Y, SET_Z = [(64, 4400, 0, 64)], [(64, 4401, 0, 64)], [(64, 4402, 0, 64)]


def cross_rows(old, claimers, vset):
    """every seal of `old` (a round of validators who left) claimed by every address of `claimers` (members of the set
    `vset`): old.n × len(claimers) rows against vset, none of which may be accepted"""
    i, j = np.repeat(np.arange(old.n), len(claimers)), np.tile(np.arange(len(claimers)), old.n)
    c = SimpleNamespace(addrs=vset.addrs, power=vset.power, n=vset.n, hash32=old.hash32[i], seal65=old.seal65[i],
                        signer20=claimers[j], pre=np.zeros(len(i), np.uint8), bad={})
    c.exp, c.tally = expect(c, placed=False)
    assert not c.exp.any() and c.tally.valid_rows == 0
    return c


def recycle_inputs():
    r = {"x0": columns(SET_X, 0), "x1": columns(SET_X, 1), "x2": spoil(columns(SET_X, 2), plan_small(64, 2)),
         "y0": columns(SET_Y, 0), "y1": columns(SET_Y, 1),
         "z0": columns(SET_Z, 0), "z1": spoil(columns(SET_Z, 1), plan_small(64, 1)), "z2": spoil(columns(SET_Z, 2), plan_small(64, 2))}
    for c in r.values():
        c.exp, c.tally = expect(c)
    x, y, z = (set(map(bytes, r[k].addrs)) for k in ("x0", "y0", "z0"))
    assert len(x) == len(y) == len(z) == 64 and not (x & y or x & z or y & z)
    # whichever freed slots the allocator hands to Z — X's, freed when B closed, or Y's, freed by the same call — their past
    # owners' seals are in the probe: 2 × 4 096 rows
    probe = cross_rows(r["x1"], r["z0"].addrs, r["z0"])
    py = cross_rows(r["y1"], r["z0"].addrs, r["z0"])
    for f in ("hash32", "seal65", "signer20", "pre"):
        setattr(probe, f, np.concatenate([getattr(probe, f), getattr(py, f)]))
    probe.exp, probe.tally = expect(probe, placed=False)
    assert len(probe.exp) == 8192 and not probe.exp.any()
    r["probe"] = probe
    m = KeyCacheModel()
    m.set_validators("a", r["x0"].addrs), m.set_validators("b", r["x0"].addrs)
    m.learned(r["x0"].addrs)
    assert m.slots_in_use == 64 and m.tables("b") == 64
    assert m.set_validators("a", r["y0"].addrs) == ([], 0) and m.slots_in_use == 128
    m.close("b")
    assert m.slots_in_use == 64
    assert m.set_validators("a", r["z0"].addrs) == ([], 0) and m.slots_in_use == 64
    return r


def _verify(bv, c, what):
    got, t = bv.is_valid_committed_seal(c.hash32, c.seal65, c.signer20, c.pre)
    assert (got == c.exp).all(), (what, "rows", np.flatnonzero(got != c.exp)[:8], "of", len(got))
    assert tally_fields(t) == tally_fields(c.tally), (what, tally_fields(t), tally_fields(c.tally))
    print(f"{what}: dispatch {bv.last_dispatch()}, tables {bv.cache_stats()[0]}")
    return bv.last_dispatch()


def run_recycle():
    r = recycle_inputs()
    import go_ibft_amd.verifier as V
    m = KeyCacheModel()
    a, b = (V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=8192) for _ in range(2))

    def take(bv, who, name, height):
        unslotted, tables = m.set_validators(who, r[name].addrs)
        bv.set_validators(height, r[name].addrs, r[name].power)
        by, used, cap, _ = bv.cache_memory()
        m.check_capacity(used, cap, by)
        assert unslotted == [] and bv.cache_stats()[0] == tables, (who, name, bv.cache_stats()[0], tables)

    try:
        take(a, "a", "x0", 1), take(b, "b", "x0", 1)
        _verify(a, r["x0"], "a learns x"), _verify(a, r["x1"], "a x again")
        m.learned(r["x0"].addrs)
        assert a.cache_stats()[0] == 64
        assert _verify(b, r["x2"], "b warm at once")[0] == 0 and b.cache_stats()[0] == 64
        take(a, "a", "y0", 2)                                        # 128 slots: B still holds X
        _verify(a, r["y0"], "a learns y"), _verify(a, r["y1"], "a y again")
        m.learned(r["y0"].addrs)
        assert a.cache_stats()[0] == 64
        b.close()
        m.close("b")
        m.check_capacity(*[a.cache_memory()[i] for i in (1, 2, 0)])  # 64: X's slots are free, their tables still in memory
        take(a, "a", "z0", 3)                                        # 64 slots, all recycled, no table counted
        assert a.cache_stats()[0] == 0
        _verify(a, r["probe"], "probe 1")
        _verify(a, r["probe"], "probe 2")
        assert _verify(a, r["z0"], "z honest")[0] != 0               # cold: nothing of Z is known
        _verify(a, r["z1"], "z byzantine 1")
        assert _verify(a, r["z2"], "z byzantine 2")[0] == 0 and a.cache_stats()[0] == 64
        assert _verify(a, r["probe"], "probe 3")[0] == 0             # against Z's own tables now
    finally:
        a.close(), b.close()


ROT = slice(20, 30)                  # who leaves in the single-context rotation


def rotation_inputs():
    old = [columns(SET_X, k) for k in range(2)]
    parts = [(64, 4400, 0, 20), (64, 4403, 0, 10), (64, 4400, 30, 64)]
    new = [columns(parts, 2), spoil(columns(parts, 3), plan_small(64, 3)), spoil(columns(parts, 4), plan_small(64, 4))]
    for c in old + new:
        c.exp, c.tally = expect(c)
    assert (new[0].addrs[:20] == old[0].addrs[:20]).all() and (new[0].addrs[30:] == old[0].addrs[30:]).all()
    assert not set(map(bytes, new[0].addrs[ROT])) & set(map(bytes, old[0].addrs))
    leavers = SimpleNamespace(n=10, hash32=old[1].hash32[ROT], seal65=old[1].seal65[ROT])
    probe = cross_rows(leavers, new[0].addrs[ROT], new[0])
    assert len(probe.exp) == 100 and not probe.exp.any()
    m = KeyCacheModel()
    m.set_validators("a", old[0].addrs)
    m.learned(old[0].addrs)
    assert m.set_validators("a", new[0].addrs) == ([], 54) and m.slots_in_use == 64
    return old, new, probe


def run_rotation():
    old, new, probe = rotation_inputs()
    import go_ibft_amd.verifier as V
    m = KeyCacheModel()
    a = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=1024)
    try:
        m.set_validators("a", old[0].addrs)
        a.set_validators(1, old[0].addrs, old[0].power)
        _verify(a, old[0], "learn"), _verify(a, old[1], "again")
        m.learned(old[0].addrs)
        assert a.cache_stats()[0] == 64
        _, tables = m.set_validators("a", new[0].addrs)
        a.set_validators(2, new[0].addrs, new[0].power)
        by, used, cap, _ = a.cache_memory()
        m.check_capacity(used, cap, by)                              # 64 in use: the newcomers sit where the leavers sat
        assert a.cache_stats()[0] == tables == 54
        warm_before = a.cache_stats()[1]
        cold, _ = _verify(a, probe, "probe 1")                       # the warm kernel runs (54 tables) and must not trust the 10
        assert cold != 0 and a.cache_stats()[1] == warm_before + 1
        _verify(a, probe, "probe 2")
        _verify(a, new[0], "newcomers honest"), _verify(a, new[1], "byzantine 1")
        assert _verify(a, new[2], "byzantine 2")[0] == 0 and a.cache_stats()[0] == 64
        assert _verify(a, probe, "probe 3")[0] == 0
    finally:
        a.close()


INPUTS = {"overflow": overflow_inputs, "budget0": budget0_inputs, "growth": growth_inputs, "recycle": recycle_inputs,
          "rotation": rotation_inputs}
RUN = {"overflow": run_overflow, "budget0": run_budget0, "growth": run_growth, "recycle": run_recycle, "rotation": run_rotation}

if __name__ == "__main__":
    scenario = sys.argv[2]
    RUN[scenario](*[int(x) for x in sys.argv[3:]])
    print(f"KEY_CACHE_{scenario.upper()}_OK")
