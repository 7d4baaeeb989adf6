"""GPU: the colliding validator sets of tests/valset_collision_cases.py through every route that ends in valset_lookup on the
device — the cold kernel families at every lane width and the warm kernels behind them (is_valid_committed_seal), the emitting
form (recover_seals), the sender route (is_valid_validator), lookup_kernel behind has_quorum / has_prepare_quorum, the union
table of a family of sets (verify_block_seals_sets / recover_block_seals_sets) and the 256-bit powers of set_validators_u256 —
each against the oracle, whose ValSet sorts and searches (no hash, no probing), exactly.

Member i has power 1 << i: a tallied power names the indices that were counted, so a row attributed to a decoy one word away
from its signer, a member the probe loop did not reach behind the wrap, or an outsider taken for the entry it collides with
changes the number.

Out of scope here: the proposer lookup of the wire-views records (wire_views_dev.h) and cert_judge_kernel — they read the
same table through the same valset_lookup."""
from collections import namedtuple

import numpy as np
import pytest

import valset_collision_cases as VC

pytestmark = pytest.mark.gpu

NAMES = sorted(VC.CORPORA)
LANES = [1, 2, 4, 8, 16, 64, 128]
Msg = namedtuple("Msg", "sender")


def _fields(t):
    return int(t.power), int(t.valid_rows), int(t.distinct_senders), int(t.has_quorum)


def _setup(oracle, name):
    c = VC.CORPORA[name]()
    col = VC.addr_column(c.addrs)
    power = np.array(c.powers, dtype=np.uint64)
    return c, col, power, oracle.ValSet(col, power)


@pytest.mark.parametrize("lanes", LANES)
def test_seal_route_every_cold_variant_then_warm(oracle, lanes, monkeypatch):
    import go_ibft_amd.verifier as V
    monkeypatch.setenv("IBFT_COLD_LANES", str(lanes))
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=1024)
    try:
        for name in NAMES:
            c, col, power, vs = _setup(oracle, name)
            bv.set_validators(1, col, power)
            hs, sigs, claimed = VC.columns(VC.rows(name))
            exp = oracle.verify_seals(vs, hs, sigs, claimed).astype(bool)
            te = oracle.tally(vs, claimed, exp.astype(np.uint8))
            assert exp.sum() == len(c.keys) == te.distinct_senders and te.power == sum(VC.final_powers(c.addrs, c.powers)[a] for a in c.keys)
            for temp in ("cold", "warm"):
                got, t = bv.is_valid_committed_seal(hs, sigs, claimed)
                assert (got == exp).all(), (name, temp, [VC.rows(name)[i].what for i in np.nonzero(got != exp)[0]])
                assert _fields(t) == _fields(te), (name, temp)
                if name == "decoys":   # (its decoys never get a key table: a cold pass of the pinned width behind every warm one;
                    assert bv.last_dispatch()[0] == lanes   # in the chains every member has one and the warm kernel decides every row)
    finally:
        bv.close()


@pytest.mark.parametrize("flags", [0, 2])
def test_emit_route_names_signer_and_index(oracle, flags):
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=flags, max_rows=1024)
    try:
        for name in NAMES:
            c, col, power, vs = _setup(oracle, name)
            bv.set_validators(1, col, power)
            rws = VC.rows(name)
            hs, sigs, _ = VC.columns(rws)
            who = np.zeros((len(rws), 20), np.uint8)
            idx = np.full(len(rws), -1, np.int32)
            for i, r in enumerate(rws):
                a = oracle.recover_address(r.hash, r.sig)
                if a is not None:
                    who[i] = np.frombuffer(a, np.uint8)
                    idx[i] = VC.list_index(c.addrs, a) if vs.index(a) >= 0 else -1
            te = oracle.tally(vs, who, (idx >= 0).astype(np.uint8))
            for _ in range(2 if flags else 1):
                signer, vidx, bits, t = bv.recover_seals(hs, sigs)
                assert (signer == who).all() and vidx.tolist() == idx.tolist() and (bits == (idx >= 0)).all(), name
                assert _fields(t) == _fields(te), name
            assert (idx >= 0).sum() >= len(c.keys) and (idx < 0).sum() >= 6
    finally:
        bv.close()


@pytest.mark.parametrize("flags", [0, 2])
def test_sender_route_looks_the_from_address_up(oracle, flags):
    """envelope signatures over keccak256(payload): From is the claimed address of the seal rows"""
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=flags, max_rows=1024)
    try:
        for name in NAMES:
            c, col, power, vs = _setup(oracle, name)
            bv.set_validators(1, col, power)
            rws = VC.rows(name)
            chunks = [b"envelope of row %d of %s" % (i, name.encode()) + bytes(i) for i in range(len(rws))]
            sigs = []
            for r, ch in zip(rws, chunks):
                sig = oracle.sign(r.sk, oracle.keccak256(ch))
                sigs.append(sig if r.what != "nothing" else VC.spoil(sig, 0 if r.sig[64] == 2 else 1))
            off = np.concatenate([[0], np.cumsum([len(ch) for ch in chunks])]).astype(np.uint32)
            payload = b"".join(chunks)
            sig65 = np.frombuffer(b"".join(sigs), np.uint8).reshape(-1, 65)
            frm = VC.columns(rws)[2]
            exp = oracle.verify_senders(vs, payload, off, sig65, frm).astype(bool)
            te = oracle.tally(vs, frm, exp.astype(np.uint8))
            assert exp.sum() == len(c.keys)
            for _ in range(2 if flags else 1):
                got, t = bv.is_valid_validator(payload, off, sig65, frm)
                assert (got == exp).all(), (name, np.nonzero(got != exp)[0])
                assert _fields(t) == _fields(te), name
    finally:
        bv.close()


def _expect_prepare(vm, proposer: bytes, senders, verdict):
    """HasPrepareQuorum(state, proposalMessage{From: proposer}, the messages whose verdict bit is set) by the plain big-int rule"""
    msgs = [Msg(bytes(s)) for s, v in zip(senders, verdict) if v]
    members = set(vm.power)
    seated = ({bytes(proposer)} | {m.sender for m in msgs}) & members
    return (vm.has_prepare_quorum(Msg(bytes(proposer)), msgs), sum(vm.power[a] for a in seated), len(seated),
            sum(1 for m in msgs if m.sender == bytes(proposer)))


@pytest.mark.parametrize("name", NAMES)
def test_tally_route_counts_exactly_the_members(oracle, name):
    """lookup_kernel behind ibft_tally and ibft_tally_prepare: sender columns that mix members, decoys as senders and
    outsiders; the proposer a member deep in the chain, a decoy that IS a member, and a one-word neighbour that is NOT"""
    import go_ibft_amd.verifier as V
    from oracle.semantics import ValidatorManager
    c, col, power, vs = _setup(oracle, name)
    members = VC.distinct(c.addrs)
    outs = [o.addr for o in c.outsiders]
    rng = np.random.default_rng(len(name))
    vm = ValidatorManager()
    assert vm.init(VC.final_powers(c.addrs, c.powers))
    deep = c.A if c.A is not None else c.addrs[-1]
    neighbour = next(o.addr for o in c.outsiders if o.sk is None and o.where == "head" and (c.A is None or o.near == c.A))
    near = next(o.near for o in c.outsiders if o.addr == neighbour)
    assert near in members and len(VC.differing_words(neighbour, near)) == 1 and (c.A is None or near == c.A)
    proposers = [deep, c.decoys[0] if c.decoys else c.addrs[0], neighbour]
    assert vs.index(proposers[0]) >= 0 and vs.index(proposers[1]) >= 0 and vs.index(neighbour) == -1
    bv = V.BatchVerifier(max_rows=1024)
    try:
        bv.set_validators(1, col, power)
        for trial in range(6):
            pick = members + outs if trial == 0 else [(members + outs)[j] for j in rng.integers(0, len(members) + len(outs), 70)]
            if trial == 1:
                pick = [a for a in members[::2]] + outs                  # every second member: the power names them
            send = VC.addr_column(pick)
            verdict = np.ones(len(pick), bool) if trial < 2 else rng.random(len(pick)) < (0.9, 0.7, 0.5, 0.3)[trial - 2]
            te = oracle.tally(vs, send, verdict.astype(np.uint8))
            assert _fields(bv.has_quorum(send, verdict)) == _fields(te), trial
            if trial == 1:
                assert te.power == sum(VC.final_powers(c.addrs, c.powers)[a] for a in members[::2])
            for k, proposer in enumerate(proposers):
                want, pw, seated, prows = _expect_prepare(vm, proposer, pick, verdict)
                t = bv.has_prepare_quorum(send, verdict, proposer)
                w = bv.last_tally_wide()
                assert (bool(t.has_quorum), w.power, t.distinct_senders, t.proposer_rows, t.valid_rows) == \
                       (want, pw, seated, prows, int(verdict.sum())), (trial, k)
        # the neighbour as proposer adds no seat: never taken for the member one word away
        none = np.zeros((0, 20), np.uint8)
        for proposer, seat in zip(proposers, (vm.power[proposers[0]], vm.power[proposers[1]], 0)):
            t = bv.has_prepare_quorum(none, np.zeros(0, bool), proposer)
            assert (bv.last_tally_wide().power, t.distinct_senders) == (seat, 1 if seat else 0)
    finally:
        bv.close()


@pytest.mark.parametrize("name", NAMES)
def test_family_of_sets_over_one_colliding_union(oracle, name):
    """three sets over one union table: the whole chain, every second member, and a part of it WITHOUT its deepest signer
    (for `decoys`: the ten decoys without A); one block per set, every row of the corpus in each.  A signer valid under set 0
    is cleared under set 2 although set 2 holds the entries it collides with"""
    import go_ibft_amd.verifier as V
    c, col, power, _ = _setup(oracle, name)
    members = VC.distinct(c.addrs)
    deep = c.A if c.A is not None else members[-1]
    part = list(c.decoys + c.bit_decoys) if c.A is not None else members[:10]
    sets = [list(c.addrs), members[::2], part]
    assert deep in sets[0] and deep not in sets[2]
    pw = [list(c.powers), [1 << i for i in range(len(sets[1]))], [3 << i for i in range(len(sets[2]))]]
    vss = [oracle.ValSet(VC.addr_column(s), np.array(p, np.uint64)) for s, p in zip(sets, pw)]
    rws = VC.rows(name)
    n = len(rws)
    hs, sigs, claimed = (np.concatenate([x] * 3) for x in VC.columns(rws))
    off = np.array([0, n, 2 * n, 3 * n], np.uint32)
    bh = np.zeros((3, 32), np.uint8)              # (the rows carry their own digests below: one hash per block is the call's form)
    # one digest per block: re-sign every row over its block's hash
    for b in range(3):
        bh[b] = np.frombuffer(VC.digest(b"%s-block-%d" % (name.encode(), b)), np.uint8)
        for i, r in enumerate(rws):
            sig = oracle.sign(r.sk, bh[b].tobytes())
            sigs[b * n + i] = np.frombuffer(sig if r.what != "nothing" else VC.spoil(sig, 0 if r.sig[64] == 2 else 1), np.uint8)
            hs[b * n + i] = bh[b]
    exp = np.zeros(3 * n, bool)
    who = np.zeros((3 * n, 20), np.uint8)
    idx = np.full(3 * n, -1, np.int32)
    for b in range(3):
        sl = slice(b * n, (b + 1) * n)
        exp[sl] = oracle.verify_seals(vss[b], hs[sl], sigs[sl], claimed[sl]).astype(bool)
        for i in range(b * n, (b + 1) * n):
            a = oracle.recover_address(hs[i].tobytes(), sigs[i].tobytes())
            if a is not None:
                who[i] = np.frombuffer(a, np.uint8)
                idx[i] = VC.list_index(sets[b], a) if vss[b].index(a) >= 0 else -1
    i_deep = next(i for i, r in enumerate(rws) if r.what == "member" and r.claimed == deep)
    assert exp[i_deep] and not exp[2 * n + i_deep] and idx[i_deep] == len(members) - 1 and idx[2 * n + i_deep] == -1
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=1024)
    try:
        bv.set_validator_sets([(VC.addr_column(s), np.array(p, np.uint64)) for s, p in zip(sets, pw)])
        assert bv.validator_sets_info()[:2] == (3, len(members))
        for temp in ("cold", "warm"):
            got, tl = bv.verify_block_seals_sets(bh, off, [0, 1, 2], sigs, claimed)
            assert (got == exp).all(), (temp, np.nonzero(got != exp)[0])
            signer, vidx, bits, rtl = bv.recover_block_seals_sets(bh, off, [0, 1, 2], sigs)
            assert (signer == who).all() and vidx.tolist() == idx.tolist() and (bits == (idx >= 0)).all(), temp
            for b in range(3):
                sl = slice(b * n, (b + 1) * n)
                assert _fields(tl[b]) == _fields(oracle.tally(vss[b], claimed[sl], exp[sl].astype(np.uint8))), (temp, b)
                assert _fields(rtl[b]) == _fields(oracle.tally(vss[b], who[sl], (idx[sl] >= 0).astype(np.uint8))), (temp, b)
    finally:
        bv.close()


def test_decoys_with_256_bit_powers(oracle):
    """set_validators_u256: member i has power 1 << (4·i + 200) — the wide sum still names the indices that were counted"""
    import go_ibft_amd.verifier as V
    c, col, power, vs = _setup(oracle, "decoys")
    wide = [1 << (4 * i + 200) for i in range(len(c.addrs))]
    final = VC.final_powers(c.addrs, wide)
    hs, sigs, claimed = VC.columns(VC.rows("decoys"))
    exp = oracle.verify_seals(vs, hs, sigs, claimed).astype(bool)
    total = sum(final.values())
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=1024)
    try:
        bv.set_validators_u256(1, col, wide)
        for temp in ("cold", "warm"):
            got, t = bv.is_valid_committed_seal(hs, sigs, claimed)
            w = bv.last_tally_wide()
            assert (got == exp).all(), temp
            assert (w.power, w.quorum, t.distinct_senders, t.valid_rows) == \
                   (final[c.A] + final[c.twice], 2 * total // 3 + 1, 2, int(exp.sum())), temp
        send = VC.addr_column(VC.distinct(c.addrs) + [o.addr for o in c.outsiders])
        t = bv.has_quorum(send, np.ones(len(send), bool))
        w = bv.last_tally_wide()
        assert (w.power, t.distinct_senders, bool(t.has_quorum)) == (total, len(final), True)
    finally:
        bv.close()
