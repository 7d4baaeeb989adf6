"""GPU: the signature edge grid of tests/sig_edge_cases.py — r, s and the digest on and next to 0, n, (n−1)/2, p and 2^256 —
through the cold kernel families at every lane width and the warm kernels behind them, the emitting form and the wire route,
under both low-s policies, against the oracle exactly.

The validator set is the 160 signers the oracle recovers somewhere in the grid plus, for each, the same address with one bit
flipped; every row of the grid appears twice, under its signer's name and under the flipped one."""
import numpy as np
import pytest

import sig_edge_cases as SE
import valset_collision_cases as VC

pytestmark = pytest.mark.gpu

LANES = [1, 2, 4, 8, 16, 64, 128]


def _members():
    s = list(SE.signers())
    return s + [SE.flipped(a) for a in s]


def _columns():
    """every grid row twice → (hash32, sig65, claimed20): under the name of the signer the oracle recovers without the strict
    rule (a fixed member where there is none) and under that name with one bit flipped"""
    g = SE.grid()
    names = [a if a is not None else SE.signers()[i % 160] for i, a in enumerate(SE.expected(0))]
    col = lambda xs, w: np.frombuffer(b"".join(xs), np.uint8).reshape(-1, w).copy()
    hs = col([r.hash for r in g] * 2, 32)
    sigs = col([r.sig for r in g] * 2, 65)
    claimed = col(names + [SE.flipped(a) for a in names], 20)
    return hs, sigs, claimed


def _fields(t):
    return int(t.power), int(t.valid_rows), int(t.distinct_senders), int(t.has_quorum)


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("lanes", LANES)
def test_seal_route_on_the_grid_cold_then_warm(oracle, lanes, strict, monkeypatch):
    import go_ibft_amd.verifier as V
    monkeypatch.setenv("IBFT_COLD_LANES", str(lanes))
    members = VC.addr_column(_members())
    power = np.arange(1, len(members) + 1, dtype=np.uint64)
    vs = oracle.ValSet(members, power)
    hs, sigs, claimed = _columns()
    exp = oracle.verify_seals(vs, hs, sigs, claimed, flags=strict, nthreads=16).astype(bool)
    te = oracle.tally(vs, claimed, exp.astype(np.uint8))
    accepted = {a for a in SE.expected(strict) if a is not None}
    # exactly the rows the oracle recovers, under the signer's own name; never under the flipped one
    assert exp[:2592].tolist() == [a is not None for a in SE.expected(strict)] and not exp[2592:].any()
    assert te.distinct_senders == len(accepted) and len(accepted) == 160
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE | (V.FLAG_STRICT_LOW_S if strict else 0), max_rows=8192)
    try:
        bv.set_validators(1, members, power)
        for temp in ("cold", "warm"):
            got, t = bv.is_valid_committed_seal(hs, sigs, claimed)
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, (temp, [(hex(r.r), hex(r.s), hex(r.z), r.v) for r in (SE.grid()[i % 2592] for i in bad[:4])])
            assert _fields(t) == _fields(te), temp
            assert bv.last_dispatch()[0] == lanes          # (the flipped members never get a key table: a cold pass every time)
        assert bv.cache_stats()[0] == len(accepted)
    finally:
        bv.close()


@pytest.mark.parametrize("strict", [0, 1])
def test_emit_route_on_the_grid(oracle, strict):
    import go_ibft_amd.verifier as V
    members = _members()
    col = VC.addr_column(members)
    power = np.arange(1, len(members) + 1, dtype=np.uint64)
    vs = oracle.ValSet(col, power)
    g = SE.grid()
    hs = np.frombuffer(b"".join(r.hash for r in g), np.uint8).reshape(-1, 32)
    sigs = np.frombuffer(b"".join(r.sig for r in g), np.uint8).reshape(-1, 65)
    who = np.zeros((len(g), 20), np.uint8)
    idx = np.full(len(g), -1, np.int32)
    for i, a in enumerate(SE.expected(strict)):
        if a is not None:
            assert vs.index(a) >= 0
            who[i] = np.frombuffer(a, np.uint8)
            idx[i] = members.index(a)
    te = oracle.tally(vs, who, (idx >= 0).astype(np.uint8))
    bv = V.BatchVerifier(flags=V.FLAG_STRICT_LOW_S if strict else 0, max_rows=8192)
    try:
        bv.set_validators(1, col, power)
        signer, vidx, bits, t = bv.recover_seals(hs, sigs)
        bad = np.nonzero((signer != who).any(axis=1))[0]
        assert len(bad) == 0, [(hex(g[i].r), hex(g[i].s), hex(g[i].z), g[i].v) for i in bad[:4]]
        assert vidx.tolist() == idx.tolist() and (bits == (idx >= 0)).all()
        assert _fields(t) == _fields(te) and te.valid_rows == (480, 240)[strict]
    finally:
        bv.close()


def test_wire_route_commit_seals_on_the_edges(oracle):
    """the rows of one digest (z = n: the reduction changes it) as COMMIT messages whose committed seal is the grid signature,
    each twice: From the grid's signer (the envelope, signed by somebody else, is refused; the seal is judged under that
    name) and From a real validator (a good envelope; the seal is somebody else's)"""
    import go_ibft_amd.verifier as V
    import wire_cases as WCASE
    from oracle import wire, wire_parse as WP
    keys = VC.key_pool(8)
    members = _members() + [k.addr for k in keys]
    col = VC.addr_column(members)
    power = np.arange(1, len(members) + 1, dtype=np.uint64)
    vs = oracle.ValSet(col, power)
    z = SE.N
    picked = [i for i, r in enumerate(SE.grid()) if r.z == z]
    assert len(picked) == 432 and sum(SE.expected(0)[i] is not None for i in picked) == 80
    msgs = []
    for j, i in enumerate(picked):
        row, k = SE.grid()[i], keys[j % len(keys)]
        name = SE.expected(0)[i] or SE.signers()[j % 160]
        for sender in (name, k.addr):
            m = wire.IbftMessage(view=wire.View(7, 0), sender=sender, type=wire.COMMIT, payload=wire.commit_body(row.hash, row.sig))
            m.signature = oracle.sign(k.sk, oracle.keccak256(m.payload_no_sig()))
            msgs.append(m.encode())
    buf, off = WCASE.pack(msgs)
    exps = [WP.expected(m) for m in msgs]
    assert all(e.status == WP.OK and not e.pre_flag for e in exps)
    want = np.zeros(len(exps), bool)
    senders = np.zeros((len(exps), 20), np.uint8)
    hash32 = np.zeros((len(exps), 32), np.uint8)
    seal65 = np.zeros((len(exps), 65), np.uint8)
    for i, e in enumerate(exps):
        got = oracle.recover_address(e.digest, e.signature)
        want[i] = got is not None and got == e.sender and vs.index(e.sender) >= 0
        senders[i] = np.frombuffer(e.sender, np.uint8)
        hash32[i] = np.frombuffer(e.proposal_hash, np.uint8)
        seal65[i] = np.frombuffer(e.committed_seal, np.uint8)
    assert want[1::2].all() and not want[0::2].any()
    exp_seals = oracle.verify_seals(vs, hash32, seal65, senders).astype(bool)
    assert exp_seals.sum() == 80 and not exp_seals[1::2].any()
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=1024)
    try:
        bv.set_validators(7, col, power)
        for temp in ("cold", "warm"):
            got, rows, t = bv.is_valid_validator_wire(buf, off)
            assert (rows["status"] == 0).all() and (got == want).all(), temp
            ot = oracle.tally(vs, senders, want.astype(np.uint8))
            assert _fields(t) == _fields(ot)
            bv.wire_stage_seals()
            bv.seals_launch(1)
            seals, _ = bv.seals_fetch()
            bad = np.nonzero(seals != exp_seals)[0]
            assert len(bad) == 0, (temp, [(hex(r.r), hex(r.s), r.v) for r in (SE.grid()[picked[i // 2]] for i in bad[:4])])
    finally:
        bv.close()
