"""IBFT_FLAG_WIRE_RECODE on the GPU: the flat wire calls judge PREPARE / COMMIT messages in a non-canonical encoding (the
recode class, include/ibftgpu.h) as their canonical re-encoding.  THE CONTRACT checked here: every output of a flag-on call
equals the flag-off call's on the batch rebuilt from the model's canonical bytes (wire_recode_model.py), but for pad[0]."""
import random

import numpy as np
import pytest

import wire_recode_cases as RC
import wire_recode_model as RM
from oracle import wire_parse as WP

pytestmark = pytest.mark.gpu

HEIGHT, ROUND = 12, 3  # the corpus round's view


def tally_tuple(t):
    return tuple(int(getattr(t, f[0])) for f in type(t)._fields_)


def rows_but_recoded(rows):
    out = rows.copy()
    out["pad"][:, 0] = 0
    return out.tobytes()


class World:
    def __init__(self):
        import go_ibft_amd.verifier as V
        self.V = V
        self.r, self.rows = RC.corpus()
        self.parts = RC.signed_parts(self.r)
        self.off_bv = V.BatchVerifier(flags=0, max_rows=8192)
        self.on_bv = V.BatchVerifier(flags=V.FLAG_WIRE_RECODE, max_rows=8192)
        for bv in (self.off_bv, self.on_bv):
            bv.set_validators(1, self.r.addrs, self.r.power)
        rng = random.Random(99)
        self.scrambled = [(m, p) for _, m, p in self.rows if p is not None and m != p.canonical]
        self.hopeless = [m for _, m in RC.named_out_of_class(self.parts[0])]
        rng.shuffle(self.scrambled)

    def close(self):
        self.off_bv.close()
        self.on_bv.close()

    def mixed(self, n):
        """n rows: canonical ones, and flagged ones — scrambled or hopeless — in only part of a wavefront: rows 10 … 20, the
        last row, and everything from row 128 on; rows 64 … 127 are a wavefront with nothing to recode"""
        msgs, honest = [], []
        for i in range(n):
            flagged = 10 <= i < 21 or i == n - 1 or i >= 128
            if flagged and i % 3 == 0 and i != n - 1:
                msgs.append(self.hopeless[i % len(self.hopeless)])
                honest.append(False)
            elif flagged:
                msgs.append(self.scrambled[i % len(self.scrambled)][0])
                honest.append(True)
            else:
                msgs.append(self.parts[i % len(self.parts)].canonical)
                honest.append(True)
        return msgs, np.array(honest)

    def check_senders(self, bv, msgs, honest=None):
        """flag-on call on msgs against the flag-off call on the rebuilt batch; returns the flag-on results"""
        model = [RM.canonical(m) for m in msgs]
        got, rows, t = bv.is_valid_validator_wire(*RC.pack(msgs))
        want, want_rows, want_t = self.off_bv.is_valid_validator_wire(*RC.pack([c for _, c in model]))
        assert (got == want).all(), np.nonzero(got != want)[0][:10]
        assert rows_but_recoded(rows) == want_rows.tobytes()
        assert tally_tuple(t) == tally_tuple(want_t)
        recoded = np.array([inside and WP.expected(m).status != WP.OK for m, (inside, _) in zip(msgs, model)], dtype=bool)
        assert (rows["pad"][:, 0] == recoded).all() and not rows["pad"][:, 1:].any()
        assert [int(s) for s in rows["status"]] == [WP.OK if inside else WP.NEEDS_HOST for inside, _ in model]
        if honest is not None:
            assert got[honest].all() and not got[~honest].any()
        return got, rows, t, recoded


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_mixed_batches(world, n):
    """canonical, recodable and hopeless rows; every honestly signed row, scrambled or not, has its sender bit SET"""
    msgs, honest = world.mixed(n)
    got, rows, t, recoded = world.check_senders(world.on_bv, msgs, honest)
    assert recoded.sum() >= 1 and got.sum() == honest.sum()


def test_random_corpus_in_one_call(world):
    """every named case, 3 000 random compositions of the scramblers and their fuzzed copies against the model"""
    msgs = [m for _, m, _ in world.rows]
    honest = np.array([p is not None for _, _, p in world.rows])
    got, rows, t, recoded = world.check_senders(world.on_bv, msgs)
    assert got[honest].all() and recoded.sum() > 2500 and (rows["status"] == WP.NEEDS_HOST).sum() > 300


def test_all_canonical_batch_is_bit_for_bit_the_flag_off_output(world):
    msgs = [p.canonical for p in world.parts] * 9  # 144 rows
    wire, off = RC.pack(msgs)
    got, rows, t = world.on_bv.is_valid_validator_wire(wire, off)
    want, want_rows, want_t = world.off_bv.is_valid_validator_wire(wire, off)
    assert (got == want).all() and got.all() and rows.tobytes() == want_rows.tobytes() and tally_tuple(t) == tally_tuple(want_t)
    assert world.on_bv.wire_stats() == (len(msgs), 0, 0)
    s, v, rows2, t2 = world.on_bv.verify_messages_wire(wire, off, HEIGHT, ROUND, raw=world.r.raw)
    ws, wv, wrows2, wt2 = world.off_bv.verify_messages_wire(wire, off, HEIGHT, ROUND, raw=world.r.raw)
    assert (s == ws).all() and (v == wv).all() and rows2.tobytes() == wrows2.tobytes() and tally_tuple(t2) == tally_tuple(wt2)
    assert world.on_bv.wire_stats() == (len(msgs), 0, 0)


def test_a_wavefront_longer_than_the_staging_buffer(world):
    """64 messages of more than 32 KiB together — each repeats its From field 30 times: the direct-HBM path"""
    msgs = []
    for i in range(64):
        p = world.parts[i % len(world.parts)]
        msgs.append((b"\x12\x14" + bytes([i]) * 20) * 29 + RC.spell(p, RC.Options(shuffle=random.Random(i), width=2)))
    assert sum(len(m) for m in msgs) > 32 * 1024
    got, rows, t, recoded = world.check_senders(world.on_bv, msgs, np.ones(64, dtype=bool))
    assert recoded.all()


def test_messages_wire_on_a_commit_round_with_every_third_row_scrambled(world):
    parts = RC.signed_parts(world.r, kinds=("commit",)) * 5  # 80 COMMITs
    rng = random.Random(5)
    msgs = [RC.spell(p, RC.random_options(rng)) if i % 3 == 0 else p.canonical for i, p in enumerate(parts)]
    canon = [p.canonical for p in parts]
    assert all(RM.canonical(m) == (True, c) for m, c in zip(msgs, canon))
    wire, off = RC.pack(msgs)
    cwire, coff = RC.pack(canon)
    s, v, rows, t = world.on_bv.verify_messages_wire(wire, off, HEIGHT, ROUND, raw=world.r.raw)
    ws, wv, wrows, wt = world.off_bv.verify_messages_wire(cwire, coff, HEIGHT, ROUND, raw=world.r.raw)
    assert (s == ws).all() and s.all() and (v == wv).all() and v.sum() > 40
    assert rows_but_recoded(rows) == wrows.tobytes() and tally_tuple(t) == tally_tuple(wt)
    _, _, cls, _ = world.on_bv.verify_messages_wire(wire, off, HEIGHT, ROUND, raw=world.r.raw, want_rows=False)
    _, _, wcls, _ = world.off_bv.verify_messages_wire(cwire, coff, HEIGHT, ROUND, raw=world.r.raw, want_rows=False)
    assert (cls == wcls).all() and not (cls & world.V.WIRE_CLASS_NEEDS_HOST).any()
    # the seals the walks found, made the resident seal batch
    world.on_bv.is_valid_validator_wire(wire, off)
    world.on_bv.wire_stage_seals()
    seals, st = world.on_bv.seals_run()
    world.off_bv.is_valid_validator_wire(cwire, coff)
    world.off_bv.wire_stage_seals()
    wseals, wst = world.off_bv.seals_run()
    assert (seals == wseals).all() and seals.sum() > 40 and tally_tuple(st) == tally_tuple(wst)


def test_flag_off_leaves_scrambled_rows_to_the_host(world):
    msgs, honest = world.mixed(130)
    got, rows, t = world.off_bv.is_valid_validator_wire(*RC.pack(msgs))
    canonical = np.array([WP.expected(m).status == WP.OK for m in msgs])
    assert (~canonical).sum() > 10
    assert (rows["status"] == np.where(canonical, WP.OK, WP.NEEDS_HOST)).all() and not rows["pad"].any()
    assert (got == canonical).all()  # every canonical row here is honestly signed; the others: bit 0
    assert world.off_bv.wire_stats() == (130, 0, int((~canonical).sum()))


def test_wire_stats_agree_with_the_model(world):
    msgs = [m for _, m, _ in world.rows[:700]]
    model = [RM.canonical(m) for m in msgs]
    recoded = sum(inside and WP.expected(m).status != WP.OK for m, (inside, _) in zip(msgs, model))
    outside = sum(not inside for inside, _ in model)
    assert recoded > 50 and outside > 20
    world.on_bv.is_valid_validator_wire(*RC.pack(msgs))
    assert world.on_bv.wire_stats() == (len(msgs), recoded, outside)
    world.on_bv.verify_messages_wire(*RC.pack(msgs[:300]), HEIGHT, ROUND, raw=world.r.raw)
    model = model[:300]
    assert world.on_bv.wire_stats() == (300, sum(inside and WP.expected(m).status != WP.OK for m, (inside, _) in zip(msgs, model)),
                                        sum(not inside for inside, _ in model))


def test_the_environment_overrides_the_flag(world, monkeypatch):
    V = world.V
    msgs, honest = world.mixed(130)
    for env, flag in (("1", 0), ("0", V.FLAG_WIRE_RECODE)):
        monkeypatch.setenv("IBFT_WIRE_RECODE", env)
        bv = V.BatchVerifier(flags=flag, max_rows=1024)
        try:
            bv.set_validators(1, world.r.addrs, world.r.power)
            assert bv.wire_stats() == (0, 0, 0)  # nothing before the first flat wire call
            if env == "1":
                world.check_senders(bv, msgs, honest)
            else:
                got, rows, _ = bv.is_valid_validator_wire(*RC.pack(msgs))
                assert not rows["pad"].any() and bv.wire_stats()[1] == 0 and got.sum() < honest.sum()
        finally:
            bv.close()


def test_host_mirror_ingests_a_scrambled_round_like_the_canonical_one(world, oracle, monkeypatch):
    """IBFT_WIRE_RECODE=1 and nothing else: the mirror's wire ingest of a round whose every message is scrambled stores what
    it stores for the canonical round, decides the same quorums, and sends no row through the per-message host route"""
    import go_ibft_amd.hostlib as H
    import go_ibft_amd.verifier as V
    from oracle import wire as W
    import test_gpu_host as TH
    r = world.r
    proposal = W.IbftMessage(view=W.View(r.height, r.round), sender=r.addrs[0].tobytes(), type=W.PREPREPARE,
                             payload=W.preprepare_body(W.Proposal(r.raw, r.round), r.proposal_hash, None))
    proposal.signature = oracle.sign(r.sks[0], oracle.keccak256(proposal.payload_no_sig()))
    parts = [p for p in RC.signed_parts(r, kinds=("prepare",)) if p.sender != r.addrs[0].tobytes()] + RC.signed_parts(r, kinds=("commit",))
    rng = random.Random(17)
    canon = [p.canonical for p in parts]
    scr = [RC.spell(p, RC.random_options(rng)) for p in parts]
    assert sum(a != b for a, b in zip(canon, scr)) > len(parts) // 2
    powers = {r.addrs[i].tobytes(): int(r.power[i]) for i in range(r.n)}
    f1, f2, f3 = TH._oracle_verifier(oracle, r)
    monkeypatch.setenv("IBFT_WIRE_RECODE", "1")
    bv = V.BatchVerifier(max_rows=1024)
    out = []
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        for wires in (canon, scr):
            h = H.Host()
            assert h.vm_init(powers)
            h.set_state(r.height, r.round, proposal.encode())
            h.set_verifier(f1, f2, f3)
            h.attach_gpu(bv)
            h.use_batch(True)
            h.enable_quorum_index()
            res, asked, hits, calls = h.ingest_wire(wires)
            set_rows = h.last_set_rows()
            nums = [h.store_num(r.height, r.round, t) for t in (1, 2)]
            okp, prepared = h.handle_prepare(r.height, r.round)
            okc, seals = h.handle_commit(r.height, r.round)
            stored = [sorted(RM.canonical(x)[1] for x in h.store_get_valid(r.height, r.round, t)) for t in (1, 2)]
            out.append((res, (asked, hits, calls), set_rows, nums, okp, sorted(RM.canonical(x)[1] for x in prepared), okc, sorted(seals), stored))
            assert bv.wire_stats()[2] == 0  # no row of the last device call was left to the host
            h.close()
    finally:
        bv.close()
    assert out[0] == out[1]
    assert out[0][4] and out[0][6] and out[0][2] == len(parts) and all(x > 0 for x in out[0][0])
