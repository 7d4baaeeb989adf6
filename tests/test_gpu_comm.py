"""GPU: the multi-GPU exchange inside libibftgpu.so (ibft_comm_* / ibft_group_*) on the single-GPU test box.

World size 1 goes through the real RCCL communicator (pack / ncclAllReduce / unpack, double-buffered hand-off, the
group entry point).  World sizes 2, 3, 4 and 8 run as a group that lists device 0 several times: one context per
rank, every rank verifies its own ibft_shard_range of the rows, packs its verdict words + distinct-sender bitmap,
and the ONLY thing replaced is ncclAllReduce itself — RCCL accepts one rank per device, so the library sums the W
buffers with its own kernel (include/ibftgpu.h, ibft_group_create).  The merged result must equal ibft_verify_seals /
ibft_verify_senders / ibft_verify_messages on the whole batch and the CPU oracle, including when ONE SENDER HAS VALID
ROWS ON BOTH SIDES OF A SHARD SEAM (HasQuorum counts addresses, core/validator_manager.go:77-96, 147-155)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_comm_world1_exchange_equals_local_fetch(oracle):
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    r = W.make_round(3000, 31, byzantine=True, weighted=True)
    vs = oracle.ValSet(r.addrs, r.power)
    exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=8).astype(bool)
    te = oracle.tally(vs, r.signer20, exp.astype(np.uint8))
    bv = V.BatchVerifier(max_rows=4096)
    try:
        bv.set_validators(1, r.addrs, r.power)
        bv.comm_init(V.comm_unique_id(), 0, 1)
        bv.seals_stage(r.hash32, r.seal65, r.signer20, r.pre_flags)
        # pipelined as bench.py drives it: exchange k overlaps launch k+1, results consumed one pass later
        bv.seals_launch(1)
        for k in range(6):
            bv.seals_exchange(r.n)
            if k + 1 < 6:
                bv.seals_launch(1)
            if k >= 1:
                got, t = bv.seals_fetch_merged()
                assert (got == exp).all()
        got, t = bv.seals_fetch_merged()
        assert (got == exp).all()
        assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum, t.quorum) == \
               (te.power, te.valid_rows, te.distinct_senders, te.has_quorum, te.quorum)
        local, tl = bv.seals_fetch()     # the un-merged results are still the local ones
        assert (local == exp).all() and tl.power == te.power
        with pytest.raises(RuntimeError):
            bv.seals_fetch_merged() if bv._xq.append(r.n) is None else None   # nothing outstanding
        bv._xq.clear()
        with pytest.raises(RuntimeError, match="not this rank's shard"):
            bv.seals_exchange(r.n + 64)
        bv.comm_destroy()
    finally:
        bv.close()


@pytest.mark.parametrize("n", [1, 64, 1000, 4096, 9000])
def test_group_of_one_device_matches_oracle(oracle, n):
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    from oracle.semantics import ValidatorManager
    r = W.make_round(n, 77 + n, byzantine=n > 64, weighted=True)
    vs = oracle.ValSet(r.addrs, r.power)
    exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=8).astype(bool)
    te = oracle.tally(vs, r.signer20, exp.astype(np.uint8))
    g = V.DeviceGroup([0], max_rows_total=max(n, 1024))
    try:
        assert g.size == 1
        g.set_validators(1, r.addrs, r.power)
        for _ in range(2):
            got, t = g.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
            assert (got == exp).all()
            assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum) == \
                   (te.power, te.valid_rows, te.distinct_senders, te.has_quorum)
        # 256-bit powers through the group: the exchange carries 8 pieces instead of 2
        stakes = [(1 + int(p)) * 10**21 for p in r.power]
        vm = ValidatorManager()
        assert vm.init({bytes(r.addrs[i]): stakes[i] for i in range(n)})
        g.set_validators_u256(1, r.addrs, stakes)
        got, t = g.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
        assert (got == exp).all()
        w = g.last_tally_wide()
        senders = {bytes(r.signer20[i]) for i in np.nonzero(exp)[0]}
        assert w.power == sum(vm.power[a] for a in senders) and w.quorum == vm.quorum
        assert bool(t.has_quorum) == (w.power >= w.quorum)
    finally:
        g.close()


def test_bench_sharded_path_with_one_rank():
    """bench.py's N>1 code path (process group + the library's RCCL exchange, pipelined) forced with one rank on
    the single-GPU box; `python bench.py --gpus N` launches the same path under torch.distributed.run."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, IBFT_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29577")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "6", "--warmup", "2",
                          "--no-cpu-baseline", "--no-sequence", "--no-warm", "--no-sweep", "--no-certificates",
                          "--no-host-mirror", "--extended-steps", "0"], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])   # the JSON line is the last thing on stdout
    assert rec["n_gpus"] == 1 and rec["config"]["validators"] == 4096 and rec["value"] > 1e5
    assert rec["roofline"]["kernel"].startswith("ecrecover_")


# ---- world > 1 on one device ---------------------------------------------------------------------------------------

def _dup_round(n, seed, world, weighted=True, envelopes=False):
    """a Byzantine round of n rows over ≈ n/2 … n validators in which rows are REPEATED across shard seams: the rows
    just before every seam appear again just after it (same sender, same seal, same envelope), and a block of rows from
    the first shard is copied into the last one"""
    import go_ibft_amd.shard as S
    from oracle import workload as W
    r = W.make_round(n, seed, byzantine=True, weighted=weighted, with_envelopes=envelopes)
    cols = {k: np.array(getattr(r, k)) for k in ("hash32", "hash_len", "seal65", "signer20", "pre_flags", "msg_sig65")}
    off = np.array(r.off, dtype=np.int64)
    chunks = [r.payload[off[i]:off[i + 1]] for i in range(n)] if envelopes else None

    def copy_rows(dst, src, k):
        for c in cols.values():
            c[dst:dst + k] = c[src:src + k]
        if chunks is not None:
            chunks[dst:dst + k] = chunks[src:src + k]
        for j in range(k):
            r.kinds[dst + j] = r.kinds[src + j]
    for rank in range(1, world):
        lo, hi = S.shard_range(n, rank, world)
        k = min(7, hi - lo, lo)
        if k > 0:
            copy_rows(lo, lo - k, k)
    lo, hi = S.shard_range(n, world - 1, world)
    k = min(20, (hi - lo) // 2, S.shard_range(n, 0, world)[1] // 2)
    if world > 1 and k > 0:
        copy_rows(hi - k, 3, k)
    for name, c in cols.items():
        setattr(r, name, c)
    if chunks is not None:
        r.payload = b"".join(chunks)
        r.off = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint32)
    return r


@pytest.mark.parametrize("world,n", [(2, 200), (2, 4096), (3, 500), (3, 64), (4, 1000), (4, 8192), (8, 65), (8, 3000), (8, 1)])
def test_group_on_one_device_equals_single_device_and_oracle(oracle, gpu_verifier, world, n):
    """every rank's exchange_pack_kernel, the summed buffers, every rank's exchange_unpack_kernel — with ragged last
    shards (n = 200 / 3000), empty tail shards (n = 64, 65, 1) and senders straddling the seams"""
    import go_ibft_amd.verifier as V
    r = _dup_round(n, 4000 + 17 * world + n, world)
    vs = oracle.ValSet(r.addrs, r.power)
    exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=8).astype(bool)
    te = oracle.tally(vs, r.signer20, exp.astype(np.uint8))
    gpu_verifier.set_validators(1, r.addrs, r.power)
    one, t1 = gpu_verifier.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
    assert (one == exp).all() and (t1.power, t1.distinct_senders) == (te.power, te.distinct_senders)
    g = V.DeviceGroup([0] * world, max_rows_total=max(n, 64 * world))
    try:
        assert g.size == world and g.is_local
        g.set_validators(1, r.addrs, r.power)
        for rep in range(3):                       # the double-buffered slots are both used
            got, t = g.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
            assert (got == exp).all(), np.flatnonzero(got != exp)[:8]
            assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum, t.quorum) == \
                   (te.power, te.valid_rows, te.distinct_senders, te.has_quorum, te.quorum)
            assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum) == \
                   (t1.power, t1.valid_rows, t1.distinct_senders, t1.has_quorum)
        if n >= 200:
            assert t.shard_overlap > 0             # the duplicated rows were valid ones on both sides of a seam
    finally:
        g.close()


def test_straddling_sender_decides_the_quorum(oracle, gpu_verifier):
    """Weak #2 of the round-2 review as a scenario: four validators of power 1 (quorum 3); validators 0 and 1 each send
    TWO valid COMMITs that land in different shards, the others are silent.  Power must be 2 and has_quorum 0 — a
    merge that adds per-shard partial sums reports 4 ≥ 3 (a safety-side error against validator_manager.go:77-96)."""
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    base = W.make_round(4, 9)
    n = 128                                        # two shards of 64 rows
    h = np.tile(base.hash32[0], (n, 1)); s = np.zeros((n, 65), np.uint8); f = np.zeros((n, 20), np.uint8)
    pre = np.full(n, V.ROW_NIL, np.uint8)
    for row, v in ((5, 0), (70, 0), (9, 1), (100, 1)):
        s[row] = base.seal65[v]; f[row] = base.signer20[v]; pre[row] = 0
    vs = oracle.ValSet(base.addrs, base.power)
    exp = oracle.verify_seals(vs, h, s, f, pre).astype(bool)
    te = oracle.tally(vs, f, exp.astype(np.uint8))
    assert exp.sum() == 4 and (te.power, te.quorum, te.has_quorum, te.distinct_senders) == (2, 3, 0, 2)
    gpu_verifier.set_validators(1, base.addrs, base.power)
    _, t1 = gpu_verifier.is_valid_committed_seal(h, s, f, pre)
    assert (t1.power, t1.has_quorum, t1.distinct_senders) == (2, 0, 2)
    g = V.DeviceGroup([0, 0], max_rows_total=128)
    try:
        g.set_validators(1, base.addrs, base.power)
        got, t = g.is_valid_committed_seal(h, s, f, pre)
        assert (got == exp).all()
        assert (t.power, t.has_quorum, t.distinct_senders, t.valid_rows, t.shard_overlap) == (2, 0, 2, 4, 2)
        # a third validator (one row) tips it: 3 ≥ 3
        s[20] = base.seal65[2]; f[20] = base.signer20[2]; pre[20] = 0
        got, t = g.is_valid_committed_seal(h, s, f, pre)
        assert (t.power, t.has_quorum, t.distinct_senders, t.valid_rows) == (3, 1, 3, 5)
    finally:
        g.close()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_group_on_one_device_wide_powers_and_golden_fixture(oracle, world):
    """256-bit voting powers through the merged bitmap (the power is re-summed from 32-bit pieces on every rank), and
    the committed Byzantine fixture (tests/golden/round_n256_byz.npz) sharded W ways"""
    import os
    import go_ibft_amd.verifier as V
    from oracle.semantics import ValidatorManager
    n = 700
    r = _dup_round(n, 5100 + world, world)
    vs = oracle.ValSet(r.addrs, r.power)
    exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=8).astype(bool)
    stakes = [(1 + int(p)) * 10**21 * (2**64 if i % 3 == 0 else 1) for i, p in enumerate(r.power)]
    vm = ValidatorManager()
    assert vm.init({bytes(r.addrs[i]): stakes[i] for i in range(n)})
    g = V.DeviceGroup([0] * world, max_rows_total=1024)
    try:
        g.set_validators_u256(1, r.addrs, stakes)
        got, t = g.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
        assert (got == exp).all()
        w = g.last_tally_wide()
        members = {bytes(a) for a in r.addrs}
        senders = {bytes(r.signer20[i]) for i in np.nonzero(exp)[0]} & members
        assert w.power == sum(vm.power[a] for a in senders) and w.quorum == vm.quorum
        assert bool(t.has_quorum) == (w.power >= w.quorum) and t.distinct_senders == len(senders)
        fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "round_n256_byz.npz"))
        g.set_validators(int(fx["height"]), fx["addrs"], fx["power"])
        got, t = g.is_valid_committed_seal(fx["hash32"], fx["seal65"], fx["signer20"], fx["pre_flags"])
        assert (got == fx["exp_seals"].astype(bool)).all()
        assert t.power == int(fx["exp_power"][0]) | (int(fx["exp_power"][1]) << 64)
        assert (t.has_quorum, t.distinct_senders) == (int(fx["exp_has_quorum"]), int(fx["exp_distinct"]))
    finally:
        g.close()


@pytest.mark.parametrize("world,n,flags", [(2, 333, 0), (4, 1000, 0), (3, 4096, 0), (8, 700, 0), (2, 1000, 2)])
def test_group_senders_and_message_sets_on_one_device(oracle, gpu_verifier, world, n, flags):
    """ibft_group_verify_senders and ibft_group_verify_messages (a COMMIT set sharded by message, K = 2 verdict arrays
    in the exchange) ≡ the single-device calls ≡ the oracle; then the PREPARE form (no seals)"""
    import go_ibft_amd.verifier as V
    r = _dup_round(n, 6100 + world + n, world, envelopes=True)
    sig = r.msg_sig65.copy()
    for j, i in enumerate(np.random.default_rng(n).choice(n, size=max(1, n // 11), replace=False)):
        sig[i, j % 64] ^= 0x20                     # some forged envelopes
    r.msg_sig65 = sig
    vs = oracle.ValSet(r.addrs, r.power)
    senders = oracle.verify_senders(vs, r.payload, r.off, r.msg_sig65, r.signer20).astype(bool)
    hashes = oracle.verify_hashes(r.raw, r.round, r.hash32, r.hash_len).astype(bool)
    seals = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=8).astype(bool)
    g = V.DeviceGroup([0] * world, flags=flags, max_rows_total=max(n, 64 * world))
    try:
        g.set_validators(r.height, r.addrs, r.power)
        for rep in range(3 if flags else 1):       # with the key cache: cold, table build on every rank, warm
            got, t = g.is_valid_validator(r.payload, r.off, r.msg_sig65, r.signer20)
            assert (got == senders).all()
            te = oracle.tally(vs, r.signer20, senders.astype(np.uint8))
            assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum) == \
                   (te.power, te.valid_rows, te.distinct_senders, te.has_quorum)
            s, v, t = g.verify_messages(r.payload, r.off, r.msg_sig65, r.signer20, r.hash32, r.hash_len, r.seal65,
                                        valid_pre=r.pre_flags, raw=r.raw, round_=r.round)
            assert (s == senders).all(), np.flatnonzero(s != senders)[:16]
            assert (v == (hashes & seals)).all(), [(int(i), r.kinds[i], bool(hashes[i]), bool(seals[i]), bool(v[i]))
                                                   for i in np.flatnonzero(v != (hashes & seals))[:16]]
            te = oracle.tally(vs, r.signer20, (senders & hashes & seals).astype(np.uint8))
            assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum) == \
                   (te.power, te.valid_rows, te.distinct_senders, te.has_quorum)
        gpu_verifier.set_validators(r.height, r.addrs, r.power)
        s1, v1, t1 = gpu_verifier.verify_messages(r.payload, r.off, r.msg_sig65, r.signer20, r.hash32, r.hash_len, r.seal65,
                                                  valid_pre=r.pre_flags, raw=r.raw, round_=r.round)
        assert (s1 == s).all() and (v1 == v).all() and (t1.power, t1.distinct_senders) == (t.power, t.distinct_senders)
        s, v, t = g.verify_messages(r.payload, r.off, r.msg_sig65, r.signer20, r.hash32, r.hash_len,
                                    digest32=r.proposal_hash)
        assert (s == senders).all() and (v == hashes).all()
        te = oracle.tally(vs, r.signer20, (senders & hashes).astype(np.uint8))
        assert (t.power, t.valid_rows, t.has_quorum) == (te.power, te.valid_rows, te.has_quorum)
    finally:
        g.close()


# ---- BASELINE configs #4 and #5 at their stated sizes, on one device -------------------------------------------------
# (round-3 review, "missing" #1: N = 16 384 × 4 and N = 65 536 × 8 with 20 % bad seals existed only in bench.py's
# world == 8 leg, which no box had ever executed)

_BIG = {}


def _big_round(n, world, byzantine, envelopes):
    key = (n, world, byzantine, envelopes)
    if key not in _BIG:
        _BIG.clear()                               # one large round alive at a time
        if byzantine:
            _BIG[key] = _dup_round(n, 7000 + n + world, world, envelopes=envelopes)
        else:
            from oracle import workload as W
            _BIG[key] = W.make_round(n, 7000 + n + world, weighted=True, with_envelopes=envelopes)
    return _BIG[key]


@pytest.mark.parametrize("world,n,byzantine", [(4, 16384, False), (4, 16384, True), (8, 65536, True)])
def test_baseline_config_4_and_5_seals_at_size(oracle, gpu_verifier, world, n, byzantine):
    """config #4: 16 384 validators sharded 4 ways (honest, then the Byzantine mix); config #5: 65 536 validators, 8
    shards of 8 192 rows, 20 % bad seals cycling over all twelve corruption kinds (core/byzantine_test.go:258-290
    is the behaviour to hold), the rows before every seam repeated behind it.  Merged mask / power / distinct senders /
    has_quorum ≡ ibft_verify_seals on the whole batch ≡ the CPU oracle; u64 powers, then 256-bit powers
    (quorum over the address SET: core/validator_manager.go:77-96, 147-155)."""
    import go_ibft_amd.verifier as V
    from oracle.semantics import ValidatorManager
    from oracle import workload as W
    r = _big_round(n, world, byzantine, False)
    if byzantine:
        assert {k for k in r.kinds if k} == set(W.CORRUPTIONS)
        assert 0.15 < sum(1 for k in r.kinds if k) / n < 0.25
    vs = oracle.ValSet(r.addrs, r.power)
    exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=16).astype(bool)
    te = oracle.tally(vs, r.signer20, exp.astype(np.uint8))
    assert exp.all() if not byzantine else (0.7 < exp.mean() < 0.9)
    gpu_verifier.set_validators(1, r.addrs, r.power)
    one, t1 = gpu_verifier.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
    assert (one == exp).all()
    assert (t1.power, t1.valid_rows, t1.distinct_senders, t1.has_quorum, t1.quorum) == \
           (te.power, te.valid_rows, te.distinct_senders, te.has_quorum, te.quorum)
    g = V.DeviceGroup([0] * world, max_rows_total=n)
    try:
        assert g.size == world and g.is_local
        g.set_validators(1, r.addrs, r.power)
        for rep in range(2):
            got, t = g.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
            assert (got == exp).all(), np.flatnonzero(got != exp)[:8]
            assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum, t.quorum) == \
                   (te.power, te.valid_rows, te.distinct_senders, te.has_quorum, te.quorum)
        assert (t.shard_overlap > 0) == byzantine  # (_dup_round repeats valid rows across every seam)
        # 256-bit powers: the merged power is re-summed from 32-bit pieces over the OR of the W bitmap segments
        stakes = [(1 + int(p)) * 10**21 * (2**64 if i % 3 == 0 else 1) for i, p in enumerate(r.power)]
        vm = ValidatorManager()
        assert vm.init({bytes(r.addrs[i]): stakes[i] for i in range(n)})
        g.set_validators_u256(1, r.addrs, stakes)
        got, t = g.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
        assert (got == exp).all()
        w = g.last_tally_wide()
        members = {bytes(a) for a in r.addrs}
        senders = {bytes(a) for a in r.signer20[exp]} & members
        assert w.power == sum(vm.power[a] for a in senders) and w.quorum == vm.quorum
        assert bool(t.has_quorum) == (w.power >= w.quorum) and t.distinct_senders == len(senders)
    finally:
        g.close()


@pytest.mark.parametrize("world,n", [(4, 16384), (8, 65536)])
def test_baseline_config_4_and_5_message_sets_at_size(oracle, gpu_verifier, world, n):
    """the same two shapes as COMMIT message sets (ibft_group_verify_messages: envelope signatures + committed seals of
    every shard in one verdict launch per rank, K = 2 verdict arrays in the exchange), Byzantine seals plus forged
    envelopes ≡ ibft_verify_messages on one device ≡ the oracle's three separate predicates"""
    import go_ibft_amd.verifier as V
    r = _big_round(n, world, True, True)
    sig = r.msg_sig65.copy()
    for j, i in enumerate(np.random.default_rng(n).choice(n, size=n // 13, replace=False)):
        sig[i, j % 64] ^= 0x20
    vs = oracle.ValSet(r.addrs, r.power)
    senders = oracle.verify_senders(vs, r.payload, r.off, sig, r.signer20, nthreads=16).astype(bool)
    hashes = oracle.verify_hashes(r.raw, r.round, r.hash32, r.hash_len).astype(bool)
    seals = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags, nthreads=16).astype(bool)
    te = oracle.tally(vs, r.signer20, (senders & hashes & seals).astype(np.uint8))
    gpu_verifier.set_validators(r.height, r.addrs, r.power)
    s1, v1, t1 = gpu_verifier.verify_messages(r.payload, r.off, sig, r.signer20, r.hash32, r.hash_len, r.seal65,
                                              valid_pre=r.pre_flags, raw=r.raw, round_=r.round)
    assert (s1 == senders).all() and (v1 == (hashes & seals)).all()
    g = V.DeviceGroup([0] * world, max_rows_total=n)
    try:
        g.set_validators(r.height, r.addrs, r.power)
        for rep in range(2):
            s, v, t = g.verify_messages(r.payload, r.off, sig, r.signer20, r.hash32, r.hash_len, r.seal65,
                                        valid_pre=r.pre_flags, raw=r.raw, round_=r.round)
            assert (s == senders).all(), np.flatnonzero(s != senders)[:16]
            assert (v == (hashes & seals)).all(), np.flatnonzero(v != (hashes & seals))[:16]
            assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum) == \
                   (te.power, te.valid_rows, te.distinct_senders, te.has_quorum) == \
                   (t1.power, t1.valid_rows, t1.distinct_senders, t1.has_quorum)
    finally:
        g.close()
    _BIG.clear()
