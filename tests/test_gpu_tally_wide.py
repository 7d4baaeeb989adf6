"""GPU: the weighted quorum tally (a8) with arbitrary-precision voting powers and across several tally
workgroups.  Oracle = oracle/semantics.ValidatorManager (Python big ints restating
/root/reference/core/validator_manager.go:61-135 — GetVotingPowers returns *big.Int)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# /root/reference/core/validator_manager_test.go:18-187 (Test_CalculateQuorum): powers, signers, hasQuorum
REF_TABLE = [
    ({'A': 1, 'B': 1, 'C': 1, 'D': 1}, ['A', 'B', 'C', 'D'], True),
    ({'A': 1, 'B': 1, 'C': 1, 'D': 1}, ['A', 'B'], False),
    ({'A': 1, 'B': 1, 'C': 1, 'D': 1, 'E': 1, 'F': 1}, ['A', 'B', 'C', 'D', 'E'], True),
    ({'A': 1, 'B': 1, 'C': 1, 'D': 1, 'E': 1, 'F': 1}, ['A', 'B', 'C', 'D'], False),
    ({'A': 2, 'B': 2, 'C': 2, 'D': 3}, ['A', 'C', 'D'], True),
    ({'A': 2, 'B': 2, 'C': 2, 'D': 3}, ['A', 'D'], False),
    ({'A': 2, 'B': 2, 'C': 3, 'D': 3}, ['A', 'B', 'D'], True),
    ({'A': 2, 'B': 2, 'C': 3, 'D': 3}, ['A', 'D'], False),
    ({'A': 2, 'B': 7, 'C': 7, 'D': 5}, ['A', 'B', 'C'], True),
    ({'A': 2, 'B': 7, 'C': 7, 'D': 5}, ['C', 'D'], False),
]


def _addr(name: str) -> bytes:
    return name.encode() * 20


@pytest.mark.parametrize("scale", [1, 10**18, 10**18 * 2**64 + 12345, (2**256 - 1) // 7])
def test_reference_quorum_table_with_scaled_powers(scale):
    """Test_CalculateQuorum with every power multiplied by `scale` (1: also through the u64 entry point):
    the decision of HasQuorum is scale-invariant only up to the floor in ⌊2·total/3⌋+1, so the expected value
    comes from the big-int oracle, and at scale 1 it must equal the reference's own table."""
    import go_ibft_amd.verifier as V
    from oracle.semantics import ValidatorManager
    bv = V.BatchVerifier(max_rows=1024)
    try:
        for powers, signers, want in REF_TABLE:
            names = sorted(powers)
            addrs = np.frombuffer(b"".join(_addr(n) for n in names), np.uint8).reshape(-1, 20)
            pw = [powers[n] * scale for n in names]
            vm = ValidatorManager()
            assert vm.init({_addr(n): powers[n] * scale for n in names})
            expect = vm.has_quorum([_addr(s) for s in signers])
            if scale == 1:
                assert expect == want
            entry = [bv.set_validators_u256] + ([bv.set_validators] if scale == 1 else [])
            for setv in entry:
                setv(1, addrs, pw)
                send = np.frombuffer(b"".join(_addr(s) for s in signers), np.uint8).reshape(-1, 20)
                t = bv.has_quorum(send, np.ones(len(signers), bool))
                w = bv.last_tally_wide()
                assert bool(t.has_quorum) == expect and bool(w.has_quorum) == expect
                assert w.quorum == vm.quorum and w.power == sum(powers[s] * scale for s in signers)
                assert t.power == w.power & (2**128 - 1) and t.quorum == w.quorum & (2**128 - 1)
    finally:
        bv.close()


@pytest.mark.parametrize("n,wide", [(300, False), (5000, False), (5000, True), (65536, False), (65536, True), (70000, True)])
def test_tally_over_many_workgroups_with_duplicates_and_nonmembers(n, wide):
    """ibft_tally on a caller-supplied mask: random verdict bits, every third sender duplicated somewhere else
    in the batch (counted once), a tenth of the senders not in the set; n > 4096 spans several tally workgroups
    (device-scope bitmap + ticket).  Run twice: the kernel must leave its bitmap / accumulators clean."""
    import go_ibft_amd.verifier as V
    from oracle.semantics import ValidatorManager
    rng = np.random.default_rng(n + wide)
    nv = n * 9 // 10
    addrs = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    if wide:
        powers = [int.from_bytes(rng.bytes(32), "big") >> int(rng.integers(0, 200)) for _ in range(nv)]
        powers[0] = 2**256 - 1
    else:
        powers = [int(x) for x in rng.integers(1, 2**63, nv, dtype=np.uint64)]
        powers[0] = 2**64 - 1
    sender = addrs.copy()
    dup = rng.permutation(n)[: n // 3]
    sender[dup] = addrs[rng.integers(0, n, len(dup))]
    verdict = rng.random(n) < 0.7
    vm = ValidatorManager()
    assert vm.init({bytes(addrs[i]): powers[i] for i in range(nv)})
    counted = {bytes(sender[i]) for i in np.nonzero(verdict)[0]}
    exp_power = sum(vm.power.get(a, 0) for a in counted)
    exp_distinct = sum(1 for a in counted if a in vm.power)
    bv = V.BatchVerifier(max_rows=max(n, 1024))
    try:
        (bv.set_validators_u256 if wide else bv.set_validators)(1, addrs[:nv], powers)
        for _ in range(2):
            t = bv.has_quorum(sender, verdict)
            w = bv.last_tally_wide()
            assert (t.valid_rows, t.distinct_senders) == (int(verdict.sum()), exp_distinct)
            assert w.power == exp_power and w.quorum == vm.quorum
            assert bool(t.has_quorum) == (exp_power >= vm.quorum)
        # a mask that reaches the quorum exactly on the boundary: accumulate senders until power ≥ quorum
        order, acc, k = np.arange(nv), 0, 0
        while acc < vm.quorum:
            acc += powers[order[k]]
            k += 1
        for kk, want in ((k - 1, False), (k, True)):
            v2 = np.zeros(n, bool)
            v2[:kk] = True
            t = bv.has_quorum(addrs, v2)
            assert bool(t.has_quorum) == want and bv.last_tally_wide().power == sum(powers[:kk])
    finally:
        bv.close()


# The workgroup's distinct-sender bitmap is in LDS while ⌈validators / 32⌉ words fit 49 152 bytes: 48 · 1024 · 8 = 393 216
# validators is the largest LDS form; one validator more and tally_kernel sends every row's bit to the HBM bitmap directly.
LDS_VALIDATORS = 48 * 1024 * 8


class _Msg:
    def __init__(self, sender):
        self.sender = sender


@pytest.fixture(scope="module")
def huge_set():
    """LDS_VALIDATORS + 1 addresses with u64 and u256 powers, built once and left unchanged; validator 0 alone outweighs the rest"""
    rng = np.random.default_rng(393217)
    addrs = rng.integers(0, 256, (LDS_VALIDATORS + 1, 20), dtype=np.uint8)
    small = [int(x) for x in rng.integers(1, 2**40, LDS_VALIDATORS + 1, dtype=np.uint64)]
    p64 = [2**64 - 1] + small[1:]
    p256 = [2**256 - 1] + [x << (i % 190) for i, x in enumerate(small)][1:]
    keys = [bytes(a) for a in addrs]
    assert len(set(keys)) == len(keys)
    return addrs, keys, {False: p64, True: p256}


def _huge_rows(addrs, n):
    """n rows: duplicates inside a workgroup of 4 096 rows and — beyond 4 096 rows — across two, non-members, the set's last
    validators (index 393 215: the last bit of the LDS form; 393 216: a member of the HBM form only), failed verdicts"""
    rng = np.random.default_rng(n)
    nv = len(addrs)
    sender = addrs[rng.integers(1, nv - 2, n)].copy()
    sender[rng.permutation(n)[: n // 10]] = rng.integers(0, 256, (n // 10, 20), dtype=np.uint8)   # not in the set
    verdict = rng.random(n) < 0.7
    sender[5], sender[6], sender[17] = addrs[nv - 1], addrs[nv - 2], addrs[nv - 2]
    verdict[[5, 6, 17]] = True
    sender[30] = sender[40] = addrs[4321]    # the same validator twice in one workgroup
    verdict[[30, 40]] = True
    sender[31], verdict[31] = addrs[7], False    # a validator whose only row failed
    if n > 4096:
        sender[10] = sender[4500] = addrs[1234]  # the same validator among the valid rows of both workgroups
        sender[4600] = addrs[nv - 1]
        sender[4700] = addrs[0]                  # the heavy validator: this batch has the quorum
        verdict[[10, 4500, 4600, 4700]] = True
    return sender, verdict


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [300, 5000])
@pytest.mark.parametrize("nv", [LDS_VALIDATORS, LDS_VALIDATORS + 1])
def test_tally_at_the_edge_of_the_lds_bitmap(huge_set, nv, n, wide):
    """tally_kernel at the largest validator set whose bitmap is in LDS and at the first one beyond it (every row's bit set
    in HBM by the row itself, lds_bitmap = 0), over one workgroup and over two, u64 and u256 powers, on a caller-supplied
    mask.  Run twice on one context: the second run must find bitmap, accumulators and ticket zero."""
    import go_ibft_amd.verifier as V
    from oracle.semantics import ValidatorManager
    addrs, keys, powers = huge_set
    sender, verdict = _huge_rows(addrs, n)
    vm = ValidatorManager()
    assert vm.init(dict(zip(keys[:nv], powers[wide][:nv])))
    counted = {bytes(sender[i]) for i in np.nonzero(verdict)[0]}
    exp_power = sum(vm.power.get(a, 0) for a in counted)
    exp_distinct = sum(1 for a in counted if a in vm.power)
    assert (keys[LDS_VALIDATORS] in vm.power) == (nv > LDS_VALIDATORS) and keys[LDS_VALIDATORS] in counted
    assert (exp_power >= vm.quorum) == (n > 4096)
    bv = V.BatchVerifier(max_rows=LDS_VALIDATORS + 4096)
    try:
        (bv.set_validators_u256 if wide else bv.set_validators)(1, addrs[:nv], powers[wide][:nv])
        for _ in range(2):
            t = bv.has_quorum(sender, verdict)
            w = bv.last_tally_wide()
            assert (t.valid_rows, t.distinct_senders) == (int(verdict.sum()), exp_distinct)
            assert w.power == exp_power and w.quorum == vm.quorum
            assert bool(t.has_quorum) == (exp_power >= vm.quorum) and t.proposer_rows == 0
    finally:
        bv.close()


def test_prepare_quorum_seat_beyond_the_lds_bitmap(huge_set):
    """HasPrepareQuorum at LDS_VALIDATORS + 1 validators: the proposer — a member without a row, here the one validator that
    outweighs the rest — takes his seat in the HBM bitmap; plain HasQuorum before and after answers without him."""
    import go_ibft_amd.verifier as V
    from oracle.semantics import ValidatorManager
    addrs, keys, powers = huge_set
    sender, verdict = _huge_rows(addrs, 300)
    vm = ValidatorManager()
    assert vm.init(dict(zip(keys, powers[False])))
    msgs = [_Msg(bytes(sender[i])) for i in np.nonzero(verdict)[0]]
    counted = {m.sender for m in msgs}
    plain_power = sum(vm.power.get(a, 0) for a in counted)
    plain_distinct = sum(1 for a in counted if a in vm.power)
    assert keys[0] not in counted and not vm.has_quorum(counted) and vm.has_prepare_quorum(_Msg(keys[0]), msgs)
    bv = V.BatchVerifier(max_rows=LDS_VALIDATORS + 4096)
    try:
        bv.set_validators(1, addrs, powers[False])
        for _ in range(2):
            t = bv.has_quorum(sender, verdict)
            assert (bool(t.has_quorum), t.distinct_senders, bv.last_tally_wide().power) == (False, plain_distinct, plain_power)
            t = bv.has_prepare_quorum(sender, verdict, keys[0])
            w = bv.last_tally_wide()
            assert (bool(t.has_quorum), t.distinct_senders, t.proposer_rows, t.valid_rows) == (True, plain_distinct + 1, 0, int(verdict.sum()))
            assert w.power == plain_power + vm.power[keys[0]] and w.quorum == vm.quorum
    finally:
        bv.close()


def test_wide_powers_through_the_seal_path(oracle):
    """IsValidCommittedSeal + HasQuorum in one call with 256-bit powers (wei-denominated stakes)."""
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    from oracle.semantics import ValidatorManager
    r = W.make_round(200, 4242, byzantine=True)
    stakes = [(1 + (i * 7919) % 1000) * 10**18 * 32 for i in range(r.n)]   # 32 … 32 000 tokens in wei: > 2^64
    vm = ValidatorManager()
    assert vm.init({bytes(r.addrs[i]): stakes[i] for i in range(r.n)})
    vs = oracle.ValSet(r.addrs, r.power)
    exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags).astype(bool)
    bv = V.BatchVerifier(max_rows=1024)
    try:
        bv.set_validators_u256(1, r.addrs, stakes)
        got, t = bv.is_valid_committed_seal(r.hash32, r.seal65, r.signer20, r.pre_flags)
        assert (got == exp).all()
        w = bv.last_tally_wide()
        ok_senders = [bytes(r.signer20[i]) for i in np.nonzero(exp)[0]]
        assert w.power == sum(vm.power[a] for a in set(ok_senders)) and w.quorum == vm.quorum
        assert bool(t.has_quorum) == vm.has_quorum(ok_senders)
    finally:
        bv.close()
