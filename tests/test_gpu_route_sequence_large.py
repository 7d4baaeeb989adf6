"""GPU: four entry points in sequence on one cold context of 98 304 rows, chosen so that each leaves the work mask in the
state the next one trusts:

 1. a small message set — the verdict rows double, the mask buffer gets its final size;
 2. is_valid_proposal_hash over 98 304 matching rows — ballot words [0, 1536) all ones, no tally: the context records 1 536
    dirty words;
 3. a COMMIT set of 20 000 messages — 40 032 verdict rows, which the lane kernel takes: whole words stored, nothing cleared in
    front; its combine step and tally consume words [0, 626);
 4. is_valid_committed_seal over 70 000 rows — two launches; the 4 464 rows beyond 65 536 go through a kernel that ORs its bits
    into words [1024, 1094), and a third of those rows carry a stolen seal.

Words [626, 1536) still hold the ones of step 2 after step 3: if step 3 records a clean mask, step 4 clears nothing and the
stolen seals come out valid — which is what happened while the step behind a set's verdict launch reset the record
unconditionally: every one of the 2 039 rows the oracle rejects among the 4 464 beyond 65 536 came out accepted, on both
legs.  Every bit and every tally field is the CPU oracle's (tests/route_pair_cases.py: Sequence;
the share of forged rows beyond the split: tests/test_route_pair_inputs.py).  Step 3 runs once through ibft_verify_messages
and once through ibft_verify_messages_wire, which share the step behind the verdict launch."""
import numpy as np
import pytest

import route_pair_cases as RP

pytestmark = pytest.mark.gpu


def _tally(t):
    return RP._tally(t)


def _dirty_the_allocator(V, s):
    """fresh device memory is zero and hides stale words: a context that ran the hash pass frees a mask full of ones"""
    junk = V.BatchVerifier(max_rows=RP.SEQ_MAX_ROWS)
    try:
        junk.set_validators(s.r.height, s.r.addrs, s.r.power)
        m = s.set_step(RP.SEQ_BASE_ROWS)
        junk.verify_messages(m.payload, m.off, m.sig, m.signer20, m.hash32, m.hash_len, m.seal65, valid_pre=m.pre, raw=s.r.raw, round_=s.r.round)
        assert junk.is_valid_proposal_hash(s.r.raw, s.r.round, *s.hash_step()).all()
    finally:
        junk.close()


@pytest.mark.parametrize("leg", ["columns", "wire"])
def test_hash_pass_large_set_split_batch(oracle, leg):
    import go_ibft_amd.verifier as V
    s = RP.sequence()
    small, big, seals = s.set_step(RP.SEQ_BASE_ROWS), s.set_step(), s.seal_step()
    hashes = s.hash_step()
    r = s.r
    _dirty_the_allocator(V, s)
    bv = V.BatchVerifier(max_rows=RP.SEQ_MAX_ROWS)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        for rep in range(2):
            where = f"{leg} leg, pass {rep}"
            # 1
            sb, vb, t = bv.verify_messages(small.payload, small.off, small.sig, small.signer20, small.hash32, small.hash_len, small.seal65,
                                           valid_pre=small.pre, raw=r.raw, round_=r.round)
            assert (sb == small.sender).all() and (vb == small.valid).all() and _tally(t) == small.tally, (where, "step 1")
            # 2
            assert bv.is_valid_proposal_hash(r.raw, r.round, *hashes).all(), (where, "step 2")
            # 3
            if leg == "columns":
                sb, vb, t = bv.verify_messages(big.payload, big.off, big.sig, big.signer20, big.hash32, big.hash_len, big.seal65,
                                               valid_pre=big.pre, raw=r.raw, round_=r.round)
                ws, wv, wt = big.sender, big.valid, big.tally
            else:
                sb, vb, _, t = bv.verify_messages_wire(big.wire, big.woff, r.height, r.round, raw=r.raw, want_rows=False)
                ws, wv, wt = big.w_sender, big.w_valid, big.w_tally
            assert bv.last_dispatch()[0] == 1 and bv.last_cold_table() == 1, (where, "step 3 did not take the lane kernel", bv.last_dispatch())
            assert (sb == ws).all(), (where, "step 3 sender rows", np.flatnonzero(sb != ws)[:10])
            assert (vb == wv).all(), (where, "step 3 valid rows", np.flatnonzero(vb != wv)[:10])
            assert _tally(t) == wt, (where, "step 3", _tally(t), wt)
            # 4
            split_before = bv.pipeline_stats()[1]
            got, t = bv.is_valid_committed_seal(seals.hash32, seals.seal65, seals.signer20, seals.pre)
            assert bv.pipeline_stats()[1] == split_before + 1, (where, "step 4 did not go out as two launches")
            bad = np.flatnonzero(got != seals.bits)
            assert len(bad) == 0, (f"{where}, step 4: {len(bad)} rows differ, the first at {bad[:10].tolist()}; "
                                   f"{int(got[bad].sum())} of them accepted, {int(seals.forged[bad].sum())} of them with a stolen seal")
            assert _tally(t) == seals.tally, (where, "step 4", _tally(t), seals.tally)
    finally:
        bv.close()
