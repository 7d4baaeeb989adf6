"""GPU: the MIXED pass — a warm kernel has decided some rows of a batch, a cold kernel takes the rest — under every cold form,
pinned by IBFT_COLD_LANES (and IBFT_ROWS_PAIR for the two row forms).  The rows the warm kernel marks and the rows left share
every wavefront, every lane group and every DPP row, so this is what holds the cold kernels' shared row head (done / need, the
stores a decided row must not repeat) to the oracle in each of them.

n = 133 = 2·64 + 5 = 33·4 + 1 rows: ragged for the lane kernel's 64-row blocks, for 2 / 4 / 8-lane groups, for the four rows of a
wavefront of the row forms and for the workgroups of the one- and two-wavefront forms.  The round is Byzantine and weighted, with
pre-flagged rows; every eleventh validator is left out of the set, so its row claims a NON-member.  Two legs, committed seals
(MODE_SEALS) and envelope senders (MODE_SENDERS), each with validator keys of its own: the key tables belong to the device and
outlive a context, so a key another leg, case or test has used would be warm from the start."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 133
CASES = [{"IBFT_COLD_LANES": "1"}, {"IBFT_COLD_LANES": "2"}, {"IBFT_COLD_LANES": "4"}, {"IBFT_COLD_LANES": "8"},
         {"IBFT_COLD_LANES": "64"}, {"IBFT_COLD_LANES": "128"},
         {"IBFT_COLD_LANES": "16", "IBFT_ROWS_PAIR": "0"}, {"IBFT_COLD_LANES": "16", "IBFT_ROWS_PAIR": "1"}]


def _round(seed):
    """(round, validator set addresses, powers, corrupted envelope signatures)"""
    from oracle import workload as W
    r = W.make_round(N, seed, byzantine=True, weighted=True, with_envelopes=True)
    member = np.arange(N) % 11 != 5
    assert (r.pre_flags != 0).any() and (r.pre_flags == 0).any() and not member.all()
    msg = r.msg_sig65.copy()                       # make_round signs every envelope honestly: some bad ones of our own
    for i in range(N):
        if i % 7 == 3:
            msg[i, 40] ^= 0x21                     # another s
        if i % 7 == 5:
            msg[i] = r.msg_sig65[(i + 1) % N]      # a neighbour's signature
    return r, r.addrs[member], r.power[member], msg


def _payload_rows(r, idx):
    chunks = [r.payload[int(r.off[i]):int(r.off[i + 1])] for i in idx]
    return b"".join(chunks), np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint32)


def _same_tally(oracle, vs, signer20, exp, t):
    te = oracle.tally(vs, signer20, exp.astype(np.uint8))
    assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum) == (te.power, te.valid_rows, te.distinct_senders, te.has_quorum)


@pytest.mark.parametrize("pins", CASES, ids=lambda p: "-".join(f"{k[5:].lower()}{v}" for k, v in p.items()))
def test_mixed_pass_under_every_pinned_cold_kernel(oracle, pins, monkeypatch):
    import go_ibft_amd.verifier as V
    for k, v in pins.items():
        monkeypatch.setenv(k, v)                   # (read when the context is created)
    lanes = int(pins["IBFT_COLD_LANES"])
    first = np.arange(0, N, 3)
    for leg in ("seals", "senders"):
        seed = 0x17C0DE00 + 32 * CASES.index(pins) + (leg == "senders")
        r, addrs, power, msg = _round(seed)
        vs = oracle.ValSet(addrs, power)
        pre = r.pre_flags
        if leg == "seals":
            exp = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, pre).astype(bool)
            run = lambda bv, idx: bv.is_valid_committed_seal(r.hash32[idx], r.seal65[idx], r.signer20[idx], pre[idx])
        else:
            exp = oracle.verify_senders(vs, r.payload, r.off, msg, r.signer20, pre).astype(bool)
            run = lambda bv, idx: bv.is_valid_validator(*_payload_rows(r, idx), msg[idx], r.signer20[idx], pre[idx])
        assert exp[first].any() and exp.any() and not exp.all()
        bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=1024)
        try:
            bv.set_validators(1, addrs, power)
            assert bv.cache_stats()[0] == 0, "these validators' keys must be new to the device"
            # rows 0, 3, 6, …: a cold pass that learns their keys; their tables are built behind it
            got, t = run(bv, first)
            assert bv.last_dispatch() == (lanes, 0)
            assert (got == exp[first]).all(), (leg, np.nonzero(got != exp[first])[0][:10])
            _same_tally(oracle, vs, r.signer20[first], exp[first], t)
            assert bv.cache_stats()[0] == int(exp[first].sum())
            # the full batch: the warm kernel decides the rows with a table, the pre-flagged ones and the non-members, the
            # pinned cold kernel the others — MIXED
            everything = np.arange(N)
            got, t = run(bv, everything)
            cold, warm = bv.last_dispatch()
            assert cold == lanes and warm > 0, (cold, warm)
            assert (got == exp).all(), (leg, np.nonzero(got != exp)[0][:10])
            _same_tally(oracle, vs, r.signer20, exp, t)
            # once more, with a table for every key the mixed pass learned
            got, t = run(bv, everything)
            assert bv.cache_stats()[0] == int(exp.sum()) and bv.last_dispatch()[1] > 0
            assert (got == exp).all(), (leg, np.nonzero(got != exp)[0][:10])
            _same_tally(oracle, vs, r.signer20, exp, t)
        finally:
            bv.close()
