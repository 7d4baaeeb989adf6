"""GPU: simulate.make_round_change_round — the ROUND_CHANGE messages of a round change with their PreparedCertificates and the new
proposer's PREPREPARE with their RoundChangeCertificate, every signature and envelope digest from the device
(ibft_sign_messages_wire, ibft_sign_envelopes_wire) — judged by ibft_verify_certificates_wire and compared with
oracle/wire_cert.py over the same bytes (cert_cases.compare), with the generator's own expected bits, and at n = 7 with the
messages cert_cases builds with the oracle's signer for the same keys."""
import types

import numpy as np
import pytest

import cert_cases as CC
from oracle import wire_cert as WC

pytestmark = pytest.mark.gpu
SEED = 3     # at n = 7 the selection stream of make_round spoils nested PREPAREs under this seed (asserted below)


@pytest.fixture(scope="module")
def bv():
    import go_ibft_amd.verifier as V
    b = V.BatchVerifier(max_rows=4096)
    yield b
    b.close()


def _judge(bv, label, msgs, addrs, want_rows, want_sender):
    """the tree of `msgs` from the device, against the oracle's over the same bytes and against the generator's bits"""
    buf, off = CC.pack(msgs)
    exp = WC.expected_tree(msgs, addrs, rows_cap=4096)
    n, nodes, rows, cls, sender, hb, sb = bv.verify_certificates_wire(buf, off, rows_cap=4096)
    CC.compare(label, exp, n, nodes, rows, cls, sender, hb, sb)
    assert n == want_rows, (label, n, want_rows)
    assert (sender[:n] == want_sender).all(), (label, np.flatnonzero(sender[:n] != want_sender))
    assert (cls[:n] == 0).all(), label
    return exp, sender[:n], hb[:n], sb[:n]


@pytest.mark.parametrize("byzantine", [False, True], ids=["honest", "byzantine"])
@pytest.mark.parametrize("nonce", ["keccak", "rfc6979"])
@pytest.mark.parametrize("distinct", [False, True], ids=["shared", "distinct"])
@pytest.mark.parametrize("n", [4, 7])
def test_round_change_round(bv, n, distinct, nonce, byzantine):
    import go_ibft_amd.simulate as S
    r = S.make_round_change_round(bv, n, seed=SEED, distinct=distinct, byzantine=byzantine, nonce=nonce)
    q = (2 * n) // 3 + 1
    assert (r.q, r.rows, r.preprepare_rows) == (q, q * (q + 1), 1 + q + q * q) and len(r.off) == q + 1 and len(r.wire) == int(r.off[q])
    assert len(r.expect) == r.rows and len(r.preprepare_expect) == r.preprepare_rows
    if byzantine and n == 7:
        assert not r.expect.all() and len(r.spoiled) >= 1
    if not byzantine:
        assert r.expect.all() and r.preprepare_expect.all() and len(r.spoiled) == 0
    bv.set_validators(r.height, r.addrs, r.power)
    msgs = [r.wire[int(r.off[i]):int(r.off[i + 1])] for i in range(q)]
    label = f"n={n} distinct={distinct} {nonce} byzantine={byzantine}"
    exp, sender, hb, sb = _judge(bv, label + " round changes", msgs, r.addrs, r.rows, r.expect)
    # every nested message is for the carried proposal; every PREPREPARE hashes its own
    assert hb[q:].all() and all(sb[k] for k in range(r.rows) if exp.rows[k].kind == 5)
    exp, sender, hb, sb = _judge(bv, label + " closing preprepare", [r.preprepare], r.addrs, r.preprepare_rows, r.preprepare_expect)
    assert sb[0] and hb[1 + q:].all()
    if not byzantine:
        assert sender.all()


@pytest.mark.parametrize("nonce", ["keccak", "rfc6979"])
def test_same_bytes_as_the_oracles_round_change_set(bv, nonce):
    """n = 7, one shared certificate: the structure is cert_cases.honest_round_change_set's (proposer prepared_round mod n, the
    first ⌊2n/3⌋ other validators prepare, senders 0 … q − 1), so under the keccak nonce rule — the oracle signer's — the
    messages are byte-identical to what cert_cases builds for the same keys; under RFC 6979 the signatures differ, the oracle
    re-signs the same structure and everything but the signature fields is identical."""
    import go_ibft_amd.simulate as S
    n = 7
    r = S.make_round_change_round(bv, n, seed=SEED, nonce=nonce)
    sk = S.secret_keys(SEED, n)
    rr = types.SimpleNamespace(n=n, raw=r.raw, sks=[sk[i].tobytes() for i in range(n)], addrs=r.addrs, proposal_hash=None)
    want = CC.honest_round_change_set(rr, r.height, r.new_round, r.prepared_round, senders=list(range(r.q)))
    msgs = [r.wire[int(r.off[i]):int(r.off[i + 1])] for i in range(r.q)]
    closing = CC.preprepare_with_rcc(rr, r.height, r.new_round, want).encode()
    if nonce == "keccak":
        assert [m.encode() for m in want] == msgs
        assert closing == r.preprepare
        return
    # the same tree with the signatures blanked on both sides (every signature field of the tree lies at [cut0, cut1) of its row)
    def blank(batch):
        t = WC.expected_tree(batch, r.addrs)
        b = bytearray(t.wire)
        for nd in t.nodes:
            b[nd["off"] + nd["cut0"] + 2:nd["off"] + nd["cut1"]] = bytes(65)
        return bytes(b), t.n_rows
    assert blank(msgs) == blank([m.encode() for m in want])
    assert blank([r.preprepare]) == blank([closing])


def test_a_long_round_cold_and_with_the_key_cache():
    """once at n = 64 (q = 43: 1 892 rows), honest, a certificate of its own per sender: row count and all bits, cold and warm"""
    import go_ibft_amd.simulate as S
    import go_ibft_amd.verifier as V
    n = 64
    for flags in (0, V.FLAG_PUBKEY_CACHE):
        b = V.BatchVerifier(flags=flags, max_rows=4096)
        try:
            r = S.make_round_change_round(b, n, seed=SEED, distinct=True)
            assert (r.q, r.rows) == (43, 1892) and r.expect.all()
            b.set_validators(r.height, r.addrs, r.power)
            for _ in range(2 if flags else 1):      # (the second pass of a caching context verifies against the learnt keys)
                rows_n, nodes, rows, cls, sender, hb, sb = b.verify_certificates_wire(r.wire, r.off, rows_cap=4096)
                assert rows_n == r.rows
                assert sender[:rows_n].all() and (cls[:rows_n] == 0).all() and hb[r.q:rows_n].all()
                assert sb[:rows_n][rows["payload_kind"][:rows_n] == 5].all() and int((rows["payload_kind"][:rows_n] == 5).sum()) == r.q
        finally:
            b.close()
