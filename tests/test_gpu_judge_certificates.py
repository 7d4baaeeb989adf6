"""ibft_judge_certificates_wire on the GPU: one record per carrier — validPC and the RoundChangeCertificate rules decided on the
device (cert_judge_kernel, cert_verdict_dev.h) — against tests/cert_verdict_model.py applied to what
ibft_verify_certificates_wire answers for the same bytes on the same context; every per-row output that is requested equals
that call's, bit for bit."""
import numpy as np
import pytest

from oracle import wire
from oracle import workload as W

import cert_cases as CC
import cert_verdict_cases as K
import cert_verdict_model as M

pytestmark = pytest.mark.gpu
CAP = 4096


def make_bv(powers, addrs, flags=0, max_rows=CAP, u256=False):
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(flags=flags, max_rows=max_rows)
    if u256:
        bv.set_validators_u256(K.H, addrs, powers)
    else:
        bv.set_validators(K.H, addrs, np.asarray(powers, dtype=np.uint64))
    return bv


def rows_of(bv, msgs, addrs, powers, rows_cap=CAP):
    """ibft_verify_certificates_wire's answer as the model reads it"""
    buf, off = CC.pack(msgs)
    n, nodes, rows, cls, sender, hb, sb = bv.verify_certificates_wire(buf, off, rows_cap=rows_cap)
    pw = {bytes(a): int(p) for a, p in zip(addrs, powers)}
    return M.Rows(n, nodes, rows, cls, sender, hb, sb, pw, 2 * sum(pw.values()) // 3 + 1)


def judged(bv, label, msgs, addrs, powers, per_row, proposers, cv=None, rows_cap=CAP):
    """the new call against the model over the old call's outputs (cv: taken from another context) → the records"""
    cv = cv or rows_of(bv, msgs, addrs, powers, rows_cap)
    buf, off = CC.pack(msgs)
    certs, n_rows, out = bv.judge_certificates_wire(buf, off, rows_cap=rows_cap, per_row=per_row)
    assert n_rows == cv.n_rows, (label, n_rows, cv.n_rows)
    M.check_records(label, cv, len(msgs), certs, proposers)
    if per_row:
        nodes, rows, cls, sender, hb, sb = out
        assert nodes.tobytes() == cv.nodes.tobytes() and rows.tobytes() == cv.rows.tobytes() and cls.tobytes() == cv.cls.tobytes(), label
        assert (sender == cv.sender).all() and (hb == cv.hash).all() and (sb == cv.self_).all(), label
    else:
        assert out is None
    return certs, cv


def applicable(cv, certs, i):
    """the verdict the construction speaks about: pc of a ROUND_CHANGE, rcc of a PREPREPARE"""
    return int(certs[i]["pc"]) if cv.rows[i]["type"] == M.ROUND_CHANGE else int(certs[i]["rcc"])


@pytest.mark.parametrize("per_row", [False, True], ids=["records only", "all outputs"])
@pytest.mark.parametrize("overlap", ["0", "1"])
def test_every_case_batch(monkeypatch, overlap, per_row):
    monkeypatch.setenv("IBFT_CERT_OVERLAP", overlap)
    r, cases = K.all_cases()
    addrs = [a.tobytes() for a in r.addrs]
    proposers = M.proposers_for(addrs)
    bv = make_bv(K.POWERS, r.addrs)
    seen = {"pc": set(), "rcc": set()}
    try:
        for c in cases:
            certs, cv = judged(bv, c.label, c.msgs, addrs, K.POWERS, per_row, proposers)
            for i, want in c.expect.items():
                assert applicable(cv, certs, i) == want, (c.label, i, applicable(cv, certs, i), want)
            for i, rec in enumerate(certs):
                w = cv.rows[int(rec["row"])]
                if w["status"] == 0 and w["type"] == M.ROUND_CHANGE:
                    seen["pc"].add(int(rec["pc"]))
                    assert c.irregular or int(rec["pc"]) != -1, (c.label, i)
                if i < len(c.msgs) and w["status"] == 0 and w["type"] == M.PREPREPARE:
                    seen["rcc"].add(int(rec["rcc"]))
                    assert c.irregular or int(rec["rcc"]) != -1, (c.label, i)
    finally:
        bv.close()
    assert seen["pc"] == {-1, 0, 1, 2} and seen["rcc"] == {-1, 0, 1, 2}


def test_u256_set():
    r, cases = K.all_cases()
    addrs = [a.tobytes() for a in r.addrs]
    bv = make_bv(K.POWERS_U256, r.addrs, u256=True)
    try:
        for c in cases:
            if c.label.startswith("handmade"):
                continue
            certs, cv = judged(bv, c.label, c.msgs, addrs, K.POWERS_U256, False, M.proposers_for(addrs, 1))
            for i, want in c.expect.items():
                assert applicable(cv, certs, i) == want, (c.label, i)
    finally:
        bv.close()


def test_key_cache_context_on_its_second_call_against_a_cold_one(monkeypatch):
    """the second call of a caching context: warm kernels and two verdict launches — the deferred rows (the ROUND_CHANGE messages
    inside a RoundChangeCertificate among them) are judged at rows of their own and only their mask bits come home, so the
    records must not lean on the verdict kernels' validator-index column"""
    import go_ibft_amd.verifier as V
    monkeypatch.delenv("IBFT_CERT_OVERLAP", raising=False)
    r, cases = K.all_cases()
    addrs = [a.tobytes() for a in r.addrs]
    proposers = M.proposers_for(addrs)
    mixed = next(c for c in cases if c.label == "mixed roots")
    cold, warm = make_bv(K.POWERS, r.addrs), make_bv(K.POWERS, r.addrs, flags=V.FLAG_PUBKEY_CACHE)
    try:
        cv = rows_of(cold, mixed.msgs, addrs, K.POWERS)
        first, _ = judged(warm, "first call", mixed.msgs, addrs, K.POWERS, True, proposers, cv=cv)
        assert warm.cache_stats()[0] > 0                      # keys were learnt: the next call verifies against their tables
        second, _ = judged(warm, "second call", mixed.msgs, addrs, K.POWERS, True, proposers, cv=cv)
        third, _ = judged(warm, "third call, records only", mixed.msgs, addrs, K.POWERS, False, proposers, cv=cv)
        assert first.tobytes() == second.tobytes() == third.tobytes()
        for i, want in mixed.expect.items():
            assert applicable(cv, second, i) == want, i
    finally:
        cold.close(); warm.close()


@pytest.fixture(scope="module")
def big_round():
    return W.make_round(130, 977, height=K.H, round_=1, raw_len=48)


def test_certificates_of_1_2_63_64_65_129_children(big_round):
    """a lane per child, 64 lanes: one short of a wavefront, exactly one, one more, two and a bit — as root ROUND_CHANGE messages
    and again inside a root PREPREPARE's certificate (level-1 records)"""
    r = big_round
    addrs = [a.tobytes() for a in r.addrs]
    powers = [1 + (i % 3) for i in range(r.n)]
    sizes = [1, 2, 63, 64, 65, 129]
    rcs = [K.sized_certificate(r, K.H, 1, carrier, k) for carrier, k in enumerate(sizes)]
    pp = CC.preprepare(r, K.proposer(r.n, K.H, 2), K.H, 2, rcc=wire.round_change_certificate(rcs))
    msgs = [m.encode() for m in rcs] + [pp.encode()]
    bv = make_bv(powers, r.addrs)
    try:
        certs, cv = judged(bv, "sizes", msgs, addrs, powers, True, M.proposers_for(addrs, 2))
        assert [int(c["n_children"]) for c in certs[:6]] == sizes and [int(c["n_children"]) for c in certs[7:]] == sizes
        q = 2 * sum(powers) // 3 + 1
        for i, k in enumerate(sizes):                         # by construction: distinct validators 0 … (without the proposer), honest
            members = [K.proposer(r.n, K.H, 1)] + [j for j in range(r.n) if j != K.proposer(r.n, K.H, 1)][:k - 1]
            want = 0 if k == 1 or sum(powers[j] for j in members) < q else 1
            assert int(certs[i]["pc"]) == want == int(certs[7 + i]["pc"]), (k, int(certs[i]["pc"]), want)
        assert int(certs[5]["pc"]) == 1 and int(certs[0]["pc"]) == 0
    finally:
        bv.close()


@pytest.mark.parametrize("n", [4, 64, 65, 130])
def test_validator_sets_of_4_64_65_130(n, big_round):
    """the distinct-validator bitmap: one word, two words exactly, two and a bit, five"""
    r = big_round if n == 130 else W.make_round(n, 900 + n, height=K.H, round_=1, raw_len=48)
    addrs = [a.tobytes() for a in r.addrs]
    powers = [1 + ((5 * i) % 4) for i in range(n)]
    rng = __import__("random").Random(n)
    senders = sorted(range(n), key=lambda i: -powers[i])[:max(3, n // 16)]
    rcs = [K.round_change_of_kind(r, powers, s, kind, rng=rng) for s, kind in zip(senders, ["honest", "duplicate_sender", "too_few_prepares", "honest"] * 3)]
    pp = CC.preprepare(r, K.proposer(n, K.H, K.RND), K.H, K.RND, rcc=wire.round_change_certificate(rcs))
    msgs = [m.encode() for m in rcs] + [pp.encode()]
    bv = make_bv(powers, r.addrs)
    try:
        certs, cv = judged(bv, f"n={n}", msgs, addrs, powers, False, M.proposers_for(addrs, 2))
        want = [1, 0, 0, 1] * 3
        assert [int(c["pc"]) for c in certs[:len(rcs)]] == want[:len(rcs)]
    finally:
        bv.close()


def test_levels_below_2_get_no_record():
    """a PreparedCertificate whose proposal message carries a RoundChangeCertificate of its own, alone and inside a root
    PREPREPARE's certificate: rows of level 2 and deeper exist, records only for level 0 and the level-1 RCC rows"""
    r = W.make_round(CC.GOLDEN_VALIDATORS, CC.GOLDEN_ROUND_SEED, height=5, round_=1)
    addrs = [a.tobytes() for a in r.addrs]
    powers = [int(p) for p in r.power]
    hm = dict(CC.handmade(r))
    msgs = hm["four levels"] + hm["five levels"]
    bv = make_bv(powers, r.addrs)
    try:
        certs, cv = judged(bv, "deep", msgs, addrs, powers, True, M.proposers_for(addrs))
        assert int(cv.nodes["level"].max()) >= 4
        assert len(certs) == 2 + int(cv.nodes[1]["n_children"]) and all(int(cv.nodes[int(c["row"])]["level"]) <= 1 for c in certs)
        deep_rc = certs[0]
        assert int(deep_rc["pc"]) == -1                       # its proposal message has nested messages: not decided from rows
        assert int(certs[2]["row"]) == int(cv.nodes[1]["first_child"]) and int(certs[2]["pc"]) == -1   # the same message inside the PREPREPARE's certificate
    finally:
        bv.close()


def test_certs_cap_exact_and_one_short():
    r, cases = K.all_cases()
    mixed = next(c for c in cases if c.label == "mixed roots")
    buf, off = CC.pack(mixed.msgs)
    bv = make_bv(K.POWERS, r.addrs)
    try:
        certs, n_rows, _ = bv.judge_certificates_wire(buf, off, rows_cap=CAP)
        k = len(certs)
        assert k > len(mixed.msgs)
        exact, n2, _ = bv.judge_certificates_wire(buf, off, rows_cap=CAP, certs_cap=k)
        assert exact.tobytes() == certs.tobytes() and n2 == n_rows
        # one short, and fewer records than roots: refused, nothing written
        import ctypes as C
        import go_ibft_amd.verifier as V
        for cap in (k - 1, len(mixed.msgs) - 1):
            out = np.full(k * 128, 0x77, dtype=np.uint8)
            per_row = [np.full(CAP * 56, 0x77, dtype=np.uint8), np.full(CAP * 80, 0x77, dtype=np.uint8), np.full(CAP, 0x77, dtype=np.uint8)] + \
                [np.full(CAP // 64, 0x7777777777777777, dtype=np.uint64) for _ in range(3)]
            a, b = C.c_size_t(0), C.c_size_t(0)
            wb = np.frombuffer(buf, dtype=np.uint8)
            rc = bv._L.ibft_judge_certificates_wire(bv._h, V._p(wb), V._p(off), len(off) - 1, CAP, cap, C.byref(a), C.byref(b), V._p(out),
                                                    *[V._p(x) for x in per_row])
            assert rc == -7 and (a.value, b.value) == (0, 0), (cap, rc)          # IBFT_E_TOOBIG
            assert (out == 0x77).all() and all((x.view(np.uint8) == 0x77).all() for x in per_row), cap
        again, _, _ = bv.judge_certificates_wire(buf, off, rows_cap=CAP)           # the context is as good as before
        assert again.tobytes() == certs.tobytes()
    finally:
        bv.close()


def test_simulated_round_change_round():
    """simulate.make_round_change_round(n = 16, byzantine): the ROUND_CHANGE batch and the closing PREPREPARE"""
    import go_ibft_amd.simulate as S
    import go_ibft_amd.verifier as V
    bv = V.BatchVerifier(max_rows=CAP)
    try:
        r = S.make_round_change_round(bv, 16, seed=3, byzantine=True)
        bv.set_validators(r.height, r.addrs, r.power)
        addrs = [a.tobytes() for a in r.addrs]
        powers = [int(p) for p in r.power]
        proposers = M.proposers_for(addrs) + [("the generator's", lambda who, h, rr: who == addrs[rr % 16])]
        msgs = [r.wire[int(r.off[i]):int(r.off[i + 1])] for i in range(r.q)]
        certs, cv = judged(bv, "round changes", msgs, addrs, powers, False, proposers)
        assert len(certs) == r.q and cv.n_rows == r.rows
        # a certificate holds iff none of its PREPAREs was spoiled (every sender carries the same one here)
        clean = bool(r.expect[r.q:2 * r.q].all())
        assert [int(c["pc"]) for c in certs] == [1 if clean else 0] * r.q
        certs, cv = judged(bv, "closing preprepare", [r.preprepare], addrs, powers, True, proposers)
        assert len(certs) == 1 + r.q and cv.n_rows == r.preprepare_rows
        assert int(certs[0]["rcc"]) == 1 and int(certs[0]["rcc_rows"]) == r.q * (r.q + 1) and int(certs[0]["first_child_cert"]) == 1
        got = M.finish_proposal(certs, 0, proposers[-1][1])
        assert got[:4] == (True, True, r.q * (r.q + 1), clean) and (not clean or (got[4], got[5]) == (r.prepared_round, bv.proposal_hash(r.raw, r.prepared_round)))
    finally:
        bv.close()


def test_a_set_whose_bitmap_does_not_fit_lds():
    """more than 393 216 validators: the distinct-validator bitmap lives in HBM and one workgroup walks every record"""
    r, cases = K.all_cases()
    mixed = next(c for c in cases if c.label == "mixed roots")
    fill = 393_300
    rng = np.random.default_rng(12)
    extra = rng.integers(0, 256, (fill, 20), dtype=np.uint8)
    addrs_all = np.concatenate([extra[:fill // 2], r.addrs, extra[fill // 2:]])       # the ten signers in the middle of the index range
    powers = [1] * (fill // 2) + [p * 1_000_000 for p in K.POWERS] + [1] * (fill - fill // 2)
    addrs = [a.tobytes() for a in addrs_all]
    bv = make_bv(powers, addrs_all)
    try:
        certs, cv = judged(bv, "hbm bitmap", mixed.msgs, addrs, powers, False, M.proposers_for([a.tobytes() for a in r.addrs], 1))
        for i, want in mixed.expect.items():
            assert applicable(cv, certs, i) == want, i
        again, _ = judged(bv, "hbm bitmap, again", mixed.msgs, addrs, powers, False, M.proposers_for([a.tobytes() for a in r.addrs], 1), cv=cv)
        assert again.tobytes() == certs.tobytes()             # the bitmap was left zero
    finally:
        bv.close()
