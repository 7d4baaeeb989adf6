"""ibft_judge_certificates_wire over batches of 1 030 and 2 049 roots, drawn by a seeded generator from the 35 single-root
messages of cert_verdict_cases.all_cases() (the rc: and pp: cases — encodings repeat, nothing new is signed):
cert_record_scan_kernel sums 2 and 3 roots per thread, the binary search of cert_judge_kernel runs over a thousand and two
thousand entries of rec_base with long stretches of equal ones (roots without certificate children), and every verdict value
occurs.  Forced positions: a PREPREPARE with a RoundChangeCertificate at roots 0, 1 023, 1 024 and the last root (1 023 / 1 024
are adjacent), as the first and as the last root of a thread's share, and a run of roots without level-1 records between two
of them.  The records against cert_verdict_model over the context's own per-row outputs, against each case's construction,
against what the same message gives alone, and against a flag-on context; the smaller batch also against the oracle's tree."""
import numpy as np
import pytest

from oracle import wire_cert as WC

import cert_cases as CC
import cert_verdict_cases as K
import cert_verdict_model as M
import test_gpu_judge_certificates as J

pytestmark = pytest.mark.gpu
CAP = 32768
NO_CHILD_RECORDS = ("pp:no_rcc", "pp:empty_rcc")      # PREPREPAREs whose record has no level-1 records behind it, like every rc: case


def singles():
    r, cases = K.all_cases()
    out = [c for c in cases if c.label.startswith(("rc:", "pp:"))]
    assert len(out) == 35 and all(len(c.msgs) == 1 for c in out)
    return r, out


def draw(n_roots, seed):
    """→ (round, the cases, pick[n_roots]: the case of every root)"""
    r, cases = singles()
    rng = np.random.default_rng(seed)
    carriers = [k for k, c in enumerate(cases) if c.label.startswith("pp:") and c.label not in NO_CHILD_RECORDS]
    plain = [k for k, c in enumerate(cases) if k not in carriers]
    per = (n_roots + 1023) // 1024                     # roots per thread of cert_record_scan_kernel
    pick = rng.integers(0, len(cases), n_roots)
    first_of_share, last_of_share = 30 * per, 40 * per + per - 1
    lo, hi = 50 * per, 50 * per + 9                    # a run of roots without level-1 records between two carriers
    pick[lo + 1:hi] = rng.choice(plain, hi - lo - 1)
    pick[lo + 1], pick[lo + 2], pick[lo + 3] = (next(k for k, c in enumerate(cases) if c.label == lab) for lab in NO_CHILD_RECORDS + ("rc:honest",))
    for at in (0, 1023, 1024, n_roots - 1, first_of_share, last_of_share, lo, hi):
        pick[at] = rng.choice(carriers)
    assert per in (2, 3) and first_of_share % per == 0 and last_of_share % per == per - 1
    return r, cases, pick


@pytest.fixture(scope="module")
def alone():
    """every single case judged alone: label → (records, its per-row outputs as the model reads them)"""
    r, cases = singles()
    addrs = [a.tobytes() for a in r.addrs]
    bv = J.make_bv(K.POWERS, r.addrs)
    try:
        return {c.label: J.judged(bv, c.label, c.msgs, addrs, K.POWERS, True, M.proposers_for(addrs)) for c in cases}
    finally:
        bv.close()


def without_offsets(certs):
    """records with the fields that number rows or records set to zero (cert_verdict_model.check_records holds them to the
    context's own node table)"""
    out = certs.copy()
    for f in ("row", "first_child", "first_child_cert"):
        out[f] = 0
    return out.tobytes()


@pytest.mark.parametrize("n_roots", [1030, 2049])
def test_many_roots(n_roots, alone):
    import go_ibft_amd.verifier as V
    r, cases, pick = draw(n_roots, 600 + n_roots)
    addrs = [a.tobytes() for a in r.addrs]
    msgs = [cases[k].msgs[0] for k in pick]
    bv, on_bv = J.make_bv(K.POWERS, r.addrs, max_rows=CAP), J.make_bv(K.POWERS, r.addrs, flags=V.FLAG_CERT_DEDUP, max_rows=CAP)
    try:
        certs, cv = J.judged(bv, f"{n_roots} roots", msgs, addrs, K.POWERS, True, M.proposers_for(addrs), rows_cap=CAP)
        buf, off = CC.pack(msgs)
        with_dedup, n_rows, _ = on_bv.judge_certificates_wire(buf, off)
        assert n_rows == cv.n_rows and with_dedup.tobytes() == certs.tobytes(), "records with IBFT_FLAG_CERT_DEDUP"
    finally:
        bv.close()
        on_bv.close()
    seen = {"pc": set(), "rcc": set()}
    next_record = n_roots
    repeats = 0
    for i, k in enumerate(pick):
        c = cases[k]
        a_certs, a_cv = alone[c.label]
        where = (n_roots, i, c.label)
        assert J.applicable(cv, certs, i) == c.expect[0] == J.applicable(a_cv, a_certs, 0), where
        below = len(a_certs) - 1                                   # its level-1 records
        assert int(certs[i]["first_child_cert"]) == (next_record if below else V.CERT_NO_RECORD), where
        assert without_offsets(certs[i:i + 1]) == without_offsets(a_certs[:1]), where
        assert without_offsets(certs[next_record:next_record + below]) == without_offsets(a_certs[1:]), where
        if below:
            rows = certs["row"][next_record:next_record + below].astype(np.int64)
            assert (rows == int(cv.nodes[i]["first_child"]) + np.arange(below)).all() and int(cv.nodes[i]["n_children"]) == below, where
        repeats += not below
        next_record += below
    assert next_record == len(certs) and repeats > n_roots // 4
    for i, rec in enumerate(certs):
        w = cv.rows[int(rec["row"])]
        if w["status"] == 0 and w["type"] == M.ROUND_CHANGE:
            seen["pc"].add(int(rec["pc"]))
        if i < n_roots and w["status"] == 0 and w["type"] == M.PREPREPARE:
            seen["rcc"].add(int(rec["rcc"]))
    assert seen["pc"] == {-1, 0, 1, 2} and seen["rcc"] == {-1, 0, 1, 2}
    if n_roots == 1030:
        CC.compare("1030 roots", WC.expected_tree(msgs, r.addrs, rows_cap=CAP), cv.n_rows, cv.nodes, cv.rows, cv.cls, cv.sender, cv.hash, cv.self_)
