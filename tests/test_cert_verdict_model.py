"""tests/cert_verdict_model.py against the C++ mirror's OBJECT walks, without a device: over the oracle's tree alone
(oracle.wire_cert.expected_tree: rows, classes, sender and hash bits) the model's verdicts equal what Host.valid_pc,
Host.proposal_matches_certificate and Host.handle_preprepare decide by walking the decoded messages with a verifier that
answers from the same oracle bits — for every case of tests/cert_verdict_cases.py that the rows decide.  The case set yields
each of −1, 0, 1, 2 for pc and for rcc, and −1 only where a case is named irregular."""
import pytest

import go_ibft_amd.hostlib as H
from oracle import binding as B
from oracle import wire_cert as WC

import cert_verdict_cases as K
import cert_verdict_model as M


def round_robin(addrs):
    return lambda who, h, r: who == addrs[(h + r) % len(addrs)]


def mirror(addrs, powers, tree):
    """a stock mirror (no batch backend) whose Verifier answers from the oracle's bits of `tree`"""
    valid = {tree.wire[nd["off"]:nd["off"] + nd["len"]] for k, nd in enumerate(tree.nodes) if tree.sender_ok[k]}
    h = H.Host()
    assert h.vm_init({a: int(p) for a, p in zip(addrs, powers)})
    h.set_verifier(is_valid_validator=lambda w: w in valid,
                   is_valid_proposal_hash=lambda prop, hsh: prop is not None and hsh == B.proposal_hash(prop[0], prop[1]),
                   is_proposer=round_robin(addrs), is_valid_proposal=lambda raw: True)
    h.set_id(b"someone else")
    return h


def pc_up_to_the_proposer(cv, row):
    """what a record's pc holds: the host function under an IsProposer that accepts exactly the certificate's proposal sender"""
    first = M.from_of(cv.rows[int(cv.nodes[row]["first_child"])]) if cv.nodes[row]["n_children"] else None
    return M.pc_verdict_from_rows(cv, row, int(cv.rows[row]["round"]), int(cv.rows[row]["height"]), True, lambda who, h, r: who == first)


def round_change_parts(msg: bytes):
    """(lastPreparedProposal bytes or None, PreparedCertificate bytes or None) of a canonical ROUND_CHANGE message"""
    body = next(v for f, wt, v, _ in WC.fields_pos(msg) if f == 8 and wt == 2)
    parts = {f: v for f, wt, v, _ in WC.fields_pos(body) if wt == 2}
    return parts.get(1), parts.get(2)


@pytest.mark.parametrize("powers", [K.POWERS, K.POWERS_U256], ids=["u64", "u256"])
def test_model_equals_the_mirrors_object_walks(powers):
    if powers is K.POWERS_U256:
        powers = [p >> 196 for p in K.POWERS_U256]        # (the mirror's voting powers are 64-bit: the same proportions)
    r, cases = K.all_cases()
    addrs = [a.tobytes() for a in r.addrs]
    is_proposer = round_robin(addrs)
    seen = {"pc": set(), "rcc": set()}
    compared = 0
    for c in cases:
        tree = WC.expected_tree(c.msgs, r.addrs)
        cv = M.rows_from_tree(tree, addrs, powers)
        host = mirror(addrs, powers, tree)
        try:
            for i, msg in enumerate(c.msgs):
                w = cv.rows[i]
                if cv.cls[i] != 0 or w["status"] != 0:
                    continue
                height, rnd = int(w["height"]), int(w["round"])
                if w["type"] == M.ROUND_CHANGE and w["payload_kind"] == 8:
                    pc = pc_up_to_the_proposer(cv, i)
                    seen["pc"].add(pc)
                    assert c.irregular or pc != -1, (c.label, i)
                    assert c.expect.get(i, pc) == pc, (c.label, i, pc)
                    v = M.round_change_verdict_from_rows(cv, i, is_proposer)
                    if v < 0:
                        continue
                    proposal, cert = round_change_parts(msg)
                    walk = host.valid_pc(cert, rnd, height) and host.proposal_matches_certificate(proposal, cert)
                    assert bool(v) == bool(walk), (c.label, i, v, walk)
                    compared += 1
                elif w["type"] == M.PREPREPARE and w["payload_kind"] == 5 and w["has_view"]:
                    decided, ok, rows, has_prepared, max_round, hsh = M.proposal_verdict_from_rows(cv, i, is_proposer)
                    rcc = -1 if not decided else (1 if ok else (0 if cv.nodes[i]["flags"] & M.HAS_CERTIFICATE else 2))
                    seen["rcc"].add(rcc)
                    assert c.irregular or rcc != -1, (c.label, i)
                    assert c.expect.get(i, rcc) == rcc, (c.label, i, rcc)
                    if not decided or not c.label.startswith("pp:"):
                        continue                           # (handlePrePrepare also asks what is not the certificate's: only the built shapes)
                    want = ok and (not has_prepared or hsh == B.proposal_hash(r.raw, max_round))
                    host.set_state(height, rnd, None)
                    assert host.ingest_wire([msg])[0] == [2], c.label
                    got = host.handle_preprepare(height, rnd)
                    assert (got is not None) == bool(want), (c.label, got is not None, want)
                    assert got in (None, msg)
                    compared += 1
        finally:
            host.close()
    assert seen["pc"] == {-1, 0, 1, 2} and seen["rcc"] == {-1, 0, 1, 2}
    assert compared >= len(K.RC_KINDS) + len(K.PP_SHAPES) - 4


def test_the_single_proposer_contract_is_what_makes_one_question_enough():
    """pc == 1 and an IsProposer that accepts exactly the certificate's proposal sender: valid; one that also accepts a PREPARE's
    sender — two addresses for one view — makes the host function answer 0 where the record's finish would say 1: such a Backend
    keeps the per-row route (include/ibftgpu.h)"""
    r, cases = K.all_cases()
    addrs = [a.tobytes() for a in r.addrs]
    c = next(c for c in cases if c.label == "rc:honest")
    cv = M.rows_from_tree(WC.expected_tree(c.msgs, r.addrs), addrs, K.POWERS)
    lo = int(cv.nodes[0]["first_child"])
    first, second = M.from_of(cv.rows[lo]), M.from_of(cv.rows[lo + 1])
    assert M.pc_verdict_from_rows(cv, 0, K.RND, K.H, True, lambda who, h, rr: who == first) == 1
    assert M.pc_verdict_from_rows(cv, 0, K.RND, K.H, True, lambda who, h, rr: who in (first, second)) == 0
    assert M.pc_verdict_from_rows(cv, 0, K.RND, K.H, True, lambda who, h, rr: who == second) == 0
