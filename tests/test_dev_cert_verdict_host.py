"""cert_verdict_dev.h on the CPU (host_cert_verdict_harness.hip, hipcc's host pass — the exact source cert_judge_kernel runs):
the heads, the per-child steps and the folds of validPC and of the RoundChangeCertificate rules, over the case set of
tests/cert_verdict_cases.py against tests/cert_verdict_model.py, and every precedence pair of the two host functions."""
import ctypes as C

import numpy as np
import pytest

import go_ibft_amd.build as build
import go_ibft_amd.verifier as V
from oracle import wire_cert as WC

import cert_verdict_cases as K
import cert_verdict_model as M

F_UNDECIDED, F_WRONG_TYPE, F_WRONG_KIND, F_MISMATCH, F_BAD_SENDER, F_BAD_HASH = 1, 2, 4, 8, 16, 32
GO = 3


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(build.build_cert_verdict_harness())
    vp = C.c_void_p
    L.cvh_record_size.restype = C.c_uint32
    L.cvh_pc_child.restype = C.c_uint32
    L.cvh_pc_child.argtypes = [vp, vp, C.c_uint8, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_int]
    L.cvh_rcc_child.restype = C.c_uint32
    L.cvh_rcc_child.argtypes = [vp, vp, C.c_uint8, C.c_int, C.c_uint64, C.c_uint64]
    L.cvh_pc_fold.argtypes = [C.c_uint32, C.c_int, C.c_int]
    L.cvh_rcc_fold.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    L.cvh_rcc_with_children.argtypes = [C.c_int, C.c_int]
    L.cvh_pc_head.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_int]
    L.cvh_rcc_head.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32]
    L.cvh_judge.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.c_uint32]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def judge(lib, cv: M.Rows, n_roots, addrs, powers, pw):
    index = {a: i for i, a in enumerate(addrs)}
    vidx = np.array([index.get(M.from_of(w), -1) if w["from_len"] == 20 else -1 for w in cv.rows], dtype=np.int32)
    words = np.zeros((len(addrs), pw), dtype=np.uint64)
    for i, p in enumerate(powers):
        for k in range(pw):
            words[i, k] = (int(p) >> (64 * k)) & (2**64 - 1)
    q = 2 * sum(int(p) for p in powers) // 3 + 1
    quorum = np.array([(q >> (64 * k)) & (2**64 - 1) for k in range(5)], dtype=np.uint64)
    out = np.zeros(cv.n_rows + 1, dtype=V.CERT_VERDICT)
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    snd, hsh, slf, cls = u8(cv.sender), u8(cv.hash), u8(cv.self_), u8(cv.cls)
    k = lib.cvh_judge(_p(cv.nodes), _p(cv.rows), _p(cls), _p(snd), _p(hsh), _p(slf), cv.n_rows, n_roots, _p(vidx), _p(words), pw, _p(quorum),
                      _p(out), len(out))
    assert k >= 0
    return out[:k]


def test_record_size_agrees(lib):
    assert lib.cvh_record_size() == V.CERT_VERDICT.itemsize == 128


@pytest.mark.parametrize("powers,pw", [(K.POWERS, 1), (K.POWERS_U256, 4)], ids=["u64", "u256"])
def test_every_case_against_the_model(lib, powers, pw):
    r, cases = K.all_cases()
    addrs = [a.tobytes() for a in r.addrs]
    proposers = M.proposers_for(addrs)
    for c in cases:
        cv = M.rows_from_tree(WC.expected_tree(c.msgs, r.addrs), addrs, powers)
        certs = judge(lib, cv, len(c.msgs), addrs, powers, pw)
        M.check_records(c.label, cv, len(c.msgs), certs, proposers)
        for i, want in c.expect.items():
            got = int(certs[i]["pc"]) if cv.rows[i]["type"] == M.ROUND_CHANGE else int(certs[i]["rcc"])
            assert got == want, (c.label, i, got, want)


def test_fold_precedence_pairs(lib):
    """the order of the host functions' return statements: −1 (irregular) ≺ 0 (wrong type) ≺ −1 (wrong payload kind) ≺ 0 (the rest)"""
    f = lib.cvh_pc_fold
    assert f(0, 1, 1) == 1
    assert f(F_WRONG_TYPE | F_WRONG_KIND, 1, 1) == 0            # both: the type is asked first
    assert f(F_WRONG_KIND, 1, 1) == -1
    assert f(F_WRONG_KIND | F_MISMATCH | F_BAD_SENDER, 0, 0) == -1
    assert f(F_UNDECIDED | F_WRONG_TYPE, 1, 1) == -1
    for flags in (F_MISMATCH, F_BAD_SENDER, F_BAD_HASH):
        assert f(flags, 1, 1) == 0
    assert f(0, 0, 1) == 0 and f(0, 1, 0) == 0
    g = lib.cvh_rcc_fold
    assert g(0, 4, 1, 1) == 1 and g(0, 0, 1, 1) == 0            # no children: not ok
    assert g(F_UNDECIDED, 0, 1, 1) == -1 and g(F_UNDECIDED | F_MISMATCH, 4, 0, 0) == -1
    assert g(F_MISMATCH, 4, 1, 1) == 0 and g(F_BAD_SENDER, 4, 1, 1) == 0 and g(0, 4, 0, 1) == 0 and g(0, 4, 1, 0) == 0
    w = lib.cvh_rcc_with_children
    assert (w(1, 1), w(1, 0), w(0, 1), w(2, 1), w(-1, 0)) == (-1, 1, 0, 2, -1)


def _child(type_, kind, hash_len=32, role=M.ROLE_PC_PREPARE, from_len=20, has_view=1, status=0, n_children=0, height=5, round_=1, h=b"\x11" * 32):
    w, nd = np.zeros(1, dtype=V.WIRE_ROW), np.zeros(1, dtype=V.CERT_NODE)
    w[0]["type"], w[0]["payload_kind"], w[0]["hash_len"], w[0]["from_len"], w[0]["has_view"], w[0]["status"] = type_, kind, hash_len, from_len, has_view, status
    w[0]["height"], w[0]["round"] = height, round_
    w[0]["proposal_hash"][:] = np.frombuffer(h, dtype=np.uint8)
    nd[0]["role"], nd[0]["n_children"] = role, n_children
    return w, nd


def test_child_steps(lib):
    ref = np.frombuffer(b"\x11" * 32, dtype=np.uint8).copy()

    def pc(w, nd, cls=0, sender=1, hashb=1, first=0, height=5, limit=2, ref_round=1, match=1):
        return lib.cvh_pc_child(_p(w), _p(nd), cls, sender, hashb, first, height, limit, ref_round, _p(ref), match)
    assert pc(*_child(M.PREPARE, 6)) == 0
    assert pc(*_child(M.PREPREPARE, 5, role=M.ROLE_PC_PROPOSAL), first=1) == 0
    # a child that is both of the wrong type and of the wrong payload kind: both flags, the fold answers 0
    both = pc(*_child(M.COMMIT, 7))
    assert both == F_WRONG_TYPE | F_WRONG_KIND and lib.cvh_pc_fold(both, 1, 1) == 0
    assert pc(*_child(M.PREPARE, 7)) == F_WRONG_KIND and pc(*_child(M.PREPARE, 6, hash_len=31)) & F_WRONG_KIND
    assert pc(*_child(M.PREPREPARE, 5)) == F_WRONG_TYPE | F_WRONG_KIND     # a second PREPREPARE among the PREPAREs
    assert pc(*_child(M.PREPREPARE, 6)) == F_WRONG_TYPE
    for odd in (dict(from_len=21), dict(has_view=0), dict(status=1), dict(n_children=1), dict(role=M.ROLE_RCC_MESSAGE)):
        assert pc(*_child(M.PREPARE, 6, **odd)) & F_UNDECIDED, odd
    assert pc(*_child(M.PREPARE, 6), cls=1) & F_UNDECIDED
    assert pc(*_child(M.PREPREPARE, 5, role=M.ROLE_RCC_MESSAGE), first=1) == 0     # the first child's role is the head's business
    assert pc(*_child(M.PREPARE, 6, height=6)) == F_MISMATCH and pc(*_child(M.PREPARE, 6, round_=2), limit=9) == F_MISMATCH
    assert pc(*_child(M.PREPARE, 6), limit=1) == F_MISMATCH                # round 1 is not below the limit 1
    assert pc(*_child(M.PREPARE, 6, h=b"\x11" * 31 + b"\x12")) == F_MISMATCH
    assert pc(*_child(M.PREPARE, 6), sender=0) == F_BAD_SENDER
    assert pc(*_child(M.PREPARE, 6), hashb=0) == F_BAD_HASH and pc(*_child(M.PREPARE, 6), hashb=0, match=0) == 0

    def rcc(w, nd, cls=0, sender=1, height=5, round_=1):
        return lib.cvh_rcc_child(_p(w), _p(nd), cls, sender, height, round_)
    assert rcc(*_child(M.ROUND_CHANGE, 8, role=M.ROLE_RCC_MESSAGE)) == 0
    assert rcc(*_child(M.ROUND_CHANGE, 8, role=M.ROLE_RCC_MESSAGE, n_children=7)) == 0     # its own certificate is its record's business
    assert rcc(*_child(M.ROUND_CHANGE, 5, role=M.ROLE_RCC_MESSAGE)) & F_UNDECIDED
    assert rcc(*_child(M.PREPARE, 6, role=M.ROLE_RCC_MESSAGE)) == F_MISMATCH
    assert rcc(*_child(M.ROUND_CHANGE, 8, role=M.ROLE_PC_PREPARE)) & F_UNDECIDED
    assert rcc(*_child(M.ROUND_CHANGE, 8, role=M.ROLE_RCC_MESSAGE, round_=2)) == F_MISMATCH
    assert rcc(*_child(M.ROUND_CHANGE, 8, role=M.ROLE_RCC_MESSAGE), sender=0) == F_BAD_SENDER


def test_heads(lib):
    """a carrier without children answers 0 before its (meaningless) first_child is looked at; bounds give −1"""
    nodes, rows, cls = np.zeros(3, dtype=V.CERT_NODE), np.zeros(3, dtype=V.WIRE_ROW), np.zeros(3, dtype=np.uint8)
    rows[0]["type"], rows[0]["payload_kind"], rows[0]["has_view"] = M.ROUND_CHANGE, 8, 1
    nodes[0]["flags"] = M.HAS_PROPOSAL | M.HAS_CERTIFICATE
    nodes[0]["first_child"], nodes[0]["n_children"] = 0xFFFFFFF0, 0
    head = lambda match=1: lib.cvh_pc_head(_p(nodes), _p(rows), _p(cls), 3, 0, match)
    assert head() == 0                                          # zero children: 0, whatever first_child says
    nodes[0]["n_children"] = 2
    assert head() == -1                                         # out of bounds
    nodes[0]["first_child"] = 1
    nodes[1]["role"] = M.ROLE_PC_PROPOSAL
    assert head() == GO
    nodes[1]["role"] = M.ROLE_PC_PREPARE
    assert head() == 0                                          # no proposal message
    nodes[1]["role"], nodes[0]["n_children"] = M.ROLE_PC_PROPOSAL, 1
    assert head() == 0                                          # no PREPAREs
    nodes[0]["flags"] = M.HAS_CERTIFICATE
    assert head(1) == -1 and head(0) == 0                       # no proposal to match: undecided — asked before the children
    nodes[0]["flags"] = M.HAS_PROPOSAL
    assert head() == 2
    cls[0] = 1
    assert head() == -1
    cls[0] = 0
    rows[0]["type"], rows[0]["payload_kind"] = M.PREPREPARE, 5
    assert head() == -1
    rhead = lambda: lib.cvh_rcc_head(_p(nodes), _p(rows), _p(cls), 3, 0)
    assert rhead() == 2
    nodes[0]["flags"], nodes[0]["n_children"], nodes[0]["first_child"] = M.HAS_CERTIFICATE, 0, 0xFFFFFFF0
    assert rhead() == GO and lib.cvh_rcc_fold(0, 0, 1, 1) == 0  # an empty certificate: the fold's 0, before any bound
    nodes[0]["n_children"] = 2
    assert rhead() == -1
    nodes[0]["first_child"] = 1
    assert rhead() == GO
    rows[0]["payload_kind"] = 8
    assert rhead() == -1
