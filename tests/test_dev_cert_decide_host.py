"""cert_decide_dev.h and the resumed sponge of cert_wave_dev.h on the CPU (host_cert_decide_harness.hip, hipcc's host pass — the
exact source cert_decide_records_kernel / cert_decide_proposals_kernel run): the table lookup and the three-valued IsProposer,
the per-record and the clause code over every case of tests/cert_decision_cases.py under every table against
tests/cert_decision_model.py, the cross-lane selection of the highest prepared round on the wave emulator, and the sponge that
starts from a saved state against the oracle's Keccak."""
import ctypes as C
import random

import numpy as np
import pytest

import go_ibft_amd.build as build
import go_ibft_amd.verifier as V
from oracle import binding as B
from oracle import wire_cert as WC

import cert_cases as CC
import cert_decision_cases as DK
import cert_decision_model as DM
import cert_verdict_cases as K
import cert_verdict_model as M


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(build.build_cert_decide_harness())
    vp = C.c_void_p
    L.cdh_decision_size.restype = C.c_uint32
    L.cdh_is_proposer.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, C.c_uint64, C.c_uint64]
    L.cdh_decide.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp, vp]
    L.cdh_select.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.cdh_resumed_proposal_hash.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp, vp]
    L.cdh_resumed_proposal_hash.restype = None
    L.cdh_proposal_hash.argtypes = [vp, C.c_uint32, C.c_uint64, vp]
    L.cdh_proposal_hash.restype = None
    return L


@pytest.fixture(scope="module")
def judge_lib():
    L = C.CDLL(build.build_cert_verdict_harness())
    vp = C.c_void_p
    L.cvh_judge.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.c_uint32]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def records(judge_lib, cv: M.Rows, n_roots, addrs, powers):
    """the records of cert_verdict_dev.h over the model's rows (tests/test_dev_cert_verdict_host.py checks them)"""
    index = {a: i for i, a in enumerate(addrs)}
    vidx = np.array([index.get(M.from_of(w), -1) if w["from_len"] == 20 else -1 for w in cv.rows], dtype=np.int32)
    words = np.array([[int(p)] for p in powers], dtype=np.uint64)
    q = 2 * sum(int(p) for p in powers) // 3 + 1
    quorum = np.array([q, 0, 0, 0, 0], dtype=np.uint64)
    out = np.zeros(cv.n_rows + 1, dtype=V.CERT_VERDICT)
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    snd, hsh, slf, cls = u8(cv.sender), u8(cv.hash), u8(cv.self_), u8(cv.cls)
    k = judge_lib.cvh_judge(_p(cv.nodes), _p(cv.rows), _p(cls), _p(snd), _p(hsh), _p(slf), cv.n_rows, n_roots, _p(vidx), _p(words), 1, _p(quorum),
                            _p(out), len(out))
    assert k >= 0
    return out[:k]


def table_args(table):
    if table is None or not table.addrs:
        return 0, 0, 0, None, None
    a = np.frombuffer(b"".join(table.addrs), dtype=np.uint8).copy()
    return table.height, table.first_round, len(table.addrs), _p(a), a


def decide(lib, cv: M.Rows, n_roots, certs, table, wire: bytes):
    h, f, n, ap, keep = table_args(table)
    wb = np.frombuffer(wire + bytes(16), dtype=np.uint8).copy()
    out = np.full(len(certs), 0x77, dtype=np.uint8).repeat(64).view(V.CERT_DECISION)
    assert lib.cdh_decide(_p(cv.nodes), _p(cv.rows), _p(certs), n_roots, cv.n_rows, len(certs), h, f, n, ap, _p(wb), _p(out)) == 0
    return out


def check_case(lib, judge_lib, r, powers, c, seen):
    addrs = [a.tobytes() for a in r.addrs]
    wire, _ = CC.pack(c.msgs)
    cv = M.rows_from_tree(WC.expected_tree(c.msgs, r.addrs), addrs, powers)
    certs = records(judge_lib, cv, len(c.msgs), addrs, powers)
    for name, table in DM.tables_for(addrs, DK.H, DK.RND):
        got = decide(lib, cv, len(c.msgs), certs, table, wire)
        want = DM.check_decisions((c.label, name), cv, len(c.msgs), table, wire, certs, got)
        expect = c.expect if name == "covering" else c.expect_under.get(name, {})
        for i, (fld, v) in expect.items():
            assert int(want[i][fld]) == v == int(got[i][fld]), (c.label, name, i, fld, int(want[i][fld]), int(got[i][fld]), v)
        if name == "covering":
            for i, (k, rnd) in c.prepared.items():
                assert int(got[i]["flags"]) == V.CERT_DECISION_HAS_PREPARED, (c.label, i)
                assert (int(got[i]["prepared_record"]), int(got[i]["prepared_round"])) == (int(certs[i]["first_child_cert"]) + k, rnd), (c.label, i)
            for i in range(len(c.msgs)):       # the model alone: a regular case is decided under the covering table
                w = cv.rows[i]
                if w["status"] == 0 and w["type"] == M.ROUND_CHANGE:
                    seen["round_change"].add(int(want[i]["round_change"]))
                    assert c.irregular or int(want[i]["round_change"]) != -1, (c.label, i)
                if w["status"] == 0 and w["type"] == M.PREPREPARE and w["payload_kind"] == 5 and w["has_view"]:
                    seen["proposal"].add(int(want[i]["proposal"]))
                    assert c.irregular or int(want[i]["proposal"]) != -1, (c.label, i)
        if table is None:
            assert (got["valid_pc"] == np.where(certs["pc"] == 1, -1, certs["pc"])).all(), (c.label, "no table: the judge call plus −1s")
            assert not got["flags"].any() and (got["prepared_record"] == V.CERT_NO_RECORD).all()


def test_decision_size_agrees(lib):
    assert lib.cdh_decision_size() == V.CERT_DECISION.itemsize == 64


def test_every_case_under_every_table_against_the_model(lib, judge_lib):
    r, cases = DK.all_cases()
    seen = {"round_change": set(), "proposal": set()}
    for c in cases:
        check_case(lib, judge_lib, r, K.POWERS, c, seen)
    assert seen["round_change"] == {-1, 0, 1} and seen["proposal"] == {-1, 0, 1}


def test_seventy_round_changes(lib, judge_lib):
    r, powers, cases = DK.big_tree_cases()
    seen = {"round_change": set(), "proposal": set()}
    for c in cases:
        check_case(lib, judge_lib, r, powers, c, seen)
    assert seen["proposal"] == {0, 1}


def test_is_proposer_is_three_valued(lib):
    addrs = np.arange(60, dtype=np.uint8).reshape(3, 20).copy()      # rounds 4, 5, 6 of height 9
    who = lambda k: addrs[k].copy()

    def ask(w, who_len, h, r, rounds=3, table=addrs):
        return lib.cdh_is_proposer(9, 4, rounds, _p(table) if table is not None else None, _p(w), who_len, h, r)
    assert [ask(who(k), 20, 9, 4 + k) for k in range(3)] == [1, 1, 1]
    assert ask(who(0), 20, 9, 5) == 0 and ask(who(1), 20, 9, 4) == 0
    assert ask(who(0), 19, 9, 4) == 0 and ask(who(0), 0, 9, 4) == 0 and ask(who(0), 21, 9, 4) == 0      # another length: false where the table knows
    assert ask(who(0), 20, 9, 3) == -1 and ask(who(2), 20, 9, 7) == -1 and ask(who(0), 20, 9, 2**64 - 1) == -1   # outside the range
    assert ask(who(0), 20, 8, 4) == -1 and ask(who(0), 20, 10, 4) == -1                                     # another height
    assert ask(who(0), 19, 8, 4) == -1                                                                      # undecided before the length is asked
    assert ask(who(0), 20, 9, 4, rounds=0) == -1 and ask(who(0), 20, 9, 4, rounds=0, table=None) == -1      # no table
    assert ask(who(1), 20, 9, 5, rounds=1) == -1 and ask(who(0), 20, 9, 4, rounds=1) == 1
    # a range that ends at 2^64 − 1
    top = lambda w, r: lib.cdh_is_proposer(9, 2**64 - 3, 3, _p(addrs), _p(w), 20, 9, r)
    assert top(who(2), 2**64 - 1) == 1 and top(who(0), 2**64 - 3) == 1 and top(who(0), 2**64 - 4) == -1 and top(who(0), 0) == -1


def reference_selection(valid_pc, pc_round):
    """validateProposal's loop: `>=` over the valid certificates in order"""
    if any(v == -1 for v in valid_pc):
        return -1, None
    winner = None
    for k, (v, rnd) in enumerate(zip(valid_pc, pc_round)):
        if v == 1 and (winner is None or rnd >= pc_round[winner]):
            winner = k
    return (1, None) if winner is None else (3, winner)


def select(lib, valid_pc, pc_round):
    v = np.array(valid_pc, dtype=np.int8)
    rnd = np.array(pc_round, dtype=np.uint64)
    has, k, round_ = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    after = lib.cdh_select(_p(v), _p(rnd), len(v), C.byref(has), C.byref(k), C.byref(round_))
    assert after != -2, "the lanes disagree about the winner"
    return after, (int(k.value), int(round_.value)) if has.value else None


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_selection_across_lanes(lib, n):
    rng = random.Random(n)
    big = 2**64 - 1
    patterns = [([1] * n, [7] * n),                                            # one round everywhere: the last child
                ([1] * n, list(range(n))), ([1] * n, list(range(n, 0, -1))),   # ascending, descending
                ([0] * n, [9] * n), ([2] * n, [0] * n),                        # nobody prepared anything
                ([1] + [0] * (n - 1), [0] + [5] * (n - 1)),                    # round 0 is a round; a higher round of an invalid certificate is not
                ([1] * n, [big if k % 7 == 3 else 2**32 + k for k in range(n)])]   # rounds beyond 32 bits: both halves take part
    for k in range(n):                                                          # ties at (k, k + 64) and across lanes
        if k + 64 < n:
            v, rnd = [0] * n, [0] * n
            v[k] = v[k + 64] = 1
            rnd[k] = rnd[k + 64] = 4
            patterns.append((v, rnd))
            v2, rnd2 = list(v), list(rnd)
            other = (k + 17) % n
            v2[other], rnd2[other] = 1, 4
            patterns.append((v2, rnd2))
            v3, rnd3 = list(v2), list(rnd2)
            rnd3[k] = 5                                                         # the earlier child of the lane has the higher round
            patterns.append((v3, rnd3))
    for _ in range(40):
        v = [rng.choice([0, 1, 1, 2]) for _ in range(n)]
        patterns.append((v, [rng.choice([1, 2, 3]) for _ in range(n)]))
    for k in (0, n // 2, n - 1):                                                # one undecided child decides, wherever it is
        v = [1] * n
        v[k] = -1
        patterns.append((v, [3] * n))
    for v, rnd in patterns:
        after, winner = select(lib, v, rnd)
        want_after, want_k = reference_selection(v, rnd)
        assert after == want_after, (n, v, rnd, after, want_after)
        if want_after == 3:
            assert winner == (want_k, rnd[want_k]), (n, v, rnd, winner, want_k)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_resumed_sponge_over_the_length_sweep(lib, shift):
    """the state behind raw's full blocks closes keccak(raw ‖ BE64(r)) for any r; sponge_message itself is what it was"""
    for n in DK.SWEEP_LENGTHS + [271, 407, 408, 2040]:
        raw = DK.sweep_raw(n)
        # the harness reads raw where numpy put it: shift the start inside a larger buffer
        buf = np.frombuffer(bytes(shift) + raw + bytes(16), dtype=np.uint8).copy()
        mid = np.full(25, 0x7777777777777777, dtype=np.uint64)
        whole, resumed, plain = (np.zeros(32, dtype=np.uint8) for _ in range(3))
        start = C.c_void_p(buf.ctypes.data + shift)
        for r0, r1 in ((2, 1), (0, 2**64 - 1), (3, 3)):
            lib.cdh_resumed_proposal_hash(start, n, r0, r1, _p(mid), _p(whole), _p(resumed))
            lib.cdh_proposal_hash(start, n, r0, _p(plain))
            assert whole.tobytes() == plain.tobytes() == B.proposal_hash(raw, r0), (n, shift, r0, "the whole sponge")
            assert resumed.tobytes() == B.proposal_hash(raw, r1), (n, shift, r1, "from the saved state")
        if n < 136:
            assert not mid.any()                       # no full block: the state saved is the empty sponge's
