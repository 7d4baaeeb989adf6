"""What ibft_judge_certificates_wire must answer, restated in plain Python (TEST INFRASTRUCTURE ONLY): the two host functions
HotPath::pcVerdictFromRows and HotPath::proposalVerdictFromRows (go-ibft_amd/host/backend.cpp) over the outputs of
ibft_verify_certificates_wire — (nodes, rows, class, sender bits, hash bits) — statement by statement, WITH their IsProposer
callback; which rows get a record; and the caller's finish over the records (include/ibftgpu.h).

The defining property a record is checked against, for any IsProposer that accepts at most one address per view:
    finish_pc(record)       == pc_verdict_from_rows(row, limit, height, match_proposal)   (the parameters: record_params)
    finish_proposal(record) == proposal_verdict_from_rows(row)                              (root records)
"""
from dataclasses import dataclass

import numpy as np

import go_ibft_amd.verifier as V

PREPREPARE, PREPARE, COMMIT, ROUND_CHANGE = 0, 1, 2, 3
ROLE_ROOT, ROLE_PC_PROPOSAL, ROLE_PC_PREPARE, ROLE_RCC_MESSAGE = 0, 1, 2, 3
HAS_PROPOSAL, HAS_CERTIFICATE = 1, 2


@dataclass
class Rows:
    """one call's per-row outputs and the validator set they were judged under"""
    n_rows: int
    nodes: np.ndarray       # V.CERT_NODE
    rows: np.ndarray        # V.WIRE_ROW
    cls: np.ndarray
    sender: np.ndarray      # bool
    hash: np.ndarray        # bool
    self_: np.ndarray       # bool
    powers: dict            # address bytes → voting power
    quorum: int

    def power_of(self, addr: bytes) -> int:
        return self.powers.get(addr, 0)


def from_of(w) -> bytes:
    return w["from"].tobytes()[:min(int(w["from_len"]), 20)]


def hash_of(w) -> bytes:
    return w["proposal_hash"].tobytes()


def pc_verdict_from_rows(cv: Rows, row: int, limit: int, height: int, match_proposal: bool, is_proposer) -> int:
    if row >= cv.n_rows or cv.cls[row] != 0:
        return -1
    rc, nd = cv.rows[row], cv.nodes[row]
    if rc["status"] != 0 or not rc["has_view"] or rc["type"] != ROUND_CHANGE or rc["payload_kind"] != 8:
        return -1
    has_proposal, has_cert = bool(nd["flags"] & HAS_PROPOSAL), bool(nd["flags"] & HAS_CERTIFICATE)
    if not has_cert:
        return 2
    if match_proposal and not has_proposal:
        return -1
    lo, n = int(nd["first_child"]), int(nd["n_children"])
    if n == 0:
        return 0
    if lo + n > cv.n_rows:
        return -1
    if cv.nodes[lo]["role"] != ROLE_PC_PROPOSAL:
        return 0
    if n == 1:
        return 0
    for c in range(lo, lo + n):
        w = cv.rows[c]
        if cv.cls[c] != 0 or w["status"] != 0 or not w["has_view"] or w["from_len"] > 20 or cv.nodes[c]["n_children"] != 0:
            return -1
        if c > lo and cv.nodes[c]["role"] != ROLE_PC_PREPARE:
            return -1
    if cv.rows[lo]["type"] != PREPREPARE:
        return 0
    for c in range(lo + 1, lo + n):
        if cv.rows[c]["type"] != PREPARE:
            return 0
    if cv.rows[lo]["payload_kind"] != 5 or cv.rows[lo]["hash_len"] != 32:
        return -1
    for c in range(lo + 1, lo + n):
        if cv.rows[c]["payload_kind"] != 6 or cv.rows[c]["hash_len"] != 32:
            return -1
    round_ = int(cv.rows[lo]["round"])
    seen, power = set(), 0
    for c in range(lo, lo + n):
        w = cv.rows[c]
        if not (int(w["height"]) == height and int(w["round"]) == round_ and int(w["round"]) < limit and hash_of(w) == hash_of(cv.rows[lo])):
            return 0
        if from_of(w) in seen:
            return 0
        seen.add(from_of(w))
        power += cv.power_of(from_of(w))
    if power < cv.quorum:
        return 0
    for c in range(lo, lo + n):
        w = cv.rows[c]
        if not cv.sender[c] or (match_proposal and not cv.hash[c]):
            return 0
        if bool(is_proposer(from_of(w), int(w["height"]), int(w["round"]))) != (c == lo):
            return 0
    return 1


def round_change_verdict_from_rows(cv: Rows, row: int, is_proposer) -> int:
    """handleRoundChangeMessage's closure: −1 undecided, 0 / 1"""
    v = pc_verdict_from_rows(cv, row, int(cv.rows[row]["round"]), int(cv.rows[row]["height"]), True, is_proposer)
    if v != 2:
        return v
    return 0 if cv.nodes[row]["flags"] & HAS_PROPOSAL else 1


def proposal_verdict_from_rows(cv: Rows, row: int, is_proposer):
    """→ (decided, ok, rows, has_prepared, max_round, hash); everything after `decided` means nothing when it is False"""
    undecided = (False, False, 0, False, 0, bytes(32))
    if row >= cv.n_rows or cv.cls[row] != 0:
        return undecided
    pp, nd = cv.rows[row], cv.nodes[row]
    if pp["status"] != 0 or not pp["has_view"] or pp["type"] != PREPREPARE or pp["payload_kind"] != 5:
        return undecided
    if not nd["flags"] & HAS_CERTIFICATE:
        return (True, False, 0, False, 0, bytes(32))
    lo, n = int(nd["first_child"]), int(nd["n_children"])
    if n and lo + n > cv.n_rows:
        return undecided
    below = 0
    for c in range(lo, lo + n):
        w = cv.rows[c]
        if cv.cls[c] != 0 or w["status"] != 0 or not w["has_view"] or w["from_len"] > 20 or cv.nodes[c]["role"] != ROLE_RCC_MESSAGE:
            return undecided
        if w["type"] == ROUND_CHANGE and w["payload_kind"] != 8:
            return undecided
        below += 1 + int(cv.nodes[c]["n_children"])
    not_ok = (True, False, below, False, 0, bytes(32))
    if n == 0:
        return not_ok
    seen, power = set(), 0
    for c in range(lo, lo + n):
        f = from_of(cv.rows[c])
        if f in seen:
            return not_ok
        seen.add(f)
        power += cv.power_of(f)
    if power < cv.quorum:
        return not_ok
    for c in range(lo, lo + n):
        w = cv.rows[c]
        if w["type"] != ROUND_CHANGE or w["height"] != pp["height"] or w["round"] != pp["round"] or not cv.sender[c]:
            return not_ok
    has_prepared, max_round, hsh = False, 0, bytes(32)
    for c in range(lo, lo + n):
        v = pc_verdict_from_rows(cv, c, int(pp["round"]), int(pp["height"]), False, is_proposer)
        if v < 0:
            return undecided
        if v != 1:
            continue
        first = cv.rows[int(cv.nodes[c]["first_child"])]
        if not has_prepared or int(first["round"]) >= max_round:
            max_round, hsh = int(first["round"]), hash_of(first)
        has_prepared = True
    return (True, True, below, has_prepared, max_round, hsh)


# ---- which rows get a record, and with which parameters -----------------------------------------------------------------
def record_rows(cv: Rows, n_roots: int) -> list:
    """every level-0 row, every level-1 row of role ROLE_RCC_MESSAGE, ascending"""
    return list(range(n_roots)) + [k for k in range(n_roots, cv.n_rows) if cv.nodes[k]["level"] == 1 and cv.nodes[k]["role"] == ROLE_RCC_MESSAGE]


def record_params(cv: Rows, row: int):
    """(limit, height, match_proposal) of the record's pc: a root is judged against its own view, a ROUND_CHANGE inside a root
    PREPREPARE's certificate against the PREPREPARE's"""
    nd = cv.nodes[row]
    if nd["level"] == 0:
        return int(cv.rows[row]["round"]), int(cv.rows[row]["height"]), True
    p = cv.rows[int(nd["parent"])]
    return int(p["round"]), int(p["height"]), False


# ---- the caller's finish over the records -------------------------------------------------------------------------------
def finish_pc(rec, height: int, is_proposer) -> int:
    """validPC up to "undecided": pc == 1 still needs the proposer rule — under the single-proposer contract ONE question"""
    if int(rec["pc"]) != 1:
        return int(rec["pc"])
    return 1 if is_proposer(rec["pc_from"].tobytes(), height, int(rec["pc_round"])) else 0


def finish_round_change(rec, is_proposer) -> int:
    v = finish_pc(rec, int(rec["height"]), is_proposer)
    if v != 2:
        return v
    return 0 if int(rec["bits"]) & V.CERT_BIT_HAS_PROPOSAL else 1


def finish_proposal(certs, i: int, is_proposer):
    """a root PREPREPARE's record → what proposal_verdict_from_rows returns: O(Q) over its certificate's records"""
    rec = certs[i]
    rcc = int(rec["rcc"])
    if rcc < 0:
        return (False, False, 0, False, 0, bytes(32))
    if rcc != 1:
        return (True, False, int(rec["rcc_rows"]), False, 0, bytes(32))
    has_prepared, max_round, hsh = False, 0, bytes(32)
    first = int(rec["first_child_cert"])
    for k in range(first, first + int(rec["n_children"])):
        c = certs[k]
        if finish_pc(c, int(rec["height"]), is_proposer) != 1:
            continue
        if not has_prepared or int(c["pc_round"]) >= max_round:
            max_round, hsh = int(c["pc_round"]), c["pc_hash"].tobytes()
        has_prepared = True
    return (True, True, int(rec["rcc_rows"]), has_prepared, max_round, hsh)


# ---- records against the model ------------------------------------------------------------------------------------------
def check_records(label, cv: Rows, n_roots: int, certs, proposers) -> None:
    """every record of `certs` against the two host functions, under each IsProposer of `proposers`; the record's own fields
    against the row it stands for"""
    want_rows = record_rows(cv, n_roots)
    assert [int(c["row"]) for c in certs] == want_rows, (label, "records", [int(c["row"]) for c in certs], want_rows)
    first_cert = {}
    for i, row in enumerate(want_rows):
        if i >= n_roots:
            first_cert.setdefault(int(cv.nodes[row]["parent"]), i)
    for i, row in enumerate(want_rows):
        rec, nd, w = certs[i], cv.nodes[row], cv.rows[row]
        where = (label, "record", i, "row", row)
        assert (int(rec["n_children"]), int(rec["cls"]), int(rec["type"]), int(rec["role"]), int(rec["level"]), int(rec["from_len"])) == \
            (int(nd["n_children"]), int(cv.cls[row]), int(w["type"]), int(nd["role"]), int(nd["level"]), int(w["from_len"])), where
        if nd["n_children"]:
            assert int(rec["first_child"]) == int(nd["first_child"]), where
        assert (int(rec["height"]), int(rec["round"]), rec["from"].tobytes()) == (int(w["height"]), int(w["round"]), w["from"].tobytes()), where
        bits = (V.CERT_BIT_SENDER if cv.sender[row] else 0) | (V.CERT_BIT_HASH if cv.hash[row] else 0) | (V.CERT_BIT_SELF if cv.self_[row] else 0) | \
            (V.CERT_BIT_HAS_PROPOSAL if nd["flags"] & HAS_PROPOSAL else 0) | (V.CERT_BIT_HAS_CERTIFICATE if nd["flags"] & HAS_CERTIFICATE else 0)
        assert int(rec["bits"]) == bits, (where, "bits", int(rec["bits"]), bits)
        assert int(rec["first_child_cert"]) == (first_cert.get(row, V.CERT_NO_RECORD) if i < n_roots else V.CERT_NO_RECORD), (where, "first_child_cert")
        assert int(rec["pc"]) in (-1, 0, 1, 2) and int(rec["rcc"]) in (-1, 0, 1, 2), where
        if int(rec["pc"]) == 1:
            first = cv.rows[int(nd["first_child"])]
            assert (int(rec["pc_round"]), rec["pc_from"].tobytes(), rec["pc_hash"].tobytes()) == (int(first["round"]), first["from"].tobytes(), hash_of(first)), where
        else:
            assert int(rec["pc_round"]) == 0 and not rec["pc_from"].any() and not rec["pc_hash"].any(), where
        limit, height, match = record_params(cv, row)
        for name, is_proposer in proposers:
            want = pc_verdict_from_rows(cv, row, limit, height, match, is_proposer)
            assert finish_pc(rec, height, is_proposer) == want, (where, "pc under", name, int(rec["pc"]), want)
            if i < n_roots:
                got, wantp = finish_proposal(certs, i, is_proposer), proposal_verdict_from_rows(cv, row, is_proposer)
                assert got[0] == wantp[0] and (not got[0] or got == wantp), (where, "rcc under", name, int(rec["rcc"]), got, wantp)
                if w["status"] == 0 and w["type"] == ROUND_CHANGE:
                    assert finish_round_change(rec, is_proposer) == round_change_verdict_from_rows(cv, row, is_proposer), (where, name)
            else:
                assert int(rec["rcc"]) == -1 and int(rec["rcc_rows"]) == 0, where


def proposers_for(addrs, n_offsets: int = 3):
    """IsProposer callbacks that accept at most one address per view: round robin from several offsets, and nobody"""
    a = [bytes(x) for x in addrs]
    out = [("nobody", lambda who, h, r: False)]
    for k in range(min(n_offsets, len(a))):
        out.append((f"round robin + {k}", (lambda k: lambda who, h, r: who == a[(h + r + k) % len(a)])(k)))
    return out


# ---- the oracle's tree as a call's outputs ------------------------------------------------------------------------------
def rows_from_tree(tree, addrs, powers) -> Rows:
    """oracle/wire_cert.Tree → the arrays ibft_verify_certificates_wire delivers (rows that are not judged keep zero fields:
    nothing reads them — their class is not 0)"""
    n = tree.n_rows
    nodes, rows = np.zeros(n, dtype=V.CERT_NODE), np.zeros(n, dtype=V.WIRE_ROW)
    for k in range(n):
        e, o = tree.nodes[k], tree.rows[k]
        for f in ("off", "len", "parent", "ordinal", "first_child", "n_children", "raw_off", "raw_len", "proposal_round", "cut0", "cut1",
                  "level", "role", "flags"):
            nodes[k][f] = e[f]
        rows[k]["status"] = 0 if tree.status[k] == 0 else 1
        if tree.status[k] != 0:
            nodes[k]["flags"] = 0
            continue
        rows[k]["height"], rows[k]["round"], rows[k]["type"], rows[k]["payload_kind"], rows[k]["has_view"] = o.height, o.round, o.type, o.kind, o.has_view
        rows[k]["hash_len"], rows[k]["from_len"], rows[k]["sig_len"] = len(o.proposal_hash), min(len(o.sender), 255), min(len(o.signature), 255)
        rows[k]["from"][:min(20, len(o.sender))] = np.frombuffer(o.sender[:20], dtype=np.uint8)
        rows[k]["proposal_hash"][:len(o.proposal_hash)] = np.frombuffer(o.proposal_hash, dtype=np.uint8)
    pw = {bytes(a): int(p) for a, p in zip(addrs, powers)}
    return Rows(n, nodes, rows, np.array(tree.cls, dtype=np.uint8), np.array(tree.sender_ok, dtype=bool), np.array(tree.hash_bit, dtype=bool),
                np.array(tree.self_bit, dtype=bool), pw, 2 * sum(pw.values()) // 3 + 1)
