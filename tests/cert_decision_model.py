"""What ibft_decide_certificates_wire must answer, restated in plain Python (TEST INFRASTRUCTURE ONLY): the decision of every
record — valid_pc, round_change, proposal and the prepared proposal — from the outputs of ibft_verify_certificates_wire
(tests/cert_verdict_model.py: pc_verdict_from_rows, proposal_verdict_from_rows, record_params), a proposer TABLE with the
three-valued IsProposer of include/ibftgpu.h, and the oracle's proposal hash for the closing comparison.

The clauses of `proposal` stand here in the order the header gives them, (a) … (i); the first one that is not true decides."""
from dataclasses import dataclass

import numpy as np

import go_ibft_amd.verifier as V
from oracle import binding as B

import cert_verdict_model as M

UNDECIDED, NO, YES = -1, 0, 1


@dataclass
class Table:
    """the proposers of rounds [first_round, first_round + len(addrs)) of one height"""
    height: int
    first_round: int
    addrs: list                     # 20 bytes each

    def lookup(self, h: int, r: int):
        """T(h, r): the entry, or None = UNKNOWN"""
        if h != self.height or not self.first_round <= r < self.first_round + len(self.addrs):
            return None
        return self.addrs[r - self.first_round]


def is_proposer(table, who: bytes, who_len: int, h: int, r: int) -> int:
    entry = table.lookup(h, r) if table is not None and table.addrs else None
    if entry is None:
        return UNDECIDED
    return YES if who_len == 20 and who == entry else NO


def pc_of(cv: M.Rows, row: int) -> int:
    """the record's pc — validPC up to the proposer rule: pc_verdict_from_rows under the IsProposer that accepts exactly the From
    of the certificate's proposal message"""
    limit, height, match = M.record_params(cv, row)
    lo = int(cv.nodes[row]["first_child"])
    return M.pc_verdict_from_rows(cv, row, limit, height, match, lambda who, h, r: who == M.from_of(cv.rows[lo]))


def valid_pc(cv: M.Rows, row: int, table) -> int:
    """validPC whole for the record of `row`: −1 / 0 / 1 / 2"""
    pc = pc_of(cv, row)
    if pc != 1:
        return pc
    first = cv.rows[int(cv.nodes[row]["first_child"])]
    _, height, _ = M.record_params(cv, row)
    return is_proposer(table, first["from"].tobytes(), 20, height, int(first["round"]))


def round_change(cv: M.Rows, row: int, table) -> int:
    """handleRoundChangeMessage's closure for a root record whose row is a judged ROUND_CHANGE; −1 for every other record"""
    w = cv.rows[row]
    if cv.nodes[row]["level"] != 0 or w["status"] != 0 or w["type"] != M.ROUND_CHANGE:
        return UNDECIDED
    v = valid_pc(cv, row, table)
    if v == 2:
        return NO if cv.nodes[row]["flags"] & M.HAS_PROPOSAL else YES
    return v


class Unknown(Exception):
    pass


def two_valued(table):
    """the table as the callback of cert_verdict_model.py; a view the table does not know ends the walk (Unknown)"""
    def ask(who, h, r):
        v = is_proposer(table, who, len(who), h, r)
        if v == UNDECIDED:
            raise Unknown
        return v == YES
    return ask


def rcc_of(cv: M.Rows, row: int) -> int:
    """the record's rcc: the RoundChangeCertificate half of validateProposal without any proposer question"""
    decided, ok, _, _, _, _ = M.proposal_verdict_from_rows(cv, row, lambda who, h, r: False)
    if not decided:
        return UNDECIDED
    if not cv.nodes[row]["flags"] & M.HAS_CERTIFICATE:
        return 2
    return YES if ok else NO


NOTHING = (False, None, 0, bytes(32))   # has_prepared, the winner's row, prepared_round, prepared_hash


def proposal(cv: M.Rows, row: int, table, wire: bytes):
    """→ (proposal, (has_prepared, winner's row, prepared_round, prepared_hash))"""
    w, nd = cv.rows[row], cv.nodes[row]
    regular = cv.cls[row] == 0 and w["status"] == 0 and w["has_view"] and w["type"] == M.PREPREPARE and w["payload_kind"] == 5
    if nd["level"] != 0 or not regular:
        return UNDECIDED, NOTHING
    height, round_ = int(w["height"]), int(w["round"])
    if not nd["flags"] & M.HAS_PROPOSAL:                                              # (a) the message carries a Proposal
        return NO, NOTHING
    if int(nd["proposal_round"]) != round_:                                          # (b) Proposal.round == the record's round
        return NO, NOTHING
    p = is_proposer(table, M.from_of(w) if w["from_len"] <= 20 else b"", int(w["from_len"]), height, round_)   # (c)
    if p != YES:
        return p, NOTHING
    if not cv.self_[row]:                                                            # (d) the self bit
        return NO, NOTHING
    if round_ == 0:                                                                  # (e) validateProposal0
        return YES, NOTHING
    rcc = rcc_of(cv, row)                                                            # (f)
    if rcc in (2, NO):
        return NO, NOTHING
    if rcc == UNDECIDED:
        return UNDECIDED, NOTHING
    lo, n = int(nd["first_child"]), int(nd["n_children"])
    children = [(c, valid_pc(cv, c, table)) for c in range(lo, lo + n)]
    if any(v == UNDECIDED for _, v in children):                                     # (g) every record of the certificate is decided
        return UNDECIDED, NOTHING
    if not any(v == YES for _, v in children):                                       # (h) nobody prepared anything
        return YES, NOTHING
    winner, max_round, hsh = None, 0, bytes(32)                                      # (i) the highest round, the LAST among equals
    for c, v in children:
        if v != YES:
            continue
        first = cv.rows[int(cv.nodes[c]["first_child"])]
        if winner is None or int(first["round"]) >= max_round:
            winner, max_round, hsh = c, int(first["round"]), M.hash_of(first)
    raw = wire[int(nd["raw_off"]):int(nd["raw_off"]) + int(nd["raw_len"])]
    return (YES if B.proposal_hash(raw, max_round) == hsh else NO), (True, winner, max_round, hsh)


def expected_decisions(cv: M.Rows, n_roots: int, table, wire: bytes) -> np.ndarray:
    rec_rows = M.record_rows(cv, n_roots)
    index = {row: i for i, row in enumerate(rec_rows)}
    out = np.zeros(len(rec_rows), dtype=V.CERT_DECISION)
    for i, row in enumerate(rec_rows):
        d = out[i]
        d["valid_pc"], d["round_change"] = valid_pc(cv, row, table), round_change(cv, row, table)
        d["proposal"], (has, winner, prepared_round, hsh) = proposal(cv, row, table, wire) if i < n_roots else (UNDECIDED, NOTHING)
        d["flags"] = V.CERT_DECISION_HAS_PREPARED if has else 0
        d["prepared_record"] = index[winner] if has else V.CERT_NO_RECORD
        d["prepared_round"] = prepared_round
        d["prepared_hash"][:] = np.frombuffer(hsh, dtype=np.uint8)
    return out


FIELDS = ("valid_pc", "round_change", "proposal", "flags", "prepared_record", "prepared_round")


def check_decisions(label, cv: M.Rows, n_roots: int, table, wire: bytes, certs, decisions) -> np.ndarray:
    """every decision against the model under `table`, and against the caller's own finish over the records where that is
    two-valued (a table that answers every question the finish asks)"""
    want = expected_decisions(cv, n_roots, table, wire)
    assert len(decisions) == len(want) == len(certs), (label, len(decisions), len(want), len(certs))
    for i in range(len(want)):
        got_t, want_t = tuple(int(decisions[i][f]) for f in FIELDS), tuple(int(want[i][f]) for f in FIELDS)
        assert got_t == want_t, (label, "record", i, "row", int(certs[i]["row"]), dict(zip(FIELDS, got_t)), dict(zip(FIELDS, want_t)))
        assert decisions[i]["prepared_hash"].tobytes() == want[i]["prepared_hash"].tobytes(), (label, "record", i, "prepared_hash")
        assert not decisions[i]["reserved"].any(), (label, "record", i, "reserved")
    against_the_host_functions(label, cv, n_roots, table, want)
    return want


def against_the_host_functions(label, cv: M.Rows, n_roots: int, table, want) -> None:
    """Where the table knows every view the two host functions of cert_verdict_model.py ask about, the model above is those
    functions: round_change is round_change_verdict_from_rows, and a proposal that reaches its certificate is
    proposal_verdict_from_rows — decided, ok, and the prepared proposal it names."""
    ask = two_valued(table)
    for i in range(n_roots):
        w, d = cv.rows[i], want[i]
        try:
            if w["status"] == 0 and w["type"] == M.ROUND_CHANGE:
                assert M.round_change_verdict_from_rows(cv, i, ask) == int(d["round_change"]), (label, "root", i, "round_change")
            if int(d["proposal"]) != UNDECIDED and rcc_of(cv, i) == YES and int(w["round"]) != 0:
                decided, ok, _, has, max_round, hsh = M.proposal_verdict_from_rows(cv, i, ask)
                reached = bool(int(d["flags"]) & V.CERT_DECISION_HAS_PREPARED)
                assert decided and ok, (label, "root", i)
                assert not reached or (has, max_round, hsh) == (True, int(d["prepared_round"]), d["prepared_hash"].tobytes()), (label, "root", i, "prepared")
                assert reached or not has or int(d["proposal"]) == NO, (label, "root", i)   # a false clause before the certificate
        except Unknown:
            continue


# ---- the tables every case runs under ----------------------------------------------------------------------------------
def tables_for(addrs, height: int, carrier_round: int, rounds: int = 8):
    """(name, Table or None): round robin from height + round — the proposer the case builders use —, the same shifted by one
    (every proposer wrong), a range that ends below the carriers' round (the prepared certificates' rounds are inside), a range
    that begins at it (theirs are outside), another height, an empty table, none"""
    a = [bytes(x) for x in addrs]
    rr = lambda shift, first, count, h=height: Table(h, first, [a[(height + r + shift) % len(a)] for r in range(first, first + count)])
    return [("covering", rr(0, 0, rounds)),
            ("shifted", rr(1, 0, rounds)),
            ("misses the carriers' round", rr(0, 0, carrier_round)),
            ("misses the certificates' rounds", rr(0, carrier_round, rounds - carrier_round)),
            ("another height", rr(0, 0, rounds, height + 1)),
            ("no table", None)]
