"""Batches for ibft_decide_round_changes_wire (tests/round_change_model.py), with REAL signatures, built with the builders of
tests/cert_cases.py / cert_verdict_cases.py under K.POWERS: ten validators, powers 30 1 2 3 1 2 3 1 2 3, quorum 33 — nothing
holds without validator 0, {0, 1, 2} is exactly the quorum, {0, 1, 4} one power short.  Test infrastructure only.

A message is named by a SPEC (sender, height, round, kind):
  "plain"    a ROUND_CHANGE without proposal and certificate: its closure holds under every proposer table;
  "cert"     one that carries the proposal prepared in round − 1 with an honest certificate: its closure is IsProposer's — true
             under the covering table, −1 without a table or under one that misses the certificate's round;
  "badcert"  the same with one PREPARE signed by somebody else: false under every table;
  "forged"   a plain one signed by somebody else (sender bit 0);  "stranger": a plain one of a non-member, validly signed;
  "preprepare" a round-0 PREPREPARE;  "for_host": a ROUND_CHANGE whose body carries an unknown field (the tree hands it to the host).
Every case records what its construction fixes: per (height, round) the record's has_quorum, and fields of the answer."""
import random
from dataclasses import dataclass, field

from oracle import binding as B
from oracle import wire
from oracle import workload as W

import cert_cases as CC
import cert_verdict_cases as K

H = K.H            # 5: the height of the proposer tables of cert_decision_model.tables_for
TABLES = ("covering", "no table", "misses the certificates' rounds")


@dataclass
class Case:
    label: str
    specs: list                                   # (sender, height, round, kind)
    table: str = "covering"
    query: tuple = (H, 0, False, 0)               # height, round, has_accepted_proposal, min_round
    rc_cap: int | None = None
    powers: str = "u64"                           # "u64": K.POWERS, "u256": K.POWERS_U256
    quorums: dict = field(default_factory=dict)   # {(height, round): has_quorum} fixed by the construction
    answer: dict = field(default_factory=dict)    # {field of the answer: value} fixed by the construction
    msgs: list = field(default_factory=list)      # the call's messages (bytes), filled by build()


_round = {}
_msg = {}


def make_round(powers="u64"):
    """one round per power form: the certificates inside the messages are built up to the quorum BY POWER"""
    if powers not in _round:
        _round[powers] = K.make_round()
    return _round[powers]


def powers_of(tag):
    return K.POWERS if tag == "u64" else K.POWERS_U256


def message(tag, spec) -> bytes:
    """the message of a spec, signed once per process"""
    if (tag, spec) in _msg:
        return _msg[(tag, spec)]
    r, powers = make_round(tag), powers_of(tag)
    i, h, rnd, kind = spec
    if kind == "plain":
        m = CC.round_change(r, i, h, rnd).encode()
    elif kind in ("cert", "badcert"):
        assert rnd >= 1
        m = K.round_change_of_kind(r, powers, i, "honest" if kind == "cert" else "bad_prepare_signature", h, rnd, rnd - 1,
                                   random.Random(1000 + rnd)).encode()
    elif kind == "forged":
        m = CC.round_change(r, i, h, rnd, sk=K.OUTSIDER).encode()
    elif kind == "stranger":
        s = wire.IbftMessage(view=wire.View(h, rnd), sender=B.address(B.pubkey(K.OUTSIDER)), type=wire.ROUND_CHANGE,
                             payload=wire.round_change_body(None, None))
        m = CC.sm(s, K.OUTSIDER).encode()
    elif kind == "preprepare":
        m = CC.preprepare(r, K.proposer(r.n, h, rnd), h, rnd).encode()
    elif kind == "for_host":
        m = CC._raw_msg(wire.View(h, rnd), r.addrs[i].tobytes(), B.sign(r.sks[i], b"\x22" * 32), wire.ROUND_CHANGE, 8, b"\x18\x01")
    else:
        raise AssertionError(kind)
    _msg[(tag, spec)] = m
    return m


def plain(senders, rnd, h=H):
    return [(i, h, rnd, "plain") for i in senders]


def pool_batch(n, seed):
    """n level-0 rows drawn from 10 senders × 12 rounds of plain messages, repeats included (a repeat replaces its original)"""
    rng = random.Random(seed)
    return [(rng.randrange(10), H, 1 + rng.randrange(12), "plain") for _ in range(n)]


def cases():
    Q, SHORT, NO_ZERO = [0, 1, 2], [0, 1, 4], list(range(1, 10))
    out = [
        # ---- around the quorum
        Case("a quorum for round 2 without certificates", plain(Q, 2), quorums={(H, 2): 1}, answer={"extended": 1, "round": 2, "record": 0}),
        Case("one power short of the quorum", plain(SHORT, 2), quorums={(H, 2): 0}, answer={"extended": 0, "round": 0}),
        Case("validator 0 missing", plain(NO_ZERO, 2), quorums={(H, 2): 0}, answer={"extended": 0}),
        # ---- the replace rule
        Case("a sender twice, valid then invalid certificate: the later one decides", [(0, H, 2, "cert")] + plain([1, 2], 2) + [(0, H, 2, "badcert")],
             quorums={(H, 2): 0}, answer={"extended": 0}),
        Case("a sender twice, invalid then valid certificate", [(0, H, 2, "badcert")] + plain([1, 2], 2) + [(0, H, 2, "cert")],
             quorums={(H, 2): 1}, answer={"extended": 1, "round": 2}),
        Case("a later row with a spoiled signature does not replace", [(0, H, 2, "cert")] + plain([1, 2], 2) + [(0, H, 2, "forged")],
             quorums={(H, 2): 1}, answer={"extended": 1}),
        # ---- a non-member takes no part
        Case("a non-member takes no part", plain([0, 1], 2) + [(0, H, 2, "stranger")] + plain([4], 2), quorums={(H, 2): 0},
             answer={"extended": 0, "most_rows": 3}),
        # ---- the selection
        Case("two rounds with a quorum: the higher wins", plain(Q, 2) + plain(Q, 3), quorums={(H, 2): 1, (H, 3): 1},
             answer={"extended": 1, "round": 3, "record": 1}),
        Case("a quorum in round 0 only", plain(Q, 0), quorums={(H, 0): 1}, answer={"extended": 0, "record": 0xFFFFFFFF, "records_of_height": 1,
                                                                                     "most_record": 0xFFFFFFFF}),
        Case("the winning round is the node's, a proposal accepted: the lower round", plain(Q, 2) + plain(Q, 3), query=(H, 3, True, 0),
             answer={"extended": 1, "round": 2, "record": 0}),
        Case("the winning round is the node's, no proposal accepted", plain(Q, 2) + plain(Q, 3), query=(H, 3, False, 0),
             answer={"extended": 1, "round": 3}),
        # ---- three values
        Case("no table: the open rows matter", [(0, H, 2, "cert")] + plain([1, 2], 2), table="no table", quorums={(H, 2): -1},
             answer={"extended": -1, "record": 0xFFFFFFFF}),
        Case("a table that misses the certificates' rounds: the open rows matter", [(0, H, 2, "cert")] + plain([1, 2], 2),
             table="misses the certificates' rounds", quorums={(H, 2): -1}, answer={"extended": -1}),
        Case("no table: the yes rows suffice", plain(Q, 2) + [(3, H, 2, "cert")], table="no table", quorums={(H, 2): 1}, answer={"extended": 1}),
        Case("no table: yes and open together fall short", [(1, H, 2, "cert")] + plain([2], 2), table="no table", quorums={(H, 2): 0},
             answer={"extended": 0}),
        Case("no table: an undecided round above a decided one", plain(Q, 2) + [(0, H, 3, "cert")] + plain([1, 2], 3), table="no table",
             quorums={(H, 2): 1, (H, 3): -1}, answer={"extended": -1, "round": 2, "record": 0}),
        Case("no table: an undecided round below a decided one", [(0, H, 2, "cert")] + plain([1, 2], 2) + plain(Q, 3), table="no table",
             quorums={(H, 2): -1, (H, 3): 1}, answer={"extended": 1, "round": 3}),
        # ---- mixed batches
        Case("two heights interleaved, PREPREPARE roots, a root for the host",
             [(0, H, 2, "plain"), (0, H + 1, 2, "cert"), (0, H, 0, "preprepare"), (1, H, 2, "plain"), (1, H + 1, 2, "plain"), (3, H, 2, "for_host"),
              (2, H + 1, 2, "plain"), (2, H, 2, "plain")],
             quorums={(H, 2): 1, (H + 1, 2): -1}, answer={"extended": 1, "round": 2, "records_of_height": 1, "unjudged_rows": 1}),
        # ---- the record cap
        Case("more keys than rc_cap", plain(Q, 2) + plain(Q, 3) + plain([1, 2], 4) + plain([1], 4) + plain(Q, 5), rc_cap=2,
             quorums={(H, 2): 1, (H, 3): 1}, answer={"extended": 1, "round": 3, "flags": 1}),
        # ---- hostile batches
        Case("70 rounds from one sender beside a quorum", plain(Q, 2) + [(1, H, 10 + k, "plain") for k in range(70)], quorums={(H, 2): 1},
             answer={"extended": 1, "round": 2, "records_of_height": 71}),
        # ---- most_*
        Case("most: a tie resolved to the lowest round", plain(Q, 3) + plain(Q, 2) + plain([1], 4), answer={"most_round": 2, "most_rows": 3, "most_record": 1}),
        Case("most: min_round above every round", plain(Q, 2) + plain(Q, 3), query=(H, 0, False, 9),
             answer={"most_record": 0xFFFFFFFF, "most_rows": 0, "most_round": 0, "extended": 1}),
        # ---- u256 powers
        Case("u256: a quorum without certificates", plain(Q, 2), powers="u256", quorums={(H, 2): 1}, answer={"extended": 1}),
        Case("u256: one power short", plain(SHORT, 2), powers="u256", quorums={(H, 2): 0}, answer={"extended": 0}),
        Case("u256, no table: the open rows matter", [(0, H, 2, "cert")] + plain([1, 2], 2), powers="u256", table="no table", quorums={(H, 2): -1},
             answer={"extended": -1}),
    ]
    # ---- batch edges: ballot-word and workgroup edges
    for n in (64, 65, 256, 257):
        out.append(Case(f"a batch of {n} level-0 rows", pool_batch(n, n)))
    return out


_built = {}


def all_cases():
    """the cases with their messages, built once per process"""
    if "all" not in _built:
        cs = cases()
        for c in cs:
            c.msgs = [message(c.powers, s) for s in c.specs]
        _built["all"] = cs
    return _built["all"]


# ---- 70 senders of one round: a set of its own ------------------------------------------------------------------------------
SEVENTY = 70
SEVENTY_POWERS = [1 + (i % 3) for i in range(SEVENTY)]


def seventy_senders_case():
    """(round, powers, Case): every one of 70 validators sends a plain ROUND_CHANGE of round 2 — one key for more than a wavefront"""
    if "seventy" not in _built:
        r = W.make_round(SEVENTY, 913, height=H, round_=1, raw_len=48)
        c = Case("70 senders of one round", plain(range(SEVENTY), 2), quorums={(H, 2): 1}, answer={"extended": 1, "round": 2, "most_rows": SEVENTY})
        c.msgs = [CC.round_change(r, i, H, 2).encode() for i in range(SEVENTY)]
        _built["seventy"] = (r, SEVENTY_POWERS, c)
    return _built["seventy"]


def check_construction(c: Case, want) -> None:
    """what the case's construction fixes, against an Expected of the model"""
    got = {(int(r["height"]), int(r["round"])): int(r["has_quorum"]) for r in want.records}
    for k, v in c.quorums.items():
        assert got.get(k) == v, (c.label, "has_quorum", k, got.get(k), v)
    for f, v in c.answer.items():
        assert int(want.answer[f]) == v, (c.label, "answer", f, int(want.answer[f]), v)
