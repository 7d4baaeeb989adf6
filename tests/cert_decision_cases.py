"""Messages for the decisions of ibft_decide_certificates_wire (tests/cert_decision_model.py), with REAL signatures: every case
of tests/cert_verdict_cases.py, and PREPREPAREs built for the clauses the records alone do not decide — the proposer rule, the
highest prepared round with its LAST-among-equals rule, and the closing hash at the proposal lengths where the remainder, the
eight round bytes and the padding fall on either side of a Keccak block edge.  Test infrastructure only.

Every case records what its construction fixes under the COVERING table (tests/cert_decision_model.tables_for: the round robin
from height + round that the builders use as the proposer): {root index: (field, value)}."""
import random
from dataclasses import dataclass, field

from oracle import binding as B
from oracle import wire
from oracle import workload as W

import cert_cases as CC
import cert_verdict_cases as K

H, RND = K.H, K.RND
RAW_A, RAW_B, RAW_C, RAW_D = (bytes([0x40 + i]) * (40 + i) for i in range(4))
SWEEP_LENGTHS = [0, 1, 119, 120, 127, 128, 129, 135, 136, 137, 263, 264, 272, 1000]


@dataclass
class Case:
    label: str
    msgs: list                                       # the call's messages (bytes)
    irregular: bool = False                          # −1 may occur under the covering table
    expect: dict = field(default_factory=dict)       # {root index: (field, value)} under the covering table
    expect_under: dict = field(default_factory=dict)  # {table name: {root index: (field, value)}}
    prepared: dict = field(default_factory=dict)     # {root index: (child index of the winner, prepared_round)} under the covering table


# a shape of cert_verdict_cases.PP_SHAPES whose certificate holds (rcc == 1) re-proposes r.raw: true where the highest valid
# prepared round prepared r.raw; every shape whose rcc is 0 or 2: false
PP_PROPOSAL = {"honest": 1, "one_invalid_pc_is_ignored": 1, "two_prepared_rounds": 1, "highest_round_prepared_another_block": 0,
               "nobody_prepared_anything": 1, "pc_round_at_the_limit": 1, "rc_with_an_irregular_pc": -1}


def base_cases():
    """tests/cert_verdict_cases.all_cases(): pc of a root ROUND_CHANGE fixes round_change, rcc of a root PREPREPARE — all built
    from the proposer, with a true hash and a matching round — fixes proposal where no certificate below it is valid"""
    r, cases = K.all_cases()
    out = []
    for c in cases:
        expect = {}
        if c.label.startswith("rc:"):
            kind = c.label[3:]
            pc = c.expect[0]
            # the proposer rule is what pc leaves open: only `proposal_not_from_proposer` fails it
            want = {2: 0 if kind == "proposal_without_certificate" else 1, 1: 0 if kind == "proposal_not_from_proposer" else 1}.get(pc, pc)
            expect[0] = ("round_change", want)
        if c.label.startswith("pp:"):
            expect[0] = ("proposal", PP_PROPOSAL.get(c.label[3:], 0))
        out.append(Case(c.label, c.msgs, c.irregular, expect))
    return r, out


def rcc_with(r, powers, height, round_, certs, senders=None):
    """a RoundChangeCertificate of (height, round_) from a quorum of senders; certs: {child index: (cert_round, raw, kind)} — the
    other ROUND_CHANGE messages carry nothing"""
    rng = random.Random(97)
    senders = K.rcc_senders(r, powers, height, round_) if senders is None else senders
    assert all(k < len(senders) for k in certs)
    rcs = []
    for k, a in enumerate(senders):
        if k not in certs:
            rcs.append(CC.round_change(r, a, height, round_))
            continue
        cert_round, raw, kind = certs[k]
        pp, prs = K.certificate(r, powers, height, cert_round, raw, kind, rng)
        rcs.append(CC.round_change(r, a, height, round_, wire.Proposal(raw, cert_round), wire.prepared_certificate(pp, prs)))
    return wire.round_change_certificate(rcs)


def proposed(r, powers, raw, round_, certs, height=H, sender=None, **kw):
    """the proposer's PREPREPARE of (height, round_) for `raw` over rcc_with(certs)"""
    sender = K.proposer(r.n, height, round_) if sender is None else sender
    return CC.preprepare(r, sender, height, round_, raw=raw, rcc=rcc_with(r, powers, height, round_, certs), **kw).encode()


def proposal_cases(r, powers=K.POWERS):
    P = lambda v: {0: ("proposal", v)}
    two_rounds = {1: (0, RAW_A, None), 3: (1, RAW_B, None)}
    out = [
        Case("re-proposal of the highest prepared round", [proposed(r, powers, RAW_B, RND, two_rounds)], expect=P(1), prepared={0: (3, 1)},
             expect_under={"misses the certificates' rounds": P(-1)}),       # a child whose valid_pc is −1 only because the table misses its round
        Case("re-proposal of a lower prepared round", [proposed(r, powers, RAW_A, RND, two_rounds)], expect=P(0), prepared={0: (3, 1)}),
        Case("prepared rounds 1 then 2", [proposed(r, powers, RAW_B, 3, {1: (1, RAW_A, None), 3: (2, RAW_B, None)})], expect=P(1), prepared={0: (3, 2)}),
        Case("prepared rounds 2 then 1", [proposed(r, powers, RAW_B, 3, {1: (2, RAW_B, None), 3: (1, RAW_A, None)})], expect=P(1), prepared={0: (1, 2)}),
        Case("prepared rounds 2 then 1, the lower one proposed", [proposed(r, powers, RAW_A, 3, {1: (2, RAW_B, None), 3: (1, RAW_A, None)})], expect=P(0),
             prepared={0: (1, 2)}),
        # the proposer of round 1 equivocates: two valid certificates of ONE round for two proposals — the last one counts
        Case("one round prepared twice, the last proposed", [proposed(r, powers, RAW_B, RND, {1: (1, RAW_A, None), 3: (1, RAW_B, None)})], expect=P(1),
             prepared={0: (3, 1)}),
        Case("one round prepared twice, the first proposed", [proposed(r, powers, RAW_B, RND, {1: (1, RAW_B, None), 3: (1, RAW_A, None)})], expect=P(0),
             prepared={0: (3, 1)}),
        Case("an invalid certificate of a higher round is ignored",
             [proposed(r, powers, RAW_A, 3, {1: (1, RAW_A, None), 2: (2, RAW_B, "bad_prepare_signature")})], expect=P(1), prepared={0: (1, 1)}),
        Case("a certificate whose proposal is not the proposer's is ignored",
             [proposed(r, powers, RAW_A, 3, {1: (1, RAW_A, None), 2: (2, RAW_B, "proposal_not_from_proposer")})], expect=P(1), prepared={0: (1, 1)}),
        Case("round 0 without a certificate", [CC.preprepare(r, K.proposer(r.n, H, 0), H, 0, raw=RAW_A).encode()], expect=P(1)),
        Case("round 0 with a certificate", [proposed(r, powers, RAW_A, 0, {1: (0, RAW_B, None)})], expect=P(1)),
        Case("round 2 without a certificate", [CC.preprepare(r, K.proposer(r.n, H, RND), H, RND, raw=RAW_A).encode()], expect=P(0)),
        Case("Proposal.round is not the view's round",
             [CC.preprepare(r, K.proposer(r.n, H, RND), H, RND, raw=RAW_A, proposal_round=1, rcc=rcc_with(r, powers, H, RND, {})).encode()], expect=P(0)),
        Case("from is not the proposer", [proposed(r, powers, RAW_A, RND, {}, sender=(K.proposer(r.n, H, RND) + 1) % r.n)], expect=P(0),
             expect_under={"shifted": P(1)}),
        Case("a wrong proposal hash", [proposed(r, powers, RAW_A, RND, {}, h=B.keccak256(b"not this"))], expect=P(0)),
        Case("nobody prepared anything", [proposed(r, powers, RAW_A, RND, {})], expect=P(1)),
    ]
    return out


def sweep_raw(length: int) -> bytes:
    return bytes((37 * length + 11 * i + 5) & 0xFF for i in range(length))


def sweep_cases(r, powers=K.POWERS):
    """one PREPREPARE per length of SWEEP_LENGTHS, each re-proposing what round 1 prepared — clause (i) with a true hash —, as four
    batches behind a first message of 0 … 3 more bytes: every proposal starts at every offset mod 4 of the call's buffer"""
    pps = [proposed(r, powers, sweep_raw(n), RND, {2: (1, sweep_raw(n), None)}) for n in SWEEP_LENGTHS]
    wrong = proposed(r, powers, sweep_raw(136), RND, {2: (1, sweep_raw(136)[:-1] + b"\x00", None)})   # the same length, another last byte: 0
    out = []
    for shift in range(4):
        filler = CC.prepare(r, 1, H, RND, h=b"\x5a" * (32 - shift)).encode()
        expect = {1 + i: ("proposal", 1) for i in range(len(pps))}
        expect[1 + len(pps)] = ("proposal", 0)
        out.append(Case(f"proposal lengths, first message {shift} byte(s) shorter", [filler] + pps + [wrong], expect=expect,
                        prepared={1 + i: (2, 1) for i in range(len(pps) + 1)}))
    return out


_cache = {}


def big_round():
    if "big" not in _cache:
        _cache["big"] = W.make_round(100, 1009, height=H, round_=1, raw_len=48)
    return _cache["big"]


def big_tree_cases():
    """100 unit-power validators, a RoundChangeCertificate of 70 ROUND_CHANGE messages: valid prepared certificates at children k
    and k + 64 (one lane) and at two children of other lanes"""
    r = big_round()
    powers = [1] * r.n
    senders = list(range(70))
    same = {2: (1, RAW_A, None), 10: (1, RAW_B, None), 37: (1, RAW_C, None), 66: (1, RAW_D, None)}
    mixed = {2: (1, RAW_A, None), 10: (2, RAW_B, None), 37: (2, RAW_C, None), 66: (1, RAW_D, None)}

    rcc = {RND: rcc_with(r, powers, H, RND, same, senders), 3: rcc_with(r, powers, H, 3, mixed, senders)}

    def pp(raw, round_):
        return CC.preprepare(r, K.proposer(r.n, H, round_), H, round_, raw=raw, rcc=rcc[round_]).encode()
    return r, powers, [
        Case("70 round changes, one round at children 2, 10, 37, 66", [pp(RAW_D, RND), pp(RAW_A, RND)],
             expect={0: ("proposal", 1), 1: ("proposal", 0)}, prepared={0: (66, 1), 1: (66, 1)}),
        Case("70 round changes, round 2 at children 10, 37 between round 1 at 2, 66", [pp(RAW_C, 3), pp(RAW_D, 3)],
             expect={0: ("proposal", 1), 1: ("proposal", 0)}, prepared={0: (37, 2), 1: (37, 2)}),
    ]


def all_cases():
    """(round, [Case …]) under K.POWERS, built once per process"""
    if "all" not in _cache:
        r, base = base_cases()
        _cache["all"] = (r, base + proposal_cases(r) + sweep_cases(r))
    return _cache["all"]
