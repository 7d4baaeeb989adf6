"""Certificates for the per-carrier verdicts (ibft_judge_certificates_wire, tests/cert_verdict_model.py), with REAL signatures
(the builders of tests/cert_cases.py): one ROUND_CHANGE message per kind of test_host_roundchange.KINDS, one PREPREPARE per
shape of test_host_cert_ingest.RCC_SHAPES, under NON-UNIT voting powers — one heavy validator, so that a certificate can reach
the quorum by count and miss it by power, and the other way round — and under a 256-bit set.  Test infrastructure only."""
import random
from dataclasses import dataclass, field

from oracle import binding as B
from oracle import wire
from oracle import workload as W

import cert_cases as CC
from test_host_cert_ingest import RCC_SHAPES
from test_host_roundchange import KINDS

H, RND = 5, 2                      # the view of the carriers
N = 10
POWERS = [30, 1, 2, 3, 1, 2, 3, 1, 2, 3]          # total 48, quorum 33: nothing holds without validator 0
POWERS_U256 = [(p << 200) + i for i, p in enumerate(POWERS)]
OUTSIDER = B.keccak256(b"outsider")              # a key that is no validator's
RC_KINDS = ["honest"] + [k for k in dict.fromkeys(KINDS) if k is not None] + ["count_quorum_power_short", "power_quorum_count_short"]
# kinds / shapes whose verdict the rows do not decide (−1): the walk over the decoded message is the authority there
IRREGULAR_KINDS = {"unknown_field_in_prepare", "short_hash_everywhere"}
PP_SHAPES = list(RCC_SHAPES) + ["rc_with_an_irregular_pc", "empty_rcc"]
IRREGULAR_SHAPES = {"rc_with_an_irregular_pc"}


def quorum(powers):
    return 2 * sum(powers) // 3 + 1


def proposer(n, height, round_):
    return (height + round_) % n


@dataclass
class Case:
    label: str
    msgs: list                      # the call's messages (bytes)
    irregular: bool = False         # −1 may occur among the verdicts that apply
    expect: dict = field(default_factory=dict)   # {root index: verdict} where the construction fixes it (pc of a ROUND_CHANGE, rcc of a PREPREPARE)


def make_round(n=N, seed=911):
    return W.make_round(n, seed, height=H, round_=1, raw_len=48)


def stranger_prepare(height, round_, h):
    m = wire.IbftMessage(view=wire.View(height, round_), sender=B.address(B.pubkey(OUTSIDER)), type=wire.PREPARE, payload=wire.prepare_body(h))
    return CC.sm(m, OUTSIDER)


def certificate(r, powers, height, round_, raw, kind=None, rng=None):
    """(proposal message, PREPAREs): the proposer's PREPREPARE of `round_` and PREPAREs of others up to the quorum BY POWER,
    then the one defect `kind` names (World.certificate of test_host_roundchange.py, signed)"""
    rng = rng or random.Random(7)
    n = r.n
    q = quorum(powers)
    prop = proposer(n, height, round_)
    hsh = B.proposal_hash(raw, round_)
    pp = CC.preprepare(r, prop, height, round_, raw=raw)
    others = [i for i in range(n) if i != prop]
    rng.shuffle(others)
    take, acc = [], powers[prop]
    for i in others:
        if acc >= q and len(take) >= 2:
            break
        take.append(i)
        acc += powers[i]
    prs = [CC.prepare(r, i, height, round_, h=hsh) for i in take]
    k = rng.randrange(len(prs))
    if kind == "bad_prepare_signature":
        prs[k] = CC.prepare(r, take[k], height, round_, h=hsh, sk=OUTSIDER)
    elif kind == "bad_proposal_signature":
        pp = CC.preprepare(r, prop, height, round_, raw=raw, sk=OUTSIDER)
    elif kind == "wrong_hash_in_prepare":
        prs[k] = CC.prepare(r, take[k], height, round_, h=B.keccak256(b"other"))
    elif kind == "too_few_prepares":
        heavy = max(range(len(take)), key=lambda j: powers[take[j]])
        del prs[heavy]                                         # the power falls below the quorum, several PREPAREs stay
    elif kind == "duplicate_sender":
        prs.append(prs[0])
    elif kind == "prepare_from_proposer":
        prs[k] = CC.prepare(r, prop, height, round_, h=hsh)
    elif kind == "proposal_not_from_proposer":
        pp = CC.preprepare(r, take[-1], height, round_, raw=raw)   # the two swap their parts: same senders, same power
        prs[-1] = CC.prepare(r, prop, height, round_, h=hsh)
    elif kind == "one_prepare_of_another_round":
        prs[k] = CC.prepare(r, take[k], height, round_ + 1, h=hsh)
    elif kind == "one_prepare_of_another_height":
        prs[k] = CC.prepare(r, take[k], height + 1, round_, h=hsh)
    elif kind == "commit_among_prepares":
        m = wire.IbftMessage(view=wire.View(height, round_), sender=r.addrs[take[k]].tobytes(), type=wire.COMMIT,
                             payload=wire.commit_body(hsh, r.seal65[take[k]].tobytes()))
        prs[k] = CC.sm(m, r.sks[take[k]])
    elif kind == "unknown_field_in_prepare":
        m = wire.IbftMessage(view=wire.View(height, round_), sender=r.addrs[take[k]].tobytes(), type=wire.PREPARE,
                             payload=wire.commit_body(hsh, b"seal"))
        prs[k] = CC.sm(m, r.sks[take[k]])
    elif kind == "short_hash_everywhere":
        pp = CC.preprepare(r, prop, height, round_, raw=raw, h=hsh[:31])
        prs = [CC.prepare(r, i, height, round_, h=hsh[:31]) for i in take]
    elif kind == "stranger_among_prepares":
        prs[k] = stranger_prepare(height, round_, hsh)
    elif kind == "quorum_minus_one_plus_stranger":
        heavy = max(range(len(take)), key=lambda j: powers[take[j]])
        prs[heavy] = stranger_prepare(height, round_, hsh)
    elif kind == "count_quorum_power_short":                   # everybody but the heavy validator: ⌊2n/3⌋ + 1 by count, not by power
        light = [i for i in range(n) if i != prop and powers[i] != max(powers)]
        assert len(light) + 1 >= 2 * n // 3 + 1 and powers[prop] + sum(powers[i] for i in light) < q
        prs = [CC.prepare(r, i, height, round_, h=hsh) for i in light]
    elif kind == "power_quorum_count_short":                   # the heavy validator and two more: the quorum by power, far from it by count
        heavy = max(range(n), key=lambda j: powers[j])
        few = [heavy] + [i for i in others if i != heavy and powers[i] == 3][:2]
        assert powers[prop] + sum(powers[i] for i in few) >= q and len(few) + 1 < 2 * n // 3 + 1
        prs = [CC.prepare(r, i, height, round_, h=hsh) for i in few]
    else:
        assert kind in (None, "honest"), kind
    return pp, prs


def round_change_of_kind(r, powers, sender, kind, height=H, round_=RND, cert_round=1, rng=None):
    raw = r.raw
    if kind == "no_certificate":
        return CC.round_change(r, sender, height, round_)
    if kind == "proposal_without_certificate":
        return CC.round_change(r, sender, height, round_, wire.Proposal(raw, cert_round), None)
    if kind == "other_proposal":
        pp, prs = certificate(r, powers, height, cert_round, b"another block", None, rng)
        return CC.round_change(r, sender, height, round_, wire.Proposal(raw, cert_round), wire.prepared_certificate(pp, prs))
    pp, prs = certificate(r, powers, height, cert_round, raw, kind, rng)
    return CC.round_change(r, sender, height, round_, wire.Proposal(raw, cert_round), wire.prepared_certificate(pp, prs))


RC_EXPECT = {"honest": 1, "no_certificate": 2, "proposal_without_certificate": 2, "proposal_not_from_proposer": 1, "power_quorum_count_short": 1,
             "unknown_field_in_prepare": -1, "short_hash_everywhere": -1}   # every other kind: 0


def rc_kind_cases(r, powers=POWERS):
    """one root ROUND_CHANGE per kind; its pc is fixed by the construction (RC_EXPECT, else 0)"""
    rng = random.Random(41)
    return [Case("rc:" + kind, [round_change_of_kind(r, powers, 3, kind, rng=rng).encode()], kind in IRREGULAR_KINDS, {0: RC_EXPECT.get(kind, 0)})
            for kind in RC_KINDS]


def rcc_senders(r, powers, height, round_):
    """senders of a RoundChangeCertificate: a quorum by power, the heavy validator in the middle"""
    q = quorum(powers)
    order = sorted(range(r.n), key=lambda i: (powers[i] != 1, i))       # the light ones first
    take, acc = [], 0
    for i in order:
        take.append(i)
        acc += powers[i]
        if acc >= q:
            break
    take.insert(len(take) // 2, take.pop())
    return take


def preprepare_of_shape(r, powers, shape, height=H, round_=RND):
    rng = random.Random(300 + PP_SHAPES.index(shape))
    raw = r.raw
    senders = rcc_senders(r, powers, height, round_)
    rcs = []
    for k, a in enumerate(senders):
        cert_round, craw, kind = 0, raw, None
        if shape == "two_prepared_rounds":
            cert_round = k % 2
        if shape == "highest_round_prepared_another_block" and k == 3:
            cert_round, craw = 1, b"another block"
        if shape == "pc_round_at_the_limit" and k == 3:
            cert_round, craw = round_, b"another block"
        if shape == "nobody_prepared_anything":
            rcs.append(CC.round_change(r, a, height, round_))
            continue
        if shape == "one_invalid_pc_is_ignored" and k == 2:
            kind = "bad_prepare_signature"
        if shape == "rc_with_an_irregular_pc" and k == 2:
            kind = "short_hash_everywhere"
        pp, prs = certificate(r, powers, height, cert_round, craw, kind, rng)
        rcs.append(CC.round_change(r, a, height, round_, wire.Proposal(craw, cert_round), wire.prepared_certificate(pp, prs)))
    if shape == "duplicate_rc_sender":
        rcs.append(rcs[0])
    elif shape == "rc_of_another_round":
        rcs[1] = round_change_of_kind(r, powers, senders[1], "honest", height, round_ + 1, 0, rng)
    elif shape == "rc_of_another_height":
        rcs[1] = round_change_of_kind(r, powers, senders[1], "honest", height + 1, round_, 0, rng)
    elif shape == "rc_forged_envelope":
        pp, prs = certificate(r, powers, height, 0, raw, None, rng)
        rcs[1] = CC.round_change(r, senders[1], height, round_, wire.Proposal(raw, 0), wire.prepared_certificate(pp, prs), sk=OUTSIDER)
    elif shape == "prepare_in_the_rcc":
        rcs[1] = CC.prepare(r, senders[1], height, round_, h=b"h" * 32)
    elif shape == "too_few_rcs":
        heavy = max(range(len(senders)), key=lambda j: powers[senders[j]])
        del rcs[heavy]
    rcc = None if shape == "no_rcc" else (b"" if shape == "empty_rcc" else wire.round_change_certificate(rcs))
    return CC.preprepare(r, proposer(r.n, height, round_), height, round_, raw=raw, rcc=rcc)


PP_EXPECT = {"honest": 1, "no_rcc": 2, "one_invalid_pc_is_ignored": 1, "two_prepared_rounds": 1, "highest_round_prepared_another_block": 1,
             "nobody_prepared_anything": 1, "pc_round_at_the_limit": 1, "rc_with_an_irregular_pc": -1}   # every other shape: 0


def pp_shape_cases(r, powers=POWERS):
    return [Case("pp:" + shape, [preprepare_of_shape(r, powers, shape).encode()], shape in IRREGULAR_SHAPES, {0: PP_EXPECT.get(shape, 0)})
            for shape in PP_SHAPES]


def handmade_cases(r):
    """the handmade batches of tests/cert_cases.py (deep nesting, non-canonical encodings, empty wrappers): shapes of every kind,
    all of them allowed to be undecided"""
    return [Case("handmade:" + label, msgs, True) for label, msgs in CC.handmade(r) if msgs]


def mixed_case(rc_cases, pp_cases):
    """root ROUND_CHANGE and root PREPREPARE messages in turn: level 1 interleaves PC children and RCC children"""
    msgs, expect = [], {}
    for a, b in zip(rc_cases, pp_cases):
        for c in (a, b):
            expect[len(msgs)] = c.expect[0]
            msgs.append(c.msgs[0])
    return Case("mixed roots", msgs, True, expect)


_cache = {}


def all_cases():
    """(round, [Case …]) under POWERS, built once per process"""
    if "all" not in _cache:
        r = make_round()
        rc, pp = rc_kind_cases(r), pp_shape_cases(r)
        _cache["all"] = (r, rc + pp + [mixed_case(rc, pp)] + handmade_cases(r))
    return _cache["all"]


def sized_certificate(r, height, round_, carrier, children):
    """a ROUND_CHANGE whose PreparedCertificate has exactly `children` messages (the proposal message and children − 1 PREPAREs of
    distinct validators)"""
    prop = proposer(r.n, height, round_)
    others = [i for i in range(r.n) if i != prop][:children - 1]
    assert len(others) == children - 1
    hsh = B.proposal_hash(r.raw, round_)
    pp = CC.preprepare(r, prop, height, round_)
    return CC.round_change(r, carrier, height, round_ + 1, wire.Proposal(r.raw, round_),
                           wire.prepared_certificate(pp, [CC.prepare(r, i, height, round_, h=hsh) for i in others]))
