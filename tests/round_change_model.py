"""What ibft_decide_round_changes_wire must answer on top of the decide call, restated in plain Python (TEST INFRASTRUCTURE
ONLY): the store's replace rule (messages/messages.go:64-82: one message per sender and view, a later one replaces an earlier
one), GetExtendedRCC (:202-245, the accumulator highestRound starts at 0), GetMostRoundChangeMessages (:248-286) and HasQuorum
(core/validator_manager.go:77-96), over the rows and masks of tests/cert_verdict_model.py and the decisions of
tests/cert_decision_model.py — with the three-valued extension of include/ibftgpu.h: a stored message whose closure is
undecided (−1) leaves a round's quorum undecided exactly where its power could still change the answer."""
from dataclasses import dataclass, field

import numpy as np

import go_ibft_amd.verifier as V

ROUND_CHANGE, KIND_ROUND_CHANGE = 3, 8
UNDECIDED, NO, YES = -1, 0, 1


def takes_part(cv, i: int) -> bool:
    """the message IBFT.AddMessage would have stored"""
    w = cv.rows[i]
    return bool(cv.cls[i] == 0 and w["status"] == 0 and w["has_view"] and w["type"] == ROUND_CHANGE and w["payload_kind"] == KIND_ROUND_CHANGE
                and w["from_len"] == 20 and cv.sender[i])


@dataclass
class Key:
    height: int
    round: int
    first_row: int
    rows: list = field(default_factory=list)        # the rows that take part, ascending
    stored: dict = field(default_factory=dict)      # From → the row the store still holds


@dataclass
class Expected:
    view: np.ndarray            # int32[n]
    stored: np.ndarray          # bool[n]
    records: np.ndarray         # V.RC_RECORD[min(n_keys, cap)]
    n_keys: int
    keys: list                  # Key per record that fits
    answer: np.ndarray | None   # V.RC_ANSWER scalar


def has_quorum(powers: dict, quorum: int, senders) -> bool:
    """HasQuorum: the summed power of the DISTINCT member senders reaches the quorum"""
    return sum(powers[a] for a in set(senders) if a in powers) >= quorum


def quorum3(powers: dict, quorum: int, yes_senders, open_senders) -> int:
    if has_quorum(powers, quorum, yes_senders):
        return YES
    return UNDECIDED if has_quorum(powers, quorum, list(yes_senders) + list(open_senders)) else NO


def tally_of(powers: dict, quorum: int, senders):
    """ibft_tally(senders, all-ones) as a dict of the Tally's fields (the senders are distinct members here)"""
    mask = (1 << 128) - 1
    p = sum(powers[a] for a in set(senders))
    return {"quorum_lo": quorum & (2**64 - 1), "quorum_hi": (quorum >> 64) & (2**64 - 1), "power_lo": p & (2**64 - 1),
            "power_hi": ((p & mask) >> 64), "valid_rows": len(senders), "distinct_senders": len(set(senders)), "has_quorum": int(p >= quorum),
            "shard_overlap": 0, "proposer_rows": 0, "reserved": 0}


def group(cv, n: int):
    """the keys in the order of their lowest row, and each participating row's key"""
    keys, of_row = {}, {}
    for i in range(n):
        if not takes_part(cv, i):
            continue
        w = cv.rows[i]
        k = (int(w["height"]), int(w["round"]))
        if k not in keys:
            keys[k] = Key(k[0], k[1], i)
        keys[k].rows.append(i)
        keys[k].stored[w["from"].tobytes()] = i          # a later message of the sender replaces the earlier one
        of_row[i] = k
    return list(keys.values()), of_row


def expected(cv, n: int, round_change, query=None, rc_cap: int | None = None) -> Expected:
    """cv: cert_verdict_model.Rows; round_change[i]: the decision's round_change of level-0 row i; query: a V.RC_QUERY scalar"""
    cap = n if rc_cap is None else min(rc_cap, n)
    keys, of_row = group(cv, n)
    index = {(k.height, k.round): v for v, k in enumerate(keys)}
    view = np.full(n, V.RC_VIEW_NONE, dtype=np.int32)
    stored = np.zeros(n, dtype=bool)
    for i, k in of_row.items():
        view[i] = index[k] if index[k] < cap else V.RC_VIEW_OVER
        stored[i] = keys[index[k]].stored[cv.rows[i]["from"].tobytes()] == i
    fit = keys[:cap]
    recs = np.zeros(len(fit), dtype=V.RC_RECORD)
    for v, k in enumerate(fit):
        held = sorted(k.stored.values())
        yes = [cv.rows[i]["from"].tobytes() for i in held if int(round_change[i]) == YES]
        open_ = [cv.rows[i]["from"].tobytes() for i in held if int(round_change[i]) == UNDECIDED]
        r = recs[v]
        r["height"], r["round"], r["first_row"], r["rows"], r["stored_rows"] = k.height, k.round, k.first_row, len(k.rows), len(held)
        r["yes_rows"], r["open_rows"] = len(yes), len(open_)
        for f, x in tally_of(cv.powers, cv.quorum, yes).items():
            r["tally"][f] = x
        op = sum(cv.powers[a] for a in open_)
        r["open_power_lo"], r["open_power_hi"] = op & (2**64 - 1), (op >> 64) & (2**64 - 1)
        r["has_quorum"] = quorum3(cv.powers, cv.quorum, yes, open_)
    ans = None
    if query is not None:
        ans = answer(recs, len(keys), cap, int(sum(1 for i in range(n) if cv.cls[i] != 0)), query)
    return Expected(view, stored, recs, len(keys), fit, ans)


def answer(recs, n_keys: int, cap: int, unjudged: int, query) -> np.ndarray:
    h, rnd, accepted, min_round = (int(query[f]) for f in ("height", "round", "has_accepted_proposal", "min_round"))
    a = np.zeros(1, dtype=V.RC_ANSWER)[0]
    of_height = [(v, r) for v, r in enumerate(recs) if int(r["height"]) == h]
    # GetExtendedRCC: highestRound = 0; a round wins when it is HIGHER and its certificate valid — round 0 never does
    r1 = ru = None
    for v, r in of_height:
        round_ = int(r["round"])
        if round_ < 1 or (accepted and round_ == rnd):
            continue
        if int(r["has_quorum"]) == YES and (r1 is None or round_ > int(recs[r1]["round"])):
            r1 = v
        if int(r["has_quorum"]) == UNDECIDED and (ru is None or round_ > int(recs[ru]["round"])):
            ru = v
    if ru is not None and (r1 is None or int(recs[ru]["round"]) > int(recs[r1]["round"])):
        a["extended"] = UNDECIDED
    else:
        a["extended"] = YES if r1 is not None else NO
    a["record"], a["round"] = (r1, int(recs[r1]["round"])) if r1 is not None else (V.CERT_NO_RECORD, 0)
    # GetMostRoundChangeMessages: the round ≥ max(min_round, 1) with the most stored messages, the lowest round among equals
    most = None
    for v, r in of_height:
        if int(r["round"]) < max(min_round, 1):
            continue
        if most is None or (int(r["stored_rows"]), -int(r["round"])) > (int(recs[most]["stored_rows"]), -int(recs[most]["round"])):
            most = v
    a["most_record"], a["most_round"], a["most_rows"] = (most, int(recs[most]["round"]), int(recs[most]["stored_rows"])) if most is not None \
        else (V.CERT_NO_RECORD, 0, 0)
    a["records_of_height"] = len(of_height)
    a["unjudged_rows"] = unjudged
    a["flags"] = V.RC_OVER if n_keys > cap else 0
    return a


def check(label, want: Expected, rc) -> None:
    """an implementation's (rc_view, rc_stored, records, n_rc, answer) against the model, byte for byte where bytes are defined"""
    view, stored, recs, n_rc, ans = rc
    assert n_rc == want.n_keys, (label, "n_rc", n_rc, want.n_keys)
    assert (np.asarray(view) == want.view).all(), (label, "rc_view", list(view), list(want.view))
    assert (np.asarray(stored) == want.stored).all(), (label, "rc_stored", list(np.flatnonzero(stored)), list(np.flatnonzero(want.stored)))
    assert len(recs) == len(want.records), (label, len(recs), len(want.records))
    for v in range(len(recs)):
        assert recs[v].tobytes() == want.records[v].tobytes(), (label, "record", v, recs[v], want.records[v])
    if want.answer is not None:
        assert ans is not None and ans.tobytes() == want.answer.tobytes(), (label, "answer", ans, want.answer)
