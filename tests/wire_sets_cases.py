"""The GPU corpus of the wire route under a family of validator sets (tests/test_gpu_wire_sets.py), built on the CPU with the
oracle's encoder and signer so that tests/test_wire_sets_inputs.py can check without a GPU that it holds every kind of row it
claims.  One key pool, four sets over it (40, 23 and 5 validators that receive rows, one of 7 that receives none), rows of
heights 100 / 101 / 105 interleaved row by row, and sprinkled among them every kind the call's row rule names."""
from dataclasses import dataclass, field

import numpy as np

import wire_recode_model as RM
import wire_sets_model as M
from oracle import binding as B
from oracle import wire
from oracle import wire_parse as WP
from oracle import workload as W

HEIGHTS = (100, 101, 105)                      # the heights of the rows of sets 0, 1, 2
MAP_A = ([100, 101, 102, 110, 111, 229], [0, 1, 2, 3, 1])            # heights below 100 — 0 included — are not mapped
MAP_B = ([0, 100, 101, 102, 110, 111, 229], [2, 0, 1, 2, 3, 1])      # … are judged under set 2
RECODE_HEIGHT = 228                            # low seven bits: 100, the range of set 0; the decoded height: a range of set 1
FUTURE_HEIGHT = 10**12
MEMBERS = (list(range(0, 40)), list(range(30, 7, -1)), list(range(36, 41)), list(range(41, 48)))
NOT_IN_SET = (40, 35, 0)                       # a member of the union that is no member of set 0 / 1 / 2
KINDS = ("good", "sig_flip", "outsider", "not_in_set", "needs_host", "no_view", "empty_view", "future", "max_height", "below",
         "padded_height")


@dataclass
class Corpus:
    msgs: list
    kinds: list
    senders: list                # the pool index of the row's signer (−1: the outsider)
    pool: object
    big: bool
    powers: list = field(default_factory=list)

    def sets(self):
        """[(height, addrs (V, 20), powers)] as BatchVerifier.set_validator_sets takes them"""
        return [(1000 + k, self.pool.addrs[ix].copy(), self.powers[k]) for k, ix in enumerate(MEMBERS)]

    def model_sets(self):
        return [M.Set([(self.pool.addrs[i].tobytes(), p) for i, p in zip(ix, self.powers[k])]) for k, ix in enumerate(MEMBERS)]


def _message(r, i, sk, height, kind, view="canonical"):
    h = r.hash32[i].tobytes()
    v = {"canonical": wire.View(height, 0), "none": None, "empty": wire.View(0, 0)}[view]
    addr = B.address(B.pubkey(sk))
    if kind == "commit":
        m = wire.IbftMessage(view=v, sender=addr, type=wire.COMMIT, payload=wire.commit_body(h, r.seal65[i].tobytes()))
    elif kind == "prepare":
        m = wire.IbftMessage(view=v, sender=addr, type=wire.PREPARE, payload=wire.prepare_body(h))
    else:
        m = wire.IbftMessage(view=v, sender=addr, type=wire.ROUND_CHANGE, payload=wire.round_change_body(None, None))
    m.signature = B.sign(sk, B.keccak256(m.payload_no_sig()))
    return m.encode()


_CACHE = {}


def corpus(n: int = 300, seed: int = 2701, big: bool = False) -> Corpus:
    if (n, seed, big) in _CACHE:
        return _CACHE[(n, seed, big)]
    r = W.make_round(48, seed, height=HEIGHTS[0], round_=0)
    outsider = W.validator_key(seed ^ 0x77, 1 << 41)
    special = {13: "no_view", 16: "empty_view", 19: "future", 22: "max_height", 25: "below", 28: "padded_height", 40: "needs_host"}
    msgs, kinds, senders = [], [], []
    for j in range(n):
        s = j % 3
        mem = MEMBERS[s]
        i = mem[(j // 3) % len(mem)]
        kind = special.get(j) or ("sig_flip" if j % 29 == 4 else "outsider" if j % 31 == 7 else "not_in_set" if j % 37 == 5 else
                                  "needs_host" if j % 41 == 9 else "good")
        body = "commit" if j % 2 == 0 else "prepare"
        sk, height = r.sks[i], HEIGHTS[s]
        if kind == "outsider":
            i, sk = -1, outsider
        elif kind == "not_in_set":
            i = NOT_IN_SET[s]
            sk = r.sks[i]
        elif kind in ("empty_view", "below"):        # members of set 2, so that map B makes them valid rows of set 2
            i = MEMBERS[2][j % 5]
            sk = r.sks[i]
        if kind == "future":
            height = FUTURE_HEIGHT
        elif kind == "max_height":
            height = 2**64 - 1
        elif kind == "below":
            height = 99
        elif kind == "padded_height":
            i = MEMBERS[1][3]
            sk, height = r.sks[i], RECODE_HEIGHT
        ri = max(i, 0)
        if kind == "needs_host":
            m = _message(r, ri, sk, height, "roundchange") if j != 40 else _message(r, ri, sk, height, body) + b"\x48\x01"
        elif kind == "no_view":
            m = _message(r, ri, sk, height, body, view="none")
        elif kind == "empty_view":
            m = _message(r, ri, sk, height, body, view="empty")
        else:
            m = _message(r, ri, sk, height, body)
        if kind == "sig_flip":
            at = m.index(b"\x1a\x41") + 2 + (7 * j) % 64
            m = m[:at] + bytes([m[at] ^ 0xFF]) + m[at + 1:]
        if kind == "padded_height":                  # 228 = e4 01 canonically; e4 81 00 is the same value, padded
            assert m.startswith(b"\x0a\x03\x08\xe4\x01")
            m = b"\x0a\x04\x08\xe4\x81\x00" + m[5:]
        msgs.append(m)
        kinds.append(kind)
        senders.append(i)
    if big:
        powers = [[(1 << 200) + (k << 130) + i for i in ix] for k, ix in enumerate(MEMBERS)]
    else:
        powers = [[(1 << 62) + 1000 * k + i for i in ix] for k, ix in enumerate(MEMBERS)]      # sums carry past 2^64
    c = Corpus(msgs, kinds, senders, r, big, powers)
    _CACHE[(n, seed, big)] = c
    return c


def pack(rows):
    off = np.zeros(len(rows) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in rows])
    return b"".join(rows), off


def parsed(msgs, recode: bool):
    """what the walks make of every message: oracle.wire_parse rows; with the recode flag, of the canonical re-encoding of a
    message the canonical walk refuses and the recode class takes → ([Row], [recoded])"""
    rows, recoded = [], []
    for m in msgs:
        e = WP.expected(m)
        rec = False
        if recode and e.status != WP.OK:
            ok, canon = RM.canonical(m)
            if ok:
                e2 = WP.expected(canon)
                if e2.status == WP.OK:
                    e, rec = e2, True
        rows.append(e)
        recoded.append(rec)
    return rows, recoded


_UNION_OK = {}


def expected(c: Corpus, n: int, height_map, recode: bool, sets=None):
    """the model's answer for the first n rows (under c's own sets, or the [M.Set] given) → (bits, out_set, out_vidx, per-set
    tallies, parsed rows)"""
    first, range_set = height_map
    rows, _ = parsed(c.msgs[:n], recode)
    judged = []
    for j, e in enumerate(rows):
        s = M.row_set(e.status, e.has_view, e.height, first, range_set)
        key = (id(c), j, recode)
        if key not in _UNION_OK:   # the signature check itself, membership aside (set-independent: computed once per row)
            _UNION_OK[key] = (not e.pre_flag) and B.recover_address(e.digest, e.signature) == e.sender
        judged.append((s, e.sender, _UNION_OK[key]))
    bits, vidx, tallies = M.judge(sets if sets is not None else c.model_sets(), judged)
    return bits, [s for s, _, _ in judged], vidx, tallies, rows
