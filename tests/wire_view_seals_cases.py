"""The corpora of ibft_verify_messages_wire_views (tests/test_gpu_wire_view_seals.py), built on the CPU with the oracle's encoder
and signer over the key pool, the four sets and the height maps of tests/wire_sets_cases.py, so that
tests/test_wire_view_seals_inputs.py can check without a GPU that each holds every case it claims.  A COMMIT's seal signs the
digest (under the corpus' seal-digest convention) of the hash the message names, unless its kind says otherwise.

  S  about 150 rows, not a multiple of 64: heights 100 / 101 / 105 (sets 0 / 1 / 2), PREPAREs interleaved with COMMITs, every
     kind of SEAL_KINDS, the superseding cases and the two quorum-edge views of height 105 (corpus_s lists them)
  T  65 COMMIT rows, all sealable: its prefixes of 1, 64 and 65 rows are the small sizes (half == n; a seal word and a source
     row straddling 64)
  B  601 rows = two full workgroups of the row kernels and a partial one: one COMMIT view with rows in every workgroup, about
     every fifth seal bad, senders whose superseding rows lie in another workgroup
  C  200 COMMIT rows, each in a round of its own (64 views in every wavefront: the per-lane fallback), every third seal bad;
     C_CAP views fit
"""
import wire_sets_cases as WS
import wire_view_seals_model as SM
import wire_views_cases as VC
from oracle import binding as B
from oracle import wire

PREPARE, COMMIT = SM.PREPARE, SM.COMMIT
HA, HB, H31, H0 = VC.HA, VC.HB, VC.H31, VC.H0
SUFFIX = b"\x02"
# envelope fine, seal as named
SEAL_KINDS = ("good", "seal_flip", "seal_other_hash", "seal_other_member", "seal_outsider", "seal_recid", "seal_64", "hash31", "hash0")
# seal fine, envelope as named
ENVELOPE_KINDS = ("sig_flip", "not_in_set", "outsider", "future", "padded_height")
SUPERSEDING = ("good_then_bad", "bad_then_good", "ha_then_hb")
EDGE_HEIGHT, EDGE_FULL_ROUND, EDGE_SHORT_ROUND = 105, 0, 1       # the two COMMIT views of set 2 (five members, quorum four)
C_ROWS, C_CAP = 200, 150
B_ROWS = 601

_SEALS = {}


def _outsider():
    return WS.W.validator_key(2701 ^ 0x77, 1 << 41)


def seal_of(sk: bytes, h: bytes, suffix) -> bytes:
    """the committed seal of the key over the digest of hash h (a hash that is not 32 bytes: over its zero-padded form — such
    a seal is never looked at)"""
    key = (sk, h, suffix)
    if key not in _SEALS:
        _SEALS[key] = B.sign(sk, SM.seal_digest(h.ljust(32, b"\0"), suffix, B.keccak256))
    return _SEALS[key]


def encode(sk: bytes, height, round_, typ, h, seal=None, suffix=None) -> bytes:
    body = wire.prepare_body(h) if typ == PREPARE else wire.commit_body(h, seal if seal is not None else seal_of(sk, h, suffix))
    m = wire.IbftMessage(view=wire.View(height, round_), sender=B.address(B.pubkey(sk)), type=wire.PREPARE if typ == PREPARE else wire.COMMIT,
                         payload=body)
    m.signature = B.sign(sk, B.keccak256(m.payload_no_sig()))
    return m.encode()


def _flip(seal: bytes, at: int = 9) -> bytes:
    return seal[:at] + bytes([seal[at] ^ 0x55]) + seal[at + 1:]


def bad_seal_commit(pool, kind, i, s, height, round_, suffix):
    """the COMMIT of pool member i (a member of set s) naming HA in (height, round) whose envelope is fine and whose seal is
    what `kind` names"""
    sk = pool.sks[i]
    good = seal_of(sk, HA, suffix)
    if kind == "good":
        return encode(sk, height, round_, COMMIT, HA, suffix=suffix)
    if kind == "seal_flip":
        return encode(sk, height, round_, COMMIT, HA, _flip(good))
    if kind == "seal_other_hash":
        return encode(sk, height, round_, COMMIT, HA, seal_of(sk, HB, suffix))
    if kind == "seal_other_member":                    # a valid seal over the right digest — by another member of the set
        other = next(k for k in WS.MEMBERS[s] if k != i)
        return encode(sk, height, round_, COMMIT, HA, seal_of(pool.sks[other], HA, suffix))
    if kind == "seal_outsider":
        return encode(sk, height, round_, COMMIT, HA, seal_of(_outsider(), HA, suffix))
    if kind == "seal_recid":
        return encode(sk, height, round_, COMMIT, HA, good[:64] + b"\x04")
    if kind == "seal_64":
        return encode(sk, height, round_, COMMIT, HA, good[:64])
    if kind == "hash31":
        return encode(sk, height, round_, COMMIT, H31, suffix=suffix)
    assert kind == "hash0"
    return encode(sk, height, round_, COMMIT, H0, suffix=suffix)


def bad_envelope_commit(pool, kind, i, s, height, round_, suffix, j=0):
    """a COMMIT naming HA whose seal is perfect — by the key the message says it is from — and whose envelope is `kind`"""
    if kind == "sig_flip":
        m = encode(pool.sks[i], height, round_, COMMIT, HA, suffix=suffix)
        at = m.index(b"\x1a\x41") + 2 + (7 * j) % 64
        return m[:at] + bytes([m[at] ^ 0xFF]) + m[at + 1:]
    if kind == "not_in_set":
        return encode(pool.sks[WS.NOT_IN_SET[s]], height, round_, COMMIT, HA, suffix=suffix)
    if kind == "outsider":
        return encode(_outsider(), height, round_, COMMIT, HA, suffix=suffix)
    if kind == "future":
        return encode(pool.sks[i], WS.FUTURE_HEIGHT, round_, COMMIT, HA, suffix=suffix)
    assert kind == "padded_height"          # the height's varint padded: NEEDS_HOST without the recode flag
    m = encode(pool.sks[i], WS.RECODE_HEIGHT, round_, COMMIT, HA, suffix=suffix)
    assert m.startswith(b"\x0a") and m[2:5] == b"\x08\xe4\x01"
    return bytes([0x0a, m[1] + 1]) + b"\x08\xe4\x81\x00" + m[5:]


class Corpus(WS.Corpus):
    suffix = None


_CACHE = {}


def _finish(key, big, msgs, kinds, senders, suffix):
    base = WS.corpus(big=big)
    c = Corpus(msgs, kinds, senders, base.pool, big, base.powers)
    c.suffix = suffix
    _CACHE[key] = c
    return c


def corpus_s(big: bool = False, suffix=None) -> Corpus:
    key = ("s", big, suffix)
    if key in _CACHE:
        return _CACHE[key]
    if big:                                 # the same messages under u256 powers
        a = corpus_s(False, suffix)
        return _finish(key, True, a.msgs, a.kinds, a.senders, suffix)
    pool = WS.corpus().pool
    msgs, kinds, senders = [], [], []

    def add(i, m, kind="good"):
        msgs.append(m)
        kinds.append(kind)
        senders.append(i)

    def pair(i, height, round_, commit, kind):
        """a special COMMIT and, behind it, the same sender's PREPARE of the round: the queue stays mixed"""
        add(i, commit, kind)
        add(i, encode(pool.sks[i], height, round_, PREPARE, HA), "prepare")

    # the body: round 0 of heights 100 and 101, ten members each, PREPARE and COMMIT alternating, all seals good
    for k in range(10):
        for s in (0, 1):
            i = WS.MEMBERS[s][k]
            add(i, encode(pool.sks[i], WS.HEIGHTS[s], 0, PREPARE, HA), "prepare")
            add(i, encode(pool.sks[i], WS.HEIGHTS[s], 0, COMMIT, HA, suffix=suffix))
    # every kind of seal under a fine envelope: round 1 of height 100, one sender each (and three good ones)
    for k, kind in enumerate(SEAL_KINDS + ("good", "good")):
        i = WS.MEMBERS[0][12 + k]
        pair(i, 100, 1, bad_seal_commit(pool, kind, i, 0, 100, 1, suffix), kind)
    # superseding, round 1 of height 101 (set 1): a sender's later COMMIT of the view replaces the earlier one
    m1 = WS.MEMBERS[1]
    a, b, c_, plain = m1[10], m1[11], m1[12], m1[13:17]
    pair(a, 101, 1, bad_seal_commit(pool, "good", a, 1, 101, 1, suffix), "good_then_bad")
    pair(b, 101, 1, bad_seal_commit(pool, "seal_flip", b, 1, 101, 1, suffix), "bad_then_good")
    pair(c_, 101, 1, bad_seal_commit(pool, "good", c_, 1, 101, 1, suffix), "ha_then_hb")
    for i in plain:
        pair(i, 101, 1, bad_seal_commit(pool, "good", i, 1, 101, 1, suffix), "good")
    pair(a, 101, 1, bad_seal_commit(pool, "seal_flip", a, 1, 101, 1, suffix), "good_then_bad")
    pair(b, 101, 1, bad_seal_commit(pool, "good", b, 1, 101, 1, suffix), "bad_then_good")
    pair(c_, 101, 1, encode(pool.sks[c_], 101, 1, COMMIT, HB, suffix=suffix), "ha_then_hb")
    # perfect seals inside bad envelopes: round 2 of height 100
    for k, kind in enumerate(ENVELOPE_KINDS):
        i = WS.MEMBERS[1][3] if kind == "padded_height" else WS.MEMBERS[0][24 + k]
        sender = {"not_in_set": WS.NOT_IN_SET[0], "outsider": -1}.get(kind, i)
        add(sender, bad_envelope_commit(pool, kind, i, 0, 100, 2, suffix, k), kind)
        add(i, encode(pool.sks[i], 100, 2, PREPARE, HA), "prepare")
    # the quorum edge: two COMMIT views of height 105 — set 2, five members of near-equal power, quorum four — with four stored
    # senders each: all four seals good in round 0, one of them bad in round 1
    m2 = WS.MEMBERS[2]
    for k in range(4):
        i = m2[k]
        pair(i, EDGE_HEIGHT, EDGE_FULL_ROUND, bad_seal_commit(pool, "good", i, 2, EDGE_HEIGHT, EDGE_FULL_ROUND, suffix), "edge_full")
        kind = "seal_other_hash" if k == 2 else "good"
        pair(i, EDGE_HEIGHT, EDGE_SHORT_ROUND, bad_seal_commit(pool, kind, i, 2, EDGE_HEIGHT, EDGE_SHORT_ROUND, suffix),
             "edge_short_bad" if k == 2 else "edge_short")
    # round 2 of height 101: more of the plain mix, to about 150 rows
    for k in range(19):
        i = WS.MEMBERS[1][k]
        add(i, encode(pool.sks[i], 101, 2, COMMIT, HA, suffix=suffix))
        if k % 2:
            add(i, encode(pool.sks[i], 101, 2, PREPARE, HB), "prepare")
    return _finish(key, big, msgs, kinds, senders, suffix)


T_ROWS, T_BAD = 65, (0, 63)


def corpus_t(n: int = T_ROWS) -> Corpus:
    """65 sealable COMMIT rows (rounds 0 and 1 of height 100), the seals of rows 0 and 63 bad; or its first n rows"""
    key = ("t", n)
    if key in _CACHE:
        return _CACHE[key]
    if n != T_ROWS:
        t = corpus_t()
        return _finish(key, False, t.msgs[:n], t.kinds[:n], t.senders[:n], None)
    pool = WS.corpus().pool
    msgs, kinds, senders = [], [], []
    for j in range(T_ROWS):
        i = WS.MEMBERS[0][j % 40]
        kind = "seal_flip" if j in T_BAD else "good"
        msgs.append(bad_seal_commit(pool, kind, i, 0, 100, j // 40, None))
        kinds.append(kind)
        senders.append(i)
    return _finish(key, False, msgs, kinds, senders, None)


def corpus_b(n: int = B_ROWS) -> Corpus:
    """n rows (default B_ROWS): COMMITs and PREPAREs interleaved, a fifth of the COMMITs with a bad seal"""
    key = ("b", n)
    if key in _CACHE:
        return _CACHE[key]
    pool = WS.corpus().pool
    msgs, kinds, senders = [], [], []
    commits = 0
    for j in range(n):
        i = WS.MEMBERS[0][j % 40]
        everywhere = j % 7 == 0                # one COMMIT view with rows in every workgroup; its senders come again 280 rows on
        typ = COMMIT if everywhere or j % 2 == 0 else PREPARE
        round_ = 0 if everywhere else 1 + j // 200
        h = HA if everywhere or j % 5 else HB
        kind = "everywhere" if everywhere else "good" if typ == COMMIT else "prepare"
        if typ == COMMIT:
            commits += 1
            if commits % 5 == 0:
                kind = "everywhere_bad" if everywhere else "seal_flip"
        seal = _flip(seal_of(pool.sks[i], h, None)) if kind in ("everywhere_bad", "seal_flip") else None
        msgs.append(encode(pool.sks[i], 100, round_, typ, h, seal))
        kinds.append(kind)
        senders.append(i)
    return _finish(key, False, msgs, kinds, senders, None)


def corpus_c() -> Corpus:
    key = ("c",)
    if key in _CACHE:
        return _CACHE[key]
    pool = WS.corpus().pool
    msgs, kinds, senders = [], [], []
    for j in range(C_ROWS):
        i = WS.MEMBERS[0][j % 40]
        bad = j % 3 == 2
        msgs.append(encode(pool.sks[i], 100, j, COMMIT, HA, _flip(seal_of(pool.sks[i], HA, None)) if bad else None))
        kinds.append("seal_flip" if bad else "good")
        senders.append(i)
    return _finish(key, False, msgs, kinds, senders, None)


_EXPECTED = {}


def expected(c: Corpus, height_map, recode: bool, views_cap: int, suffix="corpus"):
    """the models' whole answer for the corpus on a context whose seal-digest convention is `suffix` (default: the one the corpus
    was signed under) → the dictionary of wire_views_cases.expected (the views call's answer: view, stored, records as
    `views_records`) plus seal, commit_rows, seal_rows, dense and the seal-form records; computed once and shared"""
    suffix = c.suffix if suffix == "corpus" else suffix
    key = (id(c), tuple(height_map[0]), recode, views_cap, suffix)
    if key not in _EXPECTED:
        bits, rset, vidx, tallies, parsed = WS.expected(c, len(c.msgs), height_map, recode)
        sets = c.model_sets()
        rows = [(bits[j], e.type, e.height, e.round, e.proposal_hash, rset[j], e.sender) for j, e in enumerate(parsed)]

        def check(j, p):
            return B.recover_address(SM.seal_digest(p.proposal_hash, suffix, B.keccak256), p.committed_seal) == p.sender

        seal, commit_rows, seal_rows, dense = SM.seal_bits(parsed, bits, rset, sets, check)
        view, stored, n_views, plain = SM.VM.views(rows, views_cap, sets, VC.proposers(c))
        _, _, _, records = SM.views(rows, seal, views_cap, sets, VC.proposers(c))
        _EXPECTED[key] = dict(bits=bits, set=rset, vidx=vidx, tallies=tallies, parsed=parsed, view=view, stored=stored, n_views=n_views,
                              views_records=plain, records=records, seal=seal, commit_rows=commit_rows, seal_rows=seal_rows, dense=dense,
                              rows=rows)
    return _EXPECTED[key]
