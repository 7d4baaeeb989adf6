"""The GPU corpora of ibft_verify_senders_wire_views (tests/test_gpu_wire_views.py), built on the CPU with the oracle's encoder
and signer over the key pool, the four sets and the two height maps of tests/wire_sets_cases.py, so that
tests/test_wire_views_inputs.py can check without a GPU that each holds every case it claims.

  A  about 360 rows: heights 100 / 101 / 105 (sets 0 / 1 / 2), rounds 0-2, PREPARE and COMMIT, and the special rows listed in
     corpus_a — two hashes in a view, repeats, a sender who changes its hash, the proposer's PREPARE, short hashes, the empty
     View, every invalid kind of wire_sets_cases.KINDS BEHIND a valid row of the same sender and view, a recodable row
  B  601 rows = two full workgroups of the row kernels (256 rows each) and a partial one, not a multiple of 64: one view with
     rows in every workgroup, senders whose earlier and later rows lie in different workgroups
  C  1 500 valid rows, every row its own round (1 500 views: ranks across the whole scan, 64 views in every wavefront), and 20
     repeats far beyond view 100, which at views_cap = 100 are −2 rows that still supersede
"""
import numpy as np

import wire_sets_cases as WS
import wire_views_model as VM
from oracle import binding as B
from oracle import wire

PREPARE, COMMIT = VM.PREPARE, VM.COMMIT
HA = bytes(range(1, 33))
HB = bytes(range(101, 133))
H31 = HA[:31]                    # a key of its own: hash_len is part of the key
H0 = b""
PROPOSER_HEIGHT, PROPOSER_FIRST = 100, 0
PROPOSER_POOL = (3, 5)           # pool indices of the proposers of rounds 0 and 1 of height 100 (members of set 0)
TWICE, CHANGER, CROSS_ROUND = 0, 1, 2     # pool indices of the senders of the named cases in corpus A
EMPTY_VIEW_SENDER = 36           # a member of set 2: map B makes its empty View a valid row of height 0


def _encode(pool, i, height, round_, typ, h, view="canonical", sk=None):
    sk = sk if sk is not None else pool.sks[i]
    v = {"canonical": wire.View(height, round_), "none": None, "empty": wire.View(0, 0)}[view]
    body = wire.prepare_body(h) if typ == PREPARE else wire.commit_body(h, pool.seal65[i].tobytes())
    m = wire.IbftMessage(view=v, sender=B.address(B.pubkey(sk)), type=wire.PREPARE if typ == PREPARE else wire.COMMIT, payload=body)
    m.signature = B.sign(sk, B.keccak256(m.payload_no_sig()))
    return m.encode()


def _invalid(pool, kind, i, s, height, round_, typ, outsider, j):
    """the message sender i of set s would have sent in (height, round, type) with hash HB, made invalid the way `kind` names"""
    if kind == "sig_flip":
        m = _encode(pool, i, height, round_, typ, HB)
        at = m.index(b"\x1a\x41") + 2 + (7 * j) % 64
        return m[:at] + bytes([m[at] ^ 0xFF]) + m[at + 1:]
    if kind == "outsider":
        return _encode(pool, i, height, round_, typ, HB, sk=outsider)
    if kind == "not_in_set":
        return _encode(pool, WS.NOT_IN_SET[s], height, round_, typ, HB)
    if kind == "needs_host":
        return _encode(pool, i, height, round_, typ, HB) + b"\x48\x01"
    if kind == "no_view":
        return _encode(pool, i, height, round_, typ, HB, view="none")
    if kind == "empty_view":
        return _encode(pool, i, height, round_, typ, HB, view="empty")
    if kind == "future":
        return _encode(pool, i, WS.FUTURE_HEIGHT, round_, typ, HB)
    if kind == "max_height":
        return _encode(pool, i, 2**64 - 1, round_, typ, HB)
    if kind == "below":
        return _encode(pool, i, 99, round_, typ, HB)
    assert kind == "padded_height"          # the height's varint padded: NEEDS_HOST without the recode flag
    m = _encode(pool, i, WS.RECODE_HEIGHT, round_, typ, HB)
    assert m.startswith(b"\x0a") and m[2:5] == b"\x08\xe4\x01"
    return bytes([0x0a, m[1] + 1]) + b"\x08\xe4\x81\x00" + m[5:]


_CACHE = {}


def _finish(name, big, msgs, kinds, senders):
    base = WS.corpus(big=big)
    c = WS.Corpus(msgs, kinds, senders, base.pool, big, base.powers)
    _CACHE[(name, big)] = c
    return c


def corpus_a(big: bool = False) -> WS.Corpus:
    if ("a", big) in _CACHE:
        return _CACHE[("a", big)]
    if big:                                 # the same messages under u256 powers
        a = corpus_a(False)
        return _finish("a", True, a.msgs, a.kinds, a.senders)
    pool = WS.corpus(big=big).pool
    outsider = WS.W.validator_key(2701 ^ 0x77, 1 << 41)
    msgs, kinds, senders = [], [], []

    def add(i, height, round_, typ, h, kind="good", m=None):
        msgs.append(m if m is not None else _encode(pool, i, height, round_, typ, h))
        kinds.append(kind)
        senders.append(i)

    # the body: every (height, round, type) with up to 28 members of the height's set (28 of 40, 23 of 23, 5 of 5), hash HA —
    # the same senders in all three rounds, where nothing is superseded.  Left out on purpose: the proposers' own PREPAREs
    # (added below where wanted).
    for s, height in enumerate(WS.HEIGHTS):
        for round_ in range(3):
            for typ in (PREPARE, COMMIT):
                for i in WS.MEMBERS[s][:28]:
                    if typ == PREPARE and height == PROPOSER_HEIGHT and i in PROPOSER_POOL:
                        continue
                    add(i, height, round_, typ, HA)
    # two hashes in one view; a sender twice under one key; a sender with hash A then B (two records change)
    for i in (30, 31, 32):
        add(i, 100, 0, PREPARE, HB, "second_hash")
    # a key whose only row is superseded: its record stays, with S_v empty
    add(33, 100, 1, COMMIT, HB, "lone_superseded")
    add(33, 100, 1, COMMIT, HA, "lone_superseder")
    add(TWICE, 100, 0, PREPARE, HA, "twice")
    add(CHANGER, 100, 0, PREPARE, HB, "changer")
    # the proposer of round 0 sends a PREPARE naming HA: the record of (100, 0, PREPARE, HA) has no quorum whatever its power;
    # the proposer of round 1 names HB: a stored row in the VIEW but not under the key HA, whose record seats it
    for i in (34, 35):                     # (enough power under that key for a quorum, were it not for the proposer's row)
        add(i, 100, 0, PREPARE, HA)
    add(PROPOSER_POOL[0], 100, 0, PREPARE, HA, "proposer_prepare")
    add(PROPOSER_POOL[1], 100, 1, PREPARE, HB, "proposer_other_hash")
    # hash_len 31 and 0: keys of their own
    for i in (30, 29, 28):
        add(i, 101, 1, COMMIT, H31, "hash31")
        add(i, 101, 1, PREPARE, H0, "hash0")
    # an empty View: height 0, which map B gives to set 2 (and map A to none)
    add(EMPTY_VIEW_SENDER, 0, 0, PREPARE, HA, "empty_view_valid", _encode(pool, EMPTY_VIEW_SENDER, 0, 0, PREPARE, HA, view="empty"))
    add(EMPTY_VIEW_SENDER + 1, 0, 0, PREPARE, HA, "empty_view_valid", _encode(pool, EMPTY_VIEW_SENDER + 1, 0, 0, PREPARE, HA, view="empty"))
    # every invalid kind BEHIND a valid row of the same sender and view (the body's), naming HB: were it to supersede, the
    # sender's HA row would lose its stored bit and a record of HB would appear or grow
    for j, kind in enumerate(k for k in WS.KINDS if k != "good"):
        s = j % 2
        i = WS.MEMBERS[s][4 + j % 5]
        if kind == "padded_height":
            i = WS.MEMBERS[1][3]          # a member of set 1, which the decoded height 228 is judged under with the flag on
        add(i, WS.HEIGHTS[s], 2, COMMIT, HB, kind, _invalid(pool, kind, i, s, WS.HEIGHTS[s], 2, COMMIT, outsider, j))
    return _finish("a", big, msgs, kinds, senders)


B_ROWS = 601


def corpus_b() -> WS.Corpus:
    if ("b", False) in _CACHE:
        return _CACHE[("b", False)]
    pool = WS.corpus().pool
    msgs, kinds, senders = [], [], []
    for j in range(B_ROWS):
        i = WS.MEMBERS[0][j % 40]
        if j % 7 == 0:                     # one view with rows in every workgroup
            msgs.append(_encode(pool, i, 100, 0, COMMIT, HA))
            kinds.append("everywhere")
        else:
            msgs.append(_encode(pool, i, 100, j // 200, PREPARE if j % 2 else COMMIT, HA if j % 5 else HB))
            kinds.append("good")
        senders.append(i)
    return _finish("b", False, msgs, kinds, senders)


C_VIEWS, C_REPEATS = 1500, 20


def corpus_c() -> WS.Corpus:
    if ("c", False) in _CACHE:
        return _CACHE[("c", False)]
    pool = WS.corpus().pool
    msgs, kinds, senders = [], [], []
    for j in range(C_VIEWS):
        i = WS.MEMBERS[0][j % 40]
        msgs.append(_encode(pool, i, 100, j, PREPARE, HA))
        kinds.append("good")
        senders.append(i)
    for k in range(C_REPEATS):             # the same sender again in its round, far beyond view 100
        j = 200 + 61 * k
        msgs.append(msgs[j])
        kinds.append("repeat")
        senders.append(senders[j])
    return _finish("c", False, msgs, kinds, senders)


def proposers(c: WS.Corpus) -> VM.Proposers:
    return VM.Proposers(PROPOSER_HEIGHT, PROPOSER_FIRST, [c.pool.addrs[i].tobytes() for i in PROPOSER_POOL])


_EXPECTED = {}


def expected(c: WS.Corpus, height_map, recode: bool, views_cap: int, with_proposers: bool = True):
    """the model's whole answer for the corpus → dict(bits, set, vidx, tallies, parsed, view, stored, n_views, records);
    computed once per (corpus, map, flag, cap, table) and shared — nobody changes it"""
    key = (id(c), tuple(height_map[0]), recode, views_cap, with_proposers)
    if key not in _EXPECTED:
        bits, rset, vidx, tallies, parsed = WS.expected(c, len(c.msgs), height_map, recode)
        rows = [(bits[j], e.type, e.height, e.round, e.proposal_hash, rset[j], e.sender) for j, e in enumerate(parsed)]
        view, stored, n_views, records = VM.views(rows, views_cap, c.model_sets(), proposers(c) if with_proposers else None)
        _EXPECTED[key] = dict(bits=bits, set=rset, vidx=vidx, tallies=tallies, parsed=parsed, view=view, stored=stored, n_views=n_views,
                              records=records)
    return _EXPECTED[key]


def device_columns(c: WS.Corpus, height_map, recode: bool):
    """the columns the views stage reads on the device, from the model: parsed rows as ibft_wire_row_t (the fields the stage
    looks at), valid bytes, index in the row's set, the row's set"""
    e = expected(c, height_map, recode, len(c.msgs))
    n = len(c.msgs)
    rows = np.zeros(n, WS_WIRE_ROW)
    for j, p in enumerate(e["parsed"]):
        rows[j]["height"], rows[j]["round"], rows[j]["type"], rows[j]["status"] = p.height, p.round, p.type, p.status
        rows[j]["hash_len"] = len(p.proposal_hash)
        rows[j]["proposal_hash"][:len(p.proposal_hash)] = np.frombuffer(p.proposal_hash, np.uint8)
    return (rows, np.array(e["bits"], np.uint8), np.array(e["vidx"], np.int32), np.array(e["set"], np.int32))


WS_WIRE_ROW = np.dtype([("height", "<u8"), ("round", "<u8"), ("status", "u1"), ("type", "u1"), ("payload_kind", "u1"),
                        ("has_view", "u1"), ("hash_len", "u1"), ("seal_len", "u1"), ("from_len", "u1"), ("sig_len", "u1"),
                        ("from", "u1", 20), ("proposal_hash", "u1", 32), ("pad", "u1", 4)])
