"""Validator sets whose addresses collide in the open-addressing table every verdict route ends in (valset_lookup / addr_hash,
recover_dev.h).  The hash has no salt and validators grind their own keys, so whoever joins a set chooses where its address
lands; the sets of every other corpus come from random keys and never make the probe loop walk more than a few slots.

Plain Python, no call under test: a port of addr_hash, the builders' insertion rule (the smallest power of two ≥ 64 slots with
slots ≥ 2·n + 2, linear probing, a repeated address keeps its first index), and three corpora of REAL keys (oracle.binding)
picked from a fixed pool by the bucket they hash to:

  chain64   31 members (2n + 2 = 64: the table is as full as the rule lets it get), all in ONE bucket near the end of the table:
            the chain wraps through slot 63 to slot 0 and the member listed last sits 30 probes from its bucket
  chain128  32 members (2n + 2 = 66: the first size with 128 slots), half in bucket 126, half in bucket 127: the chain wraps
  decoys    a real signer A behind five addresses D_w that equal A in every 32-bit word but word w (w = 0 … 4) and five B_w
            that differ from A in ONE BIT of word w, all ground into A's bucket and listed before A; the all-zero address as
            a member; a colliding real address C listed twice with two powers (first index, last power)

and for each of them outsiders — non-members that hash into the head and into the middle of the chain, real keys with valid
signatures and one-word neighbours of members that no key stands behind: they walk the whole cluster and come back as −1.

Member i (by listing position) has power 1 << i, so a tallied power IS the set of indices that were counted.
tests/test_valset_collision_inputs.py asserts, under the model alone, that every corpus holds what is claimed here."""
import functools
import hashlib
import struct
from collections import namedtuple

MIN_SLOTS = 64
ZERO = bytes(20)

# ---- the model ------------------------------------------------------------------------------------------------------------
_MUL = (0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F, 0x165667B1)
_SHIFT = (15, 13, 16, 15)
_M32 = 0xFFFFFFFF


def words(addr20: bytes):
    """the five little-endian 32-bit words the device compares"""
    return struct.unpack("<5I", addr20)


def from_words(w) -> bytes:
    return struct.pack("<5I", *w)


def addr_hash(addr20: bytes) -> int:
    a = words(addr20)
    h = (a[0] * _MUL[0]) & _M32
    for i in range(1, 5):
        h = ((h ^ (h >> _SHIFT[i - 1])) + a[i] * _MUL[i]) & _M32
    return h ^ (h >> 16)


def slots_for(n: int) -> int:
    slots = MIN_SLOTS
    while slots < 2 * n + 2:
        slots <<= 1
    return slots


def bucket(addr20: bytes, slots: int) -> int:
    return addr_hash(addr20) & (slots - 1)


def build_table(addrs, slots=None):
    """→ (slots, table): table[s] = (address, index) or None; the index counts DISTINCT addresses in listing order"""
    slots = slots or slots_for(len(addrs))
    table = [None] * slots
    nxt = 0
    for a in addrs:
        s = bucket(a, slots)
        while True:
            if table[s] is None:
                table[s] = (a, nxt)
                nxt += 1
                break
            if table[s][0] == a:
                break
            s = (s + 1) & (slots - 1)
    return slots, table


def probe(table, addr20: bytes):
    """→ (index or −1, occupied slots passed before the answer, wrapped past the last slot?)"""
    slots = len(table)
    s = bucket(addr20, slots)
    for walked in range(slots):
        e = table[s]
        if e is None:
            return -1, walked, s < bucket(addr20, slots)
        if e[0] == addr20:
            return e[1], walked, s < bucket(addr20, slots)
        s = (s + 1) & (slots - 1)
    return -1, slots, True


def distinct(addrs):
    seen, out = set(), []
    for a in addrs:
        if a not in seen:
            seen.add(a)
            out.append(a)
    return out


def final_powers(addrs, powers):
    """address → its power as every builder keeps it: the LAST one listed"""
    return {a: p for a, p in zip(addrs, powers)}


def differing_words(a: bytes, b: bytes):
    return [i for i, (x, y) in enumerate(zip(words(a), words(b))) if x != y]


# ---- real keys ------------------------------------------------------------------------------------------------------------
Key = namedtuple("Key", "sk addr")
_pool = []


def key_pool(count: int):
    """the first `count` keys of a fixed sequence (sk = SHA-256 of a counter), with the oracle's public key → address"""
    from oracle import binding as B
    while len(_pool) < count:
        sk = hashlib.sha256(b"valset-collision-key-%d" % len(_pool)).digest()
        pub = B.pubkey(sk)
        assert pub is not None
        _pool.append(Key(sk, B.address(pub)))
    return _pool[:count]


def grind_word(addr20: bytes, w: int, slots: int, want_bucket: int, avoid=(), single_bit=False):
    """an address equal to addr20 in every word but word w that hashes to want_bucket (None if single_bit and no bit does) →
    (address, tries)"""
    a = list(words(addr20))
    tries = 0
    for t in ([1 << k for k in range(32)] if single_bit else range(1, 1 << 32)):
        tries += 1
        c = list(a)
        c[w] = a[w] ^ t
        cand = from_words(c)
        if bucket(cand, slots) == want_bucket and cand not in avoid:
            return cand, tries
    return None, tries


# ---- the corpora ----------------------------------------------------------------------------------------------------------
# an outsider: addr no member; sk its key or None (a ground neighbour of `near`); walk: the occupied slots its lookup passes
Outsider = namedtuple("Outsider", "addr sk where walk near")
Corpus = namedtuple("Corpus", "name addrs powers keys slots outsiders A decoys bit_decoys twice")
POOL = 3000


def _powers(n):
    assert n <= 62
    return [1 << i for i in range(n)]


def _outsiders(table, slots, members, head, mid, pool, n_real=2):
    out = []
    used = set(members)
    for where, b in (("head", head), ("middle", mid)):
        real = [k for k in pool if bucket(k.addr, slots) == b and k.addr not in used][:n_real]
        assert len(real) == n_real, (where, b)
        for k in real:
            used.add(k.addr)
            out.append(Outsider(k.addr, k.sk, where, probe(table, k.addr)[1], None))
        for j, w in enumerate((0, 4)):                      # a neighbour of a member in its first / its last word
            near = members[(7 * j + 3) % len(members)]
            cand, _ = grind_word(near, w, slots, b, avoid=used)
            used.add(cand)
            out.append(Outsider(cand, None, where, probe(table, cand)[1], near))
    return out


@functools.lru_cache(None)
def chain64() -> Corpus:
    pool = key_pool(POOL)
    slots = slots_for(31)
    by = {}
    for k in pool:
        by.setdefault(bucket(k.addr, slots), []).append(k)
    b = next(b for b in range(slots - 3, slots - 24, -1) if len(by.get(b, ())) >= 31 + 2)
    ks = by[b][:31]
    addrs = [k.addr for k in ks]
    _, table = build_table(addrs)
    outs = _outsiders(table, slots, addrs, b, (b + 15) & (slots - 1), pool)
    return Corpus("chain64", addrs, _powers(31), {k.addr: k.sk for k in ks}, slots, outs, None, (), (), None)


@functools.lru_cache(None)
def chain128() -> Corpus:
    slots = slots_for(32)
    count = POOL
    while True:
        pool = key_pool(count)
        lo = [k for k in pool if bucket(k.addr, slots) == slots - 2]
        hi = [k for k in pool if bucket(k.addr, slots) == slots - 1]
        if len(lo) >= 16 + 2 and len(hi) >= 16:
            break
        count += 1000
    ks = [k for pair in zip(hi[:16], lo[:16]) for k in pair]
    addrs = [k.addr for k in ks]
    _, table = build_table(addrs)
    outs = _outsiders(table, slots, addrs, slots - 2, 12, pool)
    return Corpus("chain128", addrs, _powers(32), {k.addr: k.sk for k in ks}, slots, outs, None, (), (), None)


@functools.lru_cache(None)
def decoys() -> Corpus:
    pool = key_pool(POOL)
    slots = MIN_SLOTS
    by = {}
    for k in pool:
        by.setdefault(bucket(k.addr, slots), []).append(k)
    for A in pool:                                          # the first key with a one-bit neighbour in its bucket in every word
        bA = bucket(A.addr, slots)
        if not 8 <= bA < 40 or len(by[bA]) < 4:              # (the chain stays clear of slot 0, where the zero address sits)
            continue
        bits = [grind_word(A.addr, w, slots, bA, single_bit=True)[0] for w in range(5)]
        if all(bits):
            break
    else:
        raise AssertionError("no key of the pool has one-bit neighbours in its bucket")
    D = []
    for w in range(5):
        D.append(grind_word(A.addr, w, slots, bA, avoid=set(bits) | set(D))[0])
    Ck = next(k for k in by[bA] if k.addr != A.addr)
    addrs = D + bits + [ZERO, Ck.addr, A.addr, Ck.addr]
    assert slots_for(len(addrs)) == slots
    _, table = build_table(addrs)
    members = distinct(addrs)
    outs = _outsiders(table, slots, members, bA, (bA + 5) & (slots - 1), pool)
    for w in range(5):                                      # one more one-word neighbour of A per word, NOT a member
        cand, _ = grind_word(A.addr, w, slots, bA, avoid=set(members) | {o.addr for o in outs})
        outs.append(Outsider(cand, None, "head", probe(table, cand)[1], A.addr))
    return Corpus("decoys", addrs, _powers(len(addrs)), {A.addr: A.sk, Ck.addr: Ck.sk}, slots, outs, A.addr, tuple(D), tuple(bits),
                  Ck.addr)


CORPORA = {"chain64": chain64, "chain128": chain128, "decoys": decoys}


# ---- rows -----------------------------------------------------------------------------------------------------------------
# what: "member" (its own seal, its own address), "outsider" (a real key outside the set), "keyless" (a member's seal that
# claims an address no key stands behind: an outsider's, or a decoy's that IS a member), "swap" (a member's seal that claims
# another member), "nothing" (no key is recovered; claims the zero address).  sk: the key the signature was made with.
Row = namedtuple("Row", "what hash sig claimed sk")


def digest(tag: bytes) -> bytes:
    return hashlib.sha256(b"valset-collision-digest-" + tag).digest()


def spoil(sig65: bytes, how: int) -> bytes:
    """a signature that recovers nothing: how = 0: v = 2, how = 1: r = 0"""
    return sig65[:64] + b"\x02" if how == 0 else bytes(32) + sig65[32:]


@functools.lru_cache(None)
def rows(name: str):
    """the rows of a corpus for the seal routes (every member, every outsider, members' seals that claim somebody else)"""
    from oracle import binding as B
    c = CORPORA[name]()
    out = []
    keyed = [a for a in distinct(c.addrs) if a in c.keys]
    for i, a in enumerate(keyed):
        h = digest(b"%s-%d" % (name.encode(), i))
        out.append(Row("member", h, B.sign(c.keys[a], h), a, c.keys[a]))
    for i, o in enumerate(c.outsiders):
        h = digest(b"%s-out-%d" % (name.encode(), i))
        if o.sk is not None:
            out.append(Row("outsider", h, B.sign(o.sk, h), o.addr, o.sk))
        else:
            near = o.near if o.near in c.keys else keyed[0]
            out.append(Row("keyless", h, B.sign(c.keys[near], h), o.addr, c.keys[near]))
    signer = c.A if c.A is not None else keyed[-1]
    for i, d in enumerate(c.decoys + c.bit_decoys):         # A's seal under the name of each of its decoys
        h = digest(b"%s-decoy-%d" % (name.encode(), i))
        out.append(Row("keyless", h, B.sign(c.keys[signer], h), d, c.keys[signer]))
    for i in range(min(4, len(keyed) - 1)):                 # a member's seal under another member's name
        h = digest(b"%s-swap-%d" % (name.encode(), i))
        out.append(Row("swap", h, B.sign(c.keys[keyed[i]], h), keyed[-1 - i], c.keys[keyed[i]]))
    h = digest(name.encode() + b"-nothing")
    good = B.sign(c.keys[signer], h)
    out.append(Row("nothing", h, spoil(good, 0), ZERO, c.keys[signer]))    # v = 2
    out.append(Row("nothing", h, spoil(good, 1), ZERO, c.keys[signer]))    # r = 0
    return tuple(out)


def columns(rws):
    import numpy as np
    col = lambda xs, w: np.frombuffer(b"".join(xs), np.uint8).reshape(-1, w).copy()
    return col([r.hash for r in rws], 32), col([r.sig for r in rws], 65), col([r.claimed for r in rws], 20)


def addr_column(addrs):
    import numpy as np
    return np.frombuffer(b"".join(addrs), np.uint8).reshape(-1, 20).copy()


def list_index(addrs, addr20: bytes) -> int:
    """the index every builder gives: the position among the DISTINCT addresses in listing order, −1: not listed"""
    d = distinct(addrs)
    return d.index(addr20) if addr20 in d else -1
