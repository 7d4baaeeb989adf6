"""Rows for the recode class tests (IBFT_FLAG_WIRE_RECODE): meaning-preserving scramblers over honestly signed PREPARE /
COMMIT messages of an oracle.workload round, named rows outside the class, and a seeded random composition of the
scramblers.  Every scrambled row decodes — by the protobuf rules — to the message that was signed, so its canonical
re-encoding is the signed canonical row.  Test infrastructure only (uses the oracle's encoder and signer)."""
from __future__ import annotations

import random
from dataclasses import dataclass

import numpy as np

from oracle import binding as B
from oracle import wire


def pv(v: int, width: int = 0) -> bytes:
    """varint of v, padded to `width` bytes when that is longer than the minimal form"""
    out = bytearray(wire.varint(v))
    while len(out) < width:
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


@dataclass
class Parts:
    """one signed message, field by field"""
    height: int
    round: int
    sender: bytes
    signature: bytes
    type: int
    kind: int  # 6 PrepareMessage, 7 CommitMessage
    hash: bytes
    seal: bytes = b""
    canonical: bytes = b""


def signed_parts(r, kinds=("commit", "prepare")) -> list[Parts]:
    """one honestly signed message per validator of round r, cycling through kinds"""
    out = []
    for i in range(r.n):
        commit = kinds[i % len(kinds)] == "commit"
        h, seal = r.hash32[i].tobytes(), r.seal65[i].tobytes() if commit else b""
        m = wire.IbftMessage(view=wire.View(r.height, r.round), sender=r.addrs[i].tobytes(), type=wire.COMMIT if commit else wire.PREPARE,
                             payload=wire.commit_body(h, seal) if commit else wire.prepare_body(h))
        m.signature = B.sign(r.sks[i], B.keccak256(m.payload_no_sig()))
        out.append(Parts(r.height, r.round, m.sender, m.signature, m.type, 7 if commit else 6, h, seal, m.encode()))
    return out


@dataclass
class Options:
    """how to spell a message; the default spells it canonically"""
    shuffle: random.Random | None = None  # field order at every level (occurrences of one field keep theirs)
    width: object = 0                     # bytes per varint and length prefix: an int, or a callable giving one per varint
    len_cap: int = 5                      # … but no length prefix longer than this (the class takes five bytes)
    split_view: bool = False              # View in two occurrences, one field each
    garbage_first: bool = False           # a wrong From and a wrong Signature in front of the real ones
    zero_first: bool = False              # explicit zero type, empty signature, empty From, zero height in front of the real ones
    oneof: str = ""                       # "other_first": the other member, filled, before the real one; "twice": the member in
                                          # two occurrences (a wrong hash first, then the real fields); "split": hash and seal apart


def spell(p: Parts, o: Options) -> bytes:
    def w():
        return o.width() if callable(o.width) else o.width

    def vf(num, v):
        return bytes([num << 3]) + pv(v, w())

    def lf(num, data):
        return bytes([(num << 3) | 2]) + pv(len(data), min(w(), o.len_cap)) + data

    def ordered(groups):
        """groups: lists of encoded fields, one list per field (or oneof); order inside a list is kept"""
        labels = [g for g, occ in enumerate(groups) for _ in occ]
        if o.shuffle is not None:
            o.shuffle.shuffle(labels)
        queues = [list(occ) for occ in groups]
        return b"".join(queues[g].pop(0) for g in labels)

    def view(height, round_):
        return lf(1, ordered([[vf(1, height)] if height else [], [vf(2, round_)] if round_ else []]))

    def body(kind, h, seal):
        return lf(kind, ordered([[lf(1, h)] if h else [], [lf(2, seal)] if seal and kind == 7 else []]))

    views = [view(p.height, 0), view(0, p.round)] if o.split_view else [view(p.height, p.round)]
    senders, sigs, types = [lf(2, p.sender)], [lf(3, p.signature)], [vf(4, p.type)] if p.type else []
    if o.garbage_first:
        senders.insert(0, lf(2, b"\xEE" * 20))
        sigs.insert(0, lf(3, b"\x5A" * 65))
    if o.zero_first:
        views.insert(0, lf(1, vf(1, 0) + vf(2, 0)))
        senders.insert(0, lf(2, b""))
        sigs.insert(0, lf(3, b""))
        types.insert(0, vf(4, 0))
    other = 13 - p.kind
    wrong = bytes(32 - i for i in range(32))
    if o.oneof == "other_first":
        payload = [body(other, wrong, b"\x77" * 65), body(p.kind, p.hash, p.seal)]
    elif o.oneof == "twice":
        payload = [body(p.kind, wrong, b""), body(p.kind, p.hash, p.seal)]
    elif o.oneof == "split" and p.kind == 7:
        payload = [body(7, b"", p.seal), body(7, p.hash, b"")]
    else:
        payload = [body(p.kind, p.hash, p.seal)]
    return ordered([views, senders, sigs, types, payload])


def scramblers(seed: int):
    """(name, Options) of every single scrambler"""
    out = [("reorder", Options(shuffle=random.Random(seed)))]
    out += [(f"pad{k}", Options(width=k)) for k in (2, 5, 10)]
    out += [("split view", Options(split_view=True)), ("garbage first", Options(garbage_first=True)),
            ("zero first", Options(zero_first=True)), ("other member first", Options(oneof="other_first")),
            ("member twice", Options(oneof="twice")), ("member split", Options(oneof="split"))]
    return out


def scrambled_each(parts: list[Parts], seed: int) -> list[tuple[str, bytes, Parts]]:
    """every scrambler on its own, each over some messages of both kinds: (name, bytes, the message)"""
    out = []
    for k, (name, o) in enumerate(scramblers(seed)):
        for p in (parts[(2 * k) % len(parts)], parts[(2 * k + 1) % len(parts)]):
            out.append((name, spell(p, o), p))
    return out


def random_options(rng: random.Random) -> Options:
    widths = rng.choice([(0,), (0, 0, 0, 2), (0, 1, 2, 3, 5, 10), (2,), (5,), (10,)])
    return Options(shuffle=rng if rng.random() < 0.7 else None, width=lambda: rng.choice(widths), split_view=rng.random() < 0.3,
                   garbage_first=rng.random() < 0.3, zero_first=rng.random() < 0.3,
                   oneof=rng.choice(["", "", "other_first", "twice", "split"]))


def random_scrambled(parts: list[Parts], count: int, seed: int) -> list[tuple[bytes, Parts]]:
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        p = rng.choice(parts)
        out.append((spell(p, random_options(rng)), p))
    return out


def named_in_class(p: Parts) -> list[tuple[str, bytes]]:
    """in the class, but not the encoding of an honestly signed message: defaults spelled out, odd lengths"""
    c = p.canonical
    body = wire._len_field(p.kind, wire.commit_body(p.hash, p.seal), emit_empty=True)
    return [
        ("only an explicit zero type", b"\x20\x00"),
        ("only an empty signature", b"\x1a\x00"),
        ("explicit zero type, empty signature, empty from", b"\x12\x00\x1a\x00\x20\x00" + body),
        ("empty view kept", b"\x12\x14" + p.sender + b"\x0a\x00"),
        ("view of explicit zeros", b"\x0a\x04\x10\x00\x08\x00" + body),
        ("21-byte from after the payload", body + b"\x12\x15" + p.sender + b"\x00"),
        ("64-byte signature, padded length", b"\x1a\xc0\x80\x00" + p.signature[:64] + b"\x12\x14" + p.sender),
        ("300-byte from", body + b"\x12\xac\x02" + p.sender * 15),
        ("66-byte seal", b"\x3a\x44\x12\x42" + p.seal.ljust(65, b"\x01") + b"\x01"),
        ("type 255 padded to ten bytes", b"\x20\xff\x81" + b"\x80" * 7 + b"\x00" + body),
        ("huge height in ten bytes", b"\x0a\x0b\x08" + b"\xff" * 9 + b"\x01" + body),
        ("empty payload member", b"\x32\x00"),
        ("commit emptied by an empty prepare", body + b"\x32\x00") if p.kind == 7 else ("prepare emptied by an empty commit", body + b"\x3a\x00"),
        ("the type again, to zero", c + b"\x20\x00"),
    ]


def named_out_of_class(p: Parts) -> list[tuple[str, bytes]]:
    """rows that must stay NEEDS_HOST; p is a COMMIT"""
    assert p.kind == 7
    c = p.canonical
    head = c[:c.index(b"\x20\x02\x3a")]  # View, From, Signature
    body = c[len(head) + 2:]
    scr = spell(p, Options(shuffle=random.Random(5), width=2))
    return [
        ("field 9", c + b"\x48\x01"),
        ("field 0", b"\x02\x00" + c),
        ("wire type 0 on field 2", b"\x10\x05" + c),
        ("fixed32 on field 4", head + b"\x25\x02\x00\x00\x00" + body),
        ("a two-byte tag", head + b"\xa0\x00\x02" + body),
        ("a two-byte tag of field 16", c + b"\x80\x01\x01"),
        ("field 5 in front of field 6", head + b"\x20\x01\x2a\x00\x32\x22\x0a\x20" + p.hash),
        ("field 8 behind the payload", c + b"\x42\x00"),
        ("an 11-byte varint", head + b"\x20" + b"\x80" * 10 + b"\x00" + b"\x20\x02" + body),
        ("a tenth varint byte of 2", head + b"\x20" + b"\x80" * 9 + b"\x02" + b"\x20\x02" + body),
        ("every length prefix in six bytes", spell(p, Options(width=6, len_cap=6))),
        ("every length prefix in ten bytes", spell(p, Options(width=10, len_cap=10))),
        ("one length prefix in six bytes", head + b"\x20\x02\x3a" + pv(len(body) - 2, 6) + body[2:]),
        ("a tenth length byte of 2", head + b"\x20\x02\x12" + b"\x80" * 9 + b"\x02"),
        ("a length past the end", c + b"\x12\x15" + p.sender),
        ("a hash length past its body", head + b"\x20\x02\x3a\x03\x0a\x20\x01" + c),
        ("a view length past the end", b"\x0a\x7f" + c),
        ("type 256", head + b"\x20\x80\x02" + body),
        ("type 2 + 2^32", head + b"\x20\x82\x80\x80\x80\x10" + body),
        ("a 33-byte hash arriving by merge", c + b"\x3a\x23\x0a\x21" + p.hash + b"\x00"),
        ("a seal in a prepare body", head + b"\x20\x01\x32\x24\x0a\x20" + p.hash + b"\x12\x00"),
        ("field 3 in the view", b"\x0a\x02\x18\x01" + c),
        ("field 3 in the body", c + b"\x3a\x02\x1a\x00"),
        ("a truncated row", scr[:-3]),
        ("a truncated varint", c + b"\x20\x80"),
        ("a lone tag", c + b"\x12"),
    ]


def pack(rows):
    off = np.zeros(len(rows) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in rows])
    return b"".join(rows), off


_CORPUS = {}


def corpus(count: int = 3000, seed: int = 77):
    """The tests' shared corpus, built once: [(label, bytes, the signed message or None)] — every single scrambler, the named
    rows of both sorts, canonical rows, byte-fuzzed scrambled rows, and `count` random compositions."""
    key = (count, seed)
    if key not in _CORPUS:
        from oracle import workload as W
        import wire_cases as WCASE
        r = W.make_round(16, 7001, height=12, round_=3, byzantine=True)
        parts = signed_parts(r)
        rows = [(name, m, p) for name, m, p in scrambled_each(parts, seed)]
        rows += [(name, m, None) for name, m in named_in_class(parts[0]) + named_in_class(parts[1])]
        rows += [(name, m, None) for name, m in named_out_of_class(parts[0])]
        rows += [("canonical", p.canonical, p) for p in parts]
        rows += [("canonical " + k, m, None) for k, m in zip(("preprepare", "roundchange"), WCASE.canonical_round(r, ("preprepare", "roundchange")))]
        rnd = random_scrambled(parts, count, seed)
        rows += [("random", m, p) for m, p in rnd]
        rows += [("fuzzed", m, None) for m in WCASE.fuzz([m for m, _ in rnd[:200]], count // 4, seed + 1)]
        _CORPUS[key] = (r, rows)
    return _CORPUS[key]
