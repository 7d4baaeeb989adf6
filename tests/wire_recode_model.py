"""A plain model of the recode class (include/ibftgpu.h, at ibft_verify_senders_wire; csrc/wire_recode_dev.h): from the
bytes of one flat IbftMessage to (in_class, canonical bytes with the signature).  No protobuf runtime, none of the device's
code: a generic field walk into per-level lists, the merge rules applied afterwards, the canonical encoder of oracle/wire.py.
Test infrastructure only."""
from __future__ import annotations

from dataclasses import dataclass

from oracle import wire

LEN, VARINT = 2, 0
TOP = {1: LEN, 2: LEN, 3: LEN, 4: VARINT, 6: LEN, 7: LEN}
VIEW = {1: VARINT, 2: VARINT}
PREPARE_BODY = {1: LEN}
COMMIT_BODY = {1: LEN, 2: LEN}


class OutOfClass(Exception):
    pass


def _varint(buf: bytes, pos: int, most: int = 10) -> tuple[int, int]:
    """a value: 1 to 10 bytes, padding allowed, the tenth byte 0 or 1; a length prefix (most = 5): 1 to 5 bytes"""
    v = 0
    for i in range(most):
        if pos >= len(buf):
            raise OutOfClass("truncated varint")
        b = buf[pos]
        pos += 1
        if i == 9 and b > 1:
            raise OutOfClass("tenth byte above 1 / an eleventh byte")
        v |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            return v, pos
    raise OutOfClass("a length prefix of more than five bytes")


def _fields(buf: bytes, schema: dict[int, int]) -> list[tuple[int, int | bytes]]:
    out, pos = [], 0
    while pos < len(buf):
        tag = buf[pos]
        pos += 1
        if tag & 0x80:
            raise OutOfClass("multi-byte tag")
        f, wt = tag >> 3, tag & 7
        if schema.get(f) != wt:
            raise OutOfClass(f"field {f} with wire type {wt}")
        v, pos = _varint(buf, pos, 5 if wt == LEN else 10)
        if wt == LEN:
            if v > len(buf) - pos:
                raise OutOfClass("length leaves the enclosing message")
            v, pos = buf[pos:pos + v], pos + v
        out.append((f, v))
    return out


@dataclass
class Decoded:
    view: wire.View | None = None
    sender: bytes = b""
    signature: bytes = b""
    type: int = 0
    kind: int = 0          # 0, 6 (PrepareMessage), 7 (CommitMessage)
    proposal_hash: bytes = b""
    committed_seal: bytes = b""

    def encode(self, with_signature: bool = True) -> bytes:
        out = b""
        if self.view is not None:
            out += wire._len_field(1, self.view.encode(), emit_empty=True)
        out += wire._len_field(2, self.sender)
        if with_signature:
            out += wire._len_field(3, self.signature)
        out += wire._varint_field(4, self.type)
        if self.kind:
            out += wire._len_field(self.kind, wire.commit_body(self.proposal_hash, self.committed_seal), emit_empty=True)
        return out


def decode(buf: bytes) -> Decoded | None:
    """None: outside the class"""
    d = Decoded()
    try:
        for f, v in _fields(buf, TOP):
            if f == 1:
                if d.view is None:
                    d.view = wire.View()
                for g, x in _fields(v, VIEW):  # occurrences merge: per field the last wins
                    if g == 1:
                        d.view.height = x
                    else:
                        d.view.round = x
            elif f == 2:
                d.sender = v
            elif f == 3:
                d.signature = v
            elif f == 4:
                d.type = v
            else:
                body = _fields(v, COMMIT_BODY if f == 7 else PREPARE_BODY)
                if d.kind != f:  # another member of the oneof: what the earlier one held is gone
                    d.proposal_hash = d.committed_seal = b""
                d.kind = f
                for g, x in body:
                    if g == 1:
                        d.proposal_hash = x
                    else:
                        d.committed_seal = x
    except OutOfClass:
        return None
    if d.type > 255 or len(d.proposal_hash) > 32:
        return None
    return d


def canonical(buf: bytes) -> tuple[bool, bytes]:
    """(in the class, the message re-marshalled with its signature kept); (False, the bytes as they are) otherwise"""
    d = decode(buf)
    return (True, d.encode()) if d is not None else (False, buf)
