"""Synthetic consensus rounds signed ON THE DEVICE (ibft_sign_seals, ibft_sign_messages_wire, ibft_sign_envelopes_wire, include/ibftgpu.h §f4) — for load generators,
simulators and bench.py.  A process that plays n validators needs n committed seals per height
(Backend.BuildCommitMessage, /root/reference/core/backend.go:12-34); the batch signer produces 65 536 of them in under a
millisecond, so a benchmark rank can build the WHOLE validator table of a sharded round on its own GPU in milliseconds
instead of signing with host code for minutes.

Keys are deterministic in (seed, validator index): sk = SplitMix64 stream of the seed, 32 bytes per validator, top bit
cleared (< 2^255 < n) and forced non-zero.  The Byzantine mix follows SURVEY.md §8d: every fifth row (by a SplitMix64
stream of seed ^ 0xB12) is corrupted, the kind cycling over the twelve kinds below; `expect` is what every verifier
must answer by construction (an honest row is valid, a corrupted one is not), and bench.py / the tests additionally
check the rows against the CPU oracle.

make_message_round is the same one layer up: the PREPARE or COMMIT MESSAGES of a round as wire bytes — View, From, envelope
signature, type, proposal hash and (COMMIT) committed seal, encoded and signed by ibft_sign_messages_wire — in the form
ibft_verify_senders_wire / ibft_verify_messages_wire read, with its own three kinds of spoiled rows (MESSAGE_CORRUPTIONS).

make_round_change_round is two layers up: the ROUND_CHANGE messages of a round change, each with the proposal prepared before and
its PreparedCertificate, and the new proposer's PREPREPARE whose RoundChangeCertificate holds them — the input of
ibft_verify_certificates_wire.  Nested PREPAREs come from ibft_sign_messages_wire, every PREPREPARE / ROUND_CHANGE envelope from
ibft_sign_envelopes_wire; the host only strings length-prefixed fields together."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

CORRUPTIONS = ["random65", "non_validator", "other_hash", "stolen_seal", "r_zero", "s_zero", "r_ge_n", "s_ge_n", "v_two",
               "len64", "wrong_hash_field", "nil_payload"]
MESSAGE_CORRUPTIONS = ["sig_flip", "outsider", "from_swap"]
MESSAGE_KINDS = {"prepare": 1, "commit": 2}
ROW_NIL, ROW_BADLEN, ROW_HASH_BAD = 1, 2, 4
_N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
_M64 = (1 << 64) - 1


def _splitmix(seed: int, count: int) -> np.ndarray:
    """count 64-bit outputs of SplitMix64(seed), vectorised"""
    with np.errstate(over="ignore"):
        k = np.arange(1, count + 1, dtype=np.uint64)
        z = np.uint64(seed & _M64) + k * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def secret_keys(seed: int, n: int, salt: int = 0) -> np.ndarray:
    sk = _splitmix(seed * 0x10001 + salt, 4 * n).view(np.uint8).reshape(n, 32).copy()
    sk[:, 0] &= 0x7F
    sk[:, 31] |= 1
    return sk


@dataclass
class DeviceRound:
    n: int
    raw: bytes
    round: int
    proposal_hash: bytes
    addrs: np.ndarray      # n × 20 (validator table, row i = validator i)
    power: np.ndarray      # n u64
    hash32: np.ndarray     # n × 32
    seal65: np.ndarray     # n × 65
    signer20: np.ndarray   # n × 20
    pre_flags: np.ndarray | None
    expect: np.ndarray     # n bool: the verdict every row must get
    kinds: list


def make_round(bv, n: int, seed: int = 1, *, byzantine: bool = False, weighted: bool = False, raw_len: int = 1024,
               round_: int = 0, nonce: str = "keccak") -> DeviceRound:
    """n validators, one COMMIT seal each over keccak256(raw ‖ BE64(round)) — keys, proposal hash and signatures all
    computed by `bv` (a BatchVerifier: ibft_proposal_hash, ibft_sign_seals).  Leaves bv's staged batch undefined.
    nonce: the signer's nonce rule for every seal of the round, "keccak" (default) or "rfc6979" (BatchVerifier.sign_seals)."""
    raw = _splitmix(seed, (raw_len + 7) // 8).tobytes()[:raw_len]
    H = bv.proposal_hash(raw, round_)
    sk = secret_keys(seed, n)
    hcol = np.tile(np.frombuffer(H, dtype=np.uint8), (n, 1))
    seal, addrs, ok = _sign(bv, sk, hcol, nonce=nonce)
    assert ok.all()
    power = (1 + (_splitmix(seed ^ 0x57A4E, n) % np.uint64(16))).astype(np.uint64) if weighted else np.ones(n, dtype=np.uint64)
    signer = addrs.copy()
    hash32 = hcol.copy()
    pre = np.zeros(n, dtype=np.uint8)
    expect = np.ones(n, dtype=bool)
    kinds = [""] * n
    if byzantine:
        bad = np.flatnonzero(_splitmix(seed ^ 0xB12, n) % np.uint64(5) == 0)
        H2 = bv.proposal_hash(b"other" + raw, round_)
        h2col = np.tile(np.frombuffer(H2, dtype=np.uint8), (len(bad), 1))
        outsider, _, _ = _sign(bv, secret_keys(seed, len(bad), salt=0x5EED), hcol[: len(bad)], nonce=nonce)   # keys of no validator
        other, _, _ = _sign(bv, sk[bad], h2col, nonce=nonce) if len(bad) else (np.zeros((0, 65), np.uint8), None, None)
        rnd = _splitmix(seed ^ 0xABCD, 9 * len(bad)).view(np.uint8).reshape(len(bad), 72)
        for j, i in enumerate(bad):
            kind = CORRUPTIONS[j % len(CORRUPTIONS)]
            kinds[i] = kind
            expect[i] = False
            if kind == "random65":
                seal[i, :64] = rnd[j, :64]
                seal[i, 64] = rnd[j, 64] & 1
                # a random 64-byte string is a valid signature of SOME key with probability ≈ 1/2, never of this validator's
            elif kind == "non_validator":
                seal[i] = outsider[j]
            elif kind == "other_hash":
                seal[i] = other[j]
            elif kind == "stolen_seal":
                seal[i] = seal[(i + 1) % n] if kinds[(i + 1) % n] == "" else outsider[j]
            elif kind == "r_zero":
                seal[i, :32] = 0
            elif kind == "s_zero":
                seal[i, 32:64] = 0
            elif kind == "r_ge_n":
                seal[i, :32] = np.frombuffer(_N_ORDER.to_bytes(32, "big"), dtype=np.uint8)
            elif kind == "s_ge_n":
                seal[i, 32:64] = np.frombuffer((_N_ORDER + 1).to_bytes(32, "big"), dtype=np.uint8)
            elif kind == "v_two":
                seal[i, 64] = 2
            elif kind == "len64":
                seal[i, 64] = 0
                pre[i] |= ROW_BADLEN
            elif kind == "wrong_hash_field":
                hash32[i] = h2col[0]
                pre[i] |= ROW_HASH_BAD
            elif kind == "nil_payload":
                hash32[i] = 0
                seal[i] = 0
                pre[i] |= ROW_NIL
    return DeviceRound(n, raw, round_, H, addrs, power, hash32, seal, signer, pre if byzantine else None, expect, kinds)


def _sign(bv, sk, hcol, chunk: int | None = None, nonce: str = "keccak"):
    """ibft_sign_seals (nonce = "keccak") / ibft_sign_seals_ex in pieces of at most the context's max_rows"""
    chunk = chunk or int(bv.max_rows)
    sigs, signers, oks = [], [], []
    for lo in range(0, len(sk), chunk):
        s, a, ok = bv.sign_seals(sk[lo:lo + chunk], hcol[lo:lo + chunk], nonce=nonce)
        sigs.append(s); signers.append(a); oks.append(ok)
    if not sigs:
        return np.zeros((0, 65), np.uint8), np.zeros((0, 20), np.uint8), np.zeros(0, bool)
    return np.concatenate(sigs), np.concatenate(signers), np.concatenate(oks)


@dataclass
class MessageRound:
    n: int
    kind: str              # "prepare" | "commit"
    height: int
    round: int
    raw: bytes
    proposal_hash: bytes
    wire: bytes            # the n messages back to back
    off: np.ndarray        # n + 1 u32: message i is wire[off[i]:off[i+1]]
    addrs: np.ndarray      # n × 20 (validator table, row i = validator i = the honest sender of message i)
    power: np.ndarray      # n u64
    expect: np.ndarray     # n bool: the sender verdict every row must get
    kinds: list


def _varint_len(v: int) -> int:
    return max(1, (int(v).bit_length() + 6) // 7)


def make_message_round(bv, n: int, seed: int = 1, *, kind: str = "commit", height: int = 1, round_: int = 0,
                       byzantine: bool = False, nonce: str = "keccak", raw_len: int = 1024) -> MessageRound:
    """n validators, one PREPARE or COMMIT message each for (height, round_) over keccak256(raw ‖ BE64(round_)) — keys, proposal
    hash, seals, envelope signatures and the wire bytes all computed by `bv` (ibft_proposal_hash, ibft_sign_messages_wire).
    With `byzantine`, every fifth row (the selection of make_round) is spoiled on the host after signing, the kind cycling over
    MESSAGE_CORRUPTIONS: a flipped byte inside the envelope signature, an envelope signed by a key of no validator (the whole
    message is that key's: From names it), a From swapped for a neighbour's.  Leaves bv's staged batch undefined."""
    if kind not in MESSAGE_KINDS:
        raise ValueError(f"kind must be one of {sorted(MESSAGE_KINDS)}, not {kind!r}")
    raw = _splitmix(seed, (raw_len + 7) // 8).tobytes()[:raw_len]
    H = bv.proposal_hash(raw, round_)
    sk = secret_keys(seed, n)
    hcol = np.tile(np.frombuffer(H, dtype=np.uint8), (n, 1))
    t = MESSAGE_KINDS[kind]
    wire, off, addrs, ok = _sign_messages(bv, sk, t, height, round_, hcol, nonce=nonce)
    assert ok.all()
    expect = np.ones(n, dtype=bool)
    kinds = [""] * n
    if byzantine:
        bad = np.flatnonzero(_splitmix(seed ^ 0xB12, n) % np.uint64(5) == 0)
        w = bytearray(wire)
        # every row of the round has one length and one layout: 0a len View ‖ 12 14 From ‖ 1a 41 Signature ‖ …
        view = (1 + _varint_len(height) if height else 0) + (1 + _varint_len(round_) if round_ else 0)
        from_at, sig_at = 2 + view + 2, 2 + view + 22 + 2
        outsider, o_off, _, _ = _sign_messages(bv, secret_keys(seed, len(bad), salt=0x5EED), t, height, round_, hcol[:len(bad)], nonce=nonce)
        for j, i in enumerate(bad):
            k = MESSAGE_CORRUPTIONS[j % len(MESSAGE_CORRUPTIONS)]
            kinds[i] = k
            expect[i] = False
            lo = int(off[i])
            if k == "sig_flip":
                w[lo + sig_at + (7 * j) % 64] ^= 0xFF
            elif k == "outsider":
                w[lo:int(off[i + 1])] = outsider[int(o_off[j]):int(o_off[j + 1])]
            elif k == "from_swap":
                w[lo + from_at:lo + from_at + 20] = addrs[(i + 1) % n].tobytes()
                if n == 1:
                    w[lo + from_at] ^= 0xFF
        wire = bytes(w)
    return MessageRound(n, kind, height, round_, raw, H, wire, off, addrs, np.ones(n, dtype=np.uint64), expect, kinds)


def _sign_messages(bv, sk, type_, height, round_, hcol, chunk: int | None = None, nonce: str = "keccak"):
    """ibft_sign_messages_wire in pieces of at most the context's max_rows → (wire bytes, off u32[n+1], from20, ok)"""
    chunk = chunk or int(bv.max_rows)
    wires, offs, froms, oks, base = [], [np.zeros(1, np.uint32)], [], [], 0
    for lo in range(0, len(sk), chunk):
        w, o, f, ok = bv.sign_messages(sk[lo:lo + chunk], type_, height, round_, hcol[lo:lo + chunk], nonce=nonce)
        wires.append(w); offs.append(o[1:] + np.uint32(base)); froms.append(f); oks.append(ok)
        base += len(w)
    if not wires:
        return b"", np.zeros(1, np.uint32), np.zeros((0, 20), np.uint8), np.zeros(0, bool)
    return b"".join(wires), np.concatenate(offs), np.concatenate(froms), np.concatenate(oks)


# ---- round changes: ROUND_CHANGE messages with PreparedCertificates, the PREPREPARE with their RoundChangeCertificate -----------
def _varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _field(num: int, data: bytes) -> bytes:
    """a length-prefixed field, emitted even when empty (a present sub-message)"""
    return _varint((num << 3) | 2) + _varint(len(data)) + data


def _proposal(raw: bytes, round_: int) -> bytes:
    """Proposal{rawProposal, round} (messages.proto): empty bytes and a zero round are omitted"""
    return (_field(1, raw) if raw else b"") + (b"\x10" + _varint(round_) if round_ else b"")


@dataclass
class RoundChangeRound:
    n: int
    q: int                  # ⌊2n/3⌋ + 1: ROUND_CHANGE messages in the batch, and messages in each PreparedCertificate
    height: int
    prepared_round: int
    new_round: int
    raw: bytes
    wire: bytes             # the q ROUND_CHANGE messages back to back
    off: np.ndarray         # q + 1 u32
    senders: np.ndarray     # q: the validator that sent message i
    preprepare: bytes       # the new proposer's PREPREPARE for new_round with the RoundChangeCertificate of those q messages
    addrs: np.ndarray       # n × 20 (validator table, row i = validator i)
    power: np.ndarray       # n u64
    rows: int               # rows of ibft_verify_certificates_wire over (wire, off): q · (q + 1)
    expect: np.ndarray      # rows bool: the sender bit of every row, breadth first (the q messages, then each one's q nested ones)
    preprepare_rows: int    # rows over the PREPREPARE alone: 1 + q + q · q
    preprepare_expect: np.ndarray
    spoiled: np.ndarray     # validators whose nested PREPARE carries a flipped signature byte (byzantine)


def make_round_change_round(bv, n: int, seed: int = 1, *, height: int = 5, prepared_round: int = 1, new_round: int = 2,
                            distinct: bool = False, byzantine: bool = False, nonce: str = "keccak", raw_len: int = 1024) -> RoundChangeRound:
    """n validators change from prepared_round to new_round at `height`: validators 0 … q − 1 (q = ⌊2n/3⌋ + 1) each send a
    ROUND_CHANGE carrying the proposal prepared in prepared_round and its PreparedCertificate — the PREPREPARE of that round's
    proposer (validator prepared_round mod n) and q − 1 PREPAREs —, and validator new_round mod n proposes again with the
    RoundChangeCertificate of those q messages.  Keys, proposal hashes, every signature and every envelope digest are computed by
    `bv` (ibft_proposal_hash, ibft_sign_messages_wire, ibft_sign_envelopes_wire); the host concatenates length-prefixed fields.
    distinct = False: every sender carries the same certificate (the first q − 1 validators other than the proposer), passed to the
    device once; distinct = True: sender i's certificate holds the q − 1 preparers that follow position i in the ring of the
    other n − 1 validators.  byzantine: every fifth PREPARE (the selection stream of make_round over the n − 1 preparers) has a
    byte of its envelope signature flipped before it is nested — the messages around it are signed over it as it is, so only
    those rows fail.  Leaves bv's staged batch undefined."""
    q = (2 * n) // 3 + 1
    raw = _splitmix(seed, (raw_len + 7) // 8).tobytes()[:raw_len]
    h_prepared, h_new = bv.proposal_hash(raw, prepared_round), bv.proposal_hash(raw, new_round)
    sk = secret_keys(seed, n)
    proposer, new_proposer = prepared_round % n, new_round % n
    others = [j for j in range(n) if j != proposer]
    # the n − 1 PREPAREs of prepared_round, signed once; every certificate nests a choice of them
    pw, poff, paddr, pok = _sign_messages(bv, sk[others], MESSAGE_KINDS["prepare"], height, prepared_round,
                                          np.tile(np.frombuffer(h_prepared, dtype=np.uint8), (len(others), 1)), nonce=nonce)
    assert pok.all()
    prepares = [bytearray(pw[int(poff[k]):int(poff[k + 1])]) for k in range(len(others))]
    bad = np.zeros(len(others), dtype=bool)
    if byzantine:
        bad = _splitmix(seed ^ 0xB12, len(others)) % np.uint64(5) == 0
        view = (1 + _varint_len(height) if height else 0) + (1 + _varint_len(prepared_round) if prepared_round else 0)
        for j in np.flatnonzero(bad):
            prepares[j][2 + view + 22 + 2 + (7 * int(j)) % 64] ^= 0xFF
    nested = [_field(2, bytes(m)) for m in prepares]
    # the proposer's PREPREPARE of prepared_round
    body = _field(1, _proposal(raw, prepared_round)) + _field(2, h_prepared)
    pm, _, pm_addr, ok = bv.sign_envelopes(sk[proposer:proposer + 1], 0, height, prepared_round, body, 0, len(body), nonce=nonce)
    assert ok.all()
    head = _field(1, _proposal(raw, prepared_round))
    senders = np.arange(q)
    picks = [[(i + k) % len(others) for k in range(q - 1)] if distinct else list(range(q - 1)) for i in range(q)]
    if distinct:
        bodies = [head + _field(2, _field(1, pm) + b"".join(nested[k] for k in picks[i])) for i in range(q)]
    else:
        bodies = [head + _field(2, _field(1, pm) + b"".join(nested[k] for k in picks[0]))]
    lens = np.array([len(bodies[i if distinct else 0]) for i in range(q)], dtype=np.uint32)
    ats = (np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint32) if distinct else np.zeros(q, dtype=np.uint32))
    wire, off, addrs_q, ok = _sign_envelopes(bv, sk[senders], 3, height, new_round, b"".join(bodies), ats, lens, nonce=nonce)
    assert ok.all()
    # the new proposer's PREPREPARE: Proposal, its hash, the RoundChangeCertificate of the q messages
    rcc = b"".join(_field(1, wire[int(off[i]):int(off[i + 1])]) for i in range(q))
    body = _field(1, _proposal(raw, new_round)) + _field(2, h_new) + _field(3, rcc)
    closing, _, _, ok = bv.sign_envelopes(sk[new_proposer:new_proposer + 1], 0, height, new_round, body, 0, len(body), nonce=nonce)
    assert ok.all()
    # the validator table: addresses come back with the signatures (the proposer's from its PREPREPARE)
    addrs = np.zeros((n, 20), dtype=np.uint8)
    addrs[others] = paddr
    addrs[proposer] = pm_addr[0]
    assert (addrs[senders] == addrs_q).all()
    below = np.ones((q, q), dtype=bool)       # row (i, k): nested message k of sender i — the PREPREPARE, then the PREPAREs
    for i in range(q):
        below[i, 1:] = ~bad[picks[i]]
    expect = np.concatenate([np.ones(q, dtype=bool), below.reshape(-1)])
    return RoundChangeRound(n, q, height, prepared_round, new_round, raw, wire, off, senders, closing, addrs, np.ones(n, dtype=np.uint64),
                            q * (q + 1), expect, 1 + q + q * q, np.concatenate([[True], expect]),
                            np.array(others)[np.flatnonzero(bad)])


def _sign_envelopes(bv, sk, type_, height, round_, body, body_at, body_len, chunk: int | None = None, nonce: str = "keccak"):
    """ibft_sign_envelopes_wire in pieces of at most the context's max_rows (every piece names its ranges of the one body
    buffer) → (wire bytes, off u32[n+1], from20, ok)"""
    chunk = chunk or int(bv.max_rows)
    wires, offs, froms, oks, base = [], [np.zeros(1, np.uint32)], [], [], 0
    for lo in range(0, len(sk), chunk):
        w, o, f, ok = bv.sign_envelopes(sk[lo:lo + chunk], type_, height, round_, body, body_at[lo:lo + chunk], body_len[lo:lo + chunk], nonce=nonce)
        wires.append(w); offs.append(o[1:] + np.uint32(base)); froms.append(f); oks.append(ok)
        base += len(w)
    if not wires:
        return b"", np.zeros(1, np.uint32), np.zeros((0, 20), np.uint8), np.zeros(0, bool)
    return b"".join(wires), np.concatenate(offs), np.concatenate(froms), np.concatenate(oks)
