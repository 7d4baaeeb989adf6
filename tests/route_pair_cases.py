"""The inputs of the cross-route tests (tests/test_gpu_route_pairs.py, tests/test_gpu_route_sequence_large.py), built on the CPU
so that tests/test_route_pair_inputs.py can check without a GPU that they hold what they claim.

Every verifying entry point of the library runs on one context and shares its device scratch: the work mask and its "dirty
words" record, the tally's bitmap and sums, the columns, the route-local tables that are "zero again when the call returns".
A ROUTE here is one entry point with two batches: a DIRTIER — large, every row valid, as many distinct senders as the key pool
has, so that it leaves as many verdict bits, bitmap bits and sums behind as the route can — and a PROBE — smaller, Byzantine,
weighted, with both verdicts, repeated senders and non-members.  The probe's complete expected output comes from the CPU
oracle (oracle.binding, oracle.semantics) or the route's existing Python model, once per (route, size); never from the library.

One installation serves every route: the key pool and the four sets of tests/wire_sets_cases.py.  The single validator set is
set 0 of the family (pool members 0 … 39, weighted), the height map is MAP_A, the proposer table that of wire_views_cases.
Rows are drawn from a small table of signed variants per pool key (Rows) and tiled, so a batch of thousands of rows costs a few
hundred signatures."""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import cert_cases as CC
import cert_decision_model as DM
import cert_verdict_model as CM
import wire_sets_cases as WS
import wire_view_seals_cases as SC
import wire_views_cases as VC
import wire_views_harness as VH
import wire_view_seals_harness as SH
from oracle import binding as B
from oracle import wire
from oracle import wire_cert as WC
from oracle import wire_parse as WP
from oracle import workload as W
from oracle.semantics import ValidatorManager

LOW128 = 2**128 - 1
HEIGHT, ROUND = WS.HEIGHTS[0], 0
PROPOSER = VC.PROPOSER_POOL[0]                   # pool index of the proposer of (HEIGHT, ROUND) in the installed table
VARIANTS = ("good", "seal_flip", "stolen", "sig_flip", "other_hash")
# (max_rows, dirtier rows, probe rows)
REGIMES = {"small": (300, 300, 133), "medium": (8192, 5000, 700)}
SMALLER_FIRST = (300, 100, 260)                  # the dirtier SMALLER than the probe: the probe reaches words it never covered
BLOCK_ROWS = 50                                  # seals per block of the block routes (the last block is ragged)
VERDICT_FIELDS = ("verdict", "verdict2", "sender", "valid", "seal")   # the per-row verdicts among a route's outputs
Msg = namedtuple("Msg", "sender")


def pool():
    return WS.corpus().pool


def plain_set():
    """(height, addrs, powers) of the single validator set: set 0 of the family"""
    return WS.corpus().sets()[0]


def install(bv):
    """everything any route needs, once: the single set, the family, the height map, the proposer table"""
    c = WS.corpus()
    h, a, p = plain_set()
    bv.set_validators(h, a, np.asarray(p, dtype=np.uint64))
    bv.set_validator_sets(c.sets())
    bv.set_height_sets(*WS.MAP_A)
    t = VC.proposers(c)
    bv.set_proposers(t.height, t.first_round, np.frombuffer(b"".join(t.addrs), np.uint8).reshape(-1, 20))


# ---- the table of row variants ----------------------------------------------------------------------------------------------
def _flip(b: bytes, at: int) -> bytes:
    return b[:at] + bytes([b[at] ^ 0x55]) + b[at + 1:]


class Rows:
    """per (pool key i, variant): a COMMIT and a PREPARE of view (HEIGHT, ROUND) as columns and as wire bytes, and what the CPU
    oracle says about each under the single set.  Row u = i * len(VARIANTS) + variant index."""

    def __init__(self):
        r = pool()
        self.r = r
        self.H = r.proposal_hash
        other = B.keccak256(b"other" + self.H)
        nu = r.n * len(VARIANTS)
        self.hash32 = np.zeros((nu, 32), np.uint8)
        self.seal65 = np.zeros((nu, 65), np.uint8)
        self.signer20 = np.zeros((nu, 20), np.uint8)
        self.sig_c = np.zeros((nu, 65), np.uint8)      # envelope signature of the COMMIT
        self.sig_p = np.zeros((nu, 65), np.uint8)      # … of the PREPARE
        self.pns_c, self.pns_p, self.wire_c, self.wire_p = [], [], [], []
        for i in range(r.n):
            good = r.seal65[i].tobytes()
            for v, kind in enumerate(VARIANTS):
                u = i * len(VARIANTS) + v
                h = other if kind == "other_hash" else self.H
                seal = {"seal_flip": _flip(good, 9 + i), "stolen": r.seal65[(i + 1) % r.n].tobytes()}.get(kind, good)
                self.hash32[u] = np.frombuffer(h, np.uint8)
                self.seal65[u] = np.frombuffer(seal, np.uint8)
                self.signer20[u] = r.addrs[i]
                for typ, body, pns, sig, wr in ((wire.COMMIT, wire.commit_body(h, seal), self.pns_c, self.sig_c, self.wire_c),
                                                (wire.PREPARE, wire.prepare_body(h), self.pns_p, self.sig_p, self.wire_p)):
                    m = wire.IbftMessage(view=wire.View(HEIGHT, ROUND), sender=r.addrs[i].tobytes(), type=typ, payload=body)
                    p = m.payload_no_sig()
                    s = B.sign(r.sks[i], B.keccak256(p))
                    if kind == "sig_flip":
                        s = _flip(s, 5 + i)
                    m.signature = s
                    pns.append(p)
                    sig[u] = np.frombuffer(s, np.uint8)
                    wr.append(m.encode())
        self.hash_len = np.full(nu, 32, np.uint8)
        _, a, p = plain_set()
        self.vs = B.ValSet(a, np.asarray(p, dtype=np.uint64))
        self.vm = ValidatorManager()
        assert self.vm.init({bytes(x): int(y) for x, y in zip(a, p)})
        fam = WS.corpus().sets()
        self.family = [B.ValSet(x, np.asarray(y, dtype=np.uint64)) for _, x, y in fam]
        allH = np.tile(np.frombuffer(self.H, np.uint8), (nu, 1))
        # the oracle's verdict on every row of the table
        self.e_seal = B.verify_seals(self.vs, self.hash32, self.seal65, self.signer20).astype(bool)
        self.e_hash = B.verify_hashes(r.raw, ROUND, self.hash32, self.hash_len).astype(bool)
        self.e_send_c = B.verify_senders(self.vs, *_pack(self.pns_c), self.sig_c, self.signer20).astype(bool)
        self.e_send_p = B.verify_senders(self.vs, *_pack(self.pns_p), self.sig_p, self.signer20).astype(bool)
        # a block's seals sign the BLOCK's hash (here H for every block), under the block's set
        self.e_block = [B.verify_seals(vs, allH, self.seal65, self.signer20).astype(bool) for vs in self.family]
        # bare seals: who signed, member or not
        self.rec_signer = np.zeros((nu, 20), np.uint8)
        self.rec_vidx = np.full(nu, -1, np.int32)
        place = {}
        for x in a:                                    # the index ibft_set_validators gives: the caller's order
            place.setdefault(bytes(x), len(place))
        for u in range(nu):
            got = B.recover_address(self.hash32[u].tobytes(), self.seal65[u].tobytes())
            if got is not None:
                self.rec_signer[u] = np.frombuffer(got, np.uint8)
                self.rec_vidx[u] = place[got] if self.vs.index(got) >= 0 else -1
        self.e_rec = self.rec_vidx >= 0
        # the wire walks of the two single-set wire routes
        self.w_status, self.w_sender, self.w_valid = {}, {}, {}
        for name, msgs in (("c", self.wire_c), ("p", self.wire_p)):
            st, sb, vb = [], [], []
            for m in msgs:
                e = WP.expected(m)
                ok = False
                if not e.pre_flag:
                    got = B.recover_address(e.digest, e.signature)
                    ok = got is not None and got == e.sender and self.vs.index(e.sender) >= 0
                val = False
                if e.status == WP.OK and (e.height, e.round) == (HEIGHT, ROUND) and len(e.sender) == 20 and e.proposal_hash == self.H:
                    if e.type == 1 and e.payload_kind == 6:
                        val = True
                    elif e.type == 2 and e.payload_kind == 7 and len(e.committed_seal) == 65:
                        got = B.recover_address(e.proposal_hash, e.committed_seal)
                        val = got is not None and got == e.sender and self.vs.index(e.sender) >= 0
                st.append(e.status); sb.append(ok); vb.append(val)
            self.w_status[name], self.w_sender[name], self.w_valid[name] = np.array(st), np.array(sb, bool), np.array(vb, bool)


_ROWS = []


def rows() -> Rows:
    if not _ROWS:
        _ROWS.append(Rows())
    return _ROWS[0]


def _pack(chunks):
    off = np.zeros(len(chunks) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(c) for c in chunks])
    return b"".join(chunks), off


DIRTY_SENDERS = [i for i in range(40) if i != PROPOSER]      # every member but the proposer (whose own PREPARE voids)
PROBE_SENDERS = [1, 4, PROPOSER, 7, 41, 12, 20, 4, 33, 45, 39]  # members, one twice, the proposer, two keys outside the set


def pick(kind: str, n: int) -> np.ndarray:
    """the table rows of a batch of n: the dirtier is all good rows of 39 members in turn; the probe cycles good / a bad seal /
    a bad envelope / another hash over eleven senders (4 and 11 are coprime: every sender meets every variant)"""
    k = np.arange(n)
    if kind == "dirty":
        i = np.array(DIRTY_SENDERS)[k % len(DIRTY_SENDERS)]
        v = np.zeros(n, int)
    else:
        i = np.array(PROBE_SENDERS)[k % len(PROBE_SENDERS)]
        v = np.array([0, 1, 3, 4])[k % 4]
        v[(k % 8) == 5] = 2                                    # every other bad seal is a stolen one
    return i * len(VARIANTS) + v


def _tally(t):
    """a tally of either binding as the fields every route compares"""
    return dict(power=t.power, quorum=t.quorum, valid_rows=t.valid_rows, distinct_senders=t.distinct_senders, has_quorum=t.has_quorum,
                proposer_rows=getattr(t, "proposer_rows", 0))


def _quorum_tally(T, senders, bits, vs=None):
    return _tally(B.tally(vs if vs is not None else T.vs, senders, bits.astype(np.uint8)))


def _prepare_tally(T, senders, bits):
    """HasPrepareQuorum with the installed proposer over the rows whose bit is set (oracle.semantics)"""
    prop = T.r.addrs[PROPOSER].tobytes()
    msgs = [Msg(bytes(s)) for s, v in zip(senders, bits) if v]
    distinct = ({prop} | {m.sender for m in msgs}) & set(T.vm.power)
    return dict(power=sum(T.vm.power[a] for a in distinct), quorum=T.vm.quorum, valid_rows=len(msgs), distinct_senders=len(distinct),
                has_quorum=int(T.vm.has_prepare_quorum(Msg(prop), msgs)), proposer_rows=sum(1 for m in msgs if m.sender == prop))


# ---- routes -----------------------------------------------------------------------------------------------------------------
class Route:
    """name; batch(kind, n) → SimpleNamespace(n, …inputs…, want: dict, bits: the main verdict, tally: dict or None);
    run(bv, batch) → dict with the keys of want.  probe / dirtier: whether the route serves as one."""
    probe = dirtier = True
    has_tally = True
    sets_route = False          # a message-set route: gets the order-sensitive variants

    def __init__(self):
        self._cache = {}

    def batch(self, kind, n):
        if (kind, n) not in self._cache:
            self._cache[(kind, n)] = self.make(kind, n)
        return self._cache[(kind, n)]


def _cols(T, p, envelopes=None):
    b = SimpleNamespace(n=len(p), p=p, hash32=T.hash32[p].copy(), hash_len=T.hash_len[p].copy(), seal65=T.seal65[p].copy(),
                        signer20=T.signer20[p].copy())
    if envelopes == "c":
        b.payload, b.off = _pack([T.pns_c[u] for u in p])
        b.sig = T.sig_c[p].copy()
    elif envelopes == "p":
        b.payload, b.off = _pack([T.pns_p[u] for u in p])
        b.sig = T.sig_p[p].copy()
    return b


class Seals(Route):
    name = "is_valid_committed_seal"

    def make(self, kind, n):
        T = rows()
        b = _cols(T, pick(kind, n))
        b.bits = T.e_seal[b.p]
        b.tally = _quorum_tally(T, b.signer20, b.bits)
        b.want = dict(verdict=b.bits, tally=b.tally)
        return b

    def run(self, bv, b):
        m, t = bv.is_valid_committed_seal(b.hash32, b.seal65, b.signer20)
        return dict(verdict=m, tally=_tally(t))


class Senders(Route):
    name = "is_valid_validator"

    def make(self, kind, n):
        T = rows()
        b = _cols(T, pick(kind, n), "c")
        b.bits = T.e_send_c[b.p]
        b.tally = _quorum_tally(T, b.signer20, b.bits)
        b.want = dict(verdict=b.bits, tally=b.tally)
        return b

    def run(self, bv, b):
        m, t = bv.is_valid_validator(b.payload, b.off, b.sig, b.signer20)
        return dict(verdict=m, tally=_tally(t))


class CommitSet(Route):
    name = "verify_messages[commit]"
    sets_route = True

    def make(self, kind, n):
        T = rows()
        b = _cols(T, pick(kind, n), "c")
        b.sender, b.bits = T.e_send_c[b.p], T.e_hash[b.p] & T.e_seal[b.p]
        b.tally = _quorum_tally(T, b.signer20, b.sender & b.bits)
        b.want = dict(sender=b.sender, valid=b.bits, tally=b.tally)
        return b

    def run(self, bv, b):
        T = rows()
        s, v, t = bv.verify_messages(b.payload, b.off, b.sig, b.signer20, b.hash32, b.hash_len, b.seal65, raw=T.r.raw, round_=ROUND)
        return dict(sender=s, valid=v, tally=_tally(t))


class PrepareSet(Route):
    name = "verify_messages[prepare, proposer]"
    sets_route = True

    def make(self, kind, n):
        T = rows()
        b = _cols(T, pick(kind, n), "p")
        b.sender, b.bits = T.e_send_p[b.p], T.e_hash[b.p]
        b.tally = _prepare_tally(T, b.signer20, b.sender & b.bits)
        b.want = dict(sender=b.sender, valid=b.bits, tally=b.tally)
        return b

    def run(self, bv, b):
        T = rows()
        s, v, t = bv.verify_messages(b.payload, b.off, b.sig, b.signer20, b.hash32, b.hash_len, raw=T.r.raw, round_=ROUND,
                                     proposer=T.r.addrs[PROPOSER].tobytes())
        return dict(sender=s, valid=v, tally=_tally(t))


class Hashes(Route):
    name = "is_valid_proposal_hash"
    has_tally = False

    def make(self, kind, n):
        T = rows()
        b = _cols(T, pick(kind, n))
        b.bits, b.tally = T.e_hash[b.p], None
        b.want = dict(verdict=b.bits)
        return b

    def run(self, bv, b):
        T = rows()
        return dict(verdict=bv.is_valid_proposal_hash(T.r.raw, ROUND, b.hash32, b.hash_len))


class Quorum(Route):
    name = "has_quorum"

    def make(self, kind, n):
        T = rows()
        b = _cols(T, pick(kind, n))
        b.bits = T.e_seal[b.p]                                  # the caller's mask: what a seal pass would have said
        b.tally = _quorum_tally(T, b.signer20, b.bits)
        b.want = dict(tally=b.tally)
        return b

    def run(self, bv, b):
        return dict(tally=_tally(bv.has_quorum(b.signer20, b.bits)))


class PrepareQuorum(Route):
    name = "has_prepare_quorum"

    def make(self, kind, n):
        T = rows()
        b = _cols(T, pick(kind, n))
        b.bits = T.e_send_p[b.p] & T.e_hash[b.p]
        b.tally = _prepare_tally(T, b.signer20, b.bits)
        b.want = dict(tally=b.tally)
        return b

    def run(self, bv, b):
        T = rows()
        return dict(tally=_tally(bv.has_prepare_quorum(b.signer20, b.bits, T.r.addrs[PROPOSER].tobytes())))


class Recover(Route):
    name = "recover_seals"

    def make(self, kind, n):
        T = rows()
        b = _cols(T, pick(kind, n))
        b.bits = T.e_rec[b.p]
        signer = T.rec_signer[b.p]
        b.tally = _quorum_tally(T, signer, b.bits)
        b.want = dict(signer=signer, vidx=T.rec_vidx[b.p], verdict=b.bits, tally=b.tally)
        return b

    def run(self, bv, b):
        signer, vidx, m, t = bv.recover_seals(b.hash32, b.seal65)
        return dict(signer=signer, vidx=vidx, verdict=m, tally=_tally(t))


class Blocks(Route):
    name = "verify_block_seals"
    family = False

    def make(self, kind, n):
        T = rows()
        nb = (n + BLOCK_ROWS - 1) // BLOCK_ROWS
        block_set = (np.arange(nb) % 2).astype(np.uint32)
        row_set = np.repeat(block_set, BLOCK_ROWS)[:n] if self.family else np.zeros(n, int)
        p = pick(kind, n)
        if kind == "dirty" and self.family:             # the blocks of set 1: its own members sign them
            p = np.where(row_set == 1, np.array(WS.MEMBERS[1])[np.arange(n) % len(WS.MEMBERS[1])] * len(VARIANTS), p)
        b = _cols(T, p)
        b.seal_off = np.minimum(np.arange(nb + 1) * BLOCK_ROWS, n).astype(np.uint32)
        b.block_hash = np.tile(np.frombuffer(T.H, np.uint8), (nb, 1))
        b.block_set = block_set
        b.bits = np.where(row_set == 1, T.e_block[1][b.p], T.e_block[0][b.p])
        vss = T.family if self.family else [T.vs]
        b.tallies = [_quorum_tally(T, b.signer20[lo:hi], b.bits[lo:hi], vss[int(b.block_set[k]) if self.family else 0])
                     for k, (lo, hi) in enumerate(zip(b.seal_off[:-1], b.seal_off[1:]))]
        b.tally = b.tallies[0]
        b.want = dict(verdict=b.bits, tallies=b.tallies)
        return b

    def run(self, bv, b):
        if self.family:
            m, tl = bv.verify_block_seals_sets(b.block_hash, b.seal_off, b.block_set, b.seal65, b.signer20)
        else:
            m, tl = bv.verify_block_seals(b.block_hash, b.seal_off, b.seal65, b.signer20)
        return dict(verdict=m, tallies=[_tally(t) for t in tl])


class BlocksSets(Blocks):
    name = "verify_block_seals_sets"
    family = True


class SendersWire(Route):
    name = "is_valid_validator_wire"

    def make(self, kind, n):
        T = rows()
        b = _cols(T, pick(kind, n))
        b.wire, b.woff = _pack([T.wire_c[u] for u in b.p])
        b.bits = T.w_sender["c"][b.p]
        b.tally = _quorum_tally(T, b.signer20, b.bits)
        b.want = dict(verdict=b.bits, status=T.w_status["c"][b.p], tally=b.tally)
        return b

    def run(self, bv, b):
        m, rws, t = bv.is_valid_validator_wire(b.wire, b.woff)
        return dict(verdict=m, status=rws["status"].astype(int), tally=_tally(t))


class MessagesWire(Route):
    name = "verify_messages_wire"
    sets_route = True

    def make(self, kind, n):
        T = rows()
        b = _cols(T, pick(kind, n))
        b.wire, b.woff = _pack([T.wire_c[u] for u in b.p])
        b.sender, b.bits = T.w_sender["c"][b.p], T.w_valid["c"][b.p]
        b.tally = _quorum_tally(T, b.signer20, b.sender & b.bits)
        b.want = dict(sender=b.sender, valid=b.bits, status=T.w_status["c"][b.p], tally=b.tally)
        return b

    def run(self, bv, b):
        T = rows()
        s, v, rws, t = bv.verify_messages_wire(b.wire, b.woff, HEIGHT, ROUND, raw=T.r.raw)
        return dict(sender=s, valid=v, status=rws["status"].astype(int), tally=_tally(t))


# ---- the routes under the family of sets: corpora of their own over the same pool ----------------------------------------------
_CORPORA = {}


def sets_corpus(kind: str, n: int) -> SC.Corpus:
    """messages of heights 100 / 101 / 105 row by row, each by a member of its height's set (the probe: few of them, again and
    again, with bad envelopes, bad seals, members of other sets and a second hash in between), rounds 0 … 2"""
    if (kind, n) in _CORPORA:
        return _CORPORA[(kind, n)]
    r = pool()
    msgs, kinds, senders = [], [], []
    for j in range(n):
        s = j % 3
        mem = WS.MEMBERS[s]
        typ = SC.COMMIT if j % 2 == 0 else SC.PREPARE
        if kind == "dirty":
            i, what = mem[(j // 3) % len(mem)], "good"
            if s == 0 and typ == SC.PREPARE and i in VC.PROPOSER_POOL:     # (the proposers' own PREPAREs void their records)
                i = mem[-1]
            m = SC.encode(r.sks[i], WS.HEIGHTS[s], 0, typ, VC.HA)
        else:
            i = mem[(j // 3) % min(len(mem), 4)]
            what = ("good", "sig_flip", "good", "seal_flip", "not_in_set", "second_hash", "good")[j % 7]
            rnd = (j // 21) % 3
            if what == "sig_flip":
                m = SC.bad_envelope_commit(r, what, i, s, WS.HEIGHTS[s], rnd, None, j)
            elif what == "seal_flip":
                m = SC.bad_seal_commit(r, what, i, s, WS.HEIGHTS[s], rnd, None)
            elif what == "not_in_set":
                i = WS.NOT_IN_SET[s]
                m = SC.encode(r.sks[i], WS.HEIGHTS[s], rnd, typ, VC.HA)
            else:
                m = SC.encode(r.sks[i], WS.HEIGHTS[s], rnd, typ, VC.HB if what == "second_hash" else VC.HA)
        msgs.append(m); kinds.append(what); senders.append(i)
    base = WS.corpus()
    c = SC.Corpus(msgs, kinds, senders, base.pool, False, base.powers)
    c.suffix = None
    _CORPORA[(kind, n)] = c
    return c


def _set_tallies(tl):
    return [dict(power=w["power"] & LOW128, quorum=w["quorum"] & LOW128, valid_rows=w["valid_rows"], distinct_senders=w["distinct_senders"],
                 has_quorum=w["has_quorum"], proposer_rows=0) for w in tl]


class WireSets(Route):
    name = "verify_senders_wire_sets"

    def make(self, kind, n):
        c = sets_corpus(kind, n)
        b = SimpleNamespace(n=n, c=c)
        b.wire, b.woff = WS.pack(c.msgs)
        bits, rset, vidx, tallies, parsed = WS.expected(c, n, WS.MAP_A, False)
        b.bits = np.array(bits, bool)
        b.tallies = _set_tallies(tallies)
        b.tally = b.tallies[0]
        b.want = dict(verdict=b.bits, set=np.array(rset), vidx=np.array(vidx), status=np.array([e.status for e in parsed]), tallies=b.tallies)
        return b

    def run(self, bv, b):
        m, rws, rset, vidx, tl = bv.verify_senders_wire_sets(b.wire, b.woff)
        return dict(verdict=m, set=rset, vidx=vidx, status=rws["status"].astype(int), tallies=[_tally(t) for t in tl])


class WireViews(Route):
    name = "verify_senders_wire_views"
    seals = False

    def make(self, kind, n):
        c = sets_corpus(kind, n)
        b = SimpleNamespace(n=n, c=c)
        b.wire, b.woff = WS.pack(c.msgs)
        e = SC.expected(c, WS.MAP_A, False, n)
        b.bits = np.array(e["bits"], bool)
        b.tallies = _set_tallies(e["tallies"])
        b.tally = b.tallies[0]
        recs = e["records"] if self.seals else e["views_records"]
        b.want = dict(verdict=b.bits, set=np.array(e["set"]), vidx=np.array(e["vidx"]), tallies=b.tallies, view=np.array(e["view"]),
                      stored=np.array(e["stored"], bool), n_views=e["n_views"], records=[SH.model_record(w) for w in recs])
        if self.seals:
            b.want["seal"] = np.array(e["seal"], bool)
        return b

    def run(self, bv, b):
        out = (bv.verify_messages_wire_views if self.seals else bv.verify_senders_wire_views)(b.wire, b.woff, b.n)
        got = dict(verdict=out[0], set=out[2], vidx=out[3], tallies=[_tally(t) for t in out[4]], view=out[5], stored=out[6],
                   n_views=out[8], records=[VH.record_dict(r) for r in out[7]])
        if self.seals:
            got["seal"] = out[9]
        return got


class WireViewSeals(WireViews):
    name = "verify_messages_wire_views"
    seals = True


# ---- certificates: ROUND_CHANGE messages with their PreparedCertificates, seven rows each ------------------------------------------
CERT_KEYS = 8                 # the first keys of the pool (members of the single set): one proposer, five preparers
CERT_ROWS = 7


def _cert_messages():
    r = pool()
    sub = SimpleNamespace(n=CERT_KEYS, addrs=r.addrs[:CERT_KEYS], sks=r.sks[:CERT_KEYS], raw=r.raw, proposal_hash=r.proposal_hash)
    # the certificate was prepared in round 1 under the proposer the installed table names for it
    prop = VC.PROPOSER_POOL[1]
    preparers = [j for j in range(CERT_KEYS) if j != prop][:5]
    h = B.proposal_hash(r.raw, 1)
    good = [CC.round_change(sub, i, HEIGHT, 2, wire.Proposal(r.raw, 1), CC.pc_bytes(sub, HEIGHT, 1, prop, preparers, raw=r.raw)).encode()
            for i in range(CERT_KEYS)]
    pm = CC.preprepare(sub, prop, HEIGHT, 1, raw=r.raw)
    forged_pc = wire.prepared_certificate(pm, [CC.prepare(sub, i, HEIGHT, 1, h=h, sk=sub.sks[(i + 1) % CERT_KEYS]) for i in preparers])
    honest_pc = CC.pc_bytes(sub, HEIGHT, 1, prop, preparers, raw=r.raw)
    outsider = W.validator_key(2701 ^ 0x77, 1 << 41)
    bad = [CC.round_change(sub, 2, HEIGHT, 2, wire.Proposal(r.raw, 1), forged_pc).encode(),              # forged PREPAREs inside
           CC.round_change(sub, 3, HEIGHT, 2, wire.Proposal(r.raw, 1), honest_pc, sk=outsider).encode(),  # a forged carrier
           CC.round_change(sub, 4, HEIGHT, 2, wire.Proposal(r.raw, 1), forged_pc, sk=outsider).encode()]  # both
    return good, bad


_CERTS = []
_CERT_BATCHES = {}


class Certificates(Route):
    name = "verify_certificates_wire"
    has_tally = False

    def batch(self, kind, n):                        # (one batch and one tree for the three certificate routes)
        if (kind, n) not in _CERT_BATCHES:
            _CERT_BATCHES[(kind, n)] = self.make(kind, n)
        return _CERT_BATCHES[(kind, n)]

    def make(self, kind, n):
        if not _CERTS:
            _CERTS.append(_cert_messages())
        good, bad = _CERTS[0]
        k = n // CERT_ROWS
        msgs = [good[j % len(good)] for j in range(k)] if kind == "dirty" else \
               [(good[j % 3], bad[0], bad[2], bad[1])[j % 4] for j in range(k)]
        b = SimpleNamespace(n=k * CERT_ROWS, msgs=msgs)
        b.wire, b.woff = CC.pack(msgs)
        b.tree = WC.expected_tree(msgs, plain_set()[1])
        assert b.tree.n_rows == b.n
        b.bits = np.array(b.tree.sender_ok, bool)
        b.tally = None
        _, a, p = plain_set()
        b.cv = CM.rows_from_tree(b.tree, a, p)           # the oracle's tree in the form the record and decision models read
        b.want = dict(answer=None)
        return b

    def check(self, bv, b):
        CC.compare(self.name, b.tree, *bv.verify_certificates_wire(b.wire, b.woff))

    def run(self, bv, b):
        try:
            self.check(bv, b)
        except AssertionError as e:
            return dict(answer=f"differs from the model: {e}")
        return dict(answer=None)


def _per_row(b, out):
    nodes, rws, cls, sender, hb, sb = out
    CC.compare("per-row outputs", b.tree, len(cls), nodes, rws, cls, sender, hb, sb)


class Judge(Certificates):
    name = "judge_certificates_wire"

    def check(self, bv, b):
        certs, n_rows, out = bv.judge_certificates_wire(b.wire, b.woff, per_row=True)
        assert n_rows == b.tree.n_rows, ("n_rows", n_rows)
        _per_row(b, out)
        CM.check_records(self.name, b.cv, len(b.msgs), certs, CM.proposers_for([bytes(x) for x in plain_set()[1]]))


class Decide(Certificates):
    name = "decide_certificates_wire"

    def check(self, bv, b):
        certs, dec, n_rows, out = bv.decide_certificates_wire(b.wire, b.woff, per_row=True)
        assert n_rows == b.tree.n_rows, ("n_rows", n_rows)
        _per_row(b, out)
        t = VC.proposers(WS.corpus())
        CM.check_records(self.name, b.cv, len(b.msgs), certs, CM.proposers_for([bytes(x) for x in plain_set()[1]], 1))
        DM.check_decisions(self.name, b.cv, len(b.msgs), DM.Table(t.height, t.first_round, list(t.addrs)), b.wire, certs, dec)


# ---- the signer (a dirtier only) and the pipelined seal passes ---------------------------------------------------------------------
class SignSeals(Route):
    name = "sign_seals"
    probe = has_tally = False

    def make(self, kind, n):
        T = rows()
        i = np.array(DIRTY_SENDERS)[np.arange(n) % len(DIRTY_SENDERS)]
        b = SimpleNamespace(n=n, sk=np.frombuffer(b"".join(T.r.sks[j] for j in i), np.uint8).reshape(n, 32),
                            hash32=np.tile(np.frombuffer(T.H, np.uint8), (n, 1)))
        b.bits, b.tally = np.ones(n, bool), None
        b.want = dict(sig=T.r.seal65[i], signer=T.r.addrs[i], ok=b.bits)       # (the pool's seals are the oracle's signatures over H)
        return b

    def run(self, bv, b):
        sig, signer, ok = bv.sign_seals(b.sk, b.hash32)
        return dict(sig=sig, signer=signer, ok=ok)


class Submit(Seals):
    """two passes over the staged batch in flight, then both collected"""
    name = "seals_submit x2 / seals_collect x2"

    def make(self, kind, n):
        b = Seals.make(self, kind, n)
        b.want = dict(verdict=b.bits, tally=b.tally, verdict2=b.bits, tally2=b.tally)
        return b

    def run(self, bv, b):
        bv.seals_stage(b.hash32, b.seal65, b.signer20)
        bv.seals_submit()
        bv.seals_submit()
        m, t = bv.seals_collect()
        m2, t2 = bv.seals_collect()
        return dict(verdict=m, tally=_tally(t), verdict2=m2, tally2=_tally(t2))


ROUTES = [Seals(), Senders(), CommitSet(), PrepareSet(), Hashes(), Quorum(), PrepareQuorum(), Recover(), Blocks(), BlocksSets(),
          SendersWire(), MessagesWire(), WireSets(), WireViews(), WireViewSeals(), Certificates(), Judge(), Decide(), SignSeals(),
          Submit()]


def route(name: str) -> Route:
    return next(r for r in ROUTES if r.name == name)


def first_difference(want: dict, got: dict):
    """the first field (and row) at which a route's answer differs from the expectation, or None"""
    for f, w in want.items():
        g = got[f]
        if isinstance(w, np.ndarray):
            g = np.asarray(g)
            if g.shape != w.shape:
                return f"{f}: shape {g.shape}, expected {w.shape}"
            bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1)) if len(w) else []
            if len(bad):
                return f"{f}: row {bad[0]} is {g[bad[0]]!r}, expected {w[bad[0]]!r} ({len(bad)} rows differ)"
        elif isinstance(w, list):
            if len(w) != len(g):
                return f"{f}: {len(g)} entries, expected {len(w)}"
            for k, (a, c) in enumerate(zip(w, g)):
                if a != c:
                    d = first_difference(a, c) if isinstance(a, dict) else f"is {c!r}, expected {a!r}"
                    return f"{f}[{k}]: {d}"
        elif isinstance(w, dict):
            d = first_difference(w, g)
            if d:
                return f"{f}.{d}"
        elif w != g:
            return f"{f}: is {g!r}, expected {w!r}"
    return None


# ---- the directed sequence of tests/test_gpu_route_sequence_large.py ---------------------------------------------------------------
SEQ_MAX_ROWS = 98304          # the largest batch that still goes out as two launches
SEQ_HASH_ROWS = 98304         # step 2: ballot words [0, 1536) all ones, no tally
SEQ_SET_ROWS = 20000          # step 3: 20 032 + 20 000 verdict rows — beyond what any grouped kernel takes: the lane kernel
SEQ_SEAL_ROWS = 70000         # step 4: split at 65 536; the last 4 464 rows go through a kernel that ORs into the mask
SEQ_SPLIT_AT = 65536
SEQ_BASE_ROWS, SEQ_SEED = 300, 8101


class Sequence:
    """the four steps' inputs, tiled from one Byzantine round of 300 validators and a copy of it whose seals are each the NEXT
    validator's (valid signatures by the wrong key), and what the CPU oracle says about every row"""

    def __init__(self):
        import wire_cases as WCASE
        n0 = SEQ_BASE_ROWS
        r = W.make_round(n0, SEQ_SEED, byzantine=True, weighted=True, with_envelopes=True)
        self.r = r
        self.vs = B.ValSet(r.addrs, r.power)
        stolen = np.roll(r.seal65, -1, axis=0)
        # rows 0 … 299: the round; 300 … 599: the same rows under a stolen seal
        self.hash32 = np.concatenate([r.hash32, r.hash32])
        self.hash_len = np.concatenate([r.hash_len, r.hash_len])
        self.seal65 = np.concatenate([r.seal65, stolen])
        self.signer20 = np.concatenate([r.signer20, r.signer20])
        self.pre = np.concatenate([r.pre_flags, r.pre_flags])
        self.e_seal = B.verify_seals(self.vs, self.hash32, self.seal65, self.signer20, self.pre).astype(bool)
        self.e_hash = B.verify_hashes(r.raw, r.round, r.hash32, r.hash_len).astype(bool)
        self.e_sender = B.verify_senders(self.vs, r.payload, r.off, r.msg_sig65, r.signer20).astype(bool)
        self.chunks = [r.payload[int(r.off[i]):int(r.off[i + 1])] for i in range(n0)]
        # the same COMMIT set as wire bytes, and the oracle's walk of each message
        self.msgs = WCASE.canonical_round(r, ("commit",))
        H = r.proposal_hash
        ws, wv = [], []
        for m in self.msgs:
            e = WP.expected(m)
            ok = False
            if not e.pre_flag:
                got = B.recover_address(e.digest, e.signature)
                ok = got is not None and got == e.sender and self.vs.index(e.sender) >= 0
            val = False
            if e.status == WP.OK and (e.height, e.round) == (r.height, r.round) and len(e.sender) == 20 and e.proposal_hash == H \
                    and e.type == 2 and e.payload_kind == 7 and len(e.committed_seal) == 65:
                got = B.recover_address(e.proposal_hash, e.committed_seal)
                val = got is not None and got == e.sender and self.vs.index(e.sender) >= 0
            ws.append(ok); wv.append(val)
        self.w_sender, self.w_valid = np.array(ws, bool), np.array(wv, bool)

    def tally(self, senders, bits):
        return _tally(B.tally(self.vs, senders, bits.astype(np.uint8)))

    def hash_step(self):
        n = SEQ_HASH_ROWS
        return np.tile(np.frombuffer(self.r.proposal_hash, np.uint8), (n, 1)), np.full(n, 32, np.uint8)

    def set_step(self, n=SEQ_SET_ROWS):
        """→ the columns of verify_messages over n tiled rows, the same set as wire bytes, and both expectations"""
        idx = np.arange(n) % SEQ_BASE_ROWS
        b = SimpleNamespace(n=n, idx=idx)
        b.payload, b.off = _pack([self.chunks[i] for i in idx])
        r = self.r
        b.sig, b.signer20, b.hash32, b.hash_len, b.seal65, b.pre = (x[idx] for x in (r.msg_sig65, r.signer20, r.hash32, r.hash_len, r.seal65,
                                                                                      r.pre_flags))
        b.sender, b.valid = self.e_sender[idx], (self.e_hash & self.e_seal[:SEQ_BASE_ROWS])[idx]
        b.tally = self.tally(b.signer20, b.sender & b.valid)
        b.wire, b.woff = _pack([self.msgs[i] for i in idx])
        b.w_sender, b.w_valid = self.w_sender[idx], self.w_valid[idx]
        b.w_tally = self.tally(b.signer20, b.w_sender & b.w_valid)
        return b

    def seal_step(self, n=SEQ_SEAL_ROWS):
        """→ the columns of is_valid_committed_seal over n tiled rows; beyond the split every third row carries a stolen seal"""
        k = np.arange(n)
        p = k % SEQ_BASE_ROWS + SEQ_BASE_ROWS * ((k >= SEQ_SPLIT_AT) & (k % 3 == 0))
        b = SimpleNamespace(n=n, forged=p >= SEQ_BASE_ROWS)
        b.hash32, b.seal65, b.signer20, b.pre = self.hash32[p], self.seal65[p], self.signer20[p], self.pre[p]
        b.bits = self.e_seal[p]
        b.tally = self.tally(b.signer20, b.bits)
        return b


_SEQ = []


def sequence() -> Sequence:
    if not _SEQ:
        _SEQ.append(Sequence())
    return _SEQ[0]
