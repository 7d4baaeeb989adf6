"""The message-set, flat wire and certificate routes pinned from outside, through the ctypes binding: the error codes of
ibft_verify_senders[_wire], ibft_verify_messages[_wire], ibft_verify_certificates_wire and ibft_judge_certificates_wire in
the ORDER their checks run (offsets and bytes before IBFT_E_TOOBIG, IBFT_E_TOOBIG before IBFT_E_NOVALSET), the state the
calls leave around them (ibft_wire_stats, which batch ibft_wire_stage_seals accepts, ibft_cert_stats, the tally of an empty
message set) and the smallest sizes at which the routes take another path (the 64-row padding between the two halves of a
message set; a certificate tree of one and of two levels).  Verdicts, trees, tallies and counts are compared with the CPU
oracle and the Python models the other tests of these routes use."""
import ctypes as C

import numpy as np
import pytest

import cert_cases as CC
import cert_dedup_model as DM
import cert_verdict_cases as K
import cert_verdict_model as VM
import wire_cases as WCASE
from oracle import wire_cert as WC
from oracle import wire_parse as WP
from oracle import workload as W
from oracle.semantics import ValidatorManager

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_NOVALSET, E_TOOBIG = 0, -1, -5, -7
MAX_ROWS = 256
SENTINEL = 777          # what *out_n_rows / *out_n_certs hold before a call
HEIGHT, ROUND = 5, 1
POWERS = [10, 1, 1, 1, 1, 1]   # total 15, quorum 11: validator 0 and any one other


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _z(*shape):
    return np.zeros(shape, dtype=np.uint8)


# ---- the six calls with every column the size n asks for: → (return code, *out_n_rows, *out_n_certs) ----------------
def _senders(V, bv, data, off, n, **_):
    mask = np.zeros(n // 64 + 1, np.uint64)
    return bv._L.ibft_verify_senders(bv._h, _p(data), _p(off), _p(_z(n, 65)), _p(_z(n, 20)), None, n, _p(mask), C.byref(V.Tally())), None, None


def _senders_wire(V, bv, data, off, n, **_):
    mask = np.zeros(n // 64 + 1, np.uint64)
    return bv._L.ibft_verify_senders_wire(bv._h, _p(data), _p(off), n, _p(mask), None, C.byref(V.Tally())), None, None


def _messages(V, bv, data, off, n, **_):
    ms, mv = np.zeros(n // 64 + 1, np.uint64), np.zeros(n // 64 + 1, np.uint64)
    return bv._L.ibft_verify_messages(bv._h, _p(data), _p(off), _p(_z(n, 65)), _p(_z(n, 20)), _p(_z(n, 32)), _p(_z(n)), _p(_z(n, 65)), None,
                                      None, n, None, 0, 0, _p(_z(32)), None, _p(ms), _p(mv), C.byref(V.Tally())), None, None


def _messages_wire(V, bv, data, off, n, **_):
    ms, mv = np.zeros(n // 64 + 1, np.uint64), np.zeros(n // 64 + 1, np.uint64)
    return bv._L.ibft_verify_messages_wire(bv._h, _p(data), _p(off), n, HEIGHT, ROUND, None, 0, 0, _p(_z(32)), _p(ms), _p(mv), None, None,
                                           None, C.byref(V.Tally())), None, None


def _certificates(V, bv, data, off, n, rows_cap=MAX_ROWS, **_):
    words = np.zeros(max(rows_cap, n) // 64 + 1, np.uint64)
    n_rows = C.c_size_t(SENTINEL)
    rc = bv._L.ibft_verify_certificates_wire(bv._h, _p(data), _p(off), n, rows_cap, C.byref(n_rows), None, None, None, _p(words), None, None)
    return rc, int(n_rows.value), None


def _judge(V, bv, data, off, n, rows_cap=MAX_ROWS, certs_cap=MAX_ROWS, **_):
    certs = np.zeros(max(certs_cap, n, 1), dtype=V.CERT_VERDICT)
    n_rows, n_certs = C.c_size_t(SENTINEL), C.c_size_t(SENTINEL)
    rc = bv._L.ibft_judge_certificates_wire(bv._h, _p(data), _p(off), n, rows_cap, certs_cap, C.byref(n_rows), C.byref(n_certs), _p(certs),
                                            None, None, None, None, None, None)
    return rc, int(n_rows.value), int(n_certs.value)


CALLS = {"ibft_verify_senders": _senders, "ibft_verify_senders_wire": _senders_wire, "ibft_verify_messages": _messages,
         "ibft_verify_messages_wire": _messages_wire, "ibft_verify_certificates_wire": _certificates,
         "ibft_judge_certificates_wire": _judge}
CERT_CALLS = ("ibft_verify_certificates_wire", "ibft_judge_certificates_wire")


def _off(n, step=4, decreasing_at=None):
    off = (np.arange(n + 1, dtype=np.uint32) * step).astype(np.uint32)
    if decreasing_at is not None:
        off[decreasing_at] = off[decreasing_at - 1] - 1
    return off


@pytest.fixture(scope="module")
def round6():
    return W.make_round(6, 2601, height=HEIGHT, round_=ROUND)


@pytest.fixture(scope="module")
def contexts(round6):
    """(a context with a validator set, one without): max_rows = 256 both"""
    import go_ibft_amd.verifier as V
    with_set, without = V.BatchVerifier(max_rows=MAX_ROWS), V.BatchVerifier(max_rows=MAX_ROWS)
    with_set.set_validators(HEIGHT, round6.addrs, np.asarray(POWERS, dtype=np.uint64))
    yield V, with_set, without
    with_set.close()
    without.close()


# ---- error codes and their precedence --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CALLS))
def test_error_codes_in_the_order_of_the_checks(contexts, name):
    V, with_set, without = contexts
    call = CALLS[name]
    big = MAX_ROWS + 1
    data = _z(4 * big + 8)

    def check(label, want, bv, d, off, n, **kw):
        rc, n_rows, n_certs = call(V, bv, d, off, n, **kw)
        assert rc == want, (name, label, rc, want)
        if name in CERT_CALLS:
            # a call refused for its arguments writes nothing; one refused under the lock has zeroed the counts
            counts = SENTINEL if want == E_INVAL else 0
            assert n_rows == counts, (name, label, n_rows)
            assert n_certs in (None, counts), (name, label, n_certs)

    # one fault
    check("decreasing offsets", E_INVAL, with_set, data, _off(2, decreasing_at=2), 2)
    check("NULL bytes with off[n] > 0", E_INVAL, with_set, None, _off(1), 1)
    check("n > max_rows", E_TOOBIG, with_set, data, _off(big), big)
    check("no validator set", E_NOVALSET, without, data, _off(1), 1)
    # two faults: the offsets and the bytes are judged first, the size next, the validator set last
    check("decreasing offsets, n > max_rows", E_INVAL, with_set, data, _off(big, decreasing_at=big), big)
    check("NULL bytes, n > max_rows", E_INVAL, with_set, None, _off(big), big)
    check("decreasing offsets, no validator set", E_INVAL, without, data, _off(2, decreasing_at=2), 2)
    check("NULL bytes, no validator set", E_INVAL, without, None, _off(1), 1)
    check("n > max_rows, no validator set", E_TOOBIG, without, data, _off(big), big)
    check("all three", E_INVAL, without, None, _off(big, decreasing_at=7), big)
    if name in CERT_CALLS:
        check("n > rows_cap", E_TOOBIG, with_set, data, _off(2), 2, rows_cap=1)
        check("decreasing offsets, n > rows_cap", E_INVAL, with_set, data, _off(2, decreasing_at=2), 2, rows_cap=1)
        check("n > rows_cap, no validator set", E_TOOBIG, without, data, _off(2), 2, rows_cap=1)
        check("no rows, no validator set", E_NOVALSET, without, data, _off(0), 0)
        check("no rows", OK, with_set, data, _off(0), 0)
    if name == "ibft_judge_certificates_wire":
        check("n > certs_cap", E_TOOBIG, with_set, data, _off(2), 2, certs_cap=1)
        check("decreasing offsets, n > certs_cap", E_INVAL, with_set, data, _off(2, decreasing_at=2), 2, certs_cap=1)
        check("n > rows_cap and n > certs_cap", E_TOOBIG, with_set, data, _off(2), 2, rows_cap=1, certs_cap=1)
        # the records' capacity is looked at behind the validator set
        check("n > certs_cap, no validator set", E_NOVALSET, without, data, _off(2), 2, certs_cap=1)


def test_a_tree_or_its_records_beyond_the_caps(contexts, round6):
    """IBFT_E_TOOBIG found on the way — a level that does not fit rows_cap, more records than certs_cap — zeroes the counts too"""
    V, with_set, _ = contexts
    r = round6
    rc_msg = [m.encode() for m in CC.honest_round_change_set(r, HEIGHT, 2, senders=[0])]            # 1 + 1 + 4 rows
    plain_rcs = [CC.round_change(r, i, HEIGHT, 2) for i in range(3)]
    pp_msg = [CC.preprepare_with_rcc(r, HEIGHT, 2, plain_rcs).encode()]                                # 1 + 3 rows, 4 records
    for name in CERT_CALLS:
        buf, off = CC.pack(rc_msg)
        rc, n_rows, n_certs = CALLS[name](V, with_set, np.frombuffer(buf, np.uint8), off, 1, rows_cap=5)
        assert (rc, n_rows) == (E_TOOBIG, 0) and n_certs in (None, 0), name
        rc, n_rows, n_certs = CALLS[name](V, with_set, np.frombuffer(buf, np.uint8), off, 1, rows_cap=6)
        assert (rc, n_rows) == (OK, 6) and n_certs in (None, 1), name
    buf, off = CC.pack(pp_msg)
    assert _judge(V, with_set, np.frombuffer(buf, np.uint8), off, 1, certs_cap=3) == (E_TOOBIG, 0, 0)
    assert _judge(V, with_set, np.frombuffer(buf, np.uint8), off, 1, certs_cap=4) == (OK, 4, 4)


# ---- the state around the calls --------------------------------------------------------------------------------------
def _wire_expect(oracle, vs, rows_bytes):
    exps = [WP.expected(m) for m in rows_bytes]
    verdict = np.zeros(len(exps), dtype=bool)
    for i, e in enumerate(exps):
        if not e.pre_flag:
            got = oracle.recover_address(e.digest, e.signature)
            verdict[i] = got is not None and got == e.sender and vs.index(e.sender) >= 0
    return exps, verdict


def _stage_rc(bv):
    return bv._L.ibft_wire_stage_seals(bv._h)


def test_wire_stats_and_the_resident_wire_batch(contexts, round6, oracle):
    V, bv, _ = contexts
    r = round6
    flat = WCASE.canonical_round(r, ("commit", "prepare", "preprepare"))
    odd = [m for _, m in WCASE.handmade(r)][:9]
    vs = oracle.ValSet(r.addrs, np.asarray(POWERS, dtype=np.uint64))
    env = W.make_round(6, 2601, height=HEIGHT, round_=ROUND, with_envelopes=True)
    cert = [CC.preprepare(r, 1, HEIGHT, ROUND).encode()]

    def stats_of(rows_bytes):
        exps, _ = _wire_expect(oracle, vs, rows_bytes)
        return len(exps), 0, sum(e.status == WP.NEEDS_HOST for e in exps)   # (rows, recoded: the flag is off, left to the host)

    for batch in (flat, flat + odd, odd):
        want = stats_of(batch)
        # ibft_verify_senders_wire: its rows are counted, and its batch is the one ibft_wire_stage_seals takes
        got, rows, _ = bv.is_valid_validator_wire(*WCASE.pack(batch))
        assert (got == _wire_expect(oracle, vs, batch)[1]).all()
        assert bv.wire_stats() == want
        assert _stage_rc(bv) == OK
        assert bv.wire_stats() == want
        # a refused call and a certificate call without rows change nothing
        assert _senders_wire(V, bv, None, _off(1), 1)[0] == E_INVAL
        assert _certificates(V, bv, _z(8), _off(0), 0)[:2] == (OK, 0)
        assert bv.wire_stats() == want and _stage_rc(bv) == OK
        # the column calls restage the columns and leave the parse results alone
        bv.is_valid_validator(env.payload, env.off, env.msg_sig65, env.signer20)
        assert bv.wire_stats() == want and _stage_rc(bv) == E_INVAL
        bv.is_valid_validator_wire(*WCASE.pack(batch))
        assert _stage_rc(bv) == OK
        bv.verify_messages(env.payload, env.off, env.msg_sig65, env.signer20, env.hash32, env.hash_len, env.seal65, raw=env.raw,
                           round_=env.round)
        assert bv.wire_stats() == want and _stage_rc(bv) == E_INVAL
        # ibft_verify_messages_wire: counted, not resident for ibft_wire_stage_seals
        bv.is_valid_validator_wire(*WCASE.pack(batch))
        bv.verify_messages_wire(*WCASE.pack(batch[:-1]), HEIGHT, ROUND, raw=r.raw)
        assert bv.wire_stats() == stats_of(batch[:-1]) and _stage_rc(bv) == E_INVAL
        # a certificate call with rows takes the parse results' place
        bv.is_valid_validator_wire(*WCASE.pack(batch))
        n_rows = bv.verify_certificates_wire(*CC.pack(cert))[0]
        assert n_rows == 1 and bv.wire_stats() == (0, 0, 0) and _stage_rc(bv) == E_INVAL
    # no rows at all: a resident batch of none
    bv.is_valid_validator_wire(*WCASE.pack([]))
    assert bv.wire_stats() == (0, 0, 0) and _stage_rc(bv) == OK
    bv.verify_messages_wire(*WCASE.pack([]), HEIGHT, ROUND, raw=r.raw)
    assert bv.wire_stats() == (0, 0, 0) and _stage_rc(bv) == E_INVAL


def _cert_batches(r):
    one_level = [CC.preprepare(r, 1, HEIGHT, ROUND).encode()]                                        # no certificate: one row
    two_levels = [m.encode() for m in CC.honest_round_change_set(r, HEIGHT, 2, senders=[0])]         # rows > n, records == n
    records = [CC.preprepare_with_rcc(r, HEIGHT, 2, [CC.round_change(r, i, HEIGHT, 2) for i in range(3)]).encode()]  # records > n
    three_levels = [CC.preprepare_with_rcc(r, HEIGHT, 2).encode()]
    return {"one level": one_level, "two levels": two_levels, "records beyond the roots": records, "three levels": three_levels,
            "all": one_level + two_levels + records + three_levels}


@pytest.mark.parametrize("dedup", [False, True], ids=["dedup off", "dedup on"])
def test_certificate_batches_and_their_stats(round6, dedup):
    import go_ibft_amd.verifier as V
    r = round6
    addrs = [a.tobytes() for a in r.addrs]
    bv = V.BatchVerifier(flags=V.FLAG_CERT_DEDUP if dedup else 0, max_rows=MAX_ROWS)
    try:
        bv.set_validators(HEIGHT, r.addrs, np.asarray(POWERS, dtype=np.uint64))
        assert bv.cert_stats() == (0, 0, 0, 0)
        for label, msgs in _cert_batches(r).items():
            tree = WC.expected_tree(msgs, r.addrs)
            rows, judged, distinct = DM.expected_stats(tree, two_launches=False)      # a cold context under 4 096 rows: one launch
            buf, off = CC.pack(msgs)
            n_rows, nodes, wrows, cls, sender, hb, sb = bv.verify_certificates_wire(buf, off)
            CC.compare(label, tree, n_rows, nodes, wrows, cls, sender, hb, sb)
            assert bv.cert_stats() == (rows, judged, distinct if dedup else judged, 0), label
            assert bv.wire_stats() == (0, 0, 0)
            certs, n2, out = bv.judge_certificates_wire(buf, off, per_row=True)
            assert n2 == n_rows and out[0].tobytes() == nodes.tobytes() and out[1].tobytes() == wrows.tobytes(), label
            assert (out[3] == sender).all() and (out[4] == hb).all() and (out[5] == sb).all() and out[2].tobytes() == cls.tobytes(), label
            pw = dict(zip(addrs, POWERS))
            cv = VM.Rows(n_rows, nodes, wrows, cls, sender, hb, sb, pw, 2 * sum(POWERS) // 3 + 1)
            VM.check_records(label, cv, len(msgs), certs, VM.proposers_for(addrs))
            assert bv.cert_stats() == (rows, judged, distinct if dedup else judged, 0), label
            if label == "one level":
                assert n_rows == 1 and len(certs) == 1
            if label == "two levels":
                assert n_rows == 6 and len(certs) == 1
            if label == "records beyond the roots":
                assert n_rows == 4 and len(certs) == 4
    finally:
        bv.close()


def _prepare_tally(vm, proposer, addr_power):
    """HasPrepareQuorum of no messages: the proposer's seat alone → (has_quorum, power, distinct senders)"""
    member = proposer in addr_power
    return vm.has_prepare_quorum(type("M", (), {"sender": proposer})(), []), addr_power.get(proposer, 0), int(member)


def test_the_empty_message_set(contexts, round6):
    V, bv, _ = contexts
    r = round6
    addr_power = {a.tobytes(): p for a, p in zip(r.addrs, POWERS)}
    vm = ValidatorManager()
    assert vm.init(addr_power)
    z65, z20, z32 = np.zeros((0, 65), np.uint8), np.zeros((0, 20), np.uint8), np.zeros((0, 32), np.uint8)

    def columns(proposer):
        return bv.verify_messages(b"", np.zeros(1, np.uint32), z65, z20, z32, np.zeros(0, np.uint8), z65, raw=r.raw, round_=ROUND,
                                  proposer=proposer)[2]

    def wire(proposer):
        return bv.verify_messages_wire(*WCASE.pack([]), HEIGHT, ROUND, raw=r.raw, proposer=proposer)[3]

    for route in (columns, wire):
        # a tally a call with rows left behind must not show through
        bv.is_valid_committed_seal(r.hash32, r.seal65, r.signer20)
        assert bv.last_tally_wide().power == sum(POWERS)
        t = route(None)
        assert (t.quorum, t.power, t.valid_rows, t.distinct_senders, t.has_quorum, t.proposer_rows) == (vm.quorum, 0, 0, 0, 0, 0)
        assert bv.last_tally_wide().power == 0
        outsider = b"\x07" * 20
        for proposer in (r.addrs[0].tobytes(), r.addrs[3].tobytes(), outsider):   # the heavy seat (10 < 11: no quorum), a light one, no member
            has, power, distinct = _prepare_tally(vm, proposer, addr_power)
            t = route(proposer)
            assert (t.quorum, t.power, t.valid_rows, t.distinct_senders, bool(t.has_quorum), t.proposer_rows) == \
                   (vm.quorum, power, 0, distinct, has, 0), (route.__name__, proposer.hex())
    # a set in which the proposer alone is the quorum
    heavy = [30, 1, 1, 1, 1, 1]
    vm2 = ValidatorManager()
    assert vm2.init({a.tobytes(): p for a, p in zip(r.addrs, heavy)})
    bv.set_validators(HEIGHT, r.addrs, np.asarray(heavy, dtype=np.uint64))
    try:
        for route in (columns, wire):
            t = route(r.addrs[0].tobytes())
            assert vm2.has_prepare_quorum(type("M", (), {"sender": r.addrs[0].tobytes()})(), []) is True
            assert (t.quorum, t.power, t.distinct_senders, t.has_quorum, t.proposer_rows) == (vm2.quorum, 30, 1, 1, 0)
            assert route(None).has_quorum == 0
    finally:
        bv.set_validators(HEIGHT, r.addrs, np.asarray(POWERS, dtype=np.uint64))


# ---- the sizes around the padding between the two halves of a message set ---------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_commit_sets_around_the_half_boundary(oracle, n):
    """COMMIT sets (both halves of the verdict launch in use) through the column call and through the wire call, every third
    envelope and every fifth seal forged; the tally over the rows both verdicts accept"""
    import go_ibft_amd.verifier as V
    r = W.make_round(n, 2700 + n, height=HEIGHT, round_=ROUND, byzantine=True, with_envelopes=True, weighted=True)
    sig = r.msg_sig65.copy()
    sig[::3, 5] ^= 0x20
    r.msg_sig65 = sig
    vs = oracle.ValSet(r.addrs, r.power)
    senders = oracle.verify_senders(vs, r.payload, r.off, r.msg_sig65, r.signer20).astype(bool)
    hashes = oracle.verify_hashes(r.raw, r.round, r.hash32, r.hash_len).astype(bool)
    seals = oracle.verify_seals(vs, r.hash32, r.seal65, r.signer20, r.pre_flags).astype(bool)
    valid = hashes & seals
    et = oracle.tally(vs, r.signer20, (senders & valid).astype(np.uint8))
    proposer = r.addrs[0].tobytes()
    bv = V.BatchVerifier(max_rows=MAX_ROWS)
    try:
        bv.set_validators(r.height, r.addrs, r.power)
        for digest in (None, r.proposal_hash):
            kw = dict(raw=r.raw, round_=r.round) if digest is None else dict(digest32=digest)
            s, v, t = bv.verify_messages(r.payload, r.off, r.msg_sig65, r.signer20, r.hash32, r.hash_len, r.seal65, valid_pre=r.pre_flags, **kw)
            assert (s == senders).all() and (v == valid).all(), n
            assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum, t.proposer_rows) == \
                   (et.power, et.valid_rows, et.distinct_senders, et.has_quorum, 0)
        # the same set as PREPAREs with a proposer: no seal half
        s, v, t = bv.verify_messages(r.payload, r.off, r.msg_sig65, r.signer20, r.hash32, r.hash_len, raw=r.raw, round_=r.round,
                                     proposer=proposer)
        assert (s == senders).all() and (v == hashes).all()
        assert t.proposer_rows == int((senders & hashes)[(r.signer20 == r.addrs[0]).all(axis=1)].sum())
        # from the wire bytes: COMMITs and PREPAREs alternate, the same forgeries in the envelopes
        rows_bytes = WCASE.canonical_round(r, ("commit", "prepare"))
        for i in range(0, n, 3):
            e = WP.expected(rows_bytes[i])
            at = rows_bytes[i].index(e.signature)
            rows_bytes[i] = rows_bytes[i][:at + 5] + bytes([rows_bytes[i][at + 5] ^ 0x20]) + rows_bytes[i][at + 6:]
        exps = [WP.expected(m) for m in rows_bytes]
        want_s = np.zeros(n, dtype=bool)
        want_v = np.zeros(n, dtype=bool)
        H = oracle.proposal_hash(r.raw, ROUND)
        from_col = np.zeros((n, 20), dtype=np.uint8)
        for i, e in enumerate(exps):
            assert e.status == WP.OK
            from_col[i] = np.frombuffer(e.sender, dtype=np.uint8)
            got = oracle.recover_address(e.digest, e.signature)
            want_s[i] = not e.pre_flag and got is not None and got == e.sender and vs.index(e.sender) >= 0
            if (e.height, e.round) != (HEIGHT, ROUND) or e.proposal_hash != H:
                continue
            if e.type == 1:
                want_v[i] = True
            elif len(e.committed_seal) == 65:
                got = oracle.recover_address(e.proposal_hash, e.committed_seal)
                want_v[i] = got is not None and got == e.sender and vs.index(e.sender) >= 0
        wt = oracle.tally(vs, from_col, (want_s & want_v).astype(np.uint8))
        wire, off = WCASE.pack(rows_bytes)
        for digest in (None, H):
            kw = dict(raw=r.raw) if digest is None else dict(digest32=digest)
            s, v, rows, t = bv.verify_messages_wire(wire, off, HEIGHT, ROUND, **kw)
            assert (s == want_s).all() and (v == want_v).all(), n
            assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum) == (wt.power, wt.valid_rows, wt.distinct_senders, wt.has_quorum)
            assert bv.wire_stats() == (n, 0, 0)
        assert n < 3 or ((~want_s).any() and want_s.any())
    finally:
        bv.close()
