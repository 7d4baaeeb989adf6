"""GPU: the three call forms of the device signer — ibft_sign_seals[_ex], ibft_sign_messages_wire, ibft_sign_envelopes_wire —
one after the other on ONE context, under both nonce rules.  They share their prologue and epilogue in the library (sign_call)
and their row frame in the kernels (sign_dev.h: lane_row, load_row32, store_addr20, put_sig65), and they share device columns:
the key column, the hash / digest column, the address column, the ok column.  Every call is compared byte for byte with the
oracle's rows, so a column one form left behind for the next, or a frame that reads the wrong row, shows.

n = 65 is the smallest batch with a full wavefront plus a last wavefront of one live lane and 63 idle lanes that run that row
again.  Row 5 (inside the full wavefront) carries key 0 and row 64 (the last wavefront's one row) carries key n: ok is false
exactly there.  The message batch mixes PREPARE and COMMIT inside the full wavefront and its row 64 is a COMMIT, so the last
wavefront — one live lane — takes both passes of sign_message_row.  The staged batch is run with seals_run (ibft_seals_run)."""
import numpy as np
import pytest

import sign_envelope_cases as SE
import sign_message_cases as SM
from oracle import binding as O

pytestmark = pytest.mark.gpu
N_ROWS = 65
REFUSED = {5: 0, 64: SM.N}
BODY_LENGTHS = (0, 1, 15, 16, 17, 4097)
E_INVAL, E_TOOBIG = -1, -7


def _keys():
    sk = np.frombuffer(b"".join(SM.good_keys(N_ROWS, seed=19)), np.uint8).reshape(N_ROWS, 32).copy()
    for row, key in REFUSED.items():
        sk[row] = np.frombuffer(SM.b32(key), np.uint8)
    return sk


@pytest.fixture(scope="module")
def cases():
    """the three batches and the oracle's rows for them under each nonce rule: computed once, never changed"""
    sk = _keys()
    ok = np.array([i not in REFUSED for i in range(N_ROWS)])
    hs = np.frombuffer(SE.pool(32 * N_ROWS, seed=23), np.uint8).reshape(N_ROWS, 32).copy()
    signer = np.array([np.frombuffer(O.address(O.pubkey(sk[i].tobytes())) if ok[i] else bytes(20), np.uint8) for i in range(N_ROWS)])
    msg = (sk,) + SM.batch(N_ROWS)[1:]
    assert {1, 2} <= set(msg[1][:64].tolist()) and msg[1][64] == SM.COMMIT
    # one body range per length, 1 … 4 filler bytes in front of each; row i names the range of length BODY_LENGTHS[i % 6], so
    # every range is shared by ten rows or more
    parts, where, pos = [], [], 0
    for k, blen in enumerate(BODY_LENGTHS):
        parts += [bytes(1 + k % 4), SE.pool(blen, seed=31 + k)]
        where.append(pos + 1 + k % 4)
        pos += 1 + k % 4 + blen
    i = np.arange(N_ROWS)
    views = [SE.VIEWS[k % len(SE.VIEWS)] for k in range(N_ROWS)]
    env = (sk, np.where(i % 2 == 0, SE.PREPREPARE, SE.ROUND_CHANGE).astype(np.uint8), np.array([v[0] for v in views], np.uint64),
           np.array([v[1] for v in views], np.uint64), b"".join(parts), np.array([where[k % 6] for k in i], np.uint32),
           np.array([BODY_LENGTHS[k % 6] for k in i], np.uint32))
    assert env[5][0] == env[5][6] and env[6][0] == env[6][6]      # two rows, one range
    want = {}
    for nonce in SM.NONCES:
        sign = O.sign if nonce == "keccak" else O.sign_rfc6979
        seals = np.array([np.frombuffer(sign(sk[r].tobytes(), hs[r].tobytes()) if ok[r] else bytes(65), np.uint8) for r in range(N_ROWS)])
        want[nonce] = (seals, SM.expected_batch(msg, nonce), SE.expected_batch(env, nonce))
    for a in (sk, hs, signer, ok) + msg[1:] + tuple(c for c in env[1:] if isinstance(c, np.ndarray)):
        a.setflags(write=False)
    return {"sk": sk, "hs": hs, "signer": signer, "ok": ok, "msg": msg, "env": env, "want": want}


@pytest.fixture(scope="module")
def bv(cases):
    import go_ibft_amd.verifier as V
    b = V.BatchVerifier(max_rows=256)
    members = cases["signer"][cases["ok"]]
    b.set_validators(5, members, np.ones(len(members), np.uint64))
    yield b
    b.close()


def _check_seals(cases, nonce, got):
    sig, signer, ok = got
    assert (ok == cases["ok"]).all(), np.flatnonzero(ok != cases["ok"])
    assert (sig == cases["want"][nonce][0]).all(), np.flatnonzero((sig != cases["want"][nonce][0]).any(axis=1))
    assert (signer == cases["signer"]).all(), np.flatnonzero((signer != cases["signer"]).any(axis=1))


def _check_wire(want, got):
    """want: the oracle's rows, (wire, …, from, …, ok) with From at [2] and ok last"""
    wire, off, frm, ok = got
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).tolist()
    assert len(wire) == int(off[-1])
    for i, w in enumerate(want):
        assert wire[off[i]:off[i + 1]] == w[0], f"row {i} differs"
        assert frm[i].tobytes() == w[2], i
        assert bool(ok[i]) == w[-1] == (i not in REFUSED), i


def test_the_call_forms_in_sequence_on_one_context(bv, cases):
    for nonce in SM.NONCES:
        _, want_msg, want_env = cases["want"][nonce]
        _check_seals(cases, nonce, bv.sign_seals(cases["sk"], cases["hs"], nonce=nonce))
        _check_wire(want_msg, bv.sign_messages(*cases["msg"], nonce=nonce))
        _check_wire(want_env, bv.sign_envelopes(*cases["env"], nonce=nonce))
        _check_seals(cases, nonce, bv.sign_seals(cases["sk"], cases["hs"], nonce=nonce))
        verdict, t = bv.seals_run()
        assert (verdict == cases["ok"]).all() and t.valid_rows == N_ROWS - len(REFUSED)


def test_refusals_in_front_of_the_upload_leave_the_next_call_correct(bv, cases):
    import go_ibft_amd.verifier as V
    L, p = bv._L, V._p
    n = N_ROWS
    sk, hs = cases["sk"], cases["hs"]
    sig, frm, ok = np.zeros((n, 65), np.uint8), np.zeros((n, 20), np.uint8), np.zeros(n, np.uint8)
    off = np.zeros(n + 1, np.uint32)
    # an unknown nonce rule
    assert L.ibft_sign_seals_ex(bv._h, p(sk), p(hs), n, 7, p(sig), p(frm), p(ok)) == E_INVAL
    assert b"ibft_sign_seals_ex: unknown nonce rule 7 " in L.ibft_last_error(bv._h)
    _check_seals(cases, "keccak", bv.sign_seals(sk, hs))
    # a type 0 row given to the PREPARE / COMMIT form
    _, typ, height, round_, mhs = cases["msg"]
    bad = typ.copy()
    bad[33] = 0
    wire = np.zeros(n * V.SIGN_MESSAGE_MAX, np.uint8)
    assert L.ibft_sign_messages_wire(bv._h, p(sk), p(bad), p(height), p(round_), p(mhs), n, 1, p(wire), wire.size, p(off), p(frm),
                                     p(ok)) == E_INVAL
    assert b"ibft_sign_messages_wire: row 33 has type 0 " in L.ibft_last_error(bv._h)
    _check_seals(cases, "rfc6979", bv.sign_seals(sk, hs, nonce="rfc6979"))
    # wire_cap one byte short
    _, etyp, eheight, eround, body, at, ln = cases["env"]
    total = sum(len(w[0]) for w in cases["want"]["keccak"][2])
    bb = np.frombuffer(body, np.uint8)
    wire = np.zeros(total, np.uint8)
    assert L.ibft_sign_envelopes_wire(bv._h, p(sk), p(etyp), p(eheight), p(eround), p(bb), bb.size, p(at), p(ln), n, 0, p(wire), total - 1,
                                      p(off), p(frm), p(ok)) == E_TOOBIG
    assert f"the messages take {total} bytes, wire_cap is {total - 1}".encode() in L.ibft_last_error(bv._h)
    assert not wire.any() and not off.any() and not frm.any() and not ok.any()
    _check_seals(cases, "keccak", bv.sign_seals(sk, hs))
    verdict, t = bv.seals_run()
    assert (verdict == cases["ok"]).all() and t.valid_rows == N_ROWS - len(REFUSED)
