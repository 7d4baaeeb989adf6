"""The recode walk on the CPU: csrc/wire_recode_dev.h (the device code of wire_recode_kernel, compiled for the host) behind
the canonical walk, against the plain model (wire_recode_model.py) and the canonical walk's oracle (oracle/wire_parse.py) over
the corpus of test_wire_recode_model.py."""
import ctypes as C

import numpy as np
import pytest

import wire_recode_cases as RC
import wire_recode_model as RM
from go_ibft_amd import build as B
from go_ibft_amd.verifier import WIRE_ROW
from oracle import wire_parse as WP

WIDTHS = (80, 32, 65, 20, 65, 1)  # row_info, digest, signature, From, seal, pre-flag


def run(dev, msgs):
    wire, off = RC.pack(msgs)
    buf = np.frombuffer(wire + bytes(16), dtype=np.uint8)
    n = len(msgs)
    canon = [np.full((n, w), 0xA5, dtype=np.uint8) for w in WIDTHS]
    out = [np.full((n, w), 0xA5, dtype=np.uint8) for w in WIDTHS]
    recoded = np.zeros(n, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dev.wrh_run(p(buf), p(off), n, *[p(a) for a in canon], *[p(a) for a in out], p(recoded))
    return canon, out, recoded


@pytest.fixture(scope="module")
def world():
    dev = C.CDLL(B.build_wire_recode_harness())
    rows = RC.corpus()[1]
    msgs = [m for _, m, _ in rows]
    model = [RM.canonical(m) for m in msgs]
    canon, out, recoded = run(dev, msgs)
    ref, _, ref_recoded = run(dev, [c for _, c in model])  # the canonical walk over the model's re-encodings
    assert not ref_recoded.any()
    return rows, msgs, model, canon, out, recoded, ref


def test_recoded_rows_equal_the_canonical_walk_of_the_model_bytes(world):
    """row_info (but for pad[0]), digest, signature, From, seal and pre-flag of a row of the class are what the canonical walk
    writes for the model's canonical bytes; pad[0] says which rows went through the recode walk"""
    rows, msgs, model, canon, out, recoded, ref = world
    n_recoded = 0
    for i, ((label, m, _), (inside, cbytes)) in enumerate(zip(rows, model)):
        if not inside:
            continue
        was_canonical = cbytes == m
        assert bool(recoded[i]) == (not was_canonical), (label, m.hex())
        got_ri, want_ri = out[0][i].copy(), ref[0][i].copy()
        assert got_ri[76] == (0 if was_canonical else 1) and want_ri[76] == 0, (label, m.hex())
        got_ri[76] = 0
        assert got_ri.tobytes() == want_ri.tobytes(), (label, m.hex())
        for k in range(1, 6):
            assert out[k][i].tobytes() == ref[k][i].tobytes(), (label, k, m.hex())
        n_recoded += int(recoded[i])
    assert n_recoded > 2500


def test_recoded_rows_against_the_oracle(world):
    """the same rows against the independent decode-and-re-marshal oracle on the model's bytes"""
    rows, msgs, model, canon, out, recoded, ref = world
    for i, ((label, m, _), (inside, cbytes)) in enumerate(zip(rows, model)):
        if not inside:
            continue
        e = WP.expected(cbytes)
        ri = out[0][i].view(WIRE_ROW)[0]
        assert e.status == WP.OK and int(ri["status"]) == WP.OK, (label, m.hex())
        assert out[1][i].tobytes() == e.digest, (label, m.hex())
        assert (int(ri["height"]), int(ri["round"]), int(ri["type"]), int(ri["payload_kind"]), int(ri["has_view"])) == \
            (e.height, e.round, e.type, e.payload_kind, e.has_view), (label, m.hex())
        assert int(ri["hash_len"]) == len(e.proposal_hash) and ri["proposal_hash"].tobytes() == e.proposal_hash.ljust(32, b"\0")
        assert (int(ri["from_len"]), int(ri["sig_len"]), int(ri["seal_len"])) == \
            (min(len(e.sender), 255), min(len(e.signature), 255), min(len(e.committed_seal), 255)), (label, m.hex())
        assert ri["from"].tobytes() == e.sender[:20].ljust(20, b"\0")
        assert (int(out[5][i][0]) != 0) == e.pre_flag
        assert out[2][i].tobytes() == (e.signature if len(e.signature) == 65 else bytes(65))
        assert out[3][i].tobytes() == (e.sender if len(e.sender) == 20 else bytes(20))
        assert out[4][i].tobytes() == (e.committed_seal if e.payload_kind == 7 and len(e.committed_seal) == 65 else bytes(65))


def test_honest_scrambled_rows_carry_the_signed_digest(world, oracle):
    """a scrambled, honestly signed row: its digest recovers its From"""
    rows, msgs, model, canon, out, recoded, ref = world
    seen = 0
    for i, (label, m, p) in enumerate(rows[:400]):
        if p is None:
            continue
        assert oracle.recover_address(out[1][i].tobytes(), out[2][i].tobytes()) == p.sender == out[3][i].tobytes(), label
        seen += 1
    assert seen > 30


def test_rows_outside_the_class_are_left_alone(world):
    """every output of such a row is what the canonical walk wrote: NEEDS_HOST, pre-flag set, pad[0] = 0"""
    rows, msgs, model, canon, out, recoded, ref = world
    outside = 0
    for i, ((label, m, _), (inside, _)) in enumerate(zip(rows, model)):
        if inside:
            continue
        outside += 1
        assert not recoded[i], (label, m.hex())
        for k in range(6):
            assert out[k][i].tobytes() == canon[k][i].tobytes(), (label, k, m.hex())
        assert out[0][i].view(WIRE_ROW)[0]["status"] == WP.NEEDS_HOST and out[5][i][0] & 1 and out[0][i][76] == 0
    assert outside > 300
