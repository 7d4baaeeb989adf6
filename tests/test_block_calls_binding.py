"""The sixteen block calls of BatchVerifier and both collects against a stub library, without a GPU: every call reaches the export
it names with as many arguments as include/ibftgpu.h declares, n_blocks where the header puts it, pre_flags=None as a null
pointer; `_staged` is left as each method leaves it (n == 0 and n > 0); a submit's arrays stay referenced until its collect."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECOVER, RAW, SETS = 1, 2, 4   # IBFT_BATCH_*


def _header_params():
    with open(os.path.join(ROOT, "include", "ibftgpu.h")) as f:
        h = f.read()
    out = {}
    for m in re.finditer(r"^int (ibft_\w*block_seals\w*)\(([^;]*)\);", h, re.M):
        out[m.group(1)] = [re.search(r"(\w+)$", a.strip()).group(1) for a in m.group(2).split(",")]
    return out


PARAMS = _header_params()


def _ptr(a):
    return None if a is None else (a.value if isinstance(a, C.c_void_p) else C.cast(a, C.c_void_p).value)


class StubLib:
    """records every call; plays the two slots of the streamed calls as far as the binding reads them (pending → sizes)"""

    def __init__(self):
        self.calls = []
        self.queue = []   # (rows, blocks, kind) of the batches in flight

    def __getattr__(self, name):
        if not name.startswith("ibft_"):
            raise AttributeError(name)

        def call(*args):
            rec = {"name": name, "argc": len(args), "none": [a is None for a in args], "ptrs": [], "n_blocks": None}
            params = PARAMS.get(name, [])
            if "n_blocks" in params and len(args) == len(params):
                nb = args[params.index("n_blocks")]
                assert isinstance(nb, int)
                rec["n_blocks"] = nb
                rec["ptrs"] = [_ptr(a) for a in args[1:] if not isinstance(a, int) and a is not None]
                if "_submit" in name:
                    off = (C.c_uint32 * (nb + 1)).from_address(_ptr(args[params.index("seal_off")]))
                    kind = (RECOVER if name.startswith("ibft_recover") else 0) | (RAW if name.endswith("_raw") else 0) | \
                           (SETS if "_sets" in name else 0)
                    self.queue.append((int(off[nb]), nb, kind))
            if name in ("ibft_block_seals_pending", "ibft_block_seals_pending_ex"):
                oldest = self.queue[0] if self.queue else (0, 0, 0)
                for ref, v in zip(args[1:], (len(self.queue),) + oldest):
                    ref._obj.value = v
            if name in ("ibft_block_seals_collect", "ibft_block_seals_collect_ex"):
                self.queue.pop(0)
            self.calls.append(rec)
            return 0
        return call


@pytest.fixture()
def bv(monkeypatch):
    import go_ibft_amd.verifier as V
    stub = StubLib()
    monkeypatch.setattr(V, "load_library", lambda: stub)
    b = V.BatchVerifier(device=0, max_rows=64)
    b._h = C.c_void_p(1)   # (ibft_ctx_create of the stub wrote nothing; a non-null handle that close() hands back to the stub)
    yield b
    b.close()


def _batch(n_per_block):
    """columns of a batch with the given rows per block: (hashes, raws, rounds, seal_off, block_set, sig65, signer20)"""
    nb = len(n_per_block)
    off = np.concatenate([[0], np.cumsum(n_per_block)]).astype(np.uint32)
    n = int(off[-1])
    return (np.zeros((nb, 32), np.uint8), [b"p%d" % i for i in range(nb)], list(range(nb)), off, np.zeros(nb, np.uint32),
            np.zeros((n, 65), np.uint8), np.zeros((n, 20), np.uint8))


# method → (export, how the call is made from a batch, _staged afterwards for n rows given the value before)
def _sync_cases():
    for sets in (False, True):
        for raw in (False, True):
            for bare in (False, True):
                meth = ("recover" if bare else "verify") + "_block_seals" + ("_sets" if sets else "") + ("_raw" if raw else "")
                yield meth, sets, raw, bare


def _submit_cases():
    for sets in (False, True):
        for raw in (False, True):
            for bare in (False, True):
                meth = ("recover_" if bare else "") + "block_seals_submit" + ("_sets" if sets else "") + ("_raw" if raw else "")
                yield meth, sets, raw, bare


def _args(batch, sets, raw, bare, pre):
    bh, raws, rounds, off, bset, sig, signer = batch
    a = [raws, rounds] if raw else [bh]
    a.append(off)
    if sets:
        a.append(bset)
    a.append(sig)
    if not bare:
        a.append(signer)
    return a, ({} if pre is None else {"pre_flags": pre})


def _check_record(rec, export, nb, pre_given):
    params = PARAMS[export]
    assert rec["name"] == export
    assert rec["argc"] == len(params), export
    assert rec["n_blocks"] == nb, export
    assert rec["none"][params.index("pre_flags")] == (not pre_given), export
    # nothing else is null: every other column and out buffer of these calls is passed
    assert [p for p, none in zip(params, rec["none"]) if none] == ([] if pre_given else ["pre_flags"]), export


@pytest.mark.parametrize("rows", [[0, 0], [2, 0, 3]])
@pytest.mark.parametrize("meth,sets,raw,bare", list(_sync_cases()))
def test_synchronous_calls(bv, meth, sets, raw, bare, rows):
    n, nb = sum(rows), len(rows)
    for pre in (None, np.zeros(n, np.uint8)):
        bv._staged = 77
        a, kw = _args(_batch(rows), sets, raw, bare, pre)
        out = getattr(bv, meth)(*a, **kw)
        _check_record(bv._L.calls[-1], "ibft_" + meth, nb, pre is not None)
        assert bv._staged == (0 if bare or sets else n), meth   # set whatever n is
        assert len(out) == 2 + (2 if bare else 0) + (1 if raw else 0)
        verdict, tallies = (out[2], out[3]) if bare else (out[0], out[1])
        assert verdict.shape == (n,) and len(tallies) == nb
        if bare:
            assert out[0].shape == (n, 20) and out[1].shape == (n,)
        if raw:
            assert out[-1].shape == (nb, 32)
    if raw:   # want_hashes=False: the one other null pointer these calls pass
        a, kw = _args(_batch(rows), sets, raw, bare, None)
        out = getattr(bv, meth)(*a, want_hashes=False)
        rec = bv._L.calls[-1]
        assert out[-1] is None and rec["none"][PARAMS["ibft_" + meth].index("out_block_hash32")]


@pytest.mark.parametrize("rows", [[0, 0], [2, 0, 3]])
@pytest.mark.parametrize("meth,sets,raw,bare", list(_submit_cases()))
def test_streamed_submits_and_collects(bv, meth, sets, raw, bare, rows):
    n, nb = sum(rows), len(rows)
    kind = (RECOVER if bare else 0) | (RAW if raw else 0) | (SETS if sets else 0)
    for pre in (None, np.zeros(n, np.uint8)):
        bv._staged = 77
        a, kw = _args(_batch(rows), sets, raw, bare, pre)
        assert getattr(bv, meth)(*a, **kw) == n
        rec = bv._L.calls[-1]
        _check_record(rec, "ibft_" + meth, nb, pre is not None)
        if meth == "block_seals_submit":
            assert bv._staged == n            # the oldest submit sets it even when n == 0
        else:
            assert bv._staged == (77 if n == 0 else 0 if bare or sets else n), meth
        # every array whose address went to the library is held until the collect
        assert len(bv._block_cols) == 1
        held = {x.ctypes.data for x in bv._block_cols[-1] if x is not None}
        assert set(rec["ptrs"]) <= held, meth
        assert all(isinstance(x, np.ndarray) for x in bv._block_cols[-1] if x is not None)
        staged = bv._staged
        if kind == 0 and pre is None:
            assert bv.block_seals_pending() == (1, n, nb)
            verdict, tallies = bv.block_seals_collect()
            rec = bv._L.calls[-1]
            assert (rec["name"], rec["argc"], rec["none"]) == ("ibft_block_seals_collect", len(PARAMS["ibft_block_seals_collect"]),
                                                               [False] * 3)
        else:
            assert bv.block_seals_pending_ex() == (1, n, nb, kind)
            got = bv.block_seals_collect_ex()
            rec = bv._L.calls[-1]
            assert (rec["name"], rec["argc"]) == ("ibft_block_seals_collect_ex", len(PARAMS["ibft_block_seals_collect_ex"]))
            # out_block_hash32 for a raw batch, out_signer20 / out_vidx for a recover batch, null otherwise
            assert rec["none"] == [False, not raw, not bare, not bare, False, False]
            assert got["kind"] == kind and set(got) == {"kind", "verdict", "tallies"} | ({"block_hash32"} if raw else set()) | \
                   ({"signer20", "vidx"} if bare else set())
            verdict, tallies = got["verdict"], got["tallies"]
            if raw:
                assert got["block_hash32"].shape == (nb, 32)
            if bare:
                assert got["signer20"].shape == (n, 20) and got["vidx"].shape == (n,)
        assert verdict.shape == (n,) and len(tallies) == nb
        assert bv._block_cols == [] and bv._staged == staged   # the collect pops the arrays and leaves _staged alone


def test_two_batches_in_flight_are_popped_oldest_first(bv):
    b1, b2 = _batch([1]), _batch([2, 2])
    bv.block_seals_submit(b1[0], b1[3], b1[5], b1[6])
    bv.recover_block_seals_submit_sets_raw(b2[1], b2[2], b2[3], b2[4], b2[5])
    assert len(bv._block_cols) == 2
    first, second = bv._block_cols
    bv.block_seals_collect()
    assert len(bv._block_cols) == 1 and bv._block_cols[0] is second
    bv.block_seals_collect_ex()
    assert bv._block_cols == []


def test_every_block_call_is_declared_in_the_header():
    for case, pre in ((_sync_cases, "ibft_"), (_submit_cases, "ibft_")):
        for meth, *_ in case():
            assert pre + meth in PARAMS and "n_blocks" in PARAMS[pre + meth], meth
