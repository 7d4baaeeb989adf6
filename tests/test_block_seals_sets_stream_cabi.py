"""The last corner of the block-call matrix — a set per block, from the proposals and streamed (ibft_verify_block_seals_sets_raw,
ibft_recover_block_seals_sets_raw and the four _sets submits) — without a GPU: the six symbols are exported, declared in the
header with their parameter lists, bound in verifier.py and in the Go shim; IBFT_BATCH_SETS is 4u; the version stays 4; a NULL
context is refused with IBFT_E_INVAL before any device is touched and nothing is written."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = "ctx, raw, raw_off, round, seal_off, block_set, n_blocks, sig65, "
HASHES = "ctx, block_hash32, seal_off, block_set, n_blocks, sig65, "
PARAMS = {
    "ibft_verify_block_seals_sets_raw": RAW + "signer20, pre_flags, out_block_hash32, out_mask, out_tally",
    "ibft_recover_block_seals_sets_raw": RAW + "pre_flags, out_block_hash32, out_signer20, out_vidx, out_mask, out_tally",
    "ibft_block_seals_submit_sets": HASHES + "signer20, pre_flags",
    "ibft_block_seals_submit_sets_raw": RAW + "signer20, pre_flags",
    "ibft_recover_block_seals_submit_sets": HASHES + "pre_flags",
    "ibft_recover_block_seals_submit_sets_raw": RAW + "pre_flags",
}
METHODS = ("verify_block_seals_sets_raw", "recover_block_seals_sets_raw", "block_seals_submit_sets", "block_seals_submit_sets_raw",
           "recover_block_seals_submit_sets", "recover_block_seals_submit_sets_raw")


@pytest.fixture(scope="module")
def V():
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    V.load_library()
    return V


def _header():
    with open(os.path.join(ROOT, "include", "ibftgpu.h")) as f:
        return f.read()


def test_symbols_exported_and_bound(V):
    L = V.load_library()
    for name, params in PARAMS.items():
        assert name in V.EXPORTS and name in V.OPTIONAL_EXPORTS, name
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == len(params.split(", ")), name
    assert V.ABI_VERSION == 4 and L.ibft_version() == 4   # new entry points, no new version
    for m in METHODS:
        assert callable(getattr(V.BatchVerifier, m)), m
    assert V.BatchVerifier.BATCH_SETS == 4


def test_header_declares_them_with_their_parameter_lists():
    h = _header()
    assert re.search(r"^#define IBFT_BATCH_SETS 4u\b", h, re.M)
    for name, params in PARAMS.items():
        m = re.search(r"^int " + name + r"\(([^;]*)\);", h, re.M)
        assert m, name
        names = [re.search(r"(\w+)$", a.strip()).group(1) for a in m.group(1).split(",")]
        assert names == params.split(", "), name
    flat = " ".join(h.split())
    # what stays out of scope, and what the rewritten block says of the forms that now exist
    assert "Out of scope: streamed (submit / collect) forms over a device group" in flat
    assert "ibft_proposal_hashes followed by the hashes-given _sets call" in flat
    assert "under the family that was installed at the submit" in flat


def test_go_shim_binds_them():
    with open(os.path.join(ROOT, "shim", "go", "ibftgpu", "ibftgpu.go")) as f:
        g = f.read()
    for name in PARAMS:
        assert "C." + name + "(" in g, name
    assert "C.IBFT_BATCH_SETS" in g
    # blockSet is pinned behind the last length check: a return in front of the C call that left a live pin behind would make
    # the batch's runtime.Pinner panic when it is collected
    body = g[g.index("func (c *Ctx) submitStreamed("):g.index("func (c *Ctx) BlockSealsSubmitRaw(")]
    assert body.index("b.hold(unsafe.Pointer(bs))") > body.rindex("return fmt.Errorf")
    assert body.count("b.pin.Unpin()") == 1 and body.index("b.pin.Unpin()") > body.index("b.hold(unsafe.Pointer(bs))")


def test_null_context_is_invalid_and_writes_nothing(V):
    L = V.load_library()
    p = V._p
    off = np.array([0, 1], np.uint32)
    bset = np.zeros(1, np.uint32)
    raw = np.zeros(8, np.uint8)
    roff = np.array([0, 8], np.uint32)
    rnd = np.zeros(1, np.uint64)
    bh = np.zeros((1, 32), np.uint8)
    sig = np.zeros((1, 65), np.uint8)
    signer = np.zeros((1, 20), np.uint8)
    mask = np.full(1, 7, np.uint64)
    out_h = np.full((1, 32), 9, np.uint8)
    out_s = np.full((1, 20), 9, np.uint8)
    out_v = np.full(1, 5, np.int32)
    tal = (V.Tally * 1)()
    tal[0].power_lo = 0x1234
    assert L.ibft_verify_block_seals_sets_raw(None, p(raw), p(roff), p(rnd), p(off), p(bset), 1, p(sig), p(signer), None, p(out_h),
                                              p(mask), tal) == -1
    assert L.ibft_recover_block_seals_sets_raw(None, p(raw), p(roff), p(rnd), p(off), p(bset), 1, p(sig), None, p(out_h), p(out_s),
                                               p(out_v), p(mask), tal) == -1
    assert mask[0] == 7 and tal[0].power_lo == 0x1234 and tal[0].quorum_lo == 0
    assert (out_h == 9).all() and (out_s == 9).all() and out_v[0] == 5
    assert L.ibft_block_seals_submit_sets(None, p(bh), p(off), p(bset), 1, p(sig), p(signer), None) == -1
    assert L.ibft_block_seals_submit_sets_raw(None, p(raw), p(roff), p(rnd), p(off), p(bset), 1, p(sig), p(signer), None) == -1
    assert L.ibft_recover_block_seals_submit_sets(None, p(bh), p(off), p(bset), 1, p(sig), None) == -1
    assert L.ibft_recover_block_seals_submit_sets_raw(None, p(raw), p(roff), p(rnd), p(off), p(bset), 1, p(sig), None) == -1


def test_library_without_the_symbols_raises_gpu_unavailable(V):
    bv = V.BatchVerifier.__new__(V.BatchVerifier)   # (no device: a context is never created here)
    bv._L = object()
    bv._h = C.c_void_p()
    sig0 = np.zeros((0, 65), np.uint8)
    signer0 = np.zeros((0, 20), np.uint8)
    bh = np.zeros((1, 32), np.uint8)
    with pytest.raises(V.GpuUnavailable):
        bv.verify_block_seals_sets_raw([b"x"], [0], [0, 0], [0], sig0, signer0)
    with pytest.raises(V.GpuUnavailable):
        bv.recover_block_seals_sets_raw([b"x"], [0], [0, 0], [0], sig0)
    with pytest.raises(V.GpuUnavailable):
        bv.block_seals_submit_sets(bh, [0, 0], [0], sig0, signer0)
    with pytest.raises(V.GpuUnavailable):
        bv.block_seals_submit_sets_raw([b"x"], [0], [0, 0], [0], sig0, signer0)
    with pytest.raises(V.GpuUnavailable):
        bv.recover_block_seals_submit_sets(bh, [0, 0], [0], sig0)
    with pytest.raises(V.GpuUnavailable):
        bv.recover_block_seals_submit_sets_raw([b"x"], [0], [0, 0], [0], sig0)
