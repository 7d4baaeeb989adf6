"""The signature edge grid (tests/sig_edge_cases.py) through the host-compiled device source, against the oracle, exactly:
the lane recover in its three table forms (dev_emit_row, dev_recover_address_lds, dev_recover_address_private) and, for the
rows whose key the oracle recovers, the warm form (dev_verify_known) on all 2 592 rows under both low-s policies; the emulated
one-wavefront, two-wavefront and row-layout forms on a fixed subset that holds both sides of every edge.

An off-by-one in a comparison with n or (n−1)/2, a wrong low limb of the halved order, or a digest that is not reduced mod n
fails here."""
import ctypes as C

import numpy as np
import pytest

import sig_edge_cases as SE
import valset_collision_cases as VC


@pytest.fixture(scope="module")
def dev(oracle):
    import go_ibft_amd.build as B
    lib = C.CDLL(B.build_host_harness())
    lib.dev_gtab_init()
    return lib


@pytest.fixture(scope="module")
def wh(oracle):
    import go_ibft_amd.build as B
    lib = C.CDLL(B.build_wave_harness())
    lib.wvh_init_gtab()
    return lib


def _tag(row, flags):
    return (hex(row.r), hex(row.s), hex(row.z), row.v, flags)


@pytest.mark.parametrize("flags", SE.FLAGS)
def test_lane_recover_forms_on_the_whole_grid(dev, oracle, flags):
    members = list(SE.signers()) + [SE.flipped(a) for a in SE.signers()]
    col = VC.addr_column(members)
    vs = oracle.ValSet(col, np.ones(len(members), np.uint64))
    out = C.create_string_buffer(20)
    vi = C.c_int32()
    f = lambda b: np.frombuffer(b, np.uint8)
    for row, want in zip(SE.grid(), SE.expected(flags)):
        for fn in (dev.dev_recover_address_lds, dev.dev_recover_address_private):
            ok = fn(row.hash, row.sig, flags, out)
            assert bool(ok) == (want is not None) and (want is None or out.raw == want), _tag(row, flags)
        bit = dev.dev_emit_row(row.hash, row.sig, flags, 0, col.ctypes.data_as(C.c_void_p), len(members), out, C.byref(vi))
        wi = members.index(want) if want is not None else -1
        assert (want is None) or vs.index(want) >= 0
        assert (bool(bit), vi.value, out.raw) == (want is not None, wi, want or VC.ZERO), _tag(row, flags)
        # the claimed-signer form: under the signer's name, and under the name of its one-bit neighbour (a member as well)
        name = want if want is not None else members[0]
        for claimed in (name, SE.flipped(name)):
            bit = dev.dev_claim_row(row.hash, row.sig, flags, 0, col.ctypes.data_as(C.c_void_p), len(members), claimed, C.byref(vi))
            assert bit == oracle.verify_seals(vs, f(row.hash), f(row.sig), f(claimed), flags=flags)[0], _tag(row, flags)
            assert vi.value == members.index(claimed)


def test_warm_form_against_the_recovered_keys(dev, oracle):
    """verify_known with the key the oracle recovers without the strict rule: accepted exactly where the oracle, under the
    call's own policy, recovers that key; and refused under the key of another row"""
    pubs = SE.expected_pub(0)
    other = next(p for p in pubs if p is not None)
    done = 0
    for i, row in enumerate(SE.grid()):
        pub = pubs[i]
        if pub is None:
            continue
        for flags in SE.FLAGS:
            want = SE.expected_pub(flags)[i] == pub
            assert bool(dev.dev_verify_known(row.hash, row.sig, pub, flags)) == want, _tag(row, flags)
            done += want
        if pub != other:
            assert not dev.dev_verify_known(row.hash, row.sig, other, 0), _tag(row, 0)
    assert done == 720


def _wave(fn, row, flags):
    addr = np.zeros((64, 20), dtype=np.uint8)
    ok = np.zeros(64, dtype=np.int32)
    fn(row.hash, row.sig, flags, addr.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p))
    assert (ok == ok[0]).all() and (addr == addr[0]).all(), "lanes of the wavefront disagree"
    return addr[0].tobytes() if ok[0] else None


@pytest.mark.parametrize("form", ["wvh_recover", "wvh_recover2"])
def test_wavefront_recover_on_the_edge_subset(wh, oracle, form):
    for i in SE.wave_subset():
        row = SE.grid()[i]
        for flags in SE.FLAGS:
            assert _wave(getattr(wh, form), row, flags) == SE.expected(flags)[i], _tag(row, flags)


@pytest.mark.parametrize("form", ["wvh_recover4", "wvh_recover4_pair"])
def test_row_layout_recover_on_the_edge_subset(wh, oracle, form):
    """four rows of the subset per emulated wavefront, one per DPP row (these forms take no flags: the lenient policy)"""
    idx = list(SE.wave_subset())
    idx += idx[:(-len(idx)) % 4]
    for at in range(0, len(idx), 4):
        rows = [SE.grid()[i] for i in idx[at:at + 4]]
        addr = np.zeros((64, 20), dtype=np.uint8)
        ok = np.zeros(64, dtype=np.int32)
        getattr(wh, form)(b"".join(r.hash for r in rows), b"".join(r.sig for r in rows), addr.ctypes.data_as(C.c_void_p),
                          ok.ctypes.data_as(C.c_void_p))
        for k, i in enumerate(idx[at:at + 4]):
            lanes = slice(16 * k, 16 * k + 16)
            assert (ok[lanes] == ok[16 * k]).all() and (addr[lanes] == addr[16 * k]).all()
            got = addr[16 * k].tobytes() if ok[16 * k] else None
            assert got == SE.expected(0)[i], _tag(rows[k], 0)


def test_wavefront_warm_form_on_the_edge_subset(wh, oracle):
    pubs = SE.expected_pub(0)
    qtabs = {}
    done = [0, 0]
    for i in SE.wave_subset():
        row, pub = SE.grid()[i], pubs[i]
        if pub is None:
            continue
        if pub not in qtabs:
            qtabs[pub] = np.zeros(32 * 256 * 20, dtype=np.uint32)
            wh.wvh_build_qtab(pub, qtabs[pub].ctypes.data_as(C.c_void_p))
        for flags in SE.FLAGS:
            ok = np.zeros(64, dtype=np.int32)
            wh.wvh_verify_known(qtabs[pub].ctypes.data_as(C.c_void_p), row.hash, row.sig, flags, ok.ctypes.data_as(C.c_void_p))
            want = SE.expected_pub(flags)[i] == pub
            assert (ok == ok[0]).all() and bool(ok[0]) == want, _tag(row, flags)
            done[want] += 1
    assert done[0] >= 5 and done[1] >= 20
