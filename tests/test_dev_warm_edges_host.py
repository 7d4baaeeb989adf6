"""The warm path's rare additions on the CPU: crafted rows (tests/warm_cases.py) through the exact device source of the
two warm forms that run on one lane and on one wavefront per signature — verify_known (verify_dev.h, what G = 1 runs) via
the host arithmetic harness, verify_known_wave (wave_fe_dev.h, what G = 64 runs) via the 64-coroutine emulator.

Each crafted row makes one addition of R′ = u1·G + u2·Q meet equal or opposite operands (a mixed addition inside a lane,
or a level of the join), or leaves whole lanes empty, or has R′ = ∞.  Every verdict, of the row and of its twins (v
flipped, high s, claimed by another key), under both low-s policies, must equal recover-and-compare."""
import ctypes as C

import numpy as np
import pytest

import warm_cases as WC


@pytest.fixture(scope="module")
def forms(oracle):
    import go_ibft_amd.build as B
    dev = C.CDLL(B.build_host_harness())
    wh = C.CDLL(B.build_wave_harness())
    wh.wvh_init_gtab()
    bits = dev.dev_gtab_bits()
    assert bits == wh.wvh_gtab_bits() and 256 % bits == 0
    qtabs = {}

    def lane(h, sig, pub, fl):
        return bool(dev.dev_verify_known(h, sig, pub, fl))

    def wave(h, sig, pub, fl):
        if pub not in qtabs:
            qtabs[pub] = np.zeros(WC.QTAB_WINDOWS * 256 * 20, dtype=np.uint32)
            wh.wvh_build_qtab(pub, qtabs[pub].ctypes.data_as(C.c_void_p))
        ok = np.zeros(64, dtype=np.int32)
        wh.wvh_verify_known(qtabs[pub].ctypes.data_as(C.c_void_p), h, sig, fl, ok.ctypes.data_as(C.c_void_p))
        assert (ok == ok[0]).all()                   # every lane of the wavefront reports the same verdict
        return bool(ok[0])

    return bits, lane, wave


@pytest.fixture(scope="module")
def library_bits():
    """the fixed-base window width of the gfx950 build (the G = 2 … 32 cases aim at it)"""
    import go_ibft_amd.build as B
    dt = C.CDLL(B.build_devtest())
    nw, ne, nb = C.c_int(), C.c_int(), C.c_int()
    dt.devtest_gtab_dims(C.byref(nw), C.byref(ne), C.byref(nb))
    assert nw.value * nb.value == 256 and ne.value == 1 << nb.value
    return nb.value


def _check_rows(cases, run, twin_flags=(0,)):
    """each case under both policies, then its twins; `run` is (name, form) pairs"""
    for i, c in enumerate(cases):
        other = cases[(i + 1) % len(cases)]
        assert other.addr != c.addr
        for fl in (0, 1):
            for form_name, form in run:
                assert form(c.hash, c.sig, c.pub, fl) == c.expect[fl], (form_name, c.name, fl)
        for tname, h, sig, claimed in WC.twins(c, other):
            for fl in ((0, 1) if tname == "high-s" else twin_flags):
                want = WC.verdict(h, sig, claimed.addr, fl)
                for form_name, form in run:
                    assert form(h, sig, claimed.pub, fl) == want, (form_name, c.name, tname, fl)


@pytest.mark.parametrize("width", [1, 64])
def test_crafted_rows_of_the_host_widths(forms, width):
    """G = 1 (the lane form) and G = 64 (the wave form): every targeted addition, both signs, with twins, through both
    forms (each form is also handed the other's rows: they are ordinary rows there)"""
    bits, lane, wave = forms
    cases = WC.targeted_cases(width, bits)
    assert WC.coverage(cases, width) == WC.required(width, bits)
    assert sum(c.expect[0] for c in cases) >= len(cases) - 3     # the R′ = ∞ rows aside, all valid
    _check_rows(cases, (("lane", lane), ("wave", wave)))


def test_shape_rows_leave_whole_lanes_empty(forms):
    """u1 = 0, u2 with one window, u2 = n − 1, all-0xFF bytes, u1 with only its top window"""
    bits, lane, wave = forms
    cases = WC.shape_cases(bits)
    assert all(c.expect[0] for c in cases)
    for width in (16, 32, 64):                         # some lane carries ∞ into the join: the self-check of the shapes
        assert any(("join", 0, "inf") in WC.hits(c.u1, c.u2, c.q, bits, width) for c in cases), width
    _check_rows(cases, (("lane", lane), ("wave", wave)))


def test_r_plus_n_row_against_its_known_key(forms):
    """R′ = (r + n, y) with v = parity(y): refused by both forms under both policies (a compare of R′.x with r mod n
    would accept it), while the seal that teaches that key is accepted"""
    bits, lane, wave = forms
    c = WC.r_plus_n_case()
    for form in (lane, wave):
        assert form(*c.teach, c.pub, 1) is True
        for fl in (0, 1):
            assert form(c.hash, c.sig, c.pub, fl) is False
            assert form(c.hash, c.sig[:64] + bytes([c.sig[64] ^ 1]), c.pub, fl) is False


@pytest.mark.parametrize("width", [2, 4, 8, 16, 32])
def test_group_width_rows_through_both_host_forms(forms, library_bits, width):
    """the rows aimed at G = 2 … 32 (built for the library's window width; only the GPU runs those kernels) are ordinary
    rows here: valid ones accepted, the R′ = ∞ ones refused"""
    bits, lane, wave = forms
    cases = WC.targeted_cases(width, library_bits)
    assert WC.coverage(cases, width) == WC.required(width, library_bits)
    for c in cases:
        for fl in (0, 1):
            assert lane(c.hash, c.sig, c.pub, fl) == c.expect[fl], (c.name, fl)
        assert wave(c.hash, c.sig, c.pub, 0) == c.expect[0], c.name


def test_builder_targets_every_width_and_level(library_bits):
    """the builder's own self-check, for the library's window width: equal and opposite operands in a mixed addition
    and at every butterfly level of every width, and the rows valid exactly where R′ is finite"""
    for width in WC.WIDTHS:
        cases = WC.targeted_cases(width, library_bits)
        assert WC.coverage(cases, width) == WC.required(width, library_bits), width
        lanes, join = WC.split(width)
        assert len(WC.required(width, library_bits)) == 2 + 2 * len(join)
        for c in cases:
            assert c.target is None or c.target in c.hit, c.name
            assert c.expect[0] == ((c.u1 + c.u2 * c.q) % WC.N != 0), c.name
