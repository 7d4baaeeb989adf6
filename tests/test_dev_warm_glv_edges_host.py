"""The GLV table form's rare additions on the CPU: crafted rows (tests/warm_glv_cases.py) through the exact device source of
the two warm forms that run on one lane and on one wavefront per signature — verify_known<QTAB_GLV> (what G = 1 runs) and
verify_known_wave<QTAB_GLV> (what G = 64 runs, through the 64-coroutine emulator), both via csrc/host_qtab_glv_harness.hip.

Each crafted row makes one addition of R′ = u1·G + u2·Q meet equal or opposite operands (a mixed addition inside a lane, or a
level of the join), or gives the halves of u2 a shape (a vanishing half, every combination of signs, a top digit beyond 127,
a digit of −128), or has R′ = ∞.  Every verdict, of the row and of its twins (v flipped, high s, claimed by another key),
under both low-s policies, must equal recover-and-compare."""
import ctypes as C

import numpy as np
import pytest

import row_scalar_cases as RC
import warm_cases as WC
import warm_glv_cases as GC


@pytest.fixture(scope="module")
def forms(oracle):
    import go_ibft_amd.build as B
    h = C.CDLL(B.build_qtab_glv_harness())
    h.qgh_init_gtab()
    h.qgh_slot_dwords.restype = C.c_uint32
    bits = h.qgh_gtab_bits()
    assert 256 % bits == 0
    qtabs = {}

    def table(pub):
        if pub not in qtabs:
            qtabs[pub] = np.zeros(h.qgh_slot_dwords(), dtype=np.uint32)
            h.qgh_build_qtab(pub, qtabs[pub].ctypes.data_as(C.c_void_p))
        return qtabs[pub].ctypes.data_as(C.c_void_p)

    def lane(hh, sig, pub, fl):
        return bool(h.qgh_verify_lane(table(pub), hh, sig, fl))

    def wave(hh, sig, pub, fl):
        ok = np.zeros(64, dtype=np.int32)
        h.qgh_verify_wave(table(pub), hh, sig, fl, ok.ctypes.data_as(C.c_void_p))
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


def _check_rows(cases, run):
    """each case under both policies, then its twins under both"""
    for i, c in enumerate(cases):
        other = cases[(i + 1) % len(cases)]
        assert other.addr != c.addr
        for fl in (0, 1):
            for form_name, form in run:
                assert form(c.hash, c.sig, c.pub, fl) == c.expect[fl], (form_name, c.name, fl)
        for tname, h, sig, claimed in WC.twins(c, other):
            for fl in (0, 1):
                want = WC.verdict(h, sig, claimed.addr, fl)
                for form_name, form in run:
                    assert form(h, sig, claimed.pub, fl) == want, (form_name, c.name, tname, fl)


@pytest.mark.parametrize("width", [1, 64])
def test_crafted_rows_of_the_host_widths(forms, width):
    """G = 1 and G = 64: every targeted addition, both signs, with twins under both policies, through both forms"""
    bits, lane, wave = forms
    cases = GC.targeted_cases(width, bits)
    assert GC.coverage(cases, width) == GC.required(width, bits)
    assert len(cases) == 2 * len(GC.targets(width, bits)) + 1    # no target was dropped
    assert sum(c.expect[0] for c in cases) >= len(cases) - 3     # the R′ = ∞ rows aside, all valid
    _check_rows(cases, (("lane", lane), ("wave", wave)))


def test_shape_rows(forms):
    bits, lane, wave = forms
    cases = GC.shape_cases(bits)
    assert all(c.expect[0] for c in cases)
    names = {c.name for c in cases}
    for want in ("k2=0", "k2=0/u1=0", "k1=0", "signs++", "signs+-", "signs-+", "signs--", "top>=128/k1", "top>=128/k2",
                 "digit=-128/k1", "digit=-128/k2"):
        assert f"glv/shape/{want}" in names
    # the shapes, recomputed from the rows' own scalars
    by = {c.name.split("glv/shape/")[1]: c for c in cases}
    assert RC.split(by["k2=0"].u2)[1] == 0 and RC.split(by["k1=0"].u2)[0] == 0 and by["k2=0/u1=0"].u1 == 0
    assert by["k2=0/u1=0"].hash == bytes(32)
    assert GC.recode(abs(RC.split(by["top>=128/k1"].u2)[0]))[15] >= 128
    assert -128 in GC.recode(abs(RC.split(by["digit=-128/k2"].u2)[1]))[:15]
    # a top digit of 256 needs a half of at least 2^128 − BIAS, which no scalar below n has
    assert GC.TOP_DIGIT_MAX < 256 and all(max(GC.recode(abs(k))[15] for k in RC.split(c.u2)) <= GC.TOP_DIGIT_MAX for c in cases)
    for width in (16, 32, 64):                         # some lane carries ∞ into the join
        assert any(("join", 0, "inf") in GC.hits(c.u1, c.u2, c.q, bits, width) for c in cases), width
    _check_rows(cases, (("lane", lane), ("wave", wave)))


def test_r_plus_n_row_against_its_known_key(forms):
    """R′ = (r + n, y): refused by both forms under both policies, while the seal that teaches that key is accepted"""
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
    cases = GC.targeted_cases(width, library_bits)
    assert GC.coverage(cases, width) == GC.required(width, library_bits)
    for c in cases:
        for fl in (0, 1):
            assert lane(c.hash, c.sig, c.pub, fl) == c.expect[fl], (c.name, fl)
        assert wave(c.hash, c.sig, c.pub, 0) == c.expect[0], c.name


def test_builder_targets_every_width_and_level(library_bits):
    """the builder's own self-check, for the library's window width: equal and opposite operands in a mixed addition and at
    every butterfly level of every width, no target dropped, and the rows valid exactly where R′ is finite"""
    for width in GC.WIDTHS:
        cases = GC.targeted_cases(width, library_bits)
        assert GC.coverage(cases, width) == GC.required(width, library_bits), width
        lanes, join = WC.split(width)
        assert len(GC.required(width, library_bits)) == 2 + 2 * len(join)
        assert len(cases) == 2 * len(GC.targets(width, library_bits)) + 1
        for c in cases:
            assert c.target is None or c.target in c.hit, c.name
            assert c.expect[0] == ((c.u1 + c.u2 * c.q) % WC.N != 0), c.name
