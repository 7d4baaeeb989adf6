"""The safegcd inversions on inputs SEARCHED for their rare states, on the host builds of the device headers.

tests/modinv_model.py restates both limb forms and names the rare states (events) a run passes through;
tests/golden/make_modinv_edges.py searched the families of tests/modinv_cases.py for inputs that reach them
(tests/golden/modinv_edges.json).  Here: the model equals the build limb for limb after every batch (so an event is
something the build does), the fixture reaches every required event and regenerates byte for byte, and every inversion
form equals pow(x, −1, M) on the corpus, its quadruples and 4 096 random control values per modulus.
"""
import ctypes as C
import importlib.util
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from go_ibft_amd import build as B
import modinv_cases as MC
import modinv_model as MM

THREADS = max(1, min(16, len(os.sched_getaffinity(0))))  # the emulated wavefront keeps its state per thread


@pytest.fixture(scope="module")
def dev():
    lib = C.CDLL(B.build_host_harness())
    lib.dev_divsteps_agree.argtypes = [C.c_int32, C.c_uint32, C.c_uint32]
    return lib


@pytest.fixture(scope="module")
def wh():
    return C.CDLL(B.build_wave_harness())


@pytest.fixture(scope="module")
def fix():
    return MC.load()


def _all_values(fix, name):
    """the corpus, every value of its quadruples, once each"""
    xs = list(MC.corpus_values(fix, name))
    for q in MC.corpus_quads(fix, name):
        xs += q
    return list(dict.fromkeys(xs))


def _want(x, m):
    return pow(x, -1, m) if x else 0


def _chunks(jobs, n):
    size = max(1, -(-len(jobs) // n))
    return [jobs[i:i + size] for i in range(0, len(jobs), size)]


def _wave_batch(wh, which, layout, jobs):
    """jobs: values (layout 0) or four-value lists (layout 1) → jobs × 64 × 32 bytes, the work split over threads"""
    def run(part):
        flat = part if layout == 0 else [v for q in part for v in q]
        out = C.create_string_buffer(2048 * len(part))
        assert wh.wvh_modinv_batch(which, layout, len(part), MC.pack(flat), out) == 0
        return out.raw
    with ThreadPoolExecutor(THREADS) as ex:
        return b"".join(ex.map(run, _chunks(jobs, THREADS)))


# ---- the model is the code's model -------------------------------------------------------------------------------------
def test_model_equals_canonical_build_limb_for_limb(dev, fix):
    """d, e, f, g and ζ after each of modinv<MOD>'s 20 batches, and the result"""
    for name, m in MC.MODULI.items():
        for x in _all_values(fix, name) + MC.control(name, 64):
            out = C.create_string_buffer(32)
            tr = np.zeros((20, 37), dtype=np.int32)
            dev.dev_modinv_trace(MC.WHICH[name], x.to_bytes(32, "big"), out, tr.ctypes.data_as(C.c_void_p))
            c = MM.run_canonical(x, m)
            assert int.from_bytes(out.raw, "big") == c["inv"] == _want(x, m), (name, hex(x))
            for b, (d, e, f, g, zeta) in enumerate(c["trace"]):
                assert tr[b].tolist() == d + e + f + g + [zeta], (name, hex(x), "batch", b)


def test_model_equals_wave_build_limb_for_limb(wh, fix):
    """every lane's d, e, f, g and ζ after each batch the emulated wavefront takes (idle batches of finished rows included),
    the number of batches, and the result: the value alone, in each row beside zeros, and every quadruple"""
    for name, m in MC.MODULI.items():
        jobs = [p for x in MC.corpus_values(fix, name) for p in MC.placements(x)] + MC.corpus_quads(fix, name)
        ctl = MC.control(name, 64)
        jobs += [ctl[i:i + 4] for i in range(0, 64, 4)]

        def one(xs):
            out = C.create_string_buffer(2048)
            tr = np.zeros((20, 5, 64), dtype=np.int32)
            nb = wh.wvh_modinv_trace(MC.WHICH[name], MC.pack(xs), out, tr.ctypes.data_as(C.c_void_p))
            w = MM.run_wave(xs, m)
            assert nb == w["batches"], (name, [hex(v) for v in xs], nb, w["batches"])
            for row, r in enumerate(w["rows"]):
                lanes = slice(16 * row, 16 * row + 16)
                for b, (d, e, f, g, zeta) in enumerate(r["trace"]):
                    for k, limbs in enumerate((d, e, f, g)):
                        assert tr[b, k, lanes].tolist() == limbs + [0] * 7, (name, [hex(v) for v in xs], "batch", b, "row", row, "defg"[k])
                    assert (tr[b, 4, lanes] == zeta).all()
            MC.check_wave_out(out.raw, [xs], m, "trace run")
            assert MM.LIMB_LO <= w["limb"][0] and w["limb"][1] < MM.LIMB_HI
        with ThreadPoolExecutor(THREADS) as ex:
            list(ex.map(one, jobs))


def test_three_divstep_forms_agree_on_every_batch_the_corpus_passes_through(dev, fix):
    """(ζ, f₀, g₀) entering each batch of each corpus value, idle batches included: divsteps_30, _var and _lockstep give the same
    ζ and matrix in the build, and so do the model's three"""
    for name, m in MC.MODULI.items():
        triples = set()
        for x in _all_values(fix, name):
            triples.update(MM.run_canonical(x, m)["triples"])
            triples.update(MM.run_wave([x, 0, 1, x], m)["rows"][0]["triples"])  # (a partner that idles the row to the end)
        assert len(triples) > 20 * 30
        for zeta, f0, g0 in sorted(triples):
            assert dev.dev_divsteps_agree(zeta, f0, g0) == 1, (zeta, f0, g0)
            a = MM.divsteps_30(zeta, f0, g0)
            assert a == MM.divsteps_30_var(zeta, f0, g0) == MM.divsteps_30_lockstep(zeta, f0, g0)[:2], (zeta, f0, g0)


# ---- the corpus reaches what it has to ---------------------------------------------------------------------------------
def test_fixture_covers_every_required_event(fix):
    cov = MC.coverage(fix)
    for name in MC.MODULI:
        d = fix["moduli"][name]
        assert len(d["values"]) <= MC.MAX_VALUES and len(d["quads"]) <= MC.MAX_QUADS
        for form, events in MC.required().items():
            missing = [ev for ev in events if ev not in cov[name][form]]
            assert not missing, (name, form, missing)
        # what the search did not reach is pinned: the list may not grow, and a listed event may not be covered after all
        assert sorted(d["unreached"]) == MC.DIVSTEPS_OPTIONAL and d["unreached"]["ds:batches>=19"] == d["searched"], d["unreached"]
        for ev in d["unreached"]:
            assert ev not in cov[name]["divsteps"] and ev not in cov[name]["rows"], (name, ev, "is covered: take it off the list")
        # the events the fixture records for each input are the model's
        for form in ("divsteps", "canonical", "wave"):
            for hx, evs in d["events"][form].items():
                assert MC.analyse(int(hx, 16), MC.MODULI[name])[form] == evs, (name, form, hx)
        for q in d["quads"]:
            xs = [int(v, 16) for v in q["values"]]
            w = MC.analyse_quad(xs, MC.MODULI[name])
            assert (w["first"], w["last"], w["batches"]) == (q["first"], q["last"], q["batches"])
            assert sorted(w["events"] | {e for e in w["rows"][q["pos"]]["events"] if not e.startswith("ds:")}) == q["events"]


def test_fixture_regenerates_byte_for_byte():
    spec = importlib.util.spec_from_file_location("make_modinv_edges", os.path.join(os.path.dirname(MC.FIXTURE), "make_modinv_edges.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(MC.FIXTURE) as f:
        assert gen.build() == f.read()


# ---- every inversion form equals pow -----------------------------------------------------------------------------------
def test_lane_forms_equal_pow_on_corpus_and_control(dev, fix):
    """modinv<MOD>, modinv_shared<MOD> (the run-time modulus) and the fe / sc wrappers"""
    for name, m in MC.MODULI.items():
        which = MC.WHICH[name]
        wrapper = dev.dev_fe_inv_safegcd if name == "p" else dev.dev_sc_inv_safegcd
        for x in _all_values(fix, name) + MC.control(name):
            want, xb = _want(x, m), x.to_bytes(32, "big")
            out = C.create_string_buffer(32)
            for form in (0, 1):
                dev.dev_modinv(form, which, xb, out)
                assert int.from_bytes(out.raw, "big") == want, (name, "form", form, hex(x))
            wrapper(xb, out)
            assert int.from_bytes(out.raw, "big") == want, (name, "wrapper", hex(x))


def test_wave_form_equals_pow_with_one_value_per_wavefront(wh, fix):
    for name, m in MC.MODULI.items():
        xs = _all_values(fix, name) + MC.control(name)
        MC.check_wave_out(_wave_batch(wh, MC.WHICH[name], 0, xs), [[x] * 4 for x in xs], m, "wvh_modinv")


def test_wave_form_equals_pow_with_four_values_in_lockstep(wh, fix):
    """every quadruple; every corpus value in each row beside three zeros (a ragged batch's padding rows) and four times
    itself; the control four by four"""
    for name, m in MC.MODULI.items():
        ctl = MC.control(name)
        jobs = MC.corpus_quads(fix, name) + [p for x in _all_values(fix, name) for p in MC.placements(x)] + \
            [ctl[i:i + 4] for i in range(0, len(ctl), 4)]
        MC.check_wave_out(_wave_batch(wh, MC.WHICH[name], 1, jobs), jobs, m, "wvh_modinv_rows")
