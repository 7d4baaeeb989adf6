"""The key cache's opt-in GLV table form (IBFT_QTAB_FORM=glv: 174 080 B per validator instead of 655 360) on the device.

The form belongs to the device's pool and is read when the first context of a device is created, so everything here runs in
FRESH child processes (tests/key_cache_glv_child.py), one after the other, never two at once, each under a timeout of its
own.  A child that ends by a signal or a timeout fails its test, and the remaining children of the module are skipped: nothing
more is started on a device that may be in trouble.  The CPU tests at the end run the children's input builders."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "key_cache_glv_child.py")
_broken = []                         # the child that died by a signal or ran out of time


def run_child(scenario, *args, env=None, timeout=180):
    if _broken:
        pytest.skip(f"an earlier child ({_broken[0]}) ended by a signal or a timeout")
    e = {k: v for k, v in os.environ.items() if k not in ("IBFT_QTAB_FORM", "IBFT_QTAB_BUDGET_GB", "IBFT_WARM_LANES", "IBFT_COLD_LANES")}
    e.update(env or {})
    try:
        p = subprocess.run([sys.executable, CHILD, ROOT, scenario, *map(str, args)], cwd=ROOT, env=e, capture_output=True, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired as x:
        _broken.append(scenario)
        pytest.fail(f"{scenario}: no end after {timeout} s\n{(x.stdout or b'')[-2000:]}")
    if p.returncode < 0:
        _broken.append(scenario)
    marker = f"KEY_CACHE_GLV_{scenario.upper()}_OK"
    assert p.returncode == 0 and marker in p.stdout, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return [json.loads(l.split(" ", 1)[1]) for l in p.stdout.splitlines() if l.startswith("GLV_REPORT ")]


@pytest.mark.gpu
def test_every_width_on_crafted_rows():
    """G = 1 … 64 on a glv pool: ≤ 256 validators taught by one seal each, then the crafted batch of the width (crafted row,
    honest row, twins, an odd size, a crafted row last) under flags 0 and STRICT_LOW_S: verdicts and every tally field equal
    the oracle's, last_dispatch() == (0, G), cache_form() == (1, 174080)"""
    run_child("widths", env={"IBFT_QTAB_FORM": "glv"}, timeout=300)


@pytest.mark.gpu
def test_memory_and_budget():
    """IBFT_QTAB_BUDGET_GB=1 and 1 700 validators: a glv pool (6 168 slots) gives every one a table and decides a later pass by
    the warm kernel alone; a wide pool (1 638 slots) is today's behaviour — the rest recover cold, same verdicts.  The glv
    pool's bytes stay within slots × (174 080 + 84) plus what the wide child holds outside its tables."""
    wide = run_child("budget", env={"IBFT_QTAB_FORM": "wide", "IBFT_QTAB_BUDGET_GB": "1"})[0]
    glv = run_child("budget", env={"IBFT_QTAB_FORM": "glv", "IBFT_QTAB_BUDGET_GB": "1"})[0]
    assert (wide["form"], wide["slot_bytes"], wide["tables"], wide["used"]) == (0, 655360, 1638, 1638)
    assert (glv["form"], glv["slot_bytes"], glv["tables"], glv["used"]) == (1, 174080, 1700, 1700)
    outside = wide["device_bytes"] - wide["cap"] * 655360          # the G table, keys, states: from the wide child's own report
    assert 0 < outside < 100 << 20, outside
    assert glv["device_bytes"] <= glv["cap"] * (174080 + 84) + outside, (glv, outside)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["growth", "recycle", "rotation"])
def test_pool_lifecycle_under_glv(which):
    """the growth / recycle / rotation sequences of tests/key_cache_child.py on a glv pool, the model sized by its slot bytes"""
    run_child("lifecycle", which, env={"IBFT_QTAB_FORM": "glv"})


@pytest.mark.gpu
def test_other_entry_points_on_a_glv_pool():
    """ibft_verify_messages (n = 65), ibft_verify_block_seals_sets (3 sets, 5 blocks), ibft_judge_certificates_wire (second
    call of a key-cache context), ibft_seals_submit / _collect (two passes in flight): bit for bit a cold context's output"""
    run_child("entries", env={"IBFT_QTAB_FORM": "glv"})


@pytest.mark.gpu
@pytest.mark.parametrize("value", ["bogus", "wide", None])
def test_selecting_the_form(value):
    """bogus → ibft_ctx_create fails with IBFT_E_INVAL and names the variable; unset (and wide) → (0, 655360)"""
    run_child("select", value or "wide", env={} if value is None else {"IBFT_QTAB_FORM": value}, timeout=60)


def test_budget_inputs_and_crafted_sets():
    """no GPU: what the children check before they open a context — the oracle turns down exactly the spoiled rows of the
    1 700, the model's slot counts for both forms, and a crafted set of every width fits 256 validators"""
    import ctypes as C
    import go_ibft_amd.build as B
    import key_cache_glv_child as G
    import key_cache_model as M
    import warm_cases as WC
    import warm_glv_cases as GC
    dt = C.CDLL(B.build_devtest())
    nw, ne, nb = C.c_int(), C.c_int(), C.c_int()
    dt.devtest_gtab_dims(C.byref(nw), C.byref(ne), C.byref(nb))
    for width in GC.WIDTHS:                                        # crafted keys + the 16 honest validators + the x = r + n key
        cases = GC.cases_for(width, nb.value)
        assert len({c.addr for c in cases}) == len(cases) and len(cases) + 16 + 1 <= 256, width
        assert GC.coverage(cases, width) == WC.required(width, nb.value)
    rounds = G.budget_inputs()
    assert rounds[0].n == 1700 and not rounds[1].exp.all()
    saved = M.SLOT_BYTES
    try:
        for form, (_, slot) in G.FORMS.items():
            M.SLOT_BYTES = slot
            m = M.KeyCacheModel(1 << 30)
            assert m.max_slots == {"wide": 1638, "glv": 6168}[form]
            assert len(m.set_validators("a", rounds[0].addrs)[0]) == {"wide": 62, "glv": 0}[form]
    finally:
        M.SLOT_BYTES = saved


def test_the_export_is_declared_and_bound():
    """ibft_cache_form at the C boundary, without a device: exported, declared, an optional export of the binding, bound in the
    Go shim; a NULL context is refused and nothing is written"""
    import ctypes as C
    import re
    import go_ibft_amd.build as build
    import go_ibft_amd.verifier as V
    build.build_lib()
    L = V.load_library()
    assert hasattr(L, "ibft_cache_form") and L.ibft_version() == V.ABI_VERSION        # no version step
    assert "ibft_cache_form" in V.EXPORTS and "ibft_cache_form" in V.OPTIONAL_EXPORTS and callable(V.BatchVerifier.cache_form)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibftgpu.h")).read(), flags=re.S)
    proto = re.search(r"\bint\s+ibft_cache_form\s*\((.*?)\)\s*;", hdr, re.S)
    assert proto and [" ".join(p.split()) for p in proto.group(1).split(",")] == ["ibft_ctx *ctx", "uint32_t *form", "uint64_t *slot_bytes"]
    f, b = C.c_uint32(0x7777), C.c_uint64(0x7777)
    assert L.ibft_cache_form(None, C.byref(f), C.byref(b)) == -1 and L.ibft_cache_form(None, None, None) == -1
    assert (f.value, b.value) == (0x7777, 0x7777)
    go = open(os.path.join(ROOT, "shim", "go", "ibftgpu", "ibftgpu.go")).read()
    assert "C.ibft_cache_form(" in go and "func (c *Ctx) CacheForm(" in go
