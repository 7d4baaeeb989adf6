"""The searched corpus of the safegcd inversions: candidate families, the events a corpus has to reach, its coverage.

"Searched" means: tests/golden/make_modinv_edges.py runs the event model (tests/modinv_model.py) over the families below
and keeps, for every event of required(), the first few inputs that show it.  Random 256-bit values reach almost none of
these events (the control of tests/test_modinv_edges_host.py counts them); the values here are ones a sender can put
into the s or r of a signature.  Shared by the generator, the CPU tests and the GPU tests.
"""
import json
import os
import random

import modinv_model as MM

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modinv_edges.json")
MODULI = MM.MODULI
WHICH = {"p": 0, "n": 1}          # the harnesses' and devtest's number of a modulus
KEEP = 6                          # inputs kept per event
MAX_VALUES, MAX_QUADS = 2048, 1024
CONTROL = 4096                    # seeded random values per modulus that run alongside

# inputs that have failed before, by name (a mismatch found with this corpus is added here)
NAMED = {
    "one_in_lockstep_came_out_as_M_plus_1": 1,   # 1/1 = M + 1 before the closing block was widened
}


def specials(m):
    """the hand-picked values of test_safegcd_inversion, test_gpu_arith.values and the two modinv tests of test_dev_wave_host"""
    return [0, 1, 2, 3, m - 1, m - 2, m - 3, (m + 1) // 2, (m - 1) // 2, m // 3, 2**255 % m, 2**128, 2**240, 2**30, 2**30 - 1,
            2**30 + 1, 2**60 - 1]


def families(m):
    """name → list of candidates in [0, M), in the order the search tries them"""
    inv = lambda k: pow(k, -1, m)
    fam = {}
    fam["named"] = sorted(set(NAMED.values()))
    fam["specials"] = specials(m)
    fam["k_inv"] = [inv(k) for k in range(1, 400)]
    fam["neg_k_inv"] = [m - inv(k) for k in range(1, 400)]
    fam["k_2j_inv"] = [inv(k << j) for k in (1, 3, 5, 7, 11, 255) for j in range(1, 256, 5)]
    fam["tiny"] = list(range(4, 68))
    fam["m_minus_tiny"] = [m - t for t in range(4, 68)]
    fam["pow2"] = [(1 << j) % m for j in range(2, 256)]
    fam["m_minus_pow2"] = [m - (1 << j) % m for j in range(2, 256)]
    fam["limb_boundary"] = [((1 << (30 * i)) + dl) % m for i in range(1, 9) for dl in (-2, -1, 0, 1, 2)] + \
        [((1 << (30 * i)) * ((1 << 30) - 1)) % m for i in range(1, 8)]
    # halves and thirds of small numbers: their inverses are small multiples, f and g shrink at once and d, e stay tiny
    fam["small_over_small"] = [a * inv(b) % m for a in range(2, 12) for b in range(2, 12) if a % b and b % a]
    return fam


def candidates(m):
    """every family's values once, in family order: [(value, family)]"""
    seen, out = set(), []
    for name, xs in families(m).items():
        for x in xs:
            x %= m
            if x not in seen:
                seen.add(x)
                out.append((x, name))
    return out


def control(name, count=CONTROL):
    rng = random.Random("modinv control " + name)
    return [rng.randrange(MODULI[name]) for _ in range(count)]


# ---- events -------------------------------------------------------------------------------------------------------------
DIVSTEPS = ["ds:L=%d" % L for L in range(1, 7)] + ["ds:L_by_steps_left", "ds:sentinel_cut", "ds:g0_zero_batch"]
# Divsteps events the search may miss; the fixture then lists them under "unreached" with the number of candidates tried.
#   ds:batches>=19: g reaches 0 in batch 19 or 20.  modinv<MOD> always runs 20 batches, and a batch with g = 0 (matrix
#   (2^30, 0; 0, 1)) adds M to a negative d.  Every value met so far is done after 17 or 18 batches, so d has been
#   through two such batches and is in [0, M) when normalize_30 gets it: its FIRST add (norm:add1, paths 1xx) can only
#   fire for a value that needs 19 batches or more, which is why norm:add1 stands here and not in CANONICAL.
DIVSTEPS_OPTIONAL = ["ds:batches>=19"]
# normalize_30: {add M if negative, negate if f = −1, add M if negative}.  With d in [0, M) on entry (above) the paths
# are 000 and 011 (a negated d ≠ 0 is negative).
CANONICAL = ["norm:neg", "norm:add2", "norm:path=000", "norm:path=011"] + \
    ["de:sign_d=%d,e=%d" % (a, b) for a in (0, 1) for b in (0, 1)]
# carry-save form.  close:path=abcde: {add, negate, add, add, subtract M} of modinv_wave_body's closing block; 1 = taken.
# Which paths can occur: the first add needs D < 0; after it D is in (−M − ε, M + ε); the negation is free; the second add
# needs a negative D again, the third one a D that is still negative after it (D < −M: the ε surplus), and M comes off
# when D ≥ M (the ε surplus on the other side).  Third add and subtraction exclude each other.
# cs:zero_g_in_nonzero_limbs: g has reached 0 but is held as (…, 2^30, −1, …), a pattern the carry-save update moves up one
# limb per batch without ever clearing it, so the wavefront's vote `any(g != 0)` stays true and all 20 batches run (about
# one random value in three; results are right — the batches are idle ones — but the early exit is missed).
WAVE = ["cs:d_called_negative", "cs:e_called_negative", "cs:d_called_nonnegative", "cs:e_called_nonnegative",
        "cs:out_of_range", "cs:idle_batch", "cs:zero_g_in_nonzero_limbs",
        "close:add1", "close:neg", "close:add2", "close:add3", "close:subM"] + \
    ["close:path=" + p for p in ("00000", "00001", "01100", "01110", "10000", "10100", "11000", "11100")]
ROWS = ["rows:finish_in_different_batches", "rows:idle>=3", "cs:idle_batch", "cs:out_of_range", "cs:d_called_negative",
        "cs:d_called_nonnegative", "close:add3", "close:subM"]
FORMS = ("divsteps", "canonical", "wave", "rows")


def required():
    """form → the events the corpus has to reach, for each modulus"""
    return {"divsteps": list(DIVSTEPS), "canonical": list(CANONICAL), "wave": list(WAVE), "rows": list(ROWS)}


def analyse(x, m):
    """the events of one value: canonical form, and the carry-save form with the value in all four rows"""
    c = MM.run_canonical(x, m)
    w = MM.run_wave([x] * 4, m)
    r0 = w["rows"][0]
    ds = sorted(e for e in c["events"] if e.startswith("ds:"))
    assert ds == sorted(e for e in r0["events"] if e.startswith("ds:"))
    assert c["inv"] == r0["inv"] == (pow(x, -1, m) if x else 0), hex(x)
    return dict(divsteps=ds, canonical=sorted(e for e in c["events"] if not e.startswith("ds:")),
                wave=sorted(e for e in r0["events"] if not e.startswith("ds:")),
                batches=c["batches"], zeta=c["zeta"], limb=w["limb"], canonical_run=c, wave_run=w)


def analyse_quad(xs, m):
    w = MM.run_wave(xs, m)
    for x, r in zip(xs, w["rows"]):
        assert r["inv"] == (pow(x, -1, m) if x else 0), hex(x)
    return w


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def corpus_values(fix, name):
    return [int(v, 16) for v in fix["moduli"][name]["values"]]


def corpus_quads(fix, name):
    return [[int(v, 16) for v in q["values"]] for q in fix["moduli"][name]["quads"]]


def coverage(fix):
    """modulus → form → set of events the fixture's inputs hit, recomputed with the model (not read from the fixture)"""
    cov = {}
    for name, m in MODULI.items():
        c = {"divsteps": set(), "canonical": set(), "wave": set(), "rows": set()}
        for x in corpus_values(fix, name):
            a = analyse(x, m)
            for form in ("divsteps", "canonical", "wave"):
                c[form].update(a[form])
        for q in corpus_quads(fix, name):
            w = analyse_quad(q, m)
            c["rows"].update(w["events"])
            for r in w["rows"]:
                c["rows"].update(e for e in r["events"] if not e.startswith("ds:"))
        cov[name] = c
    return cov


# ---- placements: what the tests run for every corpus value ----------------------------------------------------------------
def placements(x):
    """a value in each of the four rows beside three zeros (a ragged batch's padding rows), and four times itself"""
    return [[x if r == pos else 0 for r in range(4)] for pos in range(4)] + [[x] * 4]


def pack(values):
    return b"".join(v.to_bytes(32, "big") for v in values)


def check_wave_out(out_bytes, jobs, m, what):
    """out = jobs × 64 × 32 bytes of a wavefront's answers; jobs: list of four-value lists.  All sixteen lanes of a row agree
    and hold pow(x, −1, M) (0 for 0)."""
    assert len(out_bytes) == 2048 * len(jobs)
    for j, xs in enumerate(jobs):
        for row, x in enumerate(xs):
            base = 2048 * j + 512 * row
            first = out_bytes[base:base + 32]
            assert out_bytes[base:base + 512] == first * 16, (what, "lanes of a row disagree", j, row, hex(x))
            assert int.from_bytes(first, "big") == (pow(x, -1, m) if x else 0), (what, j, row, [hex(v) for v in xs])
