"""Crafted rows for the warm verify kernels in the GLV table form (IBFT_QTAB_FORM=glv; csrc/verify_dev.h), shared by
tests/test_dev_warm_glv_edges_host.py and tests/key_cache_glv_child.py: the split model of tests/warm_cases.py restated for
the new point order.

u2 is split into signed halves k1 + k2·λ ≡ u2 (row_scalar_cases.split: the device's split in exact integers); a half's
magnitude is recoded as b = |k| + Σ_{i<15} 128·256^i, digit i = byte i of b − 128 (i < 15), top digit b >> 120.  The 48 table
points of R′ = u1·G + u2·Q are, in order: 16 of the k1 half (sign(k1)·d·2^(8w)·Q), 16 of the k2 half (sign(k2)·d·2^(8w)·λQ),
then 256 / GTAB_BITS of G.  So a point's formal coefficient in q carries λ and the sign.  The widths deal the points as in
the wide form (warm_cases.split: lane p mod G; the wavefront form row p mod 4, which makes its steps 0–3 k1, 4–7 k2, then G).

The solver, make_valid, make_infinity, twins and the Case record are warm_cases' own.  Test infrastructure only."""
import functools
import random

import row_scalar_cases as RC
import warm_cases as WC
from oracle import pyref as R

N = WC.N
HALF_WINDOWS = 16
Q_POINTS = 2 * HALF_WINDOWS
WIDTHS = WC.WIDTHS
BIAS = sum(128 << (8 * i) for i in range(15))


def recode(k):
    """the 16 digits of a half's magnitude k < 2^128"""
    b = k + BIAS
    return [((b >> (8 * i)) & 255) - 128 for i in range(15)] + [b >> 120]


def table_points(u1, u2, bits):
    """The kernel's table points in order: (a, b) for the point a·G + b·Q, or None where the digit is 0 (skipped)."""
    pts = []
    for k, lam in zip(RC.split(u2), (1, RC.LAMBDA)):
        sign = -1 if k < 0 else 1
        for w, d in enumerate(recode(abs(k))):
            pts.append((0, sign * d * (1 << (8 * w)) * lam % N) if d else None)
    assert sum(p[1] for p in pts if p) % N == u2
    for w in range(256 // bits):
        d = (u1 >> (w * bits)) & ((1 << bits) - 1)
        pts.append((d << (w * bits), 0) if d else None)
    return pts


def events(u1, u2, bits, width):
    """warm_cases.events over this form's points"""
    pts = table_points(u1, u2, bits)
    lanes, join = WC.split(width)
    ev, acc = [], []
    for l in range(lanes):
        A = None
        for p in range(l, len(pts), lanes):
            if pts[p] is not None:
                ev.append(("madd", l, p, A, pts[p]))
                A = WC._plus(A, pts[p])
        acc.append(A)
    for lev, off in enumerate(join):
        ev += [("join", lev, l, acc[l], acc[l ^ off]) for l in range(lanes)]
        acc = [WC._plus(acc[l], acc[l ^ off]) for l in range(lanes)]
    return ev


def hits(u1, u2, q, bits, width):
    return {(e[0], e[1] if e[0] == "join" else None, WC.kind(e[3], e[4], q)) for e in events(u1, u2, bits, width)}


def _finish(name, width, bits, u1, u2, q, row, rng):
    """warm_cases._finish with this form's hits"""
    c = WC._finish(name, 0, bits, u1, u2, q, row, rng)
    c.width = width
    c.hit = hits(u1, u2, q, bits, width) if width else set()
    return c


def _madd_targets(width, bits, probe):
    """mixed additions of a G-table point into a lane's non-empty sum (a sum of Q points alone cannot be forced onto another
    Q point through q): the first one — the k2 half → G boundary — and the last one, in the first and the last such lane"""
    ev = [e for e in events(*probe, bits, width) if e[0] == "madd" and e[3] is not None and e[2] >= Q_POINTS]
    lanes = sorted({e[1] for e in ev})
    out = []
    for lane in dict.fromkeys((lanes[0], lanes[-1])):
        ps = [e[2] for e in ev if e[1] == lane]
        out.append(("madd", lane, ps[0], "boundary"))
        if ps[-1] != ps[0]:
            out.append(("madd", lane, ps[-1], "late"))
    return out


def _join_targets(width, bits, probe):
    """butterfly additions: at every level, the first pair (lane 0) and the last pair"""
    lanes, join = WC.split(width)
    ev = {(e[1], e[2]): (e[3], e[4]) for e in events(*probe, bits, width) if e[0] == "join"}
    out = []
    for lev, off in enumerate(join):
        seen = []
        for lane in (0, lanes - 1 - off):
            ops = ev[(lev, lane)]
            if ops in seen or ops[::-1] in seen:
                continue
            seen.append(ops)
            out.append(("join", lev, lane, "first" if lane == 0 else "last"))
    return out


def _targeted(width, bits, target, sign, rng):
    """random u1, u2; q solved so that the target addition meets equal (sign +1) or opposite (−1) operands.  Raises when no
    case is found: no target is ever dropped."""
    label = {1: "same", -1: "opposite"}[sign]
    for attempt in range(200):
        u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
        e = WC._find(events(u1, u2, bits, width), target)
        if e is None or e[3] is None or e[4] is None:
            continue
        q = WC._solve(e[3], e[4], sign)
        if q is None:
            continue
        row = WC.make_valid(u1, u2, q)
        if row is None and (u1 + u2 * q) % N:
            continue                               # R′.x ≥ n: draw again
        if row is not None and int.from_bytes(row[1][32:64], "big") > N // 2 and attempt < 100:
            continue                               # prefer low s: then the strict policy decides by the arithmetic too
        where = f"L{target[1]}/lane{target[2]}" if target[0] == "join" else f"lane{target[1]}/p{target[2]}"
        name = f"glv/G{width}/{target[0]}/{where}/{target[3]}/{label}" + ("/R'=inf" if row is None else "")
        c = _finish(name, width, bits, u1, u2, q, row, rng)
        Q = R.pt_mul(q, R.G)                       # the coincidence, recomputed on points: operand A = ±operand B, both finite
        pa, pb = WC._operand_point(e[3], Q), WC._operand_point(e[4], Q)
        assert pa is not None and pb is not None and pa == (pb if sign == 1 else WC._neg(pb)), name
        assert WC.kind(e[3], e[4], q) == label
        c.target = (target[0], target[1] if target[0] == "join" else None, label)
        return c
    raise AssertionError(f"no case found for {width} {target} {sign}")


@functools.lru_cache(maxsize=None)
def targets(width, bits):
    rng = random.Random(0x61F * 131 + width * 17 + bits)
    probe = (rng.randrange(1, N), rng.randrange(1, N))
    return tuple(_madd_targets(width, bits, probe) + _join_targets(width, bits, probe))


@functools.lru_cache(maxsize=None)
def targeted_cases(width, bits):
    """mixed additions and butterfly levels, equal and opposite operands, plus an R′ = ∞ row: 2·len(targets) + 1 cases"""
    rng = random.Random(0x61F * 977 + width * 17 + bits)
    cases = [_targeted(width, bits, t, sign, rng) for t in targets(width, bits) for sign in (1, -1)]
    u1, u2 = rng.randrange(1, N), rng.randrange(1, N)             # u1 ≡ −u2·q
    q = (-u1) * pow(u2, -1, N) % N
    cases.append(_finish(f"glv/G{width}/R'=inf", width, bits, u1, u2, q, None, rng))
    assert len(cases) == 2 * len(targets(width, bits)) + 1
    return tuple(cases)


# The largest top digit a half of a scalar below n can have: |k1| ≤ (a1 + a2)/2 and |k2| ≤ (|b1| + a1)/2 (the split rounds to
# the nearest lattice point), both below 2^127.4 — so the top digit stays below 164 and the table's entries 164 … 256 of window
# 15 are reached by no signature.  (They are checked where they can be: the recoding and the table build, tests/test_qtab_glv_host.py.)
HALF_MAX = max((RC.A1 + RC.A2 + 1) // 2, (RC.B1M + RC.A1 + 1) // 2)
TOP_DIGIT_MAX = (HALF_MAX + BIAS) >> 120


def _shape_of(u2):
    k1, k2 = RC.split(u2)
    d1, d2 = recode(abs(k1)), recode(abs(k2))
    return k1, k2, d1, d2


SHAPES = {
    "k2=0": lambda k1, k2, d1, d2: k2 == 0 and k1 != 0,
    "k1=0": lambda k1, k2, d1, d2: k1 == 0 and k2 != 0,
    "signs++": lambda k1, k2, d1, d2: k1 > 0 and k2 > 0,
    "signs+-": lambda k1, k2, d1, d2: k1 > 0 and k2 < 0,
    "signs-+": lambda k1, k2, d1, d2: k1 < 0 and k2 > 0,
    "signs--": lambda k1, k2, d1, d2: k1 < 0 and k2 < 0,
    "top>=128/k1": lambda k1, k2, d1, d2: d1[15] >= 128,      # beyond a signed digit's range: the top digit is unsigned
    "top>=128/k2": lambda k1, k2, d1, d2: d2[15] >= 128,
    "digit=-128/k1": lambda k1, k2, d1, d2: -128 in d1[:15],
    "digit=-128/k2": lambda k1, k2, d1, d2: -128 in d2[:15],
    "digit=0": lambda k1, k2, d1, d2: 0 in d1 and 0 in d2,
}


def _u2_candidates(name, rng, u1_zero):
    if name == "k2=0":                                   # (with u1 = 0: a single digit, one table point in all)
        while True:
            yield rng.randrange(1, 128 if u1_zero else 1 << 112)
    if name == "k1=0":
        while True:
            yield rng.randrange(1, 1 << 100) * RC.LAMBDA % N
    while True:
        yield rng.randrange(1, N)


@functools.lru_cache(maxsize=None)
def shape_cases(bits):
    """rows that serve every width (width 0): a half that vanishes, every combination of the halves' signs, a top digit
    beyond 127, a digit of −128, digits of 0 in both halves; each with a random u1, and once u1 = 0 (z = 0) with a u2 of a single
    digit: whole lanes hold no point and carry ∞ into the join"""
    rng = random.Random(0x61F5 + bits)
    out = []
    for name, holds in SHAPES.items():
        for u1_zero in ((True, False) if name == "k2=0" else (False,)):
            for u2 in _u2_candidates(name, rng, u1_zero):
                if not holds(*_shape_of(u2)):
                    continue
                u1, q = 0 if u1_zero else rng.randrange(1, N), rng.randrange(1, N)
                row = WC.make_valid(u1, u2, q)
                if row is not None and int.from_bytes(row[1][32:64], "big") <= N // 2:
                    break
            out.append(_finish(f"glv/shape/{name}" + ("/u1=0" if u1_zero else ""), 0, bits, u1, u2, q, row, rng))
    return tuple(out)


def cases_for(width, bits):
    return targeted_cases(width, bits) + shape_cases(bits)


def coverage(cases, width):
    return {c.target for c in cases if c.target and c.width == width}


def required(width, bits):
    """what coverage() must hold: equal and opposite operands in a mixed addition and at every butterfly level"""
    return WC.required(width, bits)
