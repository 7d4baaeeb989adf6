"""An event model of the safegcd inversions (csrc/modinv_dev.h, csrc/wave_fe_dev.h) in plain Python integers.

Nothing here imports the build.  Every function restates one function of the device headers limb for limb, so that the
limbs after every batch can be compared with the trace exports of the host harnesses (tests/test_modinv_edges_host.py),
and records EVENTS: the rare states a run passes through (a sign read wrongly off a carry-save top limb, a value outside
(−2M, M), each step of the closing normalisations, each width of the lockstep divsteps' cancellation, …).  An event the
model reports for an input is, once the traces agree, something the build really does on that input.

Two limb forms (radix 2^30, nine limbs):
  canonical   modinv<MOD> / modinv_rt: limbs 0..7 in [0, 2^30), limb 8 signed            → run_canonical
  carry-save  modinv_wave_body: limbs in [−4, 2^30 + 4), limb 8 unmasked, one value per
              DPP row, four rows of a wavefront in lockstep; a finished row idles         → run_wave
"""

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
MODULI = {"p": P, "n": N}
M30 = (1 << 30) - 1
M32 = (1 << 32) - 1
BATCHES = 20
LIMB_LO, LIMB_HI = -4, (1 << 30) + 4  # what wave_fe_dev.h claims for carry-save limbs 0..7: [LIMB_LO, LIMB_HI)


def s32(x):
    """the int32 a 32-bit register holds"""
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def fits32(x):
    assert -(1 << 31) <= x < (1 << 31), x
    return x


def limbs30(x):
    """s30_from_u256"""
    assert 0 <= x < 1 << 256
    return [(x >> (30 * i)) & M30 for i in range(9)]


def value(limbs):
    return sum(v << (30 * i) for i, v in enumerate(limbs))


def inv30(m):
    """the constant the headers call inv30(): M⁻¹ mod 2^30"""
    return pow(m, -1, 1 << 30)


def ctz(x):
    return (x & -x).bit_length() - 1


# ---- the three divstep forms: 30 steps on the low words → (ζ, (u, v, q, r)) --------------------------------------------

def divsteps_30(zeta, f0, g0):
    """modinv_dev.h:divsteps_30, constant time, one step per turn, 32-bit wrap-around"""
    u, v, q, r = 1, 0, 0, 1
    f, g = f0 & M32, g0 & M32
    for _ in range(30):
        c1 = M32 if zeta < 0 else 0
        c2 = M32 if g & 1 else 0
        x, y, z = ((f ^ c1) - c1) & M32, ((u ^ c1) - c1) & M32, ((v ^ c1) - c1) & M32
        g = (g + (x & c2)) & M32
        q = (q + (y & c2)) & M32
        r = (r + (z & c2)) & M32
        c1 &= c2
        zeta = s32(((zeta & M32) ^ c1) - 1)
        f = (f + (g & c1)) & M32
        u = (u + (q & c1)) & M32
        v = (v + (r & c1)) & M32
        g >>= 1
        u = (u << 1) & M32
        v = (v << 1) & M32
    return zeta, (s32(u), s32(v), s32(q), s32(r))


def divsteps_30_var(zeta, f0, g0):
    """modinv_dev.h:divsteps_30_var, zero runs stripped with one ctz"""
    u, v, q, r = 1, 0, 0, 1
    f, g, i = f0 & M32, g0 & M32, 30
    while True:
        z = ctz(g | (1 << i))
        g >>= z
        u = (u << z) & M32
        v = (v << z) & M32
        zeta -= z
        i -= z
        if i == 0:
            break
        if zeta < 0:
            zeta = -zeta - 1
            f, g = g, (g - f) & M32
            u, q = q, (q - u) & M32
            v, r = r, (r - v) & M32
        else:
            g = (g + f) & M32
            q = (q + u) & M32
            r = (r + v) & M32
    return zeta, (s32(u), s32(v), s32(q), s32(r))


def divsteps_30_lockstep(zeta, f0, g0, ev=None, live=True):
    """modinv_dev.h:divsteps_30_lockstep round by round.  (Rounds a row idles through while other rows of its wavefront
    still work change nothing — c = 0, L = 0, w = 0 — so one value's rounds are the same alone and in lockstep.)
    ev: a set that receives ds:L=k, ds:L_by_steps_left, ds:sentinel_cut; live: the whole g is not zero."""
    u, v, q, r = 1, 0, 0, 1
    f, g, i = f0 & M32, g0 & M32, 30
    rounds = 0

    def strip():
        nonlocal g, u, v, zeta, i
        if ev is not None and live and i > 0 and g & ((2 << i) - 1) == 0:
            ev.add("ds:sentinel_cut")  # bits 0..i of g are zero: the run goes on past the batch's last step
        z = ctz(g | (1 << i))
        g >>= z
        u = (u << z) & M32
        v = (v << z) & M32
        zeta -= z
        i -= z

    strip()
    while True:
        rounds += 1
        if zeta < 0 and i != 0:
            f, g = g, (-f) & M32
            u, q = q, (-u) & M32
            v, r = r, (-v) & M32
            zeta = ~zeta
        cap = min(i, 6)
        L = max(0, min(zeta + 1, cap))
        if ev is not None and L:
            ev.add("ds:L=%d" % L)
            if L == i and i < 6 and i < zeta + 1:
                ev.add("ds:L_by_steps_left")
        w = ((f * f - 2) * f * g) & ((1 << L) - 1)
        g = (g + w * f) & M32
        q = (q + w * u) & M32
        r = (r + w * v) & M32
        strip()
        if i == 0:
            break
    return zeta, (s32(u), s32(v), s32(q), s32(r)), rounds


# ---- canonical limbs -----------------------------------------------------------------------------------------------

def update_fg_30(f, g, t):
    u, v, q, r = t
    cf = u * f[0] + v * g[0]
    cg = q * f[0] + r * g[0]
    assert cf & M30 == 0 and cg & M30 == 0
    cf >>= 30
    cg >>= 30
    nf, ng = [0] * 9, [0] * 9
    for i in range(1, 9):
        cf += u * f[i] + v * g[i]
        cg += q * f[i] + r * g[i]
        nf[i - 1] = cf & M30
        ng[i - 1] = cg & M30
        cf >>= 30
        cg >>= 30
    nf[8] = fits32(cf)
    ng[8] = fits32(cg)
    return nf, ng


def _m_multiples(d8, e8, d0, e0, t, minv):
    """the multiples of M that update_de_30 and modinv_wave_body add: the sign masks come off the TOP limbs"""
    u, v, q, r = t
    sd, se = (-1 if d8 < 0 else 0), (-1 if e8 < 0 else 0)
    md = fits32((u & sd) + (v & se))
    me = fits32((q & sd) + (r & se))
    cd0 = (u * d0 + v * e0) & M32
    ce0 = (q * d0 + r * e0) & M32
    md = fits32(md - ((minv * cd0 + md) & M30))
    me = fits32(me - ((minv * ce0 + me) & M30))
    return md, me


def update_de_30(d, e, t, mod, minv):
    u, v, q, r = t
    md, me = _m_multiples(d[8], e[8], d[0], e[0], t, minv)
    cd = u * d[0] + v * e[0] + mod[0] * md
    ce = q * d[0] + r * e[0] + mod[0] * me
    assert cd & M30 == 0 and ce & M30 == 0
    cd >>= 30
    ce >>= 30
    nd, ne = [0] * 9, [0] * 9
    for i in range(1, 9):
        cd += u * d[i] + v * e[i] + mod[i] * md
        ce += q * d[i] + r * e[i] + mod[i] * me
        nd[i - 1] = cd & M30
        ne[i - 1] = ce & M30
        cd >>= 30
        ce >>= 30
    nd[8] = fits32(cd)
    ne[8] = fits32(ce)
    return nd, ne


def _ripple(r):
    for i in range(8):
        r[i + 1] = fits32(r[i + 1] + (r[i] >> 30))
        r[i] &= M30


def normalize_30(r, neg, mod, ev):
    """modinv_dev.h:normalize_30 → the canonical limbs; ev receives norm:add1 / norm:neg / norm:add2 and the path"""
    r = list(r)
    a1 = r[8] < 0
    if a1:
        r = [fits32(x + m) for x, m in zip(r, mod)]
    if neg:
        r = [-x for x in r]
    _ripple(r)
    a2 = r[8] < 0
    if a2:
        r = [fits32(x + m) for x, m in zip(r, mod)]
    _ripple(r)
    for name, hit in (("add1", a1), ("neg", neg), ("add2", a2)):
        if hit:
            ev.add("norm:" + name)
    ev.add("norm:path=%d%d%d" % (a1, neg, a2))
    return r


def _divstep_events(ev, zeta_in, f, g, live):
    """one batch's divsteps with its events; f, g: limb lists (only the low words are read)"""
    if live and g[0] & M30 == 0:
        ev.add("ds:g0_zero_batch")  # g ≠ 0 but ≡ 0 mod 2^30: the batch only halves, matrix (2^30, 0; 0, 1)
    zeta, t, rounds = divsteps_30_lockstep(zeta_in, f[0], g[0], ev, live)
    if live and g[0] & M30 == 0:
        assert t == (1 << 30, 0, 0, 1)
    return zeta, t, rounds


def run_canonical(x, m):
    """modinv<MOD>(x) → dict(inv, trace, events, …); trace[b] = (d, e, f, g, ζ) after batch b (canonical limbs)"""
    mod, minv = limbs30(m), inv30(m)
    d, e, f, g = [0] * 9, [1] + [0] * 8, list(mod), limbs30(x)
    zeta, ev, trace, triples = -1, set(), [], []
    batches, zmin, zmax = None, 0, -1
    for b in range(BATCHES):
        live = any(g)
        triples.append((zeta, f[0] & M32, g[0] & M32))
        zeta, t, _ = _divstep_events(ev, zeta, f, g, live)
        ev.add("de:sign_d=%d,e=%d" % (d[8] < 0, e[8] < 0))
        for name, w in (("d", d), ("e", e)):
            if not -2 * m < value(w) < m:
                ev.add("de:%s_out_of_range" % name)
        d, e = update_de_30(d, e, t, mod, minv)
        f, g = update_fg_30(f, g, t)
        assert (value(d) * x - value(f)) % m == 0 and (value(e) * x - value(g)) % m == 0
        trace.append((d, e, f, g, zeta))
        if live:
            zmin, zmax = min(zmin, zeta), max(zmax, zeta)
            if not any(g):
                batches = b + 1
    assert not any(g)
    if (batches or 0) >= 19:
        ev.add("ds:batches>=19")  # fewer than two batches with g = 0 behind it: d may still be negative
    out = normalize_30(d, f[8] < 0, mod, ev)
    return dict(inv=value(out), trace=trace, events=ev, batches=batches or 0, zeta=(zmin, zmax), triples=triples)


# ---- carry-save limbs, one value per row, four rows in lockstep -----------------------------------------------------

def modinv_wave_apply(m1, a, m2, b, mod, mm, lim):
    """wave_fe_dev.h:modinv_wave_apply over the nine limb lanes of a row (lanes 9..15 hold zeros and stay zero).
    lim: [lo, hi] of every limb 0..7 met, updated in place"""
    c = [m1 * a[j] + m2 * b[j] + mod[j] * mm for j in range(9)]
    lo = [x & M30 for x in c]
    assert lo[0] == 0  # the exactness limb j = lo_{j+1} + hi_j rests on
    n = [(lo[j + 1] if j < 8 else 0) + (c[j] >> 30) for j in range(9)]
    out = []
    for j in range(9):
        top = j >= 8
        keep = fits32(n[j]) if top else n[j] & M30
        carry = 0 if j == 0 else fits32(n[j - 1] >> 30)  # lane j − 1 is never the top lane here
        out.append(fits32(keep + carry))
    for x in out[:8]:
        assert LIMB_LO <= x < LIMB_HI, x
        lim[0], lim[1] = min(lim[0], x), max(lim[1], x)
    return out


def wave_close(d, fneg, mod, ev):
    """the closing block of modinv_wave_body: D in (−2M − ε, M + ε) → [0, M)"""
    D = list(d)

    def add_m_if_negative():
        neg = D[8] < 0
        if neg:
            for i in range(9):
                D[i] = fits32(D[i] + mod[i])
        _ripple(D)
        return neg

    _ripple(D)
    steps = [add_m_if_negative(), fneg]
    if fneg:
        for i in range(9):
            D[i] = -D[i]
    _ripple(D)
    steps.append(add_m_if_negative())
    steps.append(add_m_if_negative())
    E = [D[i] - mod[i] for i in range(9)]
    _ripple(E)
    sub = E[8] >= 0
    steps.append(sub)
    if sub:
        D = E
    names = ("add1", "neg", "add2", "add3", "subM")
    for name, hit in zip(names, steps):
        if hit:
            ev.add("close:" + name)
    ev.add("close:path=" + "".join("%d" % s for s in steps))
    return D


def run_wave(xs, m):
    """modinv_wave_body with xs[row] in row 0..3 → dict(batches, rows=[dict(inv, trace, events, finish, idle, …)], limb)
    rows[k].trace[b] = (d, e, f, g, ζ) after batch b of the WAVEFRONT (carry-save limbs), idle batches included."""
    assert len(xs) == 4
    mod, minv = limbs30(m), inv30(m)
    zero = [0] * 9
    # (rows that hold the same value take the same steps: each distinct value is run once)
    rows = [dict(x=x, d=[0] * 9, e=[1] + [0] * 8, f=list(mod), g=limbs30(x), zeta=-1, events=set(), trace=[], finish=None,
                 zmin=0, zmax=-1, triples=[]) for x in dict.fromkeys(xs)]
    lim = [0, 0]
    batches = 0
    for b in range(BATCHES):
        for R in rows:
            d, e, f, g, ev = R["d"], R["e"], R["f"], R["g"], R["events"]
            live = value(g) != 0
            R["triples"].append((R["zeta"], f[0] & M32, g[0] & M32))
            zeta, t, _ = _divstep_events(ev, R["zeta"], f, g, live)
            if not live:
                ev.add("cs:idle_batch")
                assert t == (1 << 30, 0, 0, 1)
                if any(g):
                    # zero held as (…, 2^30, −1, …): the wavefront's vote `g != 0` sees a live row and goes on
                    ev.add("cs:zero_g_in_nonzero_limbs")
            for name, w in (("d", d), ("e", e)):
                val = value(w)
                if w[8] < 0 <= val:
                    ev.add("cs:%s_called_negative" % name)
                if val < 0 <= w[8]:
                    ev.add("cs:%s_called_nonnegative" % name)
                if not -2 * m < val < m:
                    ev.add("cs:out_of_range")
                    ev.add("cs:%s_out_of_range" % name)
                    ev.add("cs:%s_out_of_range_%s" % (name, "idle" if not live else "live"))
            md, me = _m_multiples(d[8], e[8], d[0], e[0], t, minv)
            u, v, q, r = t
            nd = modinv_wave_apply(u, d, v, e, mod, md, lim)
            ne = modinv_wave_apply(q, d, r, e, mod, me, lim)
            nf = modinv_wave_apply(u, f, v, g, zero, 0, lim)
            ng = modinv_wave_apply(q, f, r, g, zero, 0, lim)
            R["d"], R["e"], R["f"], R["g"], R["zeta"] = nd, ne, nf, ng, zeta
            assert (value(nd) * R["x"] - value(nf)) % m == 0 and (value(ne) * R["x"] - value(ng)) % m == 0
            R["trace"].append((nd, ne, nf, ng, zeta))
            if live:
                R["zmin"], R["zmax"] = min(R["zmin"], zeta), max(R["zmax"], zeta)
                if value(ng) == 0:
                    R["finish"] = b + 1
        batches = b + 1
        if not any(any(R["g"]) for R in rows):  # !any(g != 0) over the limbs of the whole wavefront
            break
    out = []
    for R in [next(R for R in rows if R["x"] == x) for x in xs]:
        assert value(R["g"]) == 0 and (value(R["f"]) in (1, -1) or R["x"] == 0)
        fin = R["finish"] or 0
        ev = set(R["events"])
        if fin >= 19:
            ev.add("ds:batches>=19")
        fneg = (R["f"][0] & 3) == 3
        D = wave_close(R["d"], fneg, mod, ev)
        out.append(dict(inv=value(D), trace=R["trace"], events=set(ev), finish=fin, idle=batches - fin if R["x"] else 0,
                        zeta=(R["zmin"], R["zmax"]), triples=R["triples"]))
    fins = [o["finish"] for o in out if o["finish"]]
    wave_ev = set()
    if fins and min(fins) != max(fins):
        wave_ev.add("rows:finish_in_different_batches")
    for o in out:
        if o["idle"] >= 3:
            wave_ev.add("rows:idle>=3")
            o["events"].add("rows:idle>=3")
    return dict(batches=batches, rows=out, limb=tuple(lim), events=wave_ev,
                first=min(fins) if fins else 0, last=max(fins) if fins else 0)
