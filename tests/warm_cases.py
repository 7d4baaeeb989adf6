"""Crafted rows for the warm verify kernels (shared by tests/test_dev_warm_edges_host.py and tests/test_gpu_warm_edges.py).

Once a validator's key Q = q·G is known, a seal (z, r, s, v) is decided by R′ = u1·G + u2·Q with u1 = z/s, u2 = r/s:
32 points of Q's table (byte p of u2, weight 2^(8p)) and 256 / GTAB_BITS points of the generator's table (digit w of u1,
weight 2^(w·GTAB_BITS)) are summed, zero digits skipped.  Each lane width deals the points and joins the partial sums its
own way (split()).  Every operand of every addition is a·G + b·Q with a, b known from (u1, u2) alone, so with u1, u2 fixed
first, one coincidence "operand A = ±operand B" is forced by solving for the private key q, and make_valid() then turns
(u1, u2, q) into a seal the kernel sees with exactly those scalars:

    R′ = (u1 + u2·q)·G,  r = R′.x,  s = r/u2,  z = u1·s,  v = parity(R′.y)   — a VALID seal by Q.

Every case checks itself with pyref point arithmetic (the targeted operands really are equal / opposite) and records the
verdicts of pyref and of the C oracle (recover and compare), which must agree.  Test infrastructure only."""
import functools
import random
from dataclasses import dataclass, field

from oracle import pyref as R

N, P = R.N, R.P
QTAB_WINDOWS = 32
WIDTHS = (1, 2, 4, 8, 16, 32, 64)


# ---- the split model --------------------------------------------------------------------------------------------

def split(width):
    """(lanes, join): lane l adds the points p ≡ l (mod lanes) in increasing p; join lists the xor distances of the
    butterfly levels in the order they run.
      1      verify_known (verify_dev.h): one lane, Q windows 0..31 then G windows
      2..32  verify_known_group_kernel<·,G> (kernels.hip.h): lane p mod G, levels G/2, …, 1 of jac_add_t
      64     verify_known_wave (wave_fe_dev.h): row p mod 4, row-xor 1 then row-xor 2 of wjac_add"""
    if width == 1:
        return 1, ()
    if width == 64:
        return 4, (1, 2)
    assert width in WIDTHS, width
    return width, tuple(width >> k for k in range(1, width.bit_length()))


def table_points(u1, u2, bits):
    """The kernel's table points in order: (a, b) for the point a·G + b·Q, or None where the digit is 0 (skipped)."""
    pts = []
    for p in range(QTAB_WINDOWS):
        d = (u2 >> (8 * p)) & 255
        pts.append((0, d << (8 * p)) if d else None)
    for w in range(256 // bits):
        d = (u1 >> (w * bits)) & ((1 << bits) - 1)
        pts.append((d << (w * bits), 0) if d else None)
    return pts


def _plus(A, B):
    if A is None:
        return B
    if B is None:
        return A
    return (A[0] + B[0], A[1] + B[1])


def events(u1, u2, bits, width):
    """Every addition the width runs, in formal coefficients (A = None: that sum holds no point yet, i.e. ∞):
    ('madd', lane, p, A, C): the lane's sum A meets table point p (= C); ('join', level, lane, A, B): the lane's sum meets
    the sum of lane ^ off at butterfly level `level`."""
    pts = table_points(u1, u2, bits)
    lanes, join = split(width)
    ev, acc = [], []
    for l in range(lanes):
        A = None
        for p in range(l, len(pts), lanes):
            if pts[p] is not None:
                ev.append(("madd", l, p, A, pts[p]))
                A = _plus(A, pts[p])
        acc.append(A)
    for lev, off in enumerate(join):
        ev += [("join", lev, l, acc[l], acc[l ^ off]) for l in range(lanes)]
        acc = [_plus(acc[l], acc[l ^ off]) for l in range(lanes)]
    return ev


def _val(A, q):
    return 0 if A is None else (A[0] + A[1] * q) % N


def kind(A, B, q):
    """What an addition of the operands A, B meets for the key q: 'inf' (an operand is ∞), 'same', 'opposite' or 'add'."""
    a, b = _val(A, q), _val(B, q)
    if a == 0 or b == 0:
        return "inf"
    return "same" if a == b else "opposite" if (a + b) % N == 0 else "add"


def hits(u1, u2, q, bits, width):
    """{(op, level, kind)} over every addition of the width (op 'madd' has level None)."""
    return {(e[0], e[1] if e[0] == "join" else None, kind(e[3], e[4], q)) for e in events(u1, u2, bits, width)}


# ---- seals ------------------------------------------------------------------------------------------------------

def b32(x):
    return x.to_bytes(32, "big")


def _neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def make_valid(u1, u2, q):
    """(hash32, sig65) of a valid seal by Q = q·G that the kernel sees with exactly u1, u2; None when R′ = ∞ or R′.x ≥ n."""
    assert 0 <= u1 < N and 0 < u2 < N and 0 < q < N
    Rp = R.pt_mul((u1 + u2 * q) % N, R.G)
    if Rp is None or Rp[0] >= N:
        return None
    r = Rp[0]
    s = r * pow(u2, -1, N) % N
    z = u1 * s % N
    assert z * pow(s, -1, N) % N == u1 and r * pow(s, -1, N) % N == u2
    return b32(z), b32(r) + b32(s) + bytes([Rp[1] & 1])


def make_infinity(u1, u2, rng):
    """u1 + u2·q ≡ 0: R′ = ∞ and no seal is valid; some (r, s, v) with those u1, u2 (r the x of a curve point, so that
    recovery yields SOME key — never Q, whose R′ would be finite)."""
    while True:
        k = rng.randrange(1, N)
        X = R.pt_mul(k, R.G)
        if X[0] < N:
            break
    r = X[0]
    s = r * pow(u2, -1, N) % N
    z = u1 * s % N
    return b32(z), b32(r) + b32(s) + bytes([rng.randrange(2)])


def verdict(h, sig, addr, flags):
    """recover-and-compare by the C oracle, checked against pyref"""
    from oracle import binding as O
    a = O.recover_address(h, sig, flags)
    assert a == R.recover_address(h, sig, bool(flags & 1)), (h.hex(), sig.hex())
    return a is not None and a == addr


@dataclass
class Case:
    name: str
    width: int                 # the width the case aims at (0: every width)
    bits: int                  # GTAB_BITS it was built for
    u1: int
    u2: int
    q: int | None              # private key (None: the x = r + n key, taught by `teach`)
    pub: bytes                 # X ‖ Y
    addr: bytes
    hash: bytes
    sig: bytes
    expect: dict = field(default_factory=dict)   # flags → verdict of recover-and-compare (pyref = C oracle)
    hit: set = field(default_factory=set)        # hits() at the width aimed at
    teach: tuple | None = None                   # (hash, sig) recovering to this key, when there is no private key
    target: tuple | None = None                  # (op, level, kind) the case forces, checked on points


def _key(q):
    Q = R.pt_mul(q, R.G)
    return Q, R.pub_bytes(Q), R.address(Q)


def _finish(name, width, bits, u1, u2, q, row, rng):
    Q, pub, addr = _key(q)
    if row is None:
        row = make_infinity(u1, u2, rng)
    h, sig = row
    # pyref point arithmetic, independent of the scalar construction: R′ = u1·G + u2·Q
    Rp = R.pt_add(R.pt_mul(u1, R.G), R.pt_mul(u2, Q))
    if Rp is None:
        assert (u1 + u2 * q) % N == 0
    else:
        assert sig[:32] == b32(Rp[0]) and sig[64] == Rp[1] & 1
    c = Case(name, width, bits, u1, u2, q, pub, addr, h, sig)
    c.expect = {fl: verdict(h, sig, addr, fl) for fl in (0, 1)}
    assert c.expect[0] == (Rp is not None), name
    c.hit = hits(u1, u2, q, bits, width) if width else set()
    return c


def _operand_point(A, Q):
    return None if A is None else R.pt_add(R.pt_mul(A[0] % N, R.G), R.pt_mul(A[1] % N, Q))


# ---- targets ----------------------------------------------------------------------------------------------------

def _madd_targets(width, bits, probe):
    """mixed additions of a G-table point into a lane's non-empty sum: the first one (the Q → G boundary) and the last
    one, in the first and in the last lane that has such an addition"""
    ev = [e for e in events(*probe, bits, width) if e[0] == "madd" and e[3] is not None and e[2] >= QTAB_WINDOWS]
    lanes = sorted({e[1] for e in ev})
    out = []
    for lane in dict.fromkeys((lanes[0], lanes[-1])):
        ps = [e[2] for e in ev if e[1] == lane]
        out.append(("madd", lane, ps[0], "boundary"))
        if ps[-1] != ps[0]:
            out.append(("madd", lane, ps[-1], "late"))
    return out


def _join_targets(width, bits, probe):
    """butterfly additions: at every level, the first pair (lane 0) and the last pair (the highest lane that adds its
    partner from above); pairs whose operands are the same as another's are left out"""
    lanes, join = split(width)
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


def _find(ev, target):
    for e in ev:
        if e[0] == target[0] and e[1] == target[1] and e[2] == target[2]:
            return e
    return None


def _solve(A, B, sign):
    """q with A = sign·B, i.e. a_A + b_A·q ≡ sign·(a_B + b_B·q)"""
    den = (A[1] - sign * B[1]) % N
    if den == 0:
        return None
    q = (sign * B[0] - A[0]) * pow(den, -1, N) % N
    return q or None


def _targeted(width, bits, target, sign, rng, low_s=True):
    """random u1, u2; q solved so that the target addition meets equal (sign +1) or opposite (−1) operands"""
    label = {1: "same", -1: "opposite"}[sign]
    for attempt in range(200):
        u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
        e = _find(events(u1, u2, bits, width), target)
        if e is None or e[3] is None or e[4] is None:
            continue
        q = _solve(e[3], e[4], sign)
        if q is None:
            continue
        row = make_valid(u1, u2, q)
        if row is None and (u1 + u2 * q) % N:
            continue                               # R′.x ≥ n: draw again
        if row is not None and low_s and int.from_bytes(row[1][32:64], "big") > N // 2 and attempt < 100:
            continue                               # prefer low s: then the strict policy decides by the arithmetic too
        where = f"L{target[1]}/lane{target[2]}" if target[0] == "join" else f"lane{target[1]}/p{target[2]}"
        name = f"G{width}/{target[0]}/{where}/{target[3]}/{label}" + ("/R'=inf" if row is None else "")
        c = _finish(name, width, bits, u1, u2, q, row, rng)
        # the coincidence, recomputed on points: operand A = ±operand B, both finite
        Q = R.pt_mul(q, R.G)
        pa, pb = _operand_point(e[3], Q), _operand_point(e[4], Q)
        assert pa is not None and pb is not None and pa == (pb if sign == 1 else _neg(pb)), name
        assert kind(e[3], e[4], q) == label
        c.target = (target[0], target[1] if target[0] == "join" else None, label)
        return c
    raise AssertionError(f"no case found for {width} {target} {sign}")


@functools.lru_cache(maxsize=None)
def targeted_cases(width, bits):
    """(a) mixed additions and (b) butterfly levels, equal and opposite operands, plus (d) an R′ = ∞ row"""
    rng = random.Random(0x3A7 * 131 + width * 17 + bits)
    probe = (rng.randrange(1, N), rng.randrange(1, N))
    targets = _madd_targets(width, bits, probe) + _join_targets(width, bits, probe)
    cases = [_targeted(width, bits, t, sign, rng) for t in targets for sign in (1, -1)]
    u1, u2 = rng.randrange(1, N), rng.randrange(1, N)             # (d) u1 ≡ −u2·q
    q = (-u1) * pow(u2, -1, N) % N
    cases.append(_finish(f"G{width}/R'=inf", width, bits, u1, u2, q, None, rng))
    return tuple(cases)


def u2_shapes():
    return {"u2=1": 1, "u2=2^8": 1 << 8, "u2=2^248": 1 << 248, "u2=n-1": N - 1,
            "u2=0xFF*31": (1 << 248) - 1}          # every window digit 0xFF below n (the top byte 0)


@functools.lru_cache(maxsize=None)
def shape_cases(bits):
    """(c) u1 = 0 (z = 0), u2 with a single window / n − 1 / all-0xFF bytes, u1 with only its top window: whole lanes hold
    no point and carry ∞ into the join.  The same rows serve every width (width 0)."""
    rng = random.Random(0x5A9E + bits)
    top = 256 - bits
    u1s = {"u1=0": lambda: 0, "u1=rand": lambda: rng.randrange(1, N),
           "u1=top-window": lambda: rng.randrange(1, N >> top) << top}
    u2s = dict(u2_shapes(), **{"u2=rand": None})
    out = []
    for n2, u2v in u2s.items():
        for n1, f1 in u1s.items():
            if u2v is None and n1 == "u1=rand":
                continue
            while True:
                u1, u2, q = f1(), u2v or rng.randrange(1, N), rng.randrange(1, N)
                row = make_valid(u1, u2, q)
                if row is not None and int.from_bytes(row[1][32:64], "big") <= N // 2:
                    break
            out.append(_finish(f"shape/{n1}/{n2}", 0, bits, u1, u2, q, row, rng))
    return tuple(out)


def cases_for(width, bits):
    return targeted_cases(width, bits) + shape_cases(bits)


# ---- x = r + n ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def r_plus_n_case():
    """A seal whose true nonce point has x = r + n (r < p − n), claimed by the key it was made with: R′ = (r + n, y), so
    the exact compare R′.x = r rejects it — a compare mod n (libsecp256k1's verify) would accept it.  The key has no
    private key: `teach` is a recovery-valid seal of it (R = a·G + b·Q, r = R.x, s = r/b, z = a·s)."""
    rng = random.Random(0xA11 + 7)
    r = 5
    while True:
        r += rng.randrange(1, 1 << 60)
        assert r < P - N
        x = r + N
        y2 = (pow(x, 3, P) + 7) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P != y2:
            continue
        s = rng.randrange(1, N // 2)               # low s: the strict policy does not hide the compare
        z = rng.randrange(1, N)
        rinv = pow(r, -1, N)
        Q = R.pt_add(R.pt_mul(s * rinv % N, (x, y)), R.pt_mul((-z * rinv) % N, R.G))
        break
    pub, addr = R.pub_bytes(Q), R.address(Q)
    u1, u2 = z * pow(s, -1, N) % N, r * pow(s, -1, N) % N
    Rp = R.pt_add(R.pt_mul(u1, R.G), R.pt_mul(u2, Q))
    assert Rp == (x, y) and Rp[0] == r + N         # the kernel's R′ really is the x = r + n point
    h, sig = b32(z), b32(r) + b32(s) + bytes([y & 1])
    c = Case("x=r+n", 0, 0, u1, u2, None, pub, addr, h, sig)
    c.expect = {fl: verdict(h, sig, addr, fl) for fl in (0, 1)}
    assert c.expect == {0: False, 1: False}
    while True:                                    # the seal that teaches the device this key
        a, b = rng.randrange(1, N), rng.randrange(1, N)
        T = R.pt_add(R.pt_mul(a, R.G), R.pt_mul(b, Q))
        if T is None or T[0] >= N:
            continue
        rt = T[0]
        st = rt * pow(b, -1, N) % N
        if st > N // 2:
            continue
        c.teach = (b32(a * st % N), b32(rt) + b32(st) + bytes([T[1] & 1]))
        break
    assert verdict(*c.teach, addr, 1)
    return c


# ---- the rows around a case ---------------------------------------------------------------------------------------

def twins(c, other):
    """(name, hash, sig, claimed case) of the rows next to a crafted one: v flipped, the high-s twin (s → n − s, v
    flipped: the same key recovers, refused under the strict policy), and the row claimed by another key"""
    s = int.from_bytes(c.sig[32:64], "big")
    return [("v^1", c.hash, c.sig[:64] + bytes([c.sig[64] ^ 1]), c),
            ("high-s", c.hash, c.sig[:32] + b32(N - s) + bytes([c.sig[64] ^ 1]), c),
            ("other-key", c.hash, c.sig, other)]


def coverage(cases, width):
    """{(op, level, kind)} that the targeted cases of a width force (the self-check of each case asserted them)"""
    return {c.target for c in cases if c.target and c.width == width}


def required(width, bits):
    """what coverage() must hold: equal and opposite operands in a mixed addition and at every butterfly level"""
    lanes, join = split(width)
    want = {("madd", None, k) for k in ("same", "opposite")}
    want |= {("join", lev, k) for lev in range(len(join)) for k in ("same", "opposite")}
    return want
