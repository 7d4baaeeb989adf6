"""The safegcd inversions ON THE GPU on the searched corpus (tests/modinv_cases.py, tests/golden/modinv_edges.json).

Unit level: devtest_wave_modinv runs the gfx950 code object of modinv_wave_fn by itself — one value per wavefront, and
four different values in the four rows of a wavefront — and devtest_run's ops 3, 6 (the outlined modinv_rt_fn) and 9, 10
(modinv<MOD>) take the corpus one value per lane.  Product level: warm verdicts on valid seals whose s IS a corpus value,
cold recoveries of seals whose r is one, at every pinned kernel variant and at batch sizes that leave rows of a
wavefront finishing in different batches and padding rows idling.  Every expectation is pow(x, −1, M) or the oracle's.
(Z⁻¹ mod p cannot be steered from a signature: the corpus mod p is covered at the unit level only.)"""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import modinv_cases as MC
import warm_cases as WC

pytestmark = pytest.mark.gpu
N = MC.MODULI["n"]
MAX_ROWS = 512                      # rows per launch
SIZES = (1, 63, 64, 65)             # + the whole list; 1 and 65 leave a wavefront with a single live row at every width


@pytest.fixture(scope="module")
def dt():
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_devtest())
    L.devtest_run.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    L.devtest_wave_modinv.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
    return L


@functools.lru_cache(maxsize=None)
def _fix():
    return MC.load()


def _all_values(name):
    xs = list(MC.corpus_values(_fix(), name))
    for q in MC.corpus_quads(_fix(), name):
        xs += q
    return list(dict.fromkeys(xs))


def _wave(dt, which, layout, jobs):
    flat = jobs if layout == 0 else [v for q in jobs for v in q]
    out = C.create_string_buffer(2048 * len(jobs))
    assert dt.devtest_wave_modinv(which, layout, len(jobs), MC.pack(flat), out) == 0
    return out.raw


# ---- unit level ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p", "n"])
def test_wave_inversion_one_value_per_wavefront(dt, name):
    m = MC.MODULI[name]
    xs = _all_values(name) + MC.control(name)
    MC.check_wave_out(_wave(dt, MC.WHICH[name], 0, xs), [[x] * 4 for x in xs], m, "devtest_wave_modinv layout 0")


@pytest.mark.parametrize("name", ["p", "n"])
def test_wave_inversion_four_values_in_lockstep(dt, name):
    """every quadruple; every corpus value in each row beside three zeros and four times itself; random control"""
    m = MC.MODULI[name]
    ctl = MC.control(name)
    jobs = MC.corpus_quads(_fix(), name) + [p for x in _all_values(name) for p in MC.placements(x)] + \
        [ctl[i:i + 4] for i in range(0, len(ctl), 4)]
    MC.check_wave_out(_wave(dt, MC.WHICH[name], 1, jobs), jobs, m, "devtest_wave_modinv layout 1")


@pytest.mark.parametrize("name,ops", [("p", (3, 9)), ("n", (6, 10))])
def test_lane_inversions_on_the_corpus(dt, name, ops):
    """one value per lane: modinv_rt_fn through the fe / sc wrappers (ops 3, 6) and modinv<MOD> (ops 9, 10)"""
    m = MC.MODULI[name]
    xs = _all_values(name) + MC.control(name)
    a = MC.pack(xs)
    for op in ops:
        out = C.create_string_buffer(32 * len(xs))
        assert dt.devtest_run(op, len(xs), a, bytes(len(a)), out, 32 * len(xs)) == 0
        got = [int.from_bytes(out.raw[32 * i:32 * i + 32], "big") for i in range(len(xs))]
        bad = [hex(x) for x, g in zip(xs, got) if g != (pow(x, -1, m) if x else 0)]
        assert not bad, (op, bad[:4])


# ---- product level --------------------------------------------------------------------------------------------------------
def _u8(rows, width):
    return np.array([np.frombuffer(x, np.uint8) for x in rows]).reshape(-1, width)


def _batches(rows):
    """index lists: the sizes of SIZES as windows that together walk the whole list, then the list itself (≤ MAX_ROWS)"""
    n, at, out = len(rows), 0, []
    for size in SIZES:
        out.append([(at + i) % n for i in range(size)])
        at += size
    out.append(list(range(min(n, MAX_ROWS))))
    return out


@functools.lru_cache(maxsize=None)
def _warm_rows(strict):
    """valid seals of one key whose s is a corpus value mod n (z = s·k − r·sk), each followed by its twin with one bit of the
    signature flipped; strict: only s ≤ n/2"""
    from oracle import pyref as R
    rng = random.Random("modinv warm rows")
    sk = rng.randrange(1, N)
    Q = R.pt_mul(sk, R.G)
    addr = R.address(Q)
    rows = []
    for i, s in enumerate(x for x in _all_values("n") if x and (not strict or x <= N // 2)):
        while True:
            k = rng.randrange(1, N)
            X = R.pt_mul(k, R.G)
            if 0 < X[0] < N:
                break
        r = X[0]
        z = (s * k - r * sk) % N
        sig = WC.b32(r) + WC.b32(s) + bytes([X[1] & 1])
        twin = bytearray(sig)
        twin[(7 * i) % 64] ^= 1 << (i % 8)
        rows += [(WC.b32(z), sig, True), (WC.b32(z), bytes(twin), False)]
    return sk, addr, rows


@pytest.mark.parametrize("flags", [0, 1], ids=["flags0", "strict"])
@pytest.mark.parametrize("G", WC.WIDTHS)
def test_warm_verdicts_on_seals_whose_s_is_a_corpus_value(oracle, monkeypatch, G, flags):
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    sk, addr, rows = _warm_rows(bool(flags))
    assert len(rows) >= 2 * 16
    honest = W.make_round(16, 6262)
    addrs = np.concatenate([honest.addrs, _u8([addr], 20)])
    vs = oracle.ValSet(addrs, np.ones(len(addrs), np.uint64))
    d = oracle.keccak256(b"teach the modinv key")
    teach = (np.concatenate([honest.hash32, _u8([d], 32)]), np.concatenate([honest.seal65, _u8([oracle.sign(WC.b32(sk), d)], 65)]),
             np.concatenate([honest.signer20, _u8([addr], 20)]))
    h, s, f = _u8([r[0] for r in rows], 32), _u8([r[1] for r in rows], 65), _u8([addr] * len(rows), 20)
    monkeypatch.setenv("IBFT_WARM_LANES", str(G))
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE | flags, max_rows=4096)
    try:
        bv.set_validators(1, addrs, np.ones(len(addrs), np.uint64))
        for _ in range(4):
            bv.is_valid_committed_seal(*teach)
            if bv.cache_stats()[0] == len(addrs):
                break
        assert bv.cache_stats()[0] == len(addrs)
        for idx in _batches(rows):
            part = (h[idx], s[idx], f[idx])
            got, t = bv.is_valid_committed_seal(*part)
            exp = oracle.verify_seals(vs, *part, flags=flags & 1, nthreads=16).astype(bool)
            assert (got == exp).all(), (G, flags, len(idx), [s[idx[i]].tobytes()[32:64].hex() for i in np.nonzero(got != exp)[0][:4]])
            assert [bool(e) for e in exp] == [rows[i][2] for i in idx], "the rows are not what they were built to be"
            te = oracle.tally(vs, part[2], exp.astype(np.uint8))
            assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum) == (te.power, te.valid_rows, te.distinct_senders, te.has_quorum)
            assert bv.last_dispatch() == (0, G), bv.last_dispatch()
    finally:
        bv.close()


@functools.lru_cache(maxsize=None)
def _cold_rows():
    """seals whose r is a corpus value that is the x of a curve point, both parities, s and digest from the corpus and at random"""
    P = MC.MODULI["p"]
    rng = random.Random("modinv cold rows")
    on_curve = [x for x in _all_values("n") if 0 < x < N and pow((x * x * x + 7) % P, (P - 1) // 2, P) == 1]
    assert len(on_curve) >= 16
    ss = [x for x in _all_values("n") if x]
    rows, i = [], 0
    while len(rows) < 2 * 65:
        for r in on_curve:
            s = ss[i % len(ss)] if i % 3 else rng.randrange(1, N)
            rows.append((WC.b32(rng.randrange(1 << 256)), WC.b32(r) + WC.b32(s) + bytes([i & 1])))
            i += 1
    return rows[:MAX_ROWS]


@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 64, 128])
def test_cold_recovery_of_seals_whose_r_is_a_corpus_value(oracle, monkeypatch, lanes):
    import go_ibft_amd.verifier as V
    from oracle import workload as W
    rows = _cold_rows()
    h, s = _u8([r[0] for r in rows], 32), _u8([r[1] for r in rows], 65)
    exp = np.zeros((len(rows), 20), np.uint8)
    for i, (d, sig) in enumerate(rows):
        a = oracle.recover_address(d, sig, 0)
        assert a is not None, "r is on the curve and s ≠ 0: the oracle recovers some key"
        exp[i] = np.frombuffer(a, np.uint8)
    honest = W.make_round(16, 6262)
    monkeypatch.setenv("IBFT_COLD_LANES", str(lanes))
    bv = V.BatchVerifier(max_rows=4096)
    try:
        bv.set_validators(1, honest.addrs, honest.power)
        for idx in _batches(rows):
            got = bv.recover_seals(h[idx], s[idx], None)
            bad = np.nonzero((got[0] != exp[idx]).any(axis=1))[0]
            assert not len(bad), (lanes, len(idx), [rows[idx[i]][1][:32].hex() for i in bad[:4]])
            assert not got[2].any()          # nobody here is a validator
            assert bv.last_dispatch()[0] == lanes, bv.last_dispatch()
    finally:
        bv.close()
