"""The warm kernels at every lane width on crafted edge rows (tests/warm_cases.py).

Once every validator's key is known, verify_known_lane_kernel (G = 1), verify_known_group_kernel<·,G> (G = 2 … 32) or
verify_known_wave_kernel (G = 64) decides every row.  Each width splits the 32 + 256/GTAB_BITS table points of
R′ = u1·G + u2·Q its own way; the rows built for a width make one addition of that split — a mixed addition inside a lane,
or a butterfly level, first and last pair — meet equal or opposite operands, leave whole lanes empty, or give R′ = ∞.
Between them: honest rows and the crafted rows' twins, so that some lanes of a wavefront take the rare branch and others
do not; the batch ends with a crafted row at a size that leaves idle groups.  Verdicts and tally must equal the oracle's
row by row, and last_dispatch() must show that the warm kernel of the width decided every row."""
import ctypes as C
import functools

import numpy as np
import pytest

import warm_cases as WC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _library_bits():
    import go_ibft_amd.build as B
    dt = C.CDLL(B.build_devtest())
    nw, ne, nb = C.c_int(), C.c_int(), C.c_int()
    dt.devtest_gtab_dims(C.byref(nw), C.byref(ne), C.byref(nb))
    assert nw.value * nb.value == 256 and ne.value == 1 << nb.value
    return nb.value


@functools.lru_cache(maxsize=None)
def _honest():
    from oracle import workload as W
    return W.make_round(16, 6161, with_envelopes=True)


def _u8(rows, width):
    return np.array([np.frombuffer(x, np.uint8) for x in rows]).reshape(-1, width)


class _Set:
    """validators (honest round + every crafted key + the x = r + n key), the seals that teach their keys, and the rows
    of one warm batch: per crafted row [row, honest, v^1, high-s, honest, other key], the x = r + n rows, a crafted row last"""

    def __init__(self, oracle, cases):
        r = _honest()
        rpn = WC.r_plus_n_case()
        self.cases, self.rpn = cases, rpn
        keyed = {c.addr: c for c in cases}
        assert len(keyed) == len(cases)
        self.addrs = np.concatenate([r.addrs, _u8([c.addr for c in cases] + [rpn.addr], 20)])
        assert len(np.unique(self.addrs, axis=0)) == len(self.addrs) <= 256
        self.vs = oracle.ValSet(self.addrs, np.ones(len(self.addrs), np.uint64))
        th, ts, tf = [], [], []
        for c in cases:
            d = oracle.keccak256(b"teach" + c.addr)
            th.append(d); ts.append(oracle.sign(WC.b32(c.q), d)); tf.append(c.addr)
        th.append(rpn.teach[0]); ts.append(rpn.teach[1]); tf.append(rpn.addr)
        self.teach = (np.concatenate([r.hash32, _u8(th, 32)]), np.concatenate([r.seal65, _u8(ts, 65)]),
                      np.concatenate([r.signer20, _u8(tf, 20)]))
        h, s, f = [], [], []
        j = 0

        def honest():
            nonlocal j
            j += 1
            k = j % r.n
            h.append(r.hash32[k].tobytes()); s.append(r.seal65[k].tobytes()); f.append(r.signer20[k].tobytes())
        self.at = []                                  # where each crafted row sits in the batch
        for i, c in enumerate(cases):
            tw = {t[0]: t for t in WC.twins(c, cases[(i + 1) % len(cases)])}
            self.at.append(len(h))
            h.append(c.hash); s.append(c.sig); f.append(c.addr)
            honest()
            for name in ("v^1", "high-s"):
                h.append(tw[name][1]); s.append(tw[name][2]); f.append(tw[name][3].addr)
            honest()
            h.append(tw["other-key"][1]); s.append(tw["other-key"][2]); f.append(tw["other-key"][3].addr)
            if i == len(cases) // 2:
                for v in (0, 1):                      # the x = r + n seal, claimed by the key it was made with
                    h.append(rpn.hash); s.append(rpn.sig[:64] + bytes([rpn.sig[64] ^ v])); f.append(rpn.addr)
        if len(h) % 2 == 1:
            honest()
        h.append(cases[0].hash); s.append(cases[0].sig); f.append(cases[0].addr)   # odd size, a crafted row last
        self.rows = (_u8(h, 32), _u8(s, 65), _u8(f, 20))
        assert len(h) % 2 == 1

    def teach_keys(self, bv):
        for _ in range(4):
            bv.is_valid_committed_seal(*self.teach)
            if bv.cache_stats()[0] == len(self.addrs):
                break
        assert bv.cache_stats()[0] == len(self.addrs)

    def check(self, oracle, bv, rows, flags, G):
        got, t = bv.is_valid_committed_seal(*rows)
        exp = oracle.verify_seals(self.vs, *rows, flags=flags & 1, nthreads=16).astype(bool)
        bad = np.nonzero(got != exp)[0]
        assert not len(bad), (G, flags, bad[:8], [self._name(rows, i) for i in bad[:8]])
        te = oracle.tally(self.vs, rows[2], exp.astype(np.uint8))
        assert (t.power, t.valid_rows, t.distinct_senders, t.has_quorum) == \
               (te.power, te.valid_rows, te.distinct_senders, te.has_quorum)
        assert bv.last_dispatch() == (0, G), bv.last_dispatch()
        return got

    def _name(self, rows, i):
        for c in self.cases:
            if rows[1][i].tobytes()[:64] == c.sig[:64]:
                return c.name
        return "?"


@functools.lru_cache(maxsize=None)
def _set_for(oracle, widths):
    bits = _library_bits()
    cases = tuple(c for w in widths for c in WC.targeted_cases(w, bits)) + WC.shape_cases(bits)
    return _Set(oracle, cases)


def _ctx(flags, **kw):
    import go_ibft_amd.verifier as V
    return V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE | flags, max_rows=65536, **kw)


@pytest.mark.parametrize("flags", [0, 1], ids=["flags0", "strict"])
@pytest.mark.parametrize("G", WC.WIDTHS)
def test_warm_width_on_crafted_rows(oracle, monkeypatch, G, flags):
    S = _set_for(oracle, (G,))
    assert WC.coverage(S.cases, G) == WC.required(G, _library_bits())
    monkeypatch.setenv("IBFT_WARM_LANES", str(G))
    bv = _ctx(flags)
    try:
        bv.set_validators(1, S.addrs, np.ones(len(S.addrs), np.uint64))
        S.teach_keys(bv)
        got = S.check(oracle, bv, S.rows, flags, G)
        # the builder's verdicts (pyref = C oracle) for the crafted rows themselves
        for i, c in zip(S.at, S.cases):
            assert got[i] == c.expect[flags & 1], c.name
        print(f"G={G} flags={flags}: {len(got)} rows, {int(got.sum())} valid, last_dispatch={bv.last_dispatch()}")
        # MODE 1 of the same kernels: envelopes (z is a Keccak hash: nothing to craft), intact and tampered
        r = _honest()
        assert r.off[0] == 0 and r.off[-1] == len(r.payload)
        payload = r.payload + r.payload
        off = np.concatenate([r.off[:-1], r.off + len(r.payload)])
        sig = np.concatenate([r.msg_sig65, r.msg_sig65])
        frm = np.concatenate([r.signer20, r.signer20])
        sig[r.n::3, 64] ^= 1
        sig[r.n + 1::3, 40] ^= 0x10
        frm[r.n + 2::3] = np.roll(r.signer20, 1, axis=0)[2::3]
        senders, _ = bv.is_valid_validator(payload, off, sig, frm)
        es = oracle.verify_senders(S.vs, payload, off, sig, frm, flags=flags & 1).astype(bool)
        assert (senders == es).all() and es[:r.n].all() and not es[r.n:].any()
        assert bv.last_dispatch() == (0, G)
    finally:
        bv.close()


AUTO_SIZES = {1024: 64, 1025: 32, 2048: 32, 2049: 16, 4096: 16, 4097: 8, 8192: 8, 8193: 4, 16384: 4, 16385: 2,
              32768: 2, 32769: 1}


def test_auto_width_at_the_rule_boundaries(oracle):
    """no knob: the crafted rows of every width tiled to both sides of each boundary of the width rule (n·G ≤ 65 536);
    the width the rule gives decides every row; kernel=KERNEL_LANE pins 1, kernel=KERNEL_WAVE 64"""
    import go_ibft_amd.verifier as V
    S = _set_for(oracle, WC.WIDTHS)
    for kernel, sizes in ((V.KERNEL_AUTO, AUTO_SIZES), (V.KERNEL_LANE, {1025: 1}), (V.KERNEL_WAVE, {1025: 64})):
        bv = _ctx(0, kernel=kernel)
        try:
            bv.set_validators(1, S.addrs, np.ones(len(S.addrs), np.uint64))
            S.teach_keys(bv)
            for n, G in sizes.items():
                idx = np.arange(n) % len(S.rows[0])
                idx[-1] = 0                                    # a crafted row last
                S.check(oracle, bv, tuple(x[idx] for x in S.rows), 0, G)
        finally:
            bv.close()
