"""The colliding validator sets (tests/valset_collision_cases.py) through the host-compiled device source: valset_lookup behind
emit_row and claim_row (recover_dev.h), over the table the harness builds as ibft_set_validators builds it.  Index and verdict
bit of every member, every outsider and every decoy equal the oracle's (its ValSet sorts and searches: no hash, no probing);
the Python model the corpora were picked with is checked against the compiled addr_hash and table here as well.

A lookup that compared four of the five words, masked the wrap wrongly or stopped a probe early fails here."""
import ctypes as C

import numpy as np
import pytest

import valset_collision_cases as VC

NAMES = sorted(VC.CORPORA)


@pytest.fixture(scope="module")
def dev(oracle):
    import go_ibft_amd.build as B
    lib = C.CDLL(B.build_host_harness())
    lib.dev_addr_hash.restype = C.c_uint32
    lib.dev_valset_table.restype = C.c_uint32
    lib.dev_gtab_init()
    return lib


def _emit(dev, addrs_col, n, h, sig, flags=0, pre=0):
    out = C.create_string_buffer(20)
    vi = C.c_int32(-7)
    bit = dev.dev_emit_row(h, sig, flags, pre, addrs_col.ctypes.data_as(C.c_void_p), n, out, C.byref(vi))
    return bool(bit), vi.value, out.raw


def _claim(dev, addrs_col, n, h, sig, claimed, flags=0, pre=0):
    vi = C.c_int32(-7)
    bit = dev.dev_claim_row(h, sig, flags, pre, addrs_col.ctypes.data_as(C.c_void_p), n, claimed, C.byref(vi))
    return bool(bit), vi.value


def _seal(oracle, vs, h, sig, claimed):
    f = lambda b: np.frombuffer(b, np.uint8)
    return int(oracle.verify_seals(vs, f(h), f(sig), f(claimed))[0])


def _want_index(oracle, vs, addrs, a):
    """the oracle decides membership; the position a member is numbered with is its first place in the list"""
    member = vs.index(a) >= 0
    assert member == (a in addrs)
    return VC.list_index(addrs, a) if member else -1


def test_model_hash_is_the_device_hash(dev):
    rng = np.random.default_rng(5)
    sample = [rng.bytes(20) for _ in range(500)] + [VC.ZERO, b"\xff" * 20]
    for name in NAMES:
        c = VC.CORPORA[name]()
        sample += list(c.addrs) + [o.addr for o in c.outsiders]
    for a in sample:
        assert dev.dev_addr_hash(a) == VC.addr_hash(a), a.hex()


@pytest.mark.parametrize("name", NAMES)
def test_model_table_is_the_harness_table(dev, name):
    """slot for slot: address words and index + 1, zeros where the model has nothing"""
    c = VC.CORPORA[name]()
    col = VC.addr_column(c.addrs)
    tab = np.full(256 * 6, 0xA5A5A5A5, dtype=np.uint32)
    slots = dev.dev_valset_table(col.ctypes.data_as(C.c_void_p), len(c.addrs), tab.ctypes.data_as(C.c_void_p), 256)
    mslots, table = VC.build_table(c.addrs)
    assert slots == mslots == c.slots
    for s in range(slots):
        got = tab[6 * s:6 * s + 6].tolist()
        assert got == ([0] * 6 if table[s] is None else list(VC.words(table[s][0])) + [table[s][1] + 1]), s
    assert (tab[6 * slots:] == 0xA5A5A5A5).all()


@pytest.mark.parametrize("name", NAMES)
def test_lookup_of_every_address(dev, oracle, name):
    c = VC.CORPORA[name]()
    col = VC.addr_column(c.addrs)
    vs = oracle.ValSet(col, c.powers)
    for a in list(c.addrs) + [o.addr for o in c.outsiders]:
        assert dev.dev_valset_lookup(col.ctypes.data_as(C.c_void_p), len(c.addrs), a) == _want_index(oracle, vs, c.addrs, a), a.hex()


@pytest.mark.parametrize("name", NAMES)
def test_emit_and_claim_rows(dev, oracle, name):
    """every row of the corpus: emit_row names the recovered signer and ITS index; claim_row looks the CLAIMED address up —
    a member's seal under a decoy's name finds the decoy in the table and is still refused"""
    c = VC.CORPORA[name]()
    col = VC.addr_column(c.addrs)
    n = len(c.addrs)
    vs = oracle.ValSet(col, c.powers)
    rws = VC.rows(name)
    hs, sigs, claimed = VC.columns(rws)
    want_bits = oracle.verify_seals(vs, hs, sigs, claimed).astype(bool)
    assert want_bits.sum() == len(c.keys) and not want_bits.all()
    for r, want in zip(rws, want_bits):
        rec = oracle.recover_address(r.hash, r.sig)
        bit, vi, addr = _emit(dev, col, n, r.hash, r.sig)
        wi = _want_index(oracle, vs, c.addrs, rec) if rec is not None else -1
        assert (bit, vi, addr) == (wi >= 0, wi, rec or VC.ZERO), (r.what, r.claimed.hex())
        cbit, cvi = _claim(dev, col, n, r.hash, r.sig, r.claimed)
        assert (cbit, cvi) == (bool(want), _want_index(oracle, vs, c.addrs, r.claimed)), (r.what, r.claimed.hex())
        # pre-flagged: nothing is emitted, nothing is accepted; the claimed address is still looked up
        assert _emit(dev, col, n, r.hash, r.sig, pre=1) == (False, -1, VC.ZERO)
        assert _claim(dev, col, n, r.hash, r.sig, r.claimed, pre=1) == (False, cvi)


def test_decoy_sets_without_the_signer(dev, oracle):
    """the reverse of a seal under a decoy's name: the set lists the ten decoys and NOT A.  A's seal under its own name
    recovers A, finds ten entries one word away in A's bucket, and is refused; under a decoy's name the claimed address is a
    member and the recovered one is not it"""
    c = VC.decoys()
    addrs = list(c.decoys + c.bit_decoys)
    col = VC.addr_column(addrs)
    vs = oracle.ValSet(col, [1] * len(addrs))
    h = VC.digest(b"decoys-only")
    sig = oracle.sign(c.keys[c.A], h)
    assert oracle.recover_address(h, sig) == c.A and vs.index(c.A) == -1
    assert _emit(dev, col, len(addrs), h, sig) == (False, -1, c.A)
    assert _claim(dev, col, len(addrs), h, sig, c.A) == (False, -1)
    for i, d in enumerate(addrs):
        assert _seal(oracle, vs, h, sig, d) == 0
        assert _claim(dev, col, len(addrs), h, sig, d) == (False, i)
    # each decoy ALONE with A: the lookup of A must pass the decoy whichever word tells them apart
    for d in addrs:
        for order in ([d, c.A], [c.A, d]):
            col2 = VC.addr_column(order)
            vs2 = oracle.ValSet(col2, [1, 2])
            assert _seal(oracle, vs2, h, sig, c.A) == 1
            assert _emit(dev, col2, 2, h, sig) == (True, order.index(c.A), c.A)
            assert _claim(dev, col2, 2, h, sig, c.A) == (True, order.index(c.A))
            assert _claim(dev, col2, 2, h, sig, d) == (False, order.index(d))


@pytest.mark.parametrize("name", NAMES)
def test_rows_that_recover_nothing_against_a_set_with_the_zero_address(dev, oracle, name):
    """emit_row stores zeros for a row without a key; the zero address being a MEMBER must not turn that into a signer"""
    c = VC.CORPORA[name]()
    addrs = list(c.addrs) if VC.ZERO in c.addrs else list(c.addrs[:-1]) + [VC.ZERO]      # (the same slot count)
    assert VC.slots_for(len(addrs)) == c.slots
    col = VC.addr_column(addrs)
    vs = oracle.ValSet(col, [1] * len(addrs))
    zi = _want_index(oracle, vs, addrs, VC.ZERO)
    assert zi >= 0
    nothing = [r for r in VC.rows(name) if r.what == "nothing"]
    assert len(nothing) == 2 and {r.sig[64] for r in nothing} == {2, nothing[1].sig[64]} and nothing[1].sig[:32] == bytes(32)
    for r in nothing:
        assert oracle.recover_address(r.hash, r.sig) is None and _seal(oracle, vs, r.hash, r.sig, VC.ZERO) == 0
        assert _emit(dev, col, len(addrs), r.hash, r.sig) == (False, -1, VC.ZERO)
        assert _claim(dev, col, len(addrs), r.hash, r.sig, VC.ZERO) == (False, zi)
