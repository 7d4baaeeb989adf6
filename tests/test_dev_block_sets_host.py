"""The per-row decision of block_tally_kernel under a family of sets (recover_dev.h: valset_lookup over the union table, valsets_set_index,
valsets_row), compiled for the host (csrc/host_block_sets_harness.hip), against a Python restatement that knows nothing of
tables: a set is an ordered list of (address, power) in which a repeated address keeps its FIRST position and its LAST power,
and the index of an address in a set is its position among the distinct addresses — or −1.  Families are built to hit: an
address in several sets at different positions, in the union but not in the asked set, repeated inside one set's list,
hash-table collisions and long probe chains (many addresses in the smallest table the layout allows), and the union index that
sits in the table's last slot."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def dev():
    import go_ibft_amd.build as build
    L = C.CDLL(build.build_block_sets_harness())
    vp = C.c_void_p
    L.bsh_addr_hash.argtypes = [vp]
    L.bsh_addr_hash.restype = C.c_uint32
    L.bsh_lookup.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp]
    L.bsh_lookup.restype = None
    L.bsh_rows.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.bsh_rows.restype = None
    return L


M32 = 0xFFFFFFFF


def addr_hash(addr20: bytes) -> int:
    """recover_dev.h: addr_hash, restated"""
    a = np.frombuffer(addr20, "<u4").tolist()
    h = (a[0] * 0x9E3779B1) & M32
    for sh, word, mul in ((15, a[1], 0x85EBCA77), (13, a[2], 0xC2B2AE3D), (16, a[3], 0x27D4EB2F), (15, a[4], 0x165667B1)):
        h = ((h ^ (h >> sh)) + word * mul) & M32
    return h ^ (h >> 16)


class Family:
    """the restatement: sets as Python lists; the tables the library would build from them (union in order of first appearance,
    open addressing with linear probing, 6 words per slot, tag = union index + 1)"""

    def __init__(self, sets, slots=None):
        self.sets = []      # per set: [address bytes …] distinct, in order of first position
        self.power = []     # per set: {address: last power}
        self.union = []
        for lst in sets:
            order, pw = [], {}
            for a, p in lst:
                if a not in pw:
                    order.append(a)
                pw[a] = p
                if a not in self.union:
                    self.union.append(a)
            self.sets.append(order)
            self.power.append(pw)
        nu = len(self.union)
        if slots is None:
            slots = 64
            while slots < 2 * nu + 2:
                slots <<= 1
        assert slots & (slots - 1) == 0 and slots > nu
        self.slot_mask = slots - 1
        self.vtab = np.zeros((slots, 6), np.uint32)
        self.probes = 0
        self.slot_of = {}
        for u, a in enumerate(self.union):
            s = addr_hash(a) & self.slot_mask
            while self.vtab[s, 5] != 0:
                s = (s + 1) & self.slot_mask
                self.probes += 1
            self.vtab[s, :5] = np.frombuffer(a, "<u4")
            self.vtab[s, 5] = u + 1
            self.slot_of[a] = s
        self.setidx = np.full((len(sets), max(nu, 1)), -1, np.int32)
        for s, order in enumerate(self.sets):
            for i, a in enumerate(order):
                self.setidx[s, self.union.index(a)] = i
        self.n_union = nu

    def expect(self, s, a):
        """(index in set s, union index) with no table in sight"""
        return (self.sets[s].index(a) if a in self.sets[s] else -1, self.union.index(a) if a in self.union else -1)

    def lookup(self, dev, s, addrs):
        n = len(addrs)
        col = np.frombuffer(b"".join(addrs), np.uint8).copy()
        si = np.full(n, 99, np.int32)
        ui = np.full(n, 99, np.int32)
        dev.bsh_lookup(self.vtab.ctypes.data, self.slot_mask, self.setidx.ctypes.data, self.setidx.shape[1], s, col.ctypes.data, n,
                       si.ctypes.data, ui.ctypes.data)
        return list(zip(si.tolist(), ui.tolist()))


def _addrs(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        a = rng.bytes(20)
        if a not in out:
            out.append(a)
    return out


def test_hash_restatement_matches_the_device_source(dev):
    for a in _addrs(200, 1) + [bytes(20), b"\xff" * 20]:
        buf = np.frombuffer(a, np.uint8).copy()
        assert dev.bsh_addr_hash(buf.ctypes.data) == addr_hash(a)


def test_positions_and_membership_across_sets(dev):
    A = _addrs(12, 2)
    outsider = _addrs(3, 3)
    sets = [
        [(A[0], 5), (A[1], 6), (A[2], 7), (A[3], 8)],
        [(A[3], 1), (A[2], 2), (A[4], 3), (A[0], 4)],                  # the same addresses at other positions, other powers
        [(A[5], 9), (A[1], 1), (A[5], 2), (A[6], 3), (A[1], 7)],       # repeated inside the list: first position, last power
        [(A[11], 1)],
    ]
    f = Family(sets)
    assert f.sets[2] == [A[5], A[1], A[6]] and f.power[2] == {A[5]: 2, A[1]: 7, A[6]: 3}
    for s in range(len(sets)):
        got = f.lookup(dev, s, A + outsider)
        assert got == [f.expect(s, a) for a in A + outsider], s
    # spelled out: A[0] sits at 0 in set 0 and at 3 in set 1, is in the union but not in set 2; an outsider is nowhere
    assert f.lookup(dev, 0, [A[0]])[0] == (0, 0) and f.lookup(dev, 1, [A[0]])[0] == (3, 0)
    assert f.lookup(dev, 2, [A[0]])[0] == (-1, 0)
    assert f.lookup(dev, 2, [A[1], A[5]]) == [(1, 1), (0, 5)]
    assert f.lookup(dev, 3, outsider) == [(-1, -1)] * 3


def test_collisions_in_the_smallest_table(dev):
    # 63 addresses in 64 slots (the layout's smallest table, one empty slot left: what ends an unsuccessful probe)
    A = _addrs(63, 4)
    sets = [[(a, 1) for a in A[:40]], [(a, 2) for a in reversed(A[20:])], [(a, 3) for a in A[::3]]]
    f = Family(sets, slots=64)
    assert f.probes > 20, "the family was meant to collide"
    strangers = _addrs(40, 5)
    for s in range(3):
        assert f.lookup(dev, s, A + strangers) == [f.expect(s, a) for a in A + strangers]
    # a chain that wraps from the last slot to slot 0 is followed
    assert any(f.slot_of[a] < (addr_hash(a) & 63) for a in A), "no probe chain wrapped around"


def test_union_index_in_the_last_slot_and_last_union_index(dev):
    # search addresses until one hashes to the table's last slot, and make it the LAST address of the union
    pool = [a for a in _addrs(200, 6) if addr_hash(a) & 63 < 30][:30]   # (none of them near the last slot)
    assert len(pool) == 30
    rng = np.random.default_rng(7)
    while True:
        last = rng.bytes(20)
        if addr_hash(last) & 63 == 63 and last not in pool:
            break
    sets = [[(a, 1) for a in pool[:20]], [(a, 1) for a in pool[10:]] + [(last, 4)]]
    f = Family(sets)
    assert f.slot_mask == 63 and f.slot_of[last] == 63 and f.union[-1] == last
    assert f.lookup(dev, 1, [last])[0] == (20, 30)      # the last column of setidx, the last slot of the table
    assert f.lookup(dev, 0, [last])[0] == (-1, 30)


def test_row_decision(dev):
    A = _addrs(6, 8)
    f = Family([[(A[0], 1), (A[1], 1), (A[2], 1)], [(A[2], 1), (A[3], 1)]])
    #            bit  union index                         set 0: (si, bit, clear)        set 1
    cases = [(1, 0, (0, 1, 0), (-1, 0, 1)),     # member of set 0 only: kept there, CLEARED under set 1
             (1, 2, (2, 1, 0), (0, 1, 0)),      # member of both, at different indices
             (1, 3, (-1, 0, 1), (1, 1, 0)),
             (0, 1, (-1, 0, 0), (-1, 0, 0)),    # bit not set: the index column means nothing, nothing is loaded or cleared
             (0, 12345, (-1, 0, 0), (-1, 0, 0)),  # … whatever it holds
             (0, -1, (-1, 0, 0), (-1, 0, 0)),
             (1, -1, (-1, 1, 0), (-1, 1, 0))]   # a set bit without a member index is counted as valid and contributes no power
    bit = np.array([c[0] for c in cases], np.uint8)
    ui = np.array([c[1] for c in cases], np.int32)
    for s in (0, 1):
        si = np.full(len(cases), 99, np.int32)
        ob = np.full(len(cases), 99, np.uint8)
        oc = np.full(len(cases), 99, np.uint8)
        dev.bsh_rows(bit.ctypes.data, ui.ctypes.data, f.setidx.ctypes.data, f.setidx.shape[1], s, len(cases), si.ctypes.data,
                     ob.ctypes.data, oc.ctypes.data)
        assert list(zip(si.tolist(), ob.tolist(), oc.tolist())) == [c[2 + s] for c in cases], s
