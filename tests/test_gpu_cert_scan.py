"""GPU: the level scans of the certificate tree (csrc/cert_scan_dev.h) on count columns of their own, through the test library
(devtest_cert_scan: the product's kernels and the product's launch geometry) — cert_scan_kernel, one workgroup, and
cert_scan_tiles_kernel → cert_scan_offsets_kernel → cert_scan_apply_kernel, the form of a long level — each against a plain
prefix sum in 64-bit integers, compared exactly:

    first_child[i]             = base + Σ_{j<i} (c[j] & 0x7FFFFFFF)          every row, leaves included
    deferred_rows[slot_base:]  = lo + nonzero(c >> 31), ascending
    totals                     = the two sums, on the device and in the host's words

Both forms run at every size (the host's threshold only says which one the library takes), so they equal each other too.  The
buffers carry sentinel cells around everything the kernels may write; with no host words the device totals are the same."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ONE_GROUP, TILED = 0, 1
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def dt():
    import go_ibft_amd.build as B
    L = C.CDLL(B.build_devtest())
    L.devtest_cert_scan_threshold.restype = C.c_uint32
    vp = C.c_void_p
    L.devtest_cert_scan.argtypes = [C.c_int, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp, vp, vp]
    return L


def scan(dt, form, c, lo, base, slot_base, host_words=True):
    n = len(c)
    first = np.zeros(n, np.uint32)
    rows = np.zeros(n, np.uint32)
    td, th, changed = np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = dt.devtest_cert_scan(form, n, p(c), lo, base, slot_base, int(host_words), p(first), p(rows), p(td), p(th), p(changed))
    assert rc == 0, ("HIP status", rc)
    return first, rows, td, th, int(changed[0])


def columns(n, seed):
    """(label, uint32 count column with bit 31 = deferred)"""
    rng = np.random.default_rng(seed)
    D = np.uint32(1 << 31)
    out = [("zeros", np.zeros(n, np.uint32)), ("ones", np.ones(n, np.uint32)),
           ("all deferred, 0", np.full(n, D, np.uint32)), ("all deferred, 1", np.full(n, D | np.uint32(1), np.uint32)),
           ("random 0..5, a third deferred", rng.integers(0, 6, n, dtype=np.uint32) | (D * (rng.random(n) < 1 / 3).astype(np.uint32)))]
    for at in sorted({0, 1023, 1024, n - 1}):
        if at < n:
            one = np.zeros(n, np.uint32)
            one[at] = D | np.uint32(3)
            out.append((f"one row, {at}", one))
    tiles = np.zeros(n, np.uint32)
    tiles[(np.arange(n) // 1024) % 2 == 1] = D | np.uint32(3)
    out.append(("alternating tiles", tiles))
    # counts up to 2^16, as large as keeps base + total under 2^31: the sums cross 16 and 24 bits
    top = min(1 << 16, ((1 << 31) - 2 * n - 16) // n)
    out.append(("large counts", rng.integers(0, top + 1, n, dtype=np.uint32) | (D * (rng.random(n) < 0.5).astype(np.uint32))))
    return out


def check(dt, form, n):
    for label, c in columns(n, 1000 + n):
        c64 = c.astype(np.int64)
        cnt, dfr = c64 & 0x7FFFFFFF, c64 >> 31
        excl = np.cumsum(cnt) - cnt
        which = np.nonzero(dfr)[0]
        totals = [int(cnt.sum()), int(dfr.sum())]
        assert totals[0] + 2 * n + 16 < 1 << 31
        for lo, base, slot_base in ((0, 0, 0), (7, 7 + n, 345)):
            where = (("one group", "tiled")[form], n, label, lo, base, slot_base)
            first, rows, td, th, changed = scan(dt, form, c, lo, base, slot_base)
            assert changed == 0, (where, "sentinel cells changed", bin(changed))
            assert td.tolist() == totals, (where, "device totals", td.tolist(), totals)
            assert th.tolist() == td.tolist(), (where, "host totals", th.tolist())
            bad = np.nonzero(first.astype(np.int64) != base + excl)[0]
            assert bad.size == 0, (where, "first_child", int(bad[0]), int(first[bad[0]]), int(base + excl[bad[0]]))
            assert (rows[:which.size].astype(np.int64) == lo + which).all(), (where, "deferred rows")
            assert (rows[which.size:] == SENTINEL).all(), (where, "cells behind the deferred rows")
            first2, rows2, td2, _, changed2 = scan(dt, form, c, lo, base, slot_base, host_words=False)
            assert changed2 == 0 and td2.tolist() == totals, (where, "no host words", td2.tolist())
            assert (first2 == first).all() and (rows2 == rows).all(), (where, "no host words")


def sizes(dt, klass, form):
    T = int(dt.devtest_cert_scan_threshold())
    return {"small": [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049],
            "threshold": [T - 1, T, T + 1] + ([65536] if form == ONE_GROUP else []),   # 65 536: 64 rows per thread of the one workgroup
            "tiles": [1024 * 1024, 1024 * 1024 + 1]}[klass]                             # 1 025 tiles: a second pass of cert_scan_offsets_kernel


@pytest.mark.parametrize("klass", ["small", "threshold"])
def test_one_workgroup_scan(dt, klass):
    for n in sizes(dt, klass, ONE_GROUP):
        check(dt, ONE_GROUP, n)


@pytest.mark.parametrize("klass", ["small", "threshold", "tiles"])
def test_tiled_scan(dt, klass):
    for n in sizes(dt, klass, TILED):
        check(dt, TILED, n)
