"""The long-level trees of tests/cert_cases.py (long_tree) are what tests/test_gpu_cert.py claims they are — conditions on the
INPUT, checked on the oracle's tree alone (oracle/wire_cert.py), no device: a level of exactly K rows, K on either side of the
scan's threshold (cert_scan_dev.h: CERT_SCAN_ONE_GROUP_MAX, read from the test library, which loads without a GPU), in which
every 1 024-row tile of cert_scan_tiles_kernel / cert_scan_apply_kernel has rows with children and deferred rows, the counts
differ across the first tile boundary, the last row has children, and more rows are deferred than one DPP-row verdict launch
takes."""
import ctypes as C

import pytest

import cert_cases as CC
from oracle import wire_cert as WC

DEFER_BYTES = 256         # wire_dev.h: TREE_DEFER_BYTES
ROWS_KERNEL_MAX = 8192    # ibftgpu.hip: rows_kernel_max — more deferred rows than this and their verdict launch is a group kernel


def threshold():
    import go_ibft_amd.build as B
    L = C.CDLL(B.build_devtest())
    L.devtest_cert_scan_threshold.restype = C.c_uint32
    return int(L.devtest_cert_scan_threshold())


def deferred(exp, k):
    return exp.rows[k] is not None and (bool(exp.nodes[k]["flags"] & WC.HAS_CERT) or exp.nodes[k]["len"] > DEFER_BYTES)


@pytest.mark.parametrize("shape", ["flat", "nested"])
@pytest.mark.parametrize("dk", [0, 1])
def test_long_level_is_what_the_gpu_tests_say(shape, dk):
    T = threshold()
    assert T == 8192, "LONG_LEVEL_SEED was searched for this threshold: search again (the conditions below say what for)"
    K = T + dk
    r, msgs, exp, (lo, hi) = CC.long_tree(shape, K)
    assert exp is not None and exp.n_rows <= CC.LONG_LEVEL_MAX_ROWS
    level = 0 if shape == "flat" else 1
    rows_of = [k for k in range(exp.n_rows) if exp.nodes[k]["level"] == level]
    assert rows_of == list(range(lo, hi)) and hi - lo == K                                  # the long level has exactly K rows
    below = [k for k in range(exp.n_rows) if exp.nodes[k]["level"] == level + 1]
    assert len(below) > T and max(nd["level"] for nd in exp.nodes) == level + 1            # the level below is long again, and the last
    kids = [exp.nodes[k]["n_children"] for k in range(lo, hi)]
    dfr = [deferred(exp, k) for k in range(lo, hi)]
    for t0 in range(0, K, 1024):
        assert any(kids[t0:t0 + 1024]) and any(dfr[t0:t0 + 1024]), t0
    assert kids[1023] != kids[1024] and kids[-1] > 0
    pal = CC.long_level_palette(r)
    seen = {exp.wire[exp.nodes[k]["off"]:exp.nodes[k]["off"] + exp.nodes[k]["len"]] for k in range(lo, hi)}
    assert len(set(pal)) == 8 and seen == set(pal)
    # the palette is what its comments say
    one = WC.expected_tree(pal, r.addrs)
    assert [one.nodes[k]["n_children"] for k in range(8)] == [0, 1, 2, 5, 0, 3, 4, 0]
    assert [deferred(one, k) for k in range(8)] == [False, True, True, True, True, True, True, False]
    assert one.status[7] == WC.NEEDS_HOST and one.rows[7] is None and one.status[:7] == [WC.OK] * 7
    assert [deferred(one, k) for k in range(8, one.n_rows)].count(True) == 1 and deferred(one, one.nodes[5]["first_child"])
    assert not all(one.sender_ok[one.nodes[6]["first_child"]:][:4]) and all(one.sender_ok[:7])
    # offsets of the long level's scan, and the two verdict launches
    carriers_before = sum(deferred(exp, k) for k in range(lo))
    assert (lo, carriers_before) == ((0, 0) if shape == "flat" else (4, 2))
    assert sum(deferred(exp, k) for k in range(exp.n_rows)) > ROWS_KERNEL_MAX
