"""One batch of tests/test_gpu_wire_views.py in a process of its own: IBFT_WIRE_VIEWS_SLOTS is read when a context is created
from the process environment, so the table-size hook is set for a fresh child and never for the test session.

    python wire_views_child.py REPOSITORY_ROOT CORPUS(a|c) VIEWS_CAP

The child checks every output against the model (tests/wire_views_cases.py: expected), calls a second time, and prints a marker
with the SHA-256 of all output bytes, which the parent compares with its own run at the default table size."""
import hashlib
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import wire_sets_cases as WS  # noqa: E402
import wire_views_cases as VC  # noqa: E402
import wire_views_harness as H  # noqa: E402

CORPORA = {"a": VC.corpus_a, "b": VC.corpus_b, "c": VC.corpus_c}


def install(bv, c, hmap=WS.MAP_A, with_proposers=True):
    (bv.set_validator_sets_u256 if c.big else bv.set_validator_sets)(c.sets())
    bv.set_height_sets(*hmap)
    p = VC.proposers(c)
    bv.set_proposers(p.height, p.first_round, np.frombuffer(b"".join(p.addrs), np.uint8).reshape(-1, 20) if with_proposers else [])


def output_bytes(out):
    """everything the call returned, as bytes"""
    got, rows, rset, vidx, tl, view, stored, views, n_views = out
    return b"".join([np.packbits(got).tobytes(), rows.tobytes(), rset.tobytes(), vidx.tobytes(), b"".join(bytes(t) for t in tl),
                     view.tobytes(), np.packbits(stored).tobytes(), views.tobytes(), int(n_views).to_bytes(4, "little")])


def check_model(out, e, cap, n):
    """out_view, out_stored, n_views and every record field against the model's answer e"""
    got, rows, rset, vidx, tl, view, stored, views, n_views = out
    assert got.tolist() == e["bits"] and rset.tolist() == e["set"] and vidx.tolist() == e["vidx"]
    assert n_views == e["n_views"] and len(views) == min(n_views, cap, n)
    assert view.tolist() == e["view"], np.nonzero(view != np.array(e["view"]))[0][:10]
    assert stored.tolist() == e["stored"], np.nonzero(stored != np.array(e["stored"]))[0][:10]
    for v, (r, w) in enumerate(zip(views, e["records"])):
        assert H.record_dict(r) == H.model_record(w), v


def main(root, name, cap):
    import go_ibft_amd.verifier as V
    c = CORPORA[name]()
    cap = int(cap)
    n = len(c.msgs)
    bv = V.BatchVerifier(max_rows=4096)
    try:
        install(bv, c)
        wire, off = WS.pack(c.msgs)
        out = bv.verify_senders_wire_views(wire, off, cap)
        check_model(out, VC.expected(c, WS.MAP_A, False, cap), cap, n)
        again = bv.verify_senders_wire_views(wire, off, cap)
        assert output_bytes(again) == output_bytes(out)
        print(f"WIRE_VIEWS_{name.upper()}_OK {hashlib.sha256(output_bytes(out)).hexdigest()}")
    finally:
        bv.close()


if __name__ == "__main__":
    main(*sys.argv[1:4])
