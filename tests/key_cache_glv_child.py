"""One scenario of tests/test_gpu_qtab_glv.py, run in a process of its own: the key-cache pool's table form
(IBFT_QTAB_FORM) is read when the first context of a device is created, so only a fresh process picks it.

    python key_cache_glv_child.py REPOSITORY_ROOT SCENARIO [ARG]

The parent sets the environment; every scenario first checks that the pool really has the form it was started for.
Expectations come from the CPU oracle, from warm_glv_cases / key_cache_model and from a cold context of the same process,
never from the warm path under test.  A scenario that reports numbers prints one line `GLV_REPORT {json}`."""
import json
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
import key_cache_child as K  # noqa: E402
import key_cache_model as M  # noqa: E402

FORMS = {"wide": (0, 655360), "glv": (1, 174080)}
N_OVER = 1700                        # above the 1 638 slots a wide pool has for 1 GiB, below the 6 168 of a glv pool


def _V():
    import go_ibft_amd.verifier as V
    return V


def _form():
    return FORMS[os.environ.get("IBFT_QTAB_FORM", "wide")]


# ---- 1. every width on the crafted rows of the GLV point order -----------------------------------------------------------

def run_widths():
    import test_gpu_warm_edges as WE
    import warm_glv_cases as GC
    B, _ = K._oracle()
    V = _V()
    assert _form() == FORMS["glv"]
    bits = WE._library_bits()
    for G in GC.WIDTHS:
        cases = GC.cases_for(G, bits)
        assert GC.coverage(cases, G) == GC.required(G, bits)
        S = WE._Set(B, cases)
        os.environ["IBFT_WARM_LANES"] = str(G)                   # (read at ibft_ctx_create)
        for flags in (0, V.FLAG_STRICT_LOW_S):
            bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE | flags, max_rows=4096)
            try:
                assert bv.cache_form() == FORMS["glv"]
                bv.set_validators(1, S.addrs, np.ones(len(S.addrs), np.uint64))
                S.teach_keys(bv)                                 # one seal of each key
                got = S.check(B, bv, S.rows, flags, G)           # verdicts, every tally field, last_dispatch() == (0, G)
                for i, c in zip(S.at, S.cases):
                    assert got[i] == c.expect[flags & 1], c.name
                te = B.tally(S.vs, S.rows[2], got.astype(np.uint8))
                _, t = bv.is_valid_committed_seal(*S.rows)
                assert K.tally_fields(t) == K.tally_fields(te), (G, flags)
                print(f"G={G} flags={flags}: {len(got)} rows, {int(got.sum())} valid, dispatch {bv.last_dispatch()}")
            finally:
                bv.close()


# ---- 2. memory and budget ---------------------------------------------------------------------------------------------

def budget_inputs():
    part = [(N_OVER, 4100, 0, N_OVER)]
    rounds = [K.columns(part, 0), K.spoil(K.columns(part, 1), K.plan_small(N_OVER, 1)), K.spoil(K.columns(part, 2), K.plan_small(N_OVER, 2))]
    for c in rounds:
        c.exp, c.tally = K.expect(c)
    assert rounds[0].exp.all()
    return rounds


def run_budget():
    form, slot_bytes = _form()
    assert os.environ["IBFT_QTAB_BUDGET_GB"] == "1"
    rounds = budget_inputs()
    V = _V()
    bv = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=2048)
    try:
        assert bv.cache_form() == (form, slot_bytes)
        M.SLOT_BYTES = bv.cache_form()[1]                        # the model with the REPORTED slot size, in this process only
        model = M.KeyCacheModel(1 << 30)
        assert model.max_slots == (6168 if form else 1638)
        unslotted, _ = model.set_validators("a", rounds[0].addrs)
        assert len(unslotted) == max(0, N_OVER - model.max_slots)
        bv.set_validators(1, rounds[0].addrs, rounds[0].power)
        for k, c in enumerate(rounds):
            got, t = bv.is_valid_committed_seal(c.hash32, c.seal65, c.signer20, c.pre)
            assert (got == c.exp).all(), (k, np.flatnonzero(got != c.exp)[:8])
            assert K.tally_fields(t) == K.tally_fields(c.tally), k
            by, used, cap, _ = bv.cache_memory()
            model.check_capacity(used, cap, by)                  # slots in use and allocated, as the model predicts
            print(f"pass {k}: tables {bv.cache_stats()[0]}, dispatch {bv.last_dispatch()}, slots {used}/{cap}, {by} B")
        tables = bv.cache_stats()[0]
        cold, warm = bv.last_dispatch()
        if form:
            assert tables == N_OVER and used == N_OVER and (cold, warm) == (0, 32), (tables, used, cold, warm)  # all warm (AUTO: n·G ≤ 65 536)
        else:
            assert tables == 1638 and used == 1638 and cold != 0 and warm != 0, (tables, used, cold, warm)
        print("GLV_REPORT " + json.dumps({"form": form, "slot_bytes": slot_bytes, "device_bytes": by, "used": used, "cap": cap,
                                          "tables": tables}))
    finally:
        bv.close()


# ---- 3. growth, slot reuse, rotation: key_cache_child's sequences on a glv pool -------------------------------------

def run_lifecycle(which):
    assert _form() == FORMS["glv"]
    V = _V()
    probe = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=64)
    try:
        assert probe.cache_form() == FORMS["glv"]
    finally:
        probe.close()                                            # (the last context of the device: the pool goes with it)
    M.SLOT_BYTES = slot = FORMS["glv"][1]
    loose = M.KeyCacheModel.check_capacity                       # (its byte bound is the wide slot's: far too loose here)

    def check_capacity(self, used, cap, device_bytes):
        """… and the pool's bytes are those of `cap` glv slots: a table, a key (80 B) and a state (4 B) each, beside the G table"""
        loose(self, used, cap, device_bytes)
        assert cap * slot <= device_bytes <= M.G_TABLE_BYTES + cap * (slot + 84) + 4096, (device_bytes, cap)
    M.KeyCacheModel.check_capacity = check_capacity
    {"growth": K.run_growth, "recycle": K.run_recycle, "rotation": K.run_rotation}[which]()


# ---- 4. the other entry points: a glv pool against a cold context of the same process -------------------------------

def _pair(max_rows, height, addrs, power):
    V = _V()
    warm, cold = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=max_rows), V.BatchVerifier(flags=0, max_rows=max_rows)
    assert warm.cache_form() == FORMS["glv"]
    for bv in (warm, cold):
        bv.set_validators(height, addrs, power)
    return warm, cold


def _same(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), what
        elif isinstance(x, (list, tuple)):
            _same(x, y, what)
        elif hasattr(x, "_fields_"):
            assert bytes(x) == bytes(y), what
        else:
            assert x == y, (what, x, y)


def entry_messages():
    _, W = K._oracle()
    r = W.make_round(65, 7301, byzantine=True, weighted=True, with_envelopes=True)
    warm, cold = _pair(256, r.height, r.addrs, r.power)
    try:
        call = lambda bv: bv.verify_messages(r.payload, r.off, r.msg_sig65, r.signer20, r.hash32, r.hash_len, r.seal65,   # noqa: E731
                                             valid_pre=r.pre_flags, raw=r.raw, round_=r.round)
        want = call(cold)
        assert want[0].any() and want[1].any() and not want[1].all()
        for rep in range(3):
            _same(call(warm), want, ("verify_messages", rep))
        assert warm.cache_stats()[0] > 0 and warm.last_dispatch()[1] > 0          # the last call ran the warm kernel
    finally:
        warm.close(), cold.close()


def entry_block_seals_sets():
    B, W = K._oracle()
    import test_gpu_block_seals_sets as TS
    r = W.make_round(12, 7302, raw_len=64, weighted=True)
    a = r.addrs
    sets = [(1, a[0:8], [1] * 8), (2, a[2:10], [2] * 8), (3, a[4:12], [3] * 8)]
    bh = TS._block_hashes(5, 7302)
    plan = [(0, [0, 1, 2, 3, 4, 5]), (1, [2, 3, 4, 5, 6, 9]), (2, [4, 5, 6, 7, 10, 11, 0]), (0, [7, 8]), (1, [3, 4, 5, 6, 7, 8, 9])]
    bset = [p[0] for p in plan]
    off = np.concatenate([[0], np.cumsum([len(p[1]) for p in plan])]).astype(np.uint32)
    who_rows = [(i, b) for b, p in enumerate(plan) for i in p[1]]
    sig = np.array([np.frombuffer(B.sign(r.sks[i], bytes(bh[b])), np.uint8) for i, b in who_rows], np.uint8).reshape(-1, 65)
    sig[3, 40] ^= 0x55                                                            # a corrupted seal
    signer = np.array([a[i] for i, _ in who_rows], np.uint8).reshape(-1, 20)
    V = _V()
    warm, cold = V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=1024), V.BatchVerifier(flags=0, max_rows=1024)
    try:
        assert warm.cache_form() == FORMS["glv"]
        for bv in (warm, cold):
            bv.set_validator_sets(sets)
        want = cold.verify_block_seals_sets(bh, off, bset, sig, signer)
        assert want[0].sum() == len(who_rows) - 3 and {t.has_quorum for t in want[1]} == {0, 1}     # a corrupted seal, two non-members
        for rep in range(3):
            _same(warm.verify_block_seals_sets(bh, off, bset, sig, signer), want, ("verify_block_seals_sets", rep))
        assert warm.last_dispatch()[1] > 0
    finally:
        warm.close(), cold.close()


def entry_judge():
    _, W = K._oracle()
    import cert_cases as CC
    r = W.make_round(7, 7303, height=5, round_=1, raw_len=48)
    msgs = [m.encode() for m in CC.honest_round_change_set(r, height=5, new_round=2)] + [CC.preprepare_with_rcc(r, height=5, new_round=2).encode()]
    buf, off = CC.pack(msgs)
    warm, cold = _pair(4096, 5, r.addrs, r.power)
    try:
        want = cold.judge_certificates_wire(buf, off, rows_cap=4096, per_row=True)
        assert want[1] > len(msgs)
        first = warm.judge_certificates_wire(buf, off, rows_cap=4096, per_row=True)      # learns the keys
        second = warm.judge_certificates_wire(buf, off, rows_cap=4096, per_row=True)     # a warm launch, then a cold one
        _same(first, want, "judge 1"), _same(second, want, "judge 2")
        assert warm.cache_stats()[0] > 0
    finally:
        warm.close(), cold.close()


def entry_pipeline():
    r = K.spoil(K.columns([(300, 7304, 0, 300)], 0), K.plan_small(300, 3))
    r.exp, r.tally = K.expect(r)
    warm, cold = _pair(1024, 1, r.addrs, r.power)
    try:
        for bv in (warm, cold):
            bv.seals_stage(r.hash32, r.seal65, r.signer20, r.pre)
        want = cold.seals_run()
        assert (want[0] == r.exp).all()
        for _ in range(3):
            warm.seals_run()                                                      # learn, build
        warm.seals_submit(), warm.seals_submit()                                  # two passes in flight
        a, b = warm.seals_collect(), warm.seals_collect()
        _same(a, want, "pass 1"), _same(b, want, "pass 2")
        assert warm.last_dispatch()[1] > 0
    finally:
        warm.close(), cold.close()


def run_entries():
    assert _form() == FORMS["glv"]
    for f in (entry_messages, entry_block_seals_sets, entry_judge, entry_pipeline):
        f()
        print(f"{f.__name__} ok")


# ---- 5. selecting the form ----------------------------------------------------------------------------------------------

def run_select(want):
    V = _V()
    if want == "bogus":
        import ctypes as C
        L = V.load_library()
        h = C.c_void_p()
        cfg = V.Cfg(0, V.FLAG_PUBKEY_CACHE, 64, V.KERNEL_AUTO)
        rc = L.ibft_ctx_create(C.byref(cfg), C.byref(h))
        L.ibft_last_error.restype = C.c_char_p
        assert rc == -1 and not h.value, rc                                       # IBFT_E_INVAL
        assert b"IBFT_QTAB_FORM" in L.ibft_last_error(None)
        try:
            V.BatchVerifier(flags=V.FLAG_PUBKEY_CACHE, max_rows=64)
        except Exception:
            return
        raise AssertionError("a context was created under IBFT_QTAB_FORM=bogus")
    for flags in (0, V.FLAG_PUBKEY_CACHE):
        bv = V.BatchVerifier(flags=flags, max_rows=64)
        try:
            assert bv.cache_form() == FORMS[want], bv.cache_form()
        finally:
            bv.close()


RUN = {"widths": run_widths, "budget": run_budget, "lifecycle": run_lifecycle, "entries": run_entries, "select": run_select}

if __name__ == "__main__":
    RUN[sys.argv[2]](*sys.argv[3:])
    print(f"KEY_CACHE_GLV_{sys.argv[2].upper()}_OK")
