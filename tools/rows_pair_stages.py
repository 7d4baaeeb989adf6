"""Where the rows pair's time goes (devtest build, product launch shape); run on the GPU box.
Usage: python tools/rows_pair_stages.py [n_rows=4096]

The pair kernel (devtest_rows_pair_kernel: recover_pubkey_row<…, PAIR> + recover_helper_row) stamps s_memrealtime on both
sides of its two workgroup barriers: per wavefront, the stage before barrier 1, the wait there, the stage between the
barriers, the wait at barrier 2 and the rest (a helper ends where it has published u1·G: "helper resident until" is how long
it holds its registers, next to the main wavefront's length); a second run whose main wavefronts stop behind the closing chain
(devtest_rows_pair_stamps_stop, STOP = 6) splits "after barrier 2" into closing chain and address hash.  Next to it, the single-wavefront form's stage deltas (devtest_rows_stage_ms:
launches cut short after each stage) — its main loop against the pair's main loop, which shares the SIMD with the helper."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import go_ibft_amd.build as build
from oracle import workload as W

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
L = C.CDLL(os.environ.get("DEVTEST_SO") or build.build_devtest())
r = W.make_round(n, 5)
dig, sig = r.hash32.tobytes(), r.seal65.tobytes()

ms = (C.c_float * 9)()
out = np.zeros((n, 24), np.uint8)
assert L.devtest_rows_stage_ms(n, dig, sig, ms, out.ctypes.data_as(C.c_void_p)) == 0
assert (out[:, 20] == 1).all() and (out[:, :20] == r.addrs).all(), "devtest rows kernel: wrong addresses"
st1 = [ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], ms[6]]
print(f"# single form (recover_pubkey_row), {n} rows, launches cut short after each stage, ms:")
for nm, a, b in [("R' + scalars (r^-1, u1, u2, GLV)", 0.0, st1[1]), ("tables", st1[1], st1[2]), ("main loop", st1[2], st1[3]),
                 ("16 G additions", st1[3], st1[4]), ("closing chain", st1[4], st1[5]), ("Keccak, compare", st1[5], st1[6])]:
    print(f"  {nm:36s} {b - a:7.4f}")
print(f"  {'complete':36s} {st1[6]:7.4f}")

blocks = n // 16
stamps = np.zeros(blocks * 8 * 8, np.uint64)
pms = C.c_float()
out[:] = 0
assert L.devtest_rows_pair_stamps(n, dig, sig, out.ctypes.data_as(C.c_void_p), stamps.ctypes.data_as(C.c_void_p), C.byref(pms)) == 0
assert (out[:, 20] == 1).all() and (out[:, :20] == r.addrs).all(), "devtest rows pair kernel: wrong addresses"
s = stamps.reshape(blocks, 8, 8).astype(np.int64)
us = lambda a, b: np.median(s[:, :, b] - s[:, :, a], axis=0) / 100.0     # 100 MHz ticks → µs, median over workgroups
main, helper = slice(0, 4), slice(4, 8)
print(f"# rows pair, {n} rows = {blocks} workgroups of 4 main + 4 helper wavefronts; kernel {pms.value:.4f} ms (devtest build)")
print("# median over workgroups, µs, per wavefront index 0-3 (main) / 4-7 (helper)")
# a helper publishes u1·G and ends: it never stands at barrier 2, its end stamp [5] closes "between the barriers"
row = lambda v: " ".join(f"{x:7.1f}" for x in v)
gone = " ".join(f"{'-':>7s}" for _ in range(4))
for nm, a, b, hb in [("before barrier 1", 0, 1, 1), ("wait at barrier 1", 1, 2, 2), ("between the barriers", 2, 3, 5),
                     ("wait at barrier 2", 3, 4, None), ("after barrier 2", 4, 5, None), ("whole wavefront", 0, 5, 5)]:
    print(f"  {nm:24s} main {row(us(a, b)[main])}   helper {row(us(a, hb)[helper]) if hb else gone}")
print(f"# main wavefront {us(0, 5)[main].mean():.1f} µs, helper resident until {us(0, 5)[helper].mean():.1f} µs")
print(f"# main: tables {us(0, 1)[main].mean():.1f} µs (single form {1000 * (st1[2] - st1[1]):.1f}), barrier-1 wait "
      f"{us(1, 2)[main].mean():.1f}, main loop {us(2, 3)[main].mean():.1f} (single form {1000 * (st1[3] - st1[2]):.1f}), barrier-2 wait "
      f"{us(3, 4)[main].mean():.1f}; helper: scalars {us(0, 1)[helper].mean():.1f}, G additions {us(2, 5)[helper].mean():.1f}")
if hasattr(L, "devtest_rows_pair_stamps_stop"):
    # the same launches with the main wavefronts ending behind the closing chain: what is left of "after barrier 2" is the hash
    st6 = np.zeros_like(stamps)
    pms6 = C.c_float()
    junk = np.zeros((n, 24), np.uint8)
    assert L.devtest_rows_pair_stamps_stop(6, n, dig, sig, junk.ctypes.data_as(C.c_void_p), st6.ctypes.data_as(C.c_void_p), C.byref(pms6)) == 0
    s6 = st6.reshape(blocks, 8, 8).astype(np.int64)
    chain = np.median(s6[:, :4, 5] - s6[:, :4, 4], axis=0) / 100.0
    tail = us(4, 5)[main]
    print(f"  {'  closing chain (STOP 6)':24s} main {' '.join(f'{x:7.1f}' for x in chain)}")
    print(f"  {'  Keccak, compare':24s} main {' '.join(f'{x:7.1f}' for x in tail - chain)}")
    print(f"# after barrier 2: closing chain {chain.mean():.1f} µs + Keccak, compare {(tail - chain).mean():.1f} µs; kernel without the hash "
          f"{pms6.value:.4f} ms, with it {pms.value:.4f} ms")
