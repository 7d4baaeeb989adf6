// devtest.hip — TEST-ONLY library (libibft_devtest.so): runs single arithmetic primitives of
// secp256k1_dev.h / modinv_dev.h ON THE GPU so tests/test_gpu_arith.py can compare the gfx950
// code object op by op with Python big integers.  Not part of libibftgpu.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "modinv_dev.h"
#include "recover_dev.h"
#include "secp256k1_dev.h"

using namespace secp;

__global__ void devtest_kernel(int op, int n, const uint8_t *a, const uint8_t *b, uint8_t *out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u256 x = from_be32(a + 32 * i), y = from_be32(b + 32 * i);
  u256 r = zero256();
  switch (op) {
    case 0: r = fe_to_u256(fe_mul(fe_from_u256(x), fe_from_u256(y))); break;
    case 1: r = fe_to_u256(fe_sqr(fe_from_u256(x))); break;
    case 2: r = fe_to_u256(fe_inv(fe_from_u256(x))); break;
    case 3: r = fe_to_u256(fe_inv_safegcd(fe_from_u256(x))); break;
    case 4: r = sc_canon(sc_mul(sc_from_u256(x), sc_from_u256(y))); break;
    case 5: r = sc_canon(sc_inv(sc_from_u256(x))); break;
    case 6: r = sc_canon(sc_inv_safegcd(sc_from_u256(x))); break;
    case 7: r = fe_to_u256(fe_sqrt_candidate(fe_from_u256(x))); break;
    case 8: {
      glv_split s = sc_split_lambda(x);
      r = s.k1;
      to_be32(out + 32 * (n + i), s.k2);
      out[64 * n + i] = (uint8_t)((s.neg1 ? 1 : 0) | (s.neg2 ? 2 : 0));
      break;
    }
    case 12: case 13: {  // x = number of doublings of G; out = affine x of 2^k G (12: Fermat, 13: safegcd)
      jac base = jac_from_aff(generator());
      for (uint32_t k = 0; k < x.v[0]; k++) base = jac_dbl(base);
      aff af;
      if (op == 12) jac_to_aff(af, base); else jac_to_aff_fast(af, base);
      r = l26_to_u256(af.x);
      break;
    }
    case 14: {  // gtab_entry(w = x.v[0], e = y.v[0]) -> x coordinate
      uint32_t ent[20];
      ibftk::gtab_entry((int)x.v[0], (int)y.v[0], ent);
      l26 t;
      for (int k = 0; k < 10; k++) t.n[k] = ent[k];
      r = l26_to_u256(t);
      break;
    }
    case 15: case 16: {  // x = k1, y = k2: affine x of k1·G + k2·G through jac_add (15) / jac_add_aff (16); 0 = infinity
      aff g = generator();
      jac p1 = ibftk::ecmult_var(g, x), p2 = ibftk::ecmult_var(g, y);
      jac sum;
      if (op == 15) {
        sum = jac_add(p1, p2);
      } else {
        aff a2;
        bool fin2 = jac_to_aff_fast(a2, p2);
        jac viaaff = jac_add_aff(p1, a2);
        sum = jac_select(fin2, viaaff, p1);  // an infinite q is not representable in affine form
      }
      aff af;
      bool fin = jac_to_aff_fast(af, sum);
      r = fin ? l26_to_u256(af.x) : zero256();
      break;
    }
    case 9: r = modinv<ModP>(x); break;
    case 10: r = modinv<ModN>(x); break;
    case 11: {  // one batch: divsteps + both updates, output d (as raw 9 limbs packed little-endian 36 B -> first 32)
      s30 d, e, f, g = s30_from_u256(x);
      for (int k = 0; k < 9; k++) { d.v[k] = 0; e.v[k] = 0; f.v[k] = ModN::limb(k); }
      e.v[0] = 1;
      trans2x2 t;
      int32_t zeta = divsteps_30(-1, (uint32_t)f.v[0], (uint32_t)g.v[0], t);
      update_de_30<ModN>(d, e, t);
      update_fg_30(f, g, t);
      r.v[0] = (uint32_t)t.u; r.v[1] = (uint32_t)t.v; r.v[2] = (uint32_t)t.q; r.v[3] = (uint32_t)t.r;
      r.v[4] = (uint32_t)zeta; r.v[5] = (uint32_t)f.v[0]; r.v[6] = (uint32_t)g.v[0]; r.v[7] = (uint32_t)e.v[0];
      break;
    }
  }
  to_be32(out + 32 * i, r);
}

__global__ void devtest_gtab_kernel(uint32_t *gtab) {
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES) return;
  ibftk::gtab_entry(tid / ibftk::GTAB_ENTRIES, tid % ibftk::GTAB_ENTRIES, gtab + (size_t)ibftk::GTAB_ENTRY_DWORDS * tid);
}
// digest (a), sig r (b), sig s (c), v: out = 20-byte address + ok flag, 32 B per row
__global__ void devtest_recover_kernel(int n, const uint32_t *gtab, const uint8_t *dig, const uint8_t *r,
                                       const uint8_t *s, const uint8_t *v, uint8_t *out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t addr[5];
  bool ok = ibftk::recover_address(gtab, from_be32(dig + 32 * i), from_be32(r + 32 * i), from_be32(s + 32 * i),
                                   v[i], 0, addr);
  for (int k = 0; k < 5; k++) reinterpret_cast<uint32_t *>(out + 32 * i)[k] = addr[k];
  out[32 * i + 20] = ok ? 1 : 0;
}
extern "C" int devtest_recover(int n, const uint8_t *dig, const uint8_t *r, const uint8_t *s, const uint8_t *v,
                               uint8_t *out, uint32_t *gtab_out) {
  uint8_t *dd, *dr, *ds, *dv, *dout;
  uint32_t *dg;
  size_t gbytes = (size_t)ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES * ibftk::GTAB_ENTRY_DWORDS * 4;
  if (hipMalloc(&dg, gbytes) != hipSuccess) return -1;
  (void)hipMalloc(&dd, 32 * n); (void)hipMalloc(&dr, 32 * n); (void)hipMalloc(&ds, 32 * n);
  (void)hipMalloc(&dv, n); (void)hipMalloc(&dout, 32 * n);
  (void)hipMemcpy(dd, dig, 32 * n, hipMemcpyHostToDevice); (void)hipMemcpy(dr, r, 32 * n, hipMemcpyHostToDevice);
  (void)hipMemcpy(ds, s, 32 * n, hipMemcpyHostToDevice); (void)hipMemcpy(dv, v, n, hipMemcpyHostToDevice);
  devtest_gtab_kernel<<<(ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES + 63) / 64, 64>>>(dg);
  devtest_recover_kernel<<<(n + 63) / 64, 64>>>(n, dg, dd, dr, ds, dv, dout);
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  (void)hipMemcpy(out, dout, 32 * n, hipMemcpyDeviceToHost);
  if (gtab_out) (void)hipMemcpy(gtab_out, dg, gbytes, hipMemcpyDeviceToHost);
  (void)hipFree(dd); (void)hipFree(dr); (void)hipFree(ds); (void)hipFree(dv); (void)hipFree(dout); (void)hipFree(dg);
  return rc;
}

extern "C" void devtest_gtab_dims(int *windows, int *entries, int *bits) {
  *windows = ibftk::GTAB_WINDOWS;
  *entries = ibftk::GTAB_ENTRIES;
  *bits = ibftk::GTAB_BITS;
}

extern "C" int devtest_run(int op, int n, const uint8_t *a, const uint8_t *b, uint8_t *out, int out_bytes) {
  uint8_t *da, *db, *dout;
  if (hipMalloc(&da, 32 * n) != hipSuccess) return -1;
  hipMalloc(&db, 32 * n);
  hipMalloc(&dout, out_bytes);
  hipMemcpy(da, a, 32 * n, hipMemcpyHostToDevice);
  hipMemcpy(db, b, 32 * n, hipMemcpyHostToDevice);
  hipMemset(dout, 0, out_bytes);
  devtest_kernel<<<(n + 63) / 64, 64>>>(op, n, da, db, dout);
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
  hipFree(da); hipFree(db); hipFree(dout);
  return rc;
}

// ---- wave_fe_dev.h primitives (one wavefront per job; same op numbers as host_wave_harness.hip) ----
#include "wave_fe_dev.h"

__global__ void __launch_bounds__(64) devtest_wave_fe_kernel(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  const wv::wk k = wv::wk_init();
  const uint32_t *ja = a + 40 * blockIdx.x, *jb = b + 40 * blockIdx.x;
  const uint32_t x = k.li < 10 ? ja[k.row * 10 + k.li] : 0u;
  const uint32_t y = k.li < 10 ? jb[k.row * 10 + k.li] : 0u;
  uint32_t r = 0;
  switch (op) {  // wave-uniform
    case 0: r = wv::wfe_mul(x, y, k); break;
    case 1: r = wv::wfe_weak(x, k); break;
    case 2: r = wv::wfe_neg1(x, k) + y; break;
    case 3: r = wv::wfe_neg2(x, k) + y; break;
    case 4: r = wv::wfe_neg8(x, k) + y; break;
    case 5: r = wv::wfe_sqrt_candidate(x, k); break;
    case 6: r = wv::scatter(wv::gather(x), k); break;
    case 7: r = wv::wfe_is_zero(x) ? 1u : 0u; break;
    case 8: r = wv::wfe_z_maybe_zero(wv::wfe_mul(x, y, k)) ? 1u : 0u; break;  // the additions' filter on Z3
  }
  out[64 * blockIdx.x + threadIdx.x] = r;
}
__device__ __forceinline__ wv::wjac devtest_load_pt(const uint32_t *src, const wv::wk &k) {
  const uint32_t *r = src + 31 * k.row;
  wv::wjac p;
  p.x = k.li < 10 ? r[k.li] : 0u;
  p.y = k.li < 10 ? r[10 + k.li] : 0u;
  p.z = k.li < 10 ? r[20 + k.li] : 0u;
  p.inf = r[30] != 0;
  return p;
}
__global__ void __launch_bounds__(64) devtest_wave_pt_kernel(int op, const uint32_t *pp, const uint32_t *qq, uint32_t *out) {
  const wv::wk k = wv::wk_init();
  wv::wjac p = devtest_load_pt(pp + 124 * blockIdx.x, k), q = devtest_load_pt(qq + 124 * blockIdx.x, k), r;
  switch (op) {
    case 0: r = wv::wjac_dbl(p, k); break;
    case 1: r = wv::wjac_add(p, q, k); break;
    case 2: r = wv::wjac_add_aff(p, wv::waff{q.x, q.y}, k); break;
    default: r = wv::wjac_add(p, wv::wjac_lane_xor(p, 16), k); break;
  }
  uint32_t *o = out + 124 * blockIdx.x + 31 * k.row;
  if (k.li < 10) {
    o[k.li] = r.x;
    o[10 + k.li] = r.y;
    o[20 + k.li] = r.z;
  }
  if (k.li == 0) o[30] = r.inf ? 1u : 0u;
}
// one wavefront per signature; out: [n][64][24] bytes = every lane's 20-byte address + ok flag
template <int STOP>
__global__ void __launch_bounds__(64) devtest_wave_recover_kernel(const uint32_t *gtab, const uint8_t *dig, const uint8_t *sig65,
                                                                uint32_t flags, uint8_t *out) {
  const int i = blockIdx.x;
  uint32_t addr[5] = {0, 0, 0, 0, 0};
  aff Q;
  __shared__ uint32_t kscr[wv::KROW_SCRATCH_DWORDS];
  bool ok = wv::recover_pubkey_wave<STOP>(gtab, from_be32(dig + 32 * i), from_be32(sig65 + 65 * i), from_be32(sig65 + 65 * i + 32),
                                    sig65[65 * i + 64], flags, addr, Q, kscr);
  uint8_t *o = out + (size_t)24 * (64 * i + threadIdx.x);
  for (int k = 0; k < 5; k++) reinterpret_cast<uint32_t *>(o)[k] = addr[k];
  o[20] = ok ? 1 : 0;
}

template <typename T>
static T *dev_copy(const T *h, size_t n) {
  T *d = nullptr;
  if (hipMalloc(&d, n * sizeof(T)) != hipSuccess) return nullptr;
  (void)hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
  return d;
}
extern "C" int devtest_wave_fe(int op, int jobs, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  uint32_t *da = dev_copy(a, (size_t)40 * jobs), *db = dev_copy(b, (size_t)40 * jobs), *dout;
  if (!da || !db || hipMalloc(&dout, (size_t)256 * jobs) != hipSuccess) return -1;
  devtest_wave_fe_kernel<<<jobs, 64>>>(op, da, db, dout);
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  (void)hipMemcpy(out, dout, (size_t)256 * jobs, hipMemcpyDeviceToHost);
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
  return rc;
}
// modinv_wave (the outlined modinv_wave_fn) by itself: one wavefront per job.  layout 0: the job's one value in the whole
// wavefront, 1: four values, one per row of sixteen lanes.  Every lane stores its answer: out = jobs × 64 × 32 bytes.
__global__ void __launch_bounds__(64) devtest_wave_modinv_kernel(int which, int layout, const uint8_t *x, uint8_t *out) {
  const wv::wk k = wv::wk_init();
  const uint8_t *src = layout ? x + 128 * (size_t)blockIdx.x + 32 * k.row : x + 32 * (size_t)blockIdx.x;
  const u256 v = from_be32(src);
  const u256 r = which == 0 ? wv::modinv_wave<ModP>(v, k) : wv::modinv_wave<ModN>(v, k);  // `which` is uniform
  to_be32(out + 32 * ((size_t)64 * blockIdx.x + threadIdx.x), r);
}
extern "C" int devtest_wave_modinv(int which, int layout, int jobs, const uint8_t *x, uint8_t *out) {
  if (jobs <= 0 || !x || !out) return -3;
  const size_t in_bytes = (size_t)(layout ? 128 : 32) * jobs, out_bytes = (size_t)2048 * jobs;
  uint8_t *dx = dev_copy(x, in_bytes), *dout = nullptr;
  if (!dx || hipMalloc(&dout, out_bytes) != hipSuccess) return -1;
  (void)hipMemset(dout, 0xA5, out_bytes);
  devtest_wave_modinv_kernel<<<jobs, 64>>>(which, layout ? 1 : 0, dx, dout);
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  if (rc == 0) (void)hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
  (void)hipFree(dx); (void)hipFree(dout);
  return rc;
}
extern "C" int devtest_wave_pt(int op, int jobs, const uint32_t *p, const uint32_t *q, uint32_t *out) {
  uint32_t *dp = dev_copy(p, (size_t)124 * jobs), *dq = dev_copy(q, (size_t)124 * jobs), *dout;
  if (!dp || !dq || hipMalloc(&dout, (size_t)496 * jobs) != hipSuccess) return -1;
  (void)hipMemset(dout, 0, (size_t)496 * jobs);
  devtest_wave_pt_kernel<<<jobs, 64>>>(op, dp, dq, dout);
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  (void)hipMemcpy(out, dout, (size_t)496 * jobs, hipMemcpyDeviceToHost);
  (void)hipFree(dp); (void)hipFree(dq); (void)hipFree(dout);
  return rc;
}
extern "C" int devtest_wave_recover(int n, const uint8_t *dig, const uint8_t *sig65, uint32_t flags, uint8_t *out) {
  uint32_t *dg;
  size_t gbytes = (size_t)ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES * ibftk::GTAB_ENTRY_DWORDS * 4;
  if (hipMalloc(&dg, gbytes) != hipSuccess) return -1;
  uint8_t *dd = dev_copy(dig, (size_t)32 * n), *ds = dev_copy(sig65, (size_t)65 * n), *dout;
  if (!dd || !ds || hipMalloc(&dout, (size_t)24 * 64 * n) != hipSuccess) return -1;
  devtest_gtab_kernel<<<(ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES + 63) / 64, 64>>>(dg);
  devtest_wave_recover_kernel<99><<<n, 64>>>(dg, dd, ds, flags, dout);
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  (void)hipMemcpy(out, dout, (size_t)24 * 64 * n, hipMemcpyDeviceToHost);
  (void)hipFree(dd); (void)hipFree(ds); (void)hipFree(dout); (void)hipFree(dg);
  return rc;
}

// timing breakdown: the recover cut short after stage 1..6 (and complete = 99), ms per launch of n waves
extern "C" int devtest_wave_stage_ms(int n, const uint8_t *dig, const uint8_t *sig65, float *ms7) {
  uint32_t *dg;
  size_t gbytes = (size_t)ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES * ibftk::GTAB_ENTRY_DWORDS * 4;
  if (hipMalloc(&dg, gbytes) != hipSuccess) return -1;
  uint8_t *dd = dev_copy(dig, (size_t)32 * n), *ds = dev_copy(sig65, (size_t)65 * n), *dout;
  if (!dd || !ds || hipMalloc(&dout, (size_t)24 * 64 * n) != hipSuccess) return -1;
  devtest_gtab_kernel<<<(ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES + 63) / 64, 64>>>(dg);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
#define STAGE_RUN(idx, S)                                                              \
  for (int rep = 0; rep < 3; rep++) {                                                  \
    (void)hipEventRecord(e0, 0);                                                       \
    devtest_wave_recover_kernel<S><<<n, 64>>>(dg, dd, ds, 0, dout);                    \
    (void)hipEventRecord(e1, 0);                                                       \
    (void)hipEventSynchronize(e1);                                                     \
    (void)hipEventElapsedTime(&ms7[idx], e0, e1);                                      \
  }
  STAGE_RUN(0, 1) STAGE_RUN(1, 2) STAGE_RUN(2, 3) STAGE_RUN(3, 4) STAGE_RUN(4, 5) STAGE_RUN(5, 6) STAGE_RUN(6, 99)
#undef STAGE_RUN
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  (void)hipFree(dd); (void)hipFree(ds); (void)hipFree(dout); (void)hipFree(dg);
  return rc;
}

// ---- sixteen lanes per signature (recover_pubkey_row): stage timing at the product's launch shape ----
template <int STOP>
__global__ void __launch_bounds__(256) devtest_rows_recover_kernel(const uint32_t *gtab, const uint8_t *dig, const uint8_t *sig65,
                                                                 uint32_t n, uint8_t *out) {
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (wave * 4u >= n) return;
  const uint32_t row_raw = wave * 4u + (lane >> 4);
  const uint32_t i = row_raw < n ? row_raw : n - 1;
  uint32_t addr[5] = {0, 0, 0, 0, 0};
  aff Q;
  __shared__ uint32_t row_tab[4][wv::ROW_TAB_SLOTS * 64];
  bool ok = wv::recover_pubkey_row<STOP>(gtab, from_be32(dig + 32 * i), from_be32(sig65 + 65 * i), from_be32(sig65 + 65 * i + 32),
                                   sig65[65 * i + 64], 0, addr, Q, row_tab[threadIdx.x >> 6]);
  if ((lane & 15u) == 0 && row_raw < n) {
    uint8_t *o = out + (size_t)24 * i;
    for (int k = 0; k < 5; k++) reinterpret_cast<uint32_t *>(o)[k] = addr[k];
    o[20] = ok ? 1 : 0;
  }
}
// ms per launch of n rows cut short after stage 1..6 and complete; out24 (n × 24 B) = addresses + ok of the complete run
// ms7: 9 floats — stages 1, 2, 3, 4, 5, 6, complete, then the sub-stages 21 (r^-1 alone) and 22 (+ u1, u2)
extern "C" int devtest_rows_stage_ms(int n, const uint8_t *dig, const uint8_t *sig65, float *ms7, uint8_t *out24) {
  uint32_t *dg;
  size_t gbytes = (size_t)ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES * ibftk::GTAB_ENTRY_DWORDS * 4;
  if (hipMalloc(&dg, gbytes) != hipSuccess) return -1;
  uint8_t *dd = dev_copy(dig, (size_t)32 * n), *ds = dev_copy(sig65, (size_t)65 * n), *dout;
  if (!dd || !ds || hipMalloc(&dout, (size_t)24 * n) != hipSuccess) return -1;
  devtest_gtab_kernel<<<(ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES + 63) / 64, 64>>>(dg);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  const int waves = (n + 3) / 4, blocks = (waves + 3) / 4;
#define STAGE_RUN(idx, S)                                                              \
  for (int rep = 0; rep < 3; rep++) {                                                  \
    (void)hipEventRecord(e0, 0);                                                       \
    devtest_rows_recover_kernel<S><<<blocks, 256>>>(dg, dd, ds, (uint32_t)n, dout);    \
    (void)hipEventRecord(e1, 0);                                                       \
    (void)hipEventSynchronize(e1);                                                     \
    (void)hipEventElapsedTime(&ms7[idx], e0, e1);                                      \
  }
  STAGE_RUN(0, 1) STAGE_RUN(7, 21) STAGE_RUN(8, 22) STAGE_RUN(1, 2) STAGE_RUN(2, 3) STAGE_RUN(3, 4) STAGE_RUN(4, 5) STAGE_RUN(5, 6) STAGE_RUN(6, 99)
#undef STAGE_RUN
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  if (out24) (void)hipMemcpy(out24, dout, (size_t)24 * n, hipMemcpyDeviceToHost);
  (void)hipFree(dd); (void)hipFree(ds); (void)hipFree(dout); (void)hipFree(dg);
  return rc;
}

// instruction-fetch experiment: the same wavefront runs the whole recover `reps` times (on different rows), so every
// pass after the first finds the kernel's code in the instruction cache: t(2) − t(1) = one pass with warm code
__global__ void __launch_bounds__(256) devtest_rows_repeat_kernel(const uint32_t *gtab, const uint8_t *dig, const uint8_t *sig65,
                                                                uint32_t n, int reps, uint8_t *out) {
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (wave * 4u >= n) return;
  uint32_t acc[5] = {0, 0, 0, 0, 0};
  bool ok_all = true;
  __shared__ uint32_t row_tab[4][wv::ROW_TAB_SLOTS * 64];
#pragma unroll 1
  for (int rep = 0; rep < reps; rep++) {
    const uint32_t row_raw = (wave * 4u + (lane >> 4) + (uint32_t)rep * 64u) % n;
    uint32_t addr[5] = {0, 0, 0, 0, 0};
    aff Q;
    const bool ok = wv::recover_pubkey_row<99>(gtab, from_be32(dig + 32 * row_raw), from_be32(sig65 + 65 * row_raw),
                                           from_be32(sig65 + 65 * row_raw + 32), sig65[65 * row_raw + 64], 0, addr, Q,
                                           row_tab[threadIdx.x >> 6]);
    ok_all = ok_all && ok;
    for (int k = 0; k < 5; k++) acc[k] ^= addr[k];
  }
  const uint32_t i = wave * 4u + (lane >> 4);
  if ((lane & 15u) == 0 && i < n) {
    uint8_t *o = out + (size_t)24 * i;
    for (int k = 0; k < 5; k++) reinterpret_cast<uint32_t *>(o)[k] = acc[k];
    o[20] = ok_all ? 1 : 0;
  }
}
extern "C" int devtest_rows_repeat_ms(int n, const uint8_t *dig, const uint8_t *sig65, int max_reps, float *ms) {
  uint32_t *dg;
  size_t gbytes = (size_t)ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES * ibftk::GTAB_ENTRY_DWORDS * 4;
  if (hipMalloc(&dg, gbytes) != hipSuccess) return -1;
  uint8_t *dd = dev_copy(dig, (size_t)32 * n), *ds = dev_copy(sig65, (size_t)65 * n), *dout;
  if (!dd || !ds || hipMalloc(&dout, (size_t)24 * n) != hipSuccess) return -1;
  devtest_gtab_kernel<<<(ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES + 63) / 64, 64>>>(dg);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  const int waves = (n + 3) / 4, blocks = (waves + 3) / 4;
  for (int reps = 1; reps <= max_reps; reps++)
    for (int t = 0; t < 3; t++) {
      (void)hipEventRecord(e0, 0);
      devtest_rows_repeat_kernel<<<blocks, 256>>>(dg, dd, ds, (uint32_t)n, reps, dout);
      (void)hipEventRecord(e1, 0);
      (void)hipEventSynchronize(e1);
      (void)hipEventElapsedTime(&ms[reps - 1], e0, e1);
    }
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  (void)hipFree(dd); (void)hipFree(ds); (void)hipFree(dout); (void)hipFree(dg);
  return rc;
}

// ---- the rows pair (recover_pubkey_row<…, PAIR> + recover_helper_row): where each wavefront's time goes ----
// The product kernel's shape (four main wavefronts, their helpers w + 4, one workgroup per compute unit); the pair's barriers
// go through a SYNC that stamps s_memrealtime (100 MHz) on each side.  Per wavefront, 8 u64 in `stamps`: [0] start,
// [1] [2] barrier 1 reached / left, [3] [4] barrier 2 reached / left (a MAIN wavefront's; a helper never stands there and
// leaves both 0), [5] end — of a helper: behind publish_and_leave, the moment it stops being resident.  Stamps go to this
// buffer only.
// STOP = 6 ends the main wavefronts behind the closing chain (no address hash; addresses are then junk): "after barrier 2" of
// that launch is the closing chain alone, and the difference to the complete launch is the hash and the compare.
struct stamp_sync {
  uint64_t *st;
  uint32_t *cnt;  // (LDS, this wavefront's: how many barriers it has passed)
  __device__ void operator()() const {
    const uint64_t a = __builtin_amdgcn_s_memrealtime();
    __syncthreads();
    const uint64_t b = __builtin_amdgcn_s_memrealtime();
    if (__lane_id() == 0) {
      const uint32_t i = *cnt;
      st[1 + 2 * i] = a;
      st[2 + 2 * i] = b;
      *cnt = i + 1;
    }
  }
  __device__ void wait() const { (*this)(); }
  __device__ void publish_and_leave() const { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); }  // (the kernel stamps the end)
};
template <int STOP>
__global__ void __launch_bounds__(512) devtest_rows_pair_kernel(const uint32_t *gtab, const uint8_t *dig, const uint8_t *sig65,
                                                              uint32_t n, uint8_t *out, uint64_t *stamps) {
  __shared__ uint32_t row_tab[4][wv::ROW_TAB_SLOTS * 64];
  __shared__ wv::rows_pair_shared sh[4];
  __shared__ uint32_t cnt[8];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u, slot = w & 3u;
  uint64_t *st = stamps + (size_t)(blockIdx.x * 8 + w) * 8;
  if (lane == 0) {
    cnt[w] = 0;
    st[0] = __builtin_amdgcn_s_memrealtime();
  }
  const stamp_sync sync{st, &cnt[w]};
  const uint32_t row_raw = (blockIdx.x * 4 + slot) * 4u + (lane >> 4);
  const uint32_t i = row_raw < n ? row_raw : n - 1;
  const u256 r = from_be32(sig65 + 65 * i), s = from_be32(sig65 + 65 * i + 32);
  if (w >= 4) {
    wv::recover_helper_row(gtab, from_be32(dig + 32 * i), r, s, &sh[slot], sync);
    if (lane == 0) st[5] = __builtin_amdgcn_s_memrealtime();
    return;
  }
  uint32_t addr[5] = {0, 0, 0, 0, 0};
  aff Q;
  const bool ok = wv::recover_pubkey_row<STOP, true>(gtab, zero256(), r, s, sig65[65 * i + 64], 0, addr, Q, row_tab[slot], &sh[slot], sync);
  if (lane == 0) st[5] = __builtin_amdgcn_s_memrealtime();
  if ((lane & 15u) == 0 && row_raw < n) {
    uint8_t *o = out + (size_t)24 * i;
    for (int k = 0; k < 5; k++) reinterpret_cast<uint32_t *>(o)[k] = addr[k];
    o[20] = ok ? 1 : 0;
  }
}
// n rows (a multiple of 16: whole workgroups), three launches; out24 = addresses + ok, stamps8 = (n / 4) · 2 wavefronts × 8
// u64 of the last launch (main wavefronts of workgroup b at 8b … 8b + 3, helpers at 8b + 4 … 8b + 7); ms = its kernel time
// stop = 6: the launches end behind the closing chain (see STOP above); any other value: the complete recover
extern "C" int devtest_rows_pair_stamps_stop(int stop, int n, const uint8_t *dig, const uint8_t *sig65, uint8_t *out24,
                                             uint64_t *stamps8, float *ms) {
  if (n <= 0 || n % 16 != 0) return -3;
  uint32_t *dg;
  size_t gbytes = (size_t)ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES * ibftk::GTAB_ENTRY_DWORDS * 4;
  if (hipMalloc(&dg, gbytes) != hipSuccess) return -1;
  const int blocks = n / 16;
  const size_t st_words = (size_t)blocks * 8 * 8;
  uint8_t *dd = dev_copy(dig, (size_t)32 * n), *ds = dev_copy(sig65, (size_t)65 * n), *dout;
  uint64_t *dst;
  if (!dd || !ds || hipMalloc(&dout, (size_t)24 * n) != hipSuccess || hipMalloc(&dst, st_words * 8) != hipSuccess) return -1;
  if (hipMemset(dst, 0, st_words * 8) != hipSuccess) return -1;  // (the slots a wavefront never writes read 0)
  devtest_gtab_kernel<<<(ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES + 63) / 64, 64>>>(dg);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int rep = 0; rep < 3; rep++) {
    (void)hipEventRecord(e0, 0);
    if (stop == 6)
      devtest_rows_pair_kernel<6><<<blocks, 512>>>(dg, dd, ds, (uint32_t)n, dout, dst);
    else
      devtest_rows_pair_kernel<99><<<blocks, 512>>>(dg, dd, ds, (uint32_t)n, dout, dst);
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(ms, e0, e1);
  }
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  if (rc == 0) {
    (void)hipMemcpy(out24, dout, (size_t)24 * n, hipMemcpyDeviceToHost);
    (void)hipMemcpy(stamps8, dst, st_words * 8, hipMemcpyDeviceToHost);
  }
  (void)hipFree(dd); (void)hipFree(ds); (void)hipFree(dout); (void)hipFree(dst); (void)hipFree(dg);
  return rc;
}
extern "C" int devtest_rows_pair_stamps(int n, const uint8_t *dig, const uint8_t *sig65, uint8_t *out24, uint64_t *stamps8,
                                        float *ms) {
  return devtest_rows_pair_stamps_stop(99, n, dig, sig65, out24, stamps8, ms);
}

// ---- the hand-over that ends a rows pair, alone (SYNC::publish_and_leave / wait over rows_pair_shared) ----
// ONE workgroup of the pair kernel's shape.  The main wavefronts poison their `sh`, all eight pass barrier 1; then a helper
// idles for helper_delay rounds, stores a pattern (a function of salt, slot, field and lane: nothing a former launch left in
// LDS passes for it) where the product's helper stores u1·G, publishes and ENDS, while a main wavefront idles for main_delay
// rounds, waits, and copies what it finds in `sh` to `out` (slot-major, fields gx gy gz ginf, 64 lanes each).  A round is one
// s_sleep of ≈ 1 000 clocks: both loops are bounded by their argument.  Stamps as above, and [3] of a HELPER: its delay is
// over, the pattern not yet stored.  helper_delay = 0 and a long main_delay: the helpers have ended long before the first main
// wavefront stands at barrier 2; the other way round the main wavefronts stand there first and are held until the last helper
// has ended.  Either way the s_barrier counts only the wavefronts that have not ended (kernels.hip.h: rows_pair_handover).
__device__ __forceinline__ uint32_t handover_word(uint32_t salt, uint32_t slot, uint32_t field, uint32_t lane) {
  return salt * 0x9E3779B1u ^ (slot << 16 | field << 8 | lane);
}
__device__ __forceinline__ void handover_delay(uint32_t rounds) {
#pragma unroll 1
  for (uint32_t i = 0; i < rounds; i++) __builtin_amdgcn_s_sleep(16);
}
__global__ void __launch_bounds__(512) devtest_handover_kernel(uint32_t helper_delay, uint32_t main_delay, uint32_t salt,
                                                             uint32_t *out, uint64_t *stamps) {
  __shared__ wv::rows_pair_shared sh[4];
  __shared__ uint32_t cnt[8];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u, slot = w & 3u;
  uint64_t *st = stamps + (size_t)w * 8;
  if (lane == 0) {
    cnt[w] = 0;
    st[0] = __builtin_amdgcn_s_memrealtime();
  }
  const stamp_sync sync{st, &cnt[w]};
  wv::rows_pair_shared *mine = &sh[slot];
  if (w < 4) mine->gx[lane] = mine->gy[lane] = mine->gz[lane] = mine->ginf[lane] = 0xDEADDEADu;
  sync();  // barrier 1: all eight
  if (w >= 4) {
    handover_delay(helper_delay);
    if (lane == 0) st[3] = __builtin_amdgcn_s_memrealtime();
    mine->gx[lane] = handover_word(salt, slot, 0, lane);
    mine->gy[lane] = handover_word(salt, slot, 1, lane);
    mine->gz[lane] = handover_word(salt, slot, 2, lane);
    mine->ginf[lane] = handover_word(salt, slot, 3, lane);
    sync.publish_and_leave();
    if (lane == 0) st[5] = __builtin_amdgcn_s_memrealtime();
    return;
  }
  handover_delay(main_delay);
  sync.wait();  // barrier 2: the main wavefronts alone
  uint32_t *o = out + (size_t)slot * 256 + lane;
  o[0] = mine->gx[lane];
  o[64] = mine->gy[lane];
  o[128] = mine->gz[lane];
  o[192] = mine->ginf[lane];
  if (lane == 0) st[5] = __builtin_amdgcn_s_memrealtime();
}
// out1024: 4 slots × 4 fields × 64 lanes; stamps64: 8 wavefronts × 8 u64 (main wavefronts 0 … 3, helpers 4 … 7)
extern "C" int devtest_handover(uint32_t helper_delay, uint32_t main_delay, uint32_t salt, uint32_t *out1024, uint64_t *stamps64) {
  constexpr uint32_t MAX_ROUNDS = 4096;  // (≈ 2 ms)
  if (helper_delay > MAX_ROUNDS || main_delay > MAX_ROUNDS || !out1024 || !stamps64) return -3;
  uint32_t *dout;
  uint64_t *dst;
  if (hipMalloc(&dout, 1024 * 4) != hipSuccess || hipMalloc(&dst, 64 * 8) != hipSuccess) return -1;
  if (hipMemset(dout, 0, 1024 * 4) != hipSuccess || hipMemset(dst, 0, 64 * 8) != hipSuccess) return -1;
  devtest_handover_kernel<<<1, 512>>>(helper_delay, main_delay, salt, dout, dst);
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  if (rc == 0) {
    (void)hipMemcpy(out1024, dout, 1024 * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(stamps64, dst, 64 * 8, hipMemcpyDeviceToHost);
  }
  (void)hipFree(dout); (void)hipFree(dst);
  return rc;
}

// ---- the RFC 6979 DRBG of sign_dev.h: one lane per row, the first m candidates of each (a reseed between two) ----
#include "sign_dev.h"

__global__ void __launch_bounds__(64) devtest_rfc6979_kernel(uint32_t n, uint32_t m, const uint8_t *sk, const uint8_t *dig, uint8_t *out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  u256 z = from_be32(dig + 32ull * i);
  sub_const_if(z, geq_const(z, NL()), NL());
  ibftk::rfc6979_drbg g;
  g.init(from_be32(sk + 32ull * i), z);
#pragma unroll 1
  for (uint32_t t = 0; t < m; t++) {
    if (t) g.reseed();
    to_be32(out + 32ull * ((size_t)i * m + t), g.candidate());
  }
}
// sk, dig: n × 32 bytes; out: n × m × 32 bytes (row-major: row i's candidates 0 … m − 1)
extern "C" int devtest_rfc6979(int n, int m, const uint8_t *sk, const uint8_t *dig, uint8_t *out) {
  if (n <= 0 || m <= 0) return -3;
  uint8_t *ds = dev_copy(sk, (size_t)32 * n), *dd = dev_copy(dig, (size_t)32 * n), *dout;
  if (!ds || !dd || hipMalloc(&dout, (size_t)32 * n * m) != hipSuccess) return -1;
  devtest_rfc6979_kernel<<<(n + 63) / 64, 64>>>((uint32_t)n, (uint32_t)m, ds, dd, dout);
  int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
  if (rc == 0) (void)hipMemcpy(out, dout, (size_t)32 * n * m, hipMemcpyDeviceToHost);
  (void)hipFree(ds); (void)hipFree(dd); (void)hipFree(dout);
  return rc;
}

// ---- the level scans of the certificate tree (cert_scan_dev.h) on a caller's count column ----
// Either form at any size, through the product's own launch helper, in buffers with sentinel cells around everything the
// kernels may write (tests/test_gpu_cert_scan.py).
#include <stddef.h>
#include <string.h>

#include <vector>

#include "cert_scan_dev.h"

extern "C" uint32_t devtest_cert_scan_threshold(void) { return ibftk::CERT_SCAN_ONE_GROUP_MAX; }

// tiled = 0: cert_scan_kernel, 1: the three tile kernels.  child_count: n words (bit 31 = deferred).  Out: first_child of rows
// [lo, lo + n) (n words), cells [slot_base, slot_base + n) of deferred_rows (n words; those behind the deferred rows still hold
// the sentinel 0xA5A5A5A5), total_dev[2], total_host[2] (pinned host words the kernels write directly; left alone and passed as
// null when with_total_host = 0).  *sentinels_changed: bit 0 nodes [0, lo), 1 nodes behind lo + n, 2 another field than
// first_child of a node in between, 3 deferred_rows [0, slot_base), 4 deferred_rows behind the deferred rows, 5 tile cells
// behind the level's tiles, 6 the words behind either pair of totals.  Returns 0, -3 (arguments), or the HIP status that failed.
extern "C" int devtest_cert_scan(int tiled, uint32_t n, const uint32_t *child_count, uint32_t lo, uint32_t base, uint32_t slot_base,
                                 int with_total_host, uint32_t *first_child, uint32_t *deferred_rows, uint32_t *total_dev,
                                 uint32_t *total_host, uint32_t *sentinels_changed) {
  constexpr uint32_t PAD = 64, FILL = 0xA5A5A5A5u;
  if (!n || !child_count || !first_child || !deferred_rows || !total_dev || !total_host || !sentinels_changed) return -3;
  if ((uint64_t)lo + n + PAD > 0x7FFFFFFFull || (uint64_t)slot_base + n + PAD > 0x7FFFFFFFull) return -3;
  const size_t n_nodes = (size_t)lo + n + PAD, n_slots = (size_t)slot_base + n + PAD, n_tiles = (size_t)ibftk::cert_scan_tiles(n) + PAD;
  uint32_t deferred = 0;
  for (uint32_t i = 0; i < n; i++) deferred += child_count[i] >> 31;
  uint32_t *d_count = nullptr, *d_slots = nullptr, *d_total = nullptr, *h_total = nullptr;
  wire::node_info *d_nodes = nullptr;
  uint2 *d_tiles = nullptr;
  std::vector<wire::node_info> nodes(n_nodes);
  std::vector<uint32_t> slots(n_slots), tiles(2 * n_tiles), totals(PAD);
  uint32_t changed = 0;
  hipError_t e = hipSuccess;
#define SCAN_TRY(call)                     \
  if ((e = (call)) != hipSuccess) goto out
  SCAN_TRY(hipMalloc(&d_count, (size_t)n * 4));
  SCAN_TRY(hipMalloc(&d_nodes, n_nodes * sizeof(wire::node_info)));
  SCAN_TRY(hipMalloc(&d_slots, n_slots * 4));
  SCAN_TRY(hipMalloc(&d_tiles, n_tiles * 8));
  SCAN_TRY(hipMalloc(&d_total, PAD * 4));
  SCAN_TRY(hipHostMalloc((void **)&h_total, PAD * 4));
  SCAN_TRY(hipMemcpy(d_count, child_count, (size_t)n * 4, hipMemcpyHostToDevice));
  SCAN_TRY(hipMemset(d_nodes, 0xA5, n_nodes * sizeof(wire::node_info)));
  SCAN_TRY(hipMemset(d_slots, 0xA5, n_slots * 4));
  SCAN_TRY(hipMemset(d_tiles, 0xA5, n_tiles * 8));
  SCAN_TRY(hipMemset(d_total, 0xA5, PAD * 4));
  memset(h_total, 0xA5, PAD * 4);
  {
    uint32_t *host_words = nullptr;
    if (with_total_host) SCAN_TRY(hipHostGetDevicePointer((void **)&host_words, h_total, 0));
    ibftk::cert_scan_launch(nullptr, !tiled, d_count, d_nodes, lo, n, base, slot_base, d_slots, d_tiles, d_total, host_words);
  }
  SCAN_TRY(hipGetLastError());
  SCAN_TRY(hipDeviceSynchronize());
  SCAN_TRY(hipMemcpy(nodes.data(), d_nodes, n_nodes * sizeof(wire::node_info), hipMemcpyDeviceToHost));
  SCAN_TRY(hipMemcpy(slots.data(), d_slots, n_slots * 4, hipMemcpyDeviceToHost));
  SCAN_TRY(hipMemcpy(tiles.data(), d_tiles, n_tiles * 8, hipMemcpyDeviceToHost));
  SCAN_TRY(hipMemcpy(totals.data(), d_total, PAD * 4, hipMemcpyDeviceToHost));
#undef SCAN_TRY
  for (size_t k = 0; k < n_nodes; k++) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(&nodes[k]);
    const bool inside = k >= lo && k < (size_t)lo + n;
    for (size_t j = 0; j < sizeof(wire::node_info) / 4; j++)
      if (w[j] != FILL && !(inside && j == offsetof(wire::node_info, first_child) / 4)) changed |= inside ? 4u : k < lo ? 1u : 2u;
    if (inside) first_child[k - lo] = nodes[k].first_child;
  }
  for (size_t k = 0; k < n_slots; k++)
    if (slots[k] != FILL && (k < slot_base || k >= (size_t)slot_base + deferred)) changed |= k < slot_base ? 8u : 16u;
  memcpy(deferred_rows, slots.data() + slot_base, (size_t)n * 4);
  for (size_t k = tiled ? 2 * (size_t)ibftk::cert_scan_tiles(n) : 0; k < 2 * n_tiles; k++)
    if (tiles[k] != FILL) changed |= 32u;
  for (uint32_t k = 2; k < PAD; k++)
    if (totals[k] != FILL || h_total[k] != FILL) changed |= 64u;
  if (!with_total_host && (h_total[0] != FILL || h_total[1] != FILL)) changed |= 64u;
  total_dev[0] = totals[0], total_dev[1] = totals[1];
  if (with_total_host) total_host[0] = h_total[0], total_host[1] = h_total[1];
  *sentinels_changed = changed;
out:
  (void)hipFree(d_count); (void)hipFree(d_nodes); (void)hipFree(d_slots); (void)hipFree(d_tiles); (void)hipFree(d_total);
  if (h_total) (void)hipHostFree(h_total);
  return (int)e;
}

// ---- the certificate dedup's kernels (cert_dedup_kernels.h) on a caller's key columns ----
// The GPU counterpart of host_cert_dedup_harness.hip's cdh_run: the product's kernels through the product's launch helpers,
// in buffers with sentinel cells around everything they may write (tests/test_gpu_cert_dedup_kernels.py).
#include "cert_dedup_kernels.h"

namespace {
constexpr uint32_t DD_PAD = 64, DD_FILL = 0xA5A5A5A5u;
struct dd_bufs {
  std::vector<void *> dev;
  uint32_t *h_total = nullptr, *d_total = nullptr, *host_words = nullptr;
  ~dd_bufs() {
    for (void *p : dev) (void)hipFree(p);
    if (h_total) (void)hipHostFree(h_total);
  }
  // `count` elements (and one more, so that nothing is ever empty) of 0xA5 bytes
  template <class T>
  hipError_t filled(T **p, size_t count) {
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, (count + 1) * sizeof(T));
    if (e != hipSuccess) return e;
    dev.push_back(q);
    *p = (T *)q;
    return hipMemset(q, 0xA5, (count + 1) * sizeof(T));
  }
  // the words the library keeps at d_cert_total / h_cert_total: [4..5] {dense, unplaced}, [6..7] the two counts, [8..10] the
  // count kernel's accumulators (zero between launches); every other word a sentinel
  hipError_t totals() {
    hipError_t e = filled(&d_total, DD_PAD);
    if (e != hipSuccess || (e = hipMemset(d_total + 8, 0, 12)) != hipSuccess) return e;
    if ((e = hipHostMalloc((void **)&h_total, DD_PAD * 4)) != hipSuccess) return e;
    memset(h_total, 0xA5, DD_PAD * 4);
    return hipHostGetDevicePointer((void **)&host_words, h_total, 0);
  }
  // bit 8 of sentinels_changed: a word of either set of totals that no kernel may write
  hipError_t totals_changed(uint32_t *changed) {
    uint32_t w[DD_PAD];
    const hipError_t e = hipMemcpy(w, d_total, DD_PAD * 4, hipMemcpyDeviceToHost);
    for (uint32_t k = 0; k < DD_PAD && e == hipSuccess; k++)
      if ((w[k] != DD_FILL && !(k >= 4 && k <= 10)) || (h_total[k] != DD_FILL && !(k >= 4 && k <= 7))) *changed |= 256u;
    return e;
  }
};
#define DD_TRY(call) \
  if ((e = (call)) != hipSuccess) return (int)e

// cert_dedup_count_kernel twice in a row over flag columns on the device → out14: per launch {the two counts on the device, the
// two in the host's words, the three accumulator words after it}.  The result words are set back to the sentinel before each
// launch, so every launch has to deliver its own.
int dd_count_twice(dd_bufs &B, const uint8_t *d_a, uint32_t n_a, const uint8_t *d_b, uint32_t n_b, uint32_t *out14) {
  hipError_t e = hipSuccess;
  for (int pass = 0; pass < 2; pass++) {
    uint32_t w[5];
    DD_TRY(hipMemset(B.d_total + 6, 0xA5, 8));
    B.h_total[6] = B.h_total[7] = DD_FILL;
    ibftk::cert_dedup_count_launch(nullptr, d_a, n_a, d_b, n_b, B.d_total + 8, B.d_total + 6, B.host_words + 6);
    DD_TRY(hipGetLastError());
    DD_TRY(hipDeviceSynchronize());
    DD_TRY(hipMemcpy(w, B.d_total + 6, 20, hipMemcpyDeviceToHost));
    uint32_t *o = out14 + 7 * pass;
    o[0] = w[0], o[1] = w[1], o[2] = B.h_total[6], o[3] = B.h_total[7], o[4] = w[2], o[5] = w[3], o[6] = w[4];
  }
  return 0;
}
}  // namespace

extern "C" uint32_t devtest_cert_dedup_max_probes(void) { return cdd::MAX_PROBES; }
extern "C" uint32_t devtest_cert_dedup_table_slots(uint32_t rows, uint32_t cap) { return cdd::table_slots(rows, cap); }

// The count kernel alone: flag columns of n_a and n_b bytes (either may be empty, not both) → out14 as dd_count_twice gives it.
// *sentinels_changed: bit 8 only.  Returns 0, -3 (arguments), or the HIP status that failed.
extern "C" int devtest_cert_dedup_count(uint32_t n_a, const uint8_t *pre_a, uint32_t n_b, const uint8_t *pre_b, uint32_t *out14,
                                        uint32_t *sentinels_changed) {
  if ((uint64_t)n_a + n_b == 0 || (uint64_t)n_a + n_b > 0x7FFFFFFFull || (n_a && !pre_a) || (n_b && !pre_b) || !out14 || !sentinels_changed) return -3;
  dd_bufs B;
  hipError_t e = hipSuccess;
  uint8_t *d_a = nullptr, *d_b = nullptr;
  DD_TRY(B.filled(&d_a, n_a));
  DD_TRY(B.filled(&d_b, n_b));
  if (n_a) DD_TRY(hipMemcpy(d_a, pre_a, n_a, hipMemcpyHostToDevice));
  if (n_b) DD_TRY(hipMemcpy(d_b, pre_b, n_b, hipMemcpyHostToDevice));
  DD_TRY(B.totals());
  if (const int rc = dd_count_twice(B, d_a, n_a, d_b, n_b, out14)) return rc;
  *sentinels_changed = 0;
  DD_TRY(B.totals_changed(sentinels_changed));
  return 0;
}

// n rows of (digest32, sig65, from20, pre) and a slot cap (0: none) through the front (table clear, insert, mark, tile sums,
// offsets, apply), then a verdict word per 64 dense rows built HERE from the gathered bytes alone — dense row d's bit is 1 iff
// its gathered pre is 0 and the low bit of its gathered digest byte 0 is set — then the scatter, then the count twice over
// pre[0, n) and pre_b[0, n_b).  Out: rep[n] (cdd::rep_of over the final table; cdd::NO_REP for pre-flagged rows), slot_of[n],
// dense_pos[n] (the sentinel where the kernel wrote nothing), the gathered rows (only the first `dense` rows of g_* are
// written), mask[⌈n/64⌉] (pre-filled with all ones before the scatter), stat4 {dense, unplaced} on the device and in the
// host's words, count14 (dd_count_twice).  *sentinels_changed: bit 0 cells around the table, 1 around slot_of, 2 around
// dense_pos, 3 around the tile cells, 4 around the scan words, 5 column rows between the tree's rows and the dense batch or
// behind it, 6 a source row, 7 mask words around ⌈n/64⌉, 8 another word of the totals.
// Returns 0, -3 (arguments), -4 (more representatives than rows: nothing behind the front ran), or the HIP status that failed.
extern "C" int devtest_cert_dedup(uint32_t n, const uint8_t *digest32, const uint8_t *sig65, const uint8_t *from20, const uint8_t *pre,
                                  uint32_t slots_cap, uint32_t n_b, const uint8_t *pre_b, uint32_t *rep, uint32_t *slot_of, uint32_t *dense_pos,
                                  uint8_t *g_digest32, uint8_t *g_sig65, uint8_t *g_from20, uint8_t *g_pre, uint64_t *mask, uint32_t *stat4,
                                  uint32_t *count14, uint32_t *sentinels_changed) {
  constexpr uint32_t PAD = DD_PAD;
  if (!n || n > 0x20000000u || n_b > 0x20000000u || !digest32 || !sig65 || !from20 || !pre || (n_b && !pre_b) || !rep || !slot_of || !dense_pos ||
      !g_digest32 || !g_sig65 || !g_from20 || !g_pre || !mask || !stat4 || !count14 || !sentinels_changed)
    return -3;
  const uint32_t slots = cdd::table_slots(n, slots_cap), tiles = ibftk::cert_scan_tiles(n), dense_base = (n + 63u) & ~63u, words = (n + 63u) / 64u;
  const size_t col_rows = (size_t)dense_base + n + PAD;  // the tree's rows, a dense batch of up to n rows behind them, sentinel rows
  const size_t widths[4] = {32, 65, 20, 1};
  const uint8_t *src[4] = {digest32, sig65, from20, pre};
  uint8_t *g_out[4] = {g_digest32, g_sig65, g_from20, g_pre};
  dd_bufs B;
  hipError_t e = hipSuccess;
  uint8_t *d_col[4] = {}, *d_pre_b = nullptr;
  uint32_t *d_table = nullptr, *d_slot = nullptr, *d_word = nullptr, *d_pos = nullptr;
  uint2 *d_tiles = nullptr;
  uint64_t *d_mask = nullptr, *d_dense_mask = nullptr;
  uint32_t changed = 0;
  for (int k = 0; k < 4; k++) {
    DD_TRY(B.filled(&d_col[k], col_rows * widths[k]));
    DD_TRY(hipMemcpy(d_col[k], src[k], (size_t)n * widths[k], hipMemcpyHostToDevice));
  }
  DD_TRY(B.filled(&d_pre_b, n_b));
  if (n_b) DD_TRY(hipMemcpy(d_pre_b, pre_b, n_b, hipMemcpyHostToDevice));
  DD_TRY(B.filled(&d_table, (size_t)slots + 2 * PAD));
  DD_TRY(B.filled(&d_slot, (size_t)n + 2 * PAD));
  DD_TRY(B.filled(&d_word, (size_t)n + 2 * PAD));
  DD_TRY(B.filled(&d_pos, (size_t)n + 2 * PAD));
  DD_TRY(B.filled(&d_tiles, (size_t)tiles + 2 * PAD));
  DD_TRY(B.filled(&d_mask, (size_t)words + 2 * PAD));
  DD_TRY(B.totals());
  const cdd::columns cols{d_col[0], d_col[1], d_col[2], d_col[3]};
  DD_TRY(ibftk::cert_dedup_front_launch(nullptr, cols, n, slots, dense_base, d_table + PAD, d_slot + PAD, d_word + PAD, d_tiles + PAD, d_pos + PAD,
                                        B.d_total + 4, B.host_words + 4));
  DD_TRY(hipGetLastError());
  DD_TRY(hipDeviceSynchronize());
  std::vector<uint32_t> table((size_t)slots + 2 * PAD), slot((size_t)n + 2 * PAD), word((size_t)n + 2 * PAD), pos((size_t)n + 2 * PAD),
      tile(2 * ((size_t)tiles + 2 * PAD));
  uint32_t stat_dev[2];
  DD_TRY(hipMemcpy(table.data(), d_table, table.size() * 4, hipMemcpyDeviceToHost));
  DD_TRY(hipMemcpy(slot.data(), d_slot, slot.size() * 4, hipMemcpyDeviceToHost));
  DD_TRY(hipMemcpy(word.data(), d_word, word.size() * 4, hipMemcpyDeviceToHost));
  DD_TRY(hipMemcpy(pos.data(), d_pos, pos.size() * 4, hipMemcpyDeviceToHost));
  DD_TRY(hipMemcpy(tile.data(), d_tiles, tile.size() * 4, hipMemcpyDeviceToHost));
  DD_TRY(hipMemcpy(stat_dev, B.d_total + 4, 8, hipMemcpyDeviceToHost));
  const uint32_t dense = stat_dev[0];
  stat4[0] = stat_dev[0], stat4[1] = stat_dev[1], stat4[2] = B.h_total[4], stat4[3] = B.h_total[5];
  if (dense > n) return -4;
  const auto around = [&](const std::vector<uint32_t> &v, size_t inner, size_t pad) {  // `pad` words before and behind `inner` words
    for (size_t k = 0; k < pad; k++)
      if (v[k] != DD_FILL || v[pad + inner + k] != DD_FILL) return true;
    return false;
  };
  if (around(table, slots, PAD)) changed |= 1u;
  if (around(slot, n, PAD)) changed |= 2u;
  if (around(pos, n, PAD)) changed |= 4u;
  if (around(tile, 2 * (size_t)tiles, 2 * PAD)) changed |= 8u;  // (two words per cell)
  if (around(word, n, PAD)) changed |= 16u;
  std::vector<uint8_t> col[4];
  for (int k = 0; k < 4; k++) {
    const size_t w = widths[k];
    col[k].resize(col_rows * w);
    DD_TRY(hipMemcpy(col[k].data(), d_col[k], col_rows * w, hipMemcpyDeviceToHost));
    if (memcmp(col[k].data(), src[k], (size_t)n * w) != 0) changed |= 64u;
    for (size_t i = (size_t)n * w; i < col_rows * w; i++)
      if (col[k][i] != 0xA5 && (i < (size_t)dense_base * w || i >= ((size_t)dense_base + dense) * w)) changed |= 32u;
    memcpy(g_out[k], col[k].data() + (size_t)dense_base * w, (size_t)dense * w);
  }
  // the dense batch's verdict words, from the gathered bytes and nothing else
  std::vector<uint64_t> dense_mask((dense + 63u) / 64u + 1u, 0);
  for (uint32_t d = 0; d < dense; d++)
    if (g_pre[d] == 0 && (g_digest32[32ull * d] & 1u)) dense_mask[d >> 6] |= 1ull << (d & 63u);
  DD_TRY(B.filled(&d_dense_mask, dense_mask.size()));
  DD_TRY(hipMemcpy(d_dense_mask, dense_mask.data(), dense_mask.size() * 8, hipMemcpyHostToDevice));
  DD_TRY(hipMemset(d_mask + PAD, 0xFF, (size_t)words * 8));  // the tree's own words: the scatter has to store each of them whole
  ibftk::cert_dedup_scatter_launch(nullptr, d_table + PAD, d_slot + PAD, d_pos + PAD, d_dense_mask, n, d_mask + PAD);
  DD_TRY(hipGetLastError());
  DD_TRY(hipDeviceSynchronize());
  std::vector<uint64_t> m((size_t)words + 2 * PAD);
  DD_TRY(hipMemcpy(m.data(), d_mask, m.size() * 8, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < PAD; k++)
    if (m[k] != 0xA5A5A5A5A5A5A5A5ull || m[PAD + words + k] != 0xA5A5A5A5A5A5A5A5ull) changed |= 128u;
  memcpy(mask, m.data() + PAD, (size_t)words * 8);
  for (uint32_t r = 0; r < n; r++) {
    slot_of[r] = slot[PAD + r];
    dense_pos[r] = pos[PAD + r];
    const bool placed = slot_of[r] != cdd::SLOT_SKIP && slot_of[r] != cdd::SLOT_UNPLACED;
    if (placed && slot_of[r] >= slots) return -4;  // (never index the copy of the table with it)
    rep[r] = cdd::rep_of(table.data() + PAD, slot_of[r], r);
  }
  if (const int rc = dd_count_twice(B, d_col[3], n, d_pre_b, n_b, count14)) return rc;
  DD_TRY(B.totals_changed(&changed));
  *sentinels_changed = changed;
  return 0;
}
#undef DD_TRY
