// host_row_scalars_harness.hip — TEST-ONLY: runs wv::row_scalars (wave_fe_dev.h: the scalar stage of the row forms, the
// two halves of a row computing different numbers) on the CPU through the 64-coroutine lockstep emulator in wave_emul.h,
// next to the lane-layout route it replaced (sc_mul twice, sc_split_lambda), for tests/test_dev_row_scalars_host.py.
// Built with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#define IBFT_GTAB_BITS 8
#define IBFT_WAVE_EMUL 1
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "wave_fe_dev.h"

namespace {

constexpr int OUT_BYTES = 100;  // u1 (32, big-endian) ‖ |k1| (32) ‖ |k2| (32) ‖ k1 < 0 ‖ k2 < 0 ‖ handed over (1) ‖ 0

void put(uint8_t *o, const secp::u256 &u1, const secp::glv_split &sp, uint8_t handed) {
  secp::to_be32(o, u1);
  secp::to_be32(o + 32, sp.k1);
  secp::to_be32(o + 64, sp.k2);
  o[96] = sp.neg1 ? 1 : 0;
  o[97] = sp.neg2 ? 1 : 0;
  o[98] = handed;
  o[99] = 0;
}

struct job {
  const uint8_t *zrs;  // [4][96]: z ‖ r ‖ s big-endian, one triple per row
  uint8_t *out;        // [64][OUT_BYTES]: every lane's answer
};
void lane_scalars(void *vp) {
  job *j = (job *)vp;
  const uint32_t lane = wv::lane_id(), row = lane >> 4;
  const uint8_t *in = j->zrs + 96 * row;
  const wv::wk k = wv::wk_init();
  // the hand-over sees the split every lane returns
  secp::glv_split seen;
  seen.k1 = seen.k2 = secp::zero256();
  seen.neg1 = seen.neg2 = false;
  int calls = 0;
  const wv::row_scalars_out rs = wv::row_scalars(secp::from_be32(in), secp::from_be32(in + 32), secp::from_be32(in + 64), k,
                                                 [&](const secp::glv_split &sp) {
                                                   seen = sp;
                                                   calls++;
                                                 });
  const bool same = calls == 1 && secp::eq(seen.k1, rs.sp.k1) && secp::eq(seen.k2, rs.sp.k2) && seen.neg1 == rs.sp.neg1 &&
                    seen.neg2 == rs.sp.neg2;
  put(j->out + OUT_BYTES * lane, rs.u1, rs.sp, same ? 1 : 0);
}

}  // namespace

// n_waves wavefronts of four triples each: zrs [n_waves][4][96] → out [n_waves][64][100]
extern "C" void row_scalars_waves(const uint8_t *zrs, int n_waves, uint8_t *out) {
  for (int w = 0; w < n_waves; w++) {
    job j{zrs + 384 * w, out + 64 * OUT_BYTES * w};
    wave_emul::run(lane_scalars, &j);
  }
}

// the lane-layout route, one triple: zrs [96] → out [100]
extern "C" void lane_scalars_one(const uint8_t *zrs, uint8_t *out) {
  const secp::sc rinv = secp::sc_inv_safegcd(secp::sc_from_u256(secp::from_be32(zrs + 32)));
  const secp::u256 u1 = secp::sc_neg_canon(secp::sc_canon(secp::sc_mul(secp::sc_from_u256(secp::from_be32(zrs)), rinv)));
  const secp::u256 u2 = secp::sc_canon(secp::sc_mul(secp::sc_from_u256(secp::from_be32(zrs + 64)), rinv));
  put(out, u1, secp::sc_split_lambda(u2), 1);
}

extern "C" int row_scalars_out_bytes() { return OUT_BYTES; }
