// host_proposal_digest_harness.hip — TEST-ONLY: the two absorb-with-spliced-tail routines behind proposal_digest_kernel on the CPU,
// so tests/test_dev_proposal_digest_host.py can check the exact device source without a GPU: the lane form
// (keccak::hash_range_tail_dwords) called directly, the wave form (cw::sponge_message with a tail) through the 64-coroutine lockstep
// emulator in wave_emul.h.  Built with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#define IBFT_WAVE_EMUL 1
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "cert_wave_dev.h"

namespace {

// what is LDS on the device: memory shared by the 64 coroutines
alignas(16) uint64_t g_A[32], g_B[32];

struct wave_job {
  const uint8_t *raw;
  uint32_t len;
  uint64_t tail;
  uint64_t out[4];
};
void lane_sponge(void *p) {
  wave_job *j = (wave_job *)p;
  const uint32_t lane = cw::lane_id();
  const uint64_t w = cw::sponge_message(j->raw, j->len, 0u, j->len + 8u, j->tail, true, lane, g_A, g_B);
  if (lane < 4) j->out[lane] = w;
}

}  // namespace

extern "C" {

// keccak256(raw[0, len) ‖ BE64(round)) the way one lane of proposal_digest_kernel<1> computes it.  The caller's buffer must be
// readable from raw rounded down to a multiple of 4 up to 7 bytes past raw + len (the staged buffer's slack).
void pdh_lane(const uint8_t *raw, uint32_t len, uint64_t round, uint8_t *out32) {
  uint64_t d[4];
  keccak::hash_range_tail_dwords(raw, len, keccak::round_tail(round), d);
  memcpy(out32, d, 32);
}
// … and the way the wavefront of proposal_digest_kernel<64> computes it
void pdh_wave(const uint8_t *raw, uint32_t len, uint64_t round, uint8_t *out32) {
  wave_job j{raw, len, keccak::round_tail(round), {0, 0, 0, 0}};
  wave_emul::run(lane_sponge, &j);
  memcpy(out32, j.out, 32);
}

}  // extern "C"
