// host_row_keccak_harness.hip — TEST-ONLY: runs wv::address_from_xy_row (keccak_row_dev.h: the Keccak state of a row's
// hash spread over the row's lanes) on the CPU through the 64-coroutine lockstep emulator in wave_emul.h, next to the
// lane-layout keccak::address_from_xy, for tests/test_dev_row_keccak_host.py.
// Built with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#define IBFT_GTAB_BITS 8
#define IBFT_WAVE_EMUL 1
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "wave_fe_dev.h"

namespace {

struct job {
  const uint8_t *xy;  // [4][64]: X‖Y big-endian, one key per row
  uint8_t *addr;      // [64][20]: every lane's answer
  uint32_t *scr;
};
void lane_addr(void *vp) {
  job *j = (job *)vp;
  const uint32_t lane = wv::lane_id(), row = lane >> 4;
  const secp::fe X = secp::fe_from_u256(secp::from_be32(j->xy + 64 * row));
  const secp::fe Y = secp::fe_from_u256(secp::from_be32(j->xy + 64 * row + 32));
  uint32_t a[5];
  wv::address_from_xy_row(X, Y, a, j->scr);
  memcpy(j->addr + 20 * lane, a, 20);
}

}  // namespace

// n_waves wavefronts of four keys each: xy [n_waves][4][64] → addr [n_waves][64][20]
extern "C" void row_keccak_addresses(const uint8_t *xy, int n_waves, uint8_t *addr) {
  static uint32_t scr[wv::KROW_SCRATCH_DWORDS];
  for (int w = 0; w < n_waves; w++) {
    // what the previous wavefront left in the scratch must not matter; neither must a pattern
    memset(scr, w & 1 ? 0xA5 : 0, sizeof scr);
    job j{xy + 256 * w, addr + 1280 * w, scr};
    wave_emul::run(lane_addr, &j);
  }
}

// the lane-layout form, one key: xy [64] → addr [20]
extern "C" void lane_keccak_address(const uint8_t *xy, uint8_t *addr) {
  const secp::u256 x = secp::from_be32(xy), y = secp::from_be32(xy + 32);
  uint32_t a[5];
  keccak::address_from_xy(x.v, y.v, a);
  memcpy(addr, a, 20);
}

extern "C" int row_keccak_scratch_dwords() { return wv::KROW_SCRATCH_DWORDS; }
