// host_block_head_harness.hip — TEST-ONLY: the per-row body of block_head_kernel on the CPU, so that
// tests/test_dev_block_head_host.py can check the exact device source without a GPU: a row's block (block_of_row) and the
// hash its seal signs under the seal-digest convention (block_head_row).  Built with hipcc's host pass; never linked into
// libibftgpu.so, never a fallback.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "recover_dev.h"

extern "C" {

// n rows over n_blocks blocks: out_hash32[32·row …] = what block_head_kernel stores for the row, out_block[row] = its block.
// digest32: n_blocks × 32, 8-byte aligned (read only).  suffix_words: the nine words ibft_set_seal_digest derives.
void bhh_rows(const uint8_t *digest32, const uint32_t *off, uint32_t n_blocks, uint32_t n, uint32_t convert, const uint64_t *suffix_words,
              uint8_t *out_hash32, uint32_t *out_block) {
  for (uint32_t row = 0; row < n; row++) {
    const ibftk::block_head_t h = ibftk::block_head_row(reinterpret_cast<const uint64_t *>(digest32), off, n_blocks, row, convert, suffix_words);
    memcpy(out_hash32 + 32ull * row, h.w, 32);
    out_block[row] = ibftk::block_of_row(off, n_blocks, row);
  }
}

}  // extern "C"
