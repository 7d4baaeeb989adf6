// host_block_sets_harness.hip — TEST-ONLY: the per-row decision of block_tally_kernel under a family of sets on the CPU, so that
// tests/test_dev_block_sets_host.py can check the exact device source without a GPU: union table → union index
// (valset_lookup), union index + set → index in the set (valsets_set_index), and what becomes of a row's verdict bit
// (valsets_row).  Built with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "recover_dev.h"

extern "C" {

// the hash the tables are built with (the Python restatement is checked against it)
uint32_t bsh_addr_hash(const uint8_t *addr20) {
  uint32_t a[5];
  memcpy(a, addr20, 20);
  return ibftk::addr_hash(a);
}

// n addresses → out_set_idx[i] = index of addr i in set `set` (−1: no member), out_union_idx[i] = its union index (−1: in no set)
void bsh_lookup(const uint32_t *vtab, uint32_t slot_mask, const int32_t *setidx, uint32_t n_union, uint32_t set,
                const uint8_t *addr20, uint32_t n, int32_t *out_set_idx, int32_t *out_union_idx) {
  for (uint32_t i = 0; i < n; i++) {
    uint32_t a[5];
    memcpy(a, addr20 + 20ull * i, 20);
    const int u = ibftk::valset_lookup(vtab, slot_mask, a);  // what a verdict kernel leaves in the index column
    out_set_idx[i] = ibftk::valsets_set_index(setidx, n_union, set, u);
    out_union_idx[i] = u;
  }
}

// n rows of one block: verdict bit and union index as the verdict kernel left them → {index in the set, bit, clear}
void bsh_rows(const uint8_t *bit, const int32_t *union_idx, const int32_t *setidx, uint32_t n_union, uint32_t set, uint32_t n,
              int32_t *out_si, uint8_t *out_bit, uint8_t *out_clear) {
  for (uint32_t i = 0; i < n; i++) {
    const ibftk::valsets_row_t r = ibftk::valsets_row(bit[i] != 0, union_idx[i], setidx, n_union, set);
    out_si[i] = r.si;
    out_bit[i] = r.bit ? 1 : 0;
    out_clear[i] = r.clear ? 1 : 0;
  }
}

}  // extern "C"
