// host_cert_dedup_harness.hip — TEST-ONLY: cert_dedup_dev.h (the certificate dedup's row logic: table insert, representatives,
// gather, scatter) on the CPU, so that tests/test_dev_cert_dedup_host.py can check the exact device source without a GPU.
// cdh_run walks the steps certificates_wire_impl enqueues, one row after the other — the two atomics are plain operations
// here, and the rows are inserted in the order the test gives (the atomics themselves, with thousands of lanes on one table
// word: devtest.hip's devtest_cert_dedup, tests/test_gpu_cert_dedup_kernels.py).  Built with hipcc's host pass; never linked
// into libibftgpu.so, never a fallback.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "cert_dedup_dev.h"

extern "C" {

uint32_t cdh_max_probes() { return cdd::MAX_PROBES; }
uint32_t cdh_table_slots(uint32_t rows, uint32_t cap) { return cdd::table_slots(rows, cap); }
uint32_t cdh_key_hash(uint8_t *digest32, uint8_t *sig65, uint32_t row) {
  const cdd::columns k{digest32, sig65, nullptr, nullptr};
  return cdd::key_hash(k, row);
}

// The columns hold n rows and room for n more behind them (the dense batch at rows [n, 2n)).  order: the n rows in the order
// they are inserted.  row_bit[r]: the verdict row r gets when it is judged on its own — the dense batch's "verdict launch"
// hands dense row d the bit of the row it was gathered from.  Out: rep[n] (cdd::NO_REP for pre-flagged rows), dense_row[n]
// (the representative behind each dense row), bit[n], counts = {dense rows, unplaced rows, judged rows, slots}.
void cdh_run(uint8_t *digest32, uint8_t *sig65, uint8_t *from20, uint8_t *pre, uint32_t n, uint32_t slots_cap, const uint32_t *order,
             const uint8_t *row_bit, uint32_t *rep, uint32_t *dense_row, uint8_t *bit, uint32_t *counts) {
  const cdd::columns k{digest32, sig65, from20, pre};
  const uint32_t slots = cdd::table_slots(n, slots_cap);
  std::vector<uint32_t> table(slots, cdd::EMPTY), slot_of(n), word(n), dense_pos(n, 0);
  for (uint32_t i = 0; i < n; i++) slot_of[order[i]] = cdd::insert_row(k, order[i], table.data(), slots - 1u);
  uint32_t dense = 0, unplaced = 0, judged = 0;
  for (uint32_t r = 0; r < n; r++) {
    word[r] = cdd::scan_word(table.data(), slot_of[r], r);
    rep[r] = cdd::rep_of(table.data(), slot_of[r], r);
    unplaced += word[r] >> 31;
    judged += pre[r] == 0;
  }
  for (uint32_t r = 0; r < n; r++) {  // (the scan: ascending)
    if (!(word[r] & 1u)) continue;
    dense_pos[r] = dense;
    dense_row[dense] = r;
    cdd::gather_row(k, r, n + dense);
    dense++;
  }
  std::vector<uint64_t> dense_mask((dense + 63) / 64 + 1, 0);
  for (uint32_t d = 0; d < dense; d++)
    if (pre[n + d] == 0 && row_bit[dense_row[d]]) dense_mask[d >> 6] |= 1ull << (d & 63u);
  for (uint32_t r = 0; r < n; r++) bit[r] = cdd::scatter_bit(table.data(), slot_of.data(), dense_pos.data(), dense_mask.data(), r) ? 1 : 0;
  counts[0] = dense;
  counts[1] = unplaced;
  counts[2] = judged;
  counts[3] = slots;
}

}  // extern "C"
