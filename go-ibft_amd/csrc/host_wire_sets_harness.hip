// host_wire_sets_harness.hip — TEST-ONLY: the per-row bodies of wire_row_set_kernel and wire_sets_tally_kernel
// (wire_sets_dev.h) on the CPU, so that tests/test_dev_wire_sets_host.py can check the exact device source without a GPU: a
// height → its set, a parsed message → its set and pre-flag, a row's verdict bit + union index + set → bit / index / entry,
// the per-set records, and tally_record on sums of the caller's.  The cross-row part — who is first for an entry, the sums — is a plain loop here where the kernel
// has its bitmap merge and its wavefront turns.  Built with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "wire_sets_dev.h"

extern "C" {

// n heights → their sets under the map (−1: none)
void wsh_heights(const uint64_t *first, const uint32_t *range_set, uint32_t n_ranges, const uint64_t *height, uint32_t n, int32_t *out_set) {
  const ibftk::height_map m{first, range_set, n_ranges};
  for (uint32_t i = 0; i < n; i++) out_set[i] = ibftk::height_map_set(m, height[i]);
}

// n parsed messages (ibft_wire_row_t, 80 bytes each) → their sets; pre_flags as wire_row_set_kernel leaves the column
void wsh_row_sets(const uint8_t *rows80, uint32_t n, const uint64_t *first, const uint32_t *range_set, uint32_t n_ranges, int32_t *out_set,
                  uint8_t *pre_flags) {
  const ibftk::height_map m{first, range_set, n_ranges};
  for (uint32_t i = 0; i < n; i++) {
    wire::row_info ri;
    memcpy(&ri, rows80 + 80ull * i, 80);
    out_set[i] = ibftk::wire_row_set_row(ri, m);
    if (out_set[i] < 0) pre_flags[i] = 1;
  }
}

// The tally over n rows as the verdict launch left them: bit / union_idx in, bit / index in the row's set out; records:
// n_sets × 4 words {power_lo, power_hi, valid | distinct << 32, has_quorum}.  set_meta: n_sets × {first entry, members};
// vpower32: entries × n_pieces; quorum: n_sets × 5 words.
void wsh_tally(uint8_t *bit, int32_t *vidx, const int32_t *row_set, uint32_t n, const int32_t *setidx, uint32_t n_union,
               const uint32_t *set_meta, const uint32_t *vpower32, uint32_t n_pieces, const uint64_t *quorum, uint32_t n_sets,
               uint64_t *records) {
  const uint2 *meta = reinterpret_cast<const uint2 *>(set_meta);
  uint32_t entries = 0;
  for (uint32_t s = 0; s < n_sets; s++) entries += meta[s].y;
  std::vector<uint8_t> seen(entries, 0);
  std::vector<uint64_t> acc((size_t)n_sets * (n_pieces + 1), 0);
  for (uint32_t r = 0; r < n; r++) {
    const ibftk::wire_sets_row_t sr = ibftk::wire_sets_row(bit[r] != 0, vidx[r], row_set[r], setidx, n_union, meta);
    vidx[r] = sr.si;
    bit[r] = sr.bit ? 1 : 0;
    if (!sr.bit) continue;
    uint64_t *a = &acc[(size_t)row_set[r] * (n_pieces + 1)];
    a[n_pieces] += 1;
    if (!sr.counts || seen[sr.entry]) continue;
    seen[sr.entry] = 1;
    a[n_pieces] += 1ull << 32;
    for (uint32_t k = 0; k < n_pieces; k++) a[k] += vpower32[(size_t)sr.entry * n_pieces + k];
  }
  for (uint32_t s = 0; s < n_sets; s++) {
    const uint64_t *a = &acc[(size_t)s * (n_pieces + 1)];
    ibftk::tally_record(a, (int)n_pieces, a[n_pieces], quorum + (size_t)s * ibftk::TALLY_SUM_WORDS, 0ull, records + 4ull * s);
  }
}

// tally_record (tally_dev.h) itself: n_pieces piece sums, the counts word, 5 quorum words, the proposer's rows → the record's
// 4 words and the power in full (5 words)
void wsh_tally_record(const uint64_t *piece, uint32_t n_pieces, uint64_t counts, const uint64_t *quorum, uint64_t proposer_rows, uint64_t *out4,
                      uint64_t *wide5) {
  ibftk::tally_record(piece, (int)n_pieces, counts, quorum, proposer_rows, out4, wide5);
}

}  // extern "C"
