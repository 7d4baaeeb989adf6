// wire_sets_dev.h — the live route under a FAMILY of validator sets (ibft_verify_senders_wire_sets): every message is judged
// under the validator set of ITS OWN height (core/backend.go:41-45), whatever heights a receive-queue batch mixes.
//
//   the height map      ranges [first[k], first[k + 1]) of heights → a set of the installed family (ibft_set_height_sets)
//   wire_row_set_row    what wire_row_set_kernel decides for one parsed message: its set, or −1 and a pre-flag
//   wire_sets_row       what wire_sets_tally_kernel decides for one row from its verdict bit, the UNION index the verdict
//                       kernel left (recover_dev.h: valsets_row) and the row's set: the bit, the index in the set, and which
//                       (set, member) entry of the family's packed power column — and of the distinct-sender bitmap — it is
// A set's sums become its record through tally_record (tally_dev.h, included here), with no proposer rows.
//
// Everything here is __host__ __device__: csrc/host_wire_sets_harness.hip runs it on the CPU against tests/wire_sets_model.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recover_dev.h"
#include "tally_dev.h"
#include "wire_dev.h"

namespace ibftk {

// ---- the height map ---------------------------------------------------------------------------------------------------------
// first: n_ranges + 1 strictly increasing heights, range_set: n_ranges set indices (both checked on the host).  The set of
// height h: range_set[k] for the LAST k with first[k] ≤ h (block_of_row's search), −1 below first[0], from first[n_ranges] on
// — so 2^64 − 1 is never mapped — and without ranges.
struct height_map {
  const uint64_t *first;
  const uint32_t *range_set;
  uint32_t n_ranges;
};
__host__ __device__ __forceinline__ int32_t height_map_set(const height_map &m, uint64_t h) {
  if (m.n_ranges == 0 || h < m.first[0] || h >= m.first[m.n_ranges]) return -1;
  uint32_t lo = 0, hi = m.n_ranges - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (m.first[mid] <= h) lo = mid;
    else hi = mid - 1;
  }
  return (int32_t)m.range_set[lo];
}

// The set a parsed message is judged under: none (−1) when the walks left it NEEDS_HOST (nothing about it is decided here),
// when it has no View (there is no height to speak of), or when its height is in no range.  A View that is present but empty
// has height 0, which is a height like any other.  Rows recoded by wire_recode_kernel carry their decoded height by now.
__host__ __device__ __forceinline__ int32_t wire_row_set_row(const wire::row_info &ri, const height_map &m) {
  if (ri.status != wire::STATUS_OK || !ri.has_view) return -1;
  return height_map_set(m, ri.height);
}

// ---- one row of the tally ---------------------------------------------------------------------------------------------------
struct wire_sets_row_t {
  int si;          // index of the sender in the row's set, −1: no verdict bit or no member
  bool bit;        // the row's verdict under its set
  bool clear;      // the work mask holds a bit for this row that has to go
  bool counts;     // a member of its set: the row may add the member's power
  uint32_t entry;  // (counts) the member's entry in the packed power column = its bit in the distinct-sender bitmap
};
// set_meta[s] = {first entry of set s in the packed columns, its distinct addresses} (ibft_set_validator_sets)
__host__ __device__ __forceinline__ wire_sets_row_t wire_sets_row(bool bit, int union_idx, int32_t set, const int32_t *__restrict__ setidx,
                                                                  uint32_t n_union, const uint2 *__restrict__ set_meta) {
  wire_sets_row_t r;
  if (set < 0) {  // pre-flagged in front of the verdict launch: no kernel sets its bit; should one, it goes
    r.si = -1;
    r.bit = false;
    r.clear = bit;
    r.counts = false;
    r.entry = 0;
    return r;
  }
  const valsets_row_t v = valsets_row(bit, union_idx, setidx, n_union, (uint32_t)set);
  r.si = v.si;
  r.bit = v.bit;
  r.clear = v.clear;
  r.counts = v.si >= 0;  // unknown signers contribute 0 (validator_manager.go:88-92)
  r.entry = r.counts ? set_meta[set].x + (uint32_t)v.si : 0u;
  return r;
}

}  // namespace ibftk
