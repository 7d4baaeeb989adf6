// wire_seals_dev.h — the committed seals of the live route's COMMIT records (ibft_verify_messages_wire_views): handleCommit
// counts a stored COMMIT only if IsValidCommittedSeal(proposalHash, seal) holds (core/ibft.go:931-946), so the seal of every
// COMMIT that can count is a second row of the SAME verdict launch that judges the envelopes — sender rows [0, n), seal rows
// DENSE behind them from half = ⌈n/64⌉·64 on: the k-th sealable row in ascending row order is seal row half + k.
//
//   row_flags     what is decided about a parsed row before any ECDSA: ROW_COMMIT — a COMMIT (type 2, CommitMessage) that has
//                 a set —, ROW_SEALABLE — such a row with a 20-byte From, a 65-byte seal, a 32-byte proposal hash, whose From
//                 is a MEMBER of the row's set (the union's address table, then the family's setidx).  An outsider, or a
//                 member of the union outside the row's set, loses its sender bit whatever its signature says: its seal buys
//                 no second ECDSA.  A hash that is not 32 bytes equals no proposal hash (IsValidProposalHash): no arithmetic.
//   seal_bit      a row's bit of out_seal: the row is VALID (final sender bit), sealable, and its seal row's verdict bit is
//                 set — the seal recovers to From over the digest the seal-digest convention derives from the carried hash.
//   counts        whether a stored row adds its sender's power to its view's record: always for a view that is no COMMIT
//                 view, for a COMMIT view only when the row is sealed (messages.GetValidMessages filters the store).
//
// The record's seal form is wviews::view_record(…, seal_form = true) (wire_views_dev.h).  Everything here is
// __host__ __device__: csrc/host_wire_view_seals_harness.hip runs it on the CPU against tests/wire_view_seals_model.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_views_dev.h"

namespace wseals {

constexpr uint32_t NONE = 0xFFFFFFFFu;  // seal row of a row that is not sealable
constexpr uint8_t ROW_COMMIT = 1, ROW_SEALABLE = 2;

// f: only the lookup fields are read (vtab, vslot_mask, setidx, n_union)
__host__ __device__ inline uint8_t row_flags(const wire::row_info &ri, int32_t set, const wviews::family &f) {
  if (ri.status != wire::STATUS_OK || set < 0 || ri.type != wviews::TYPE_COMMIT || ri.payload_kind != wire::KIND_COMMIT) return 0;
  if (ri.from_len != 20 || ri.seal_len != 65 || ri.hash_len != 32) return ROW_COMMIT;
  uint32_t a[5];
  for (int i = 0; i < 5; i++)
    a[i] = (uint32_t)ri.from[4 * i] | ((uint32_t)ri.from[4 * i + 1] << 8) | ((uint32_t)ri.from[4 * i + 2] << 16) | ((uint32_t)ri.from[4 * i + 3] << 24);
  const int si = ibftk::valsets_set_index(f.setidx, f.n_union, (uint32_t)set, ibftk::valset_lookup(f.vtab, f.vslot_mask, a));
  return si >= 0 ? (uint8_t)(ROW_COMMIT | ROW_SEALABLE) : ROW_COMMIT;
}

// seal_words: the verdict words of the seal half (seal row half + k is bit k)
__host__ __device__ inline bool seal_bit(bool valid, uint32_t seal_row, const uint64_t *seal_words) {
  return valid && seal_row != NONE && ((seal_words[seal_row >> 6] >> (seal_row & 63)) & 1ull);
}

__host__ __device__ inline bool counts(uint8_t type, bool stored, bool sealed) { return stored && (type != wviews::TYPE_COMMIT || sealed); }

}  // namespace wseals
