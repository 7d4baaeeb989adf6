// wire_views_dev.h — the live route's quorum records (ibft_verify_senders_wire_views): behind the sets call's kernels every
// VALID row (final verdict bit 1: a member of its height's set) is grouped on the device the way the reference's store and
// handlers group messages (messages/messages.go:64, core/ibft.go:855-873, :931-946):
//
//   view          (height, round, type) of the parsed row
//   key           the view plus (hash_len, proposal_hash[0 .. hash_len)): one record per key
//   stored        a row no later valid row of the same view and the same sender follows — what a Messages store fed the
//                 batch in row order still holds.  Per VIEW, not per key: a sender's later message with another hash replaces
//                 the earlier one.
//
//   insert_row    a valid row into two open-addressing tables of 32-bit row numbers in HBM (cert_dedup_dev.h's scheme: a power
//                 of two of slots cleared to EMPTY, linear probing, compare-and-swap to claim, a slot's owner only ever
//                 changes among rows of EQUAL key and a slot is never freed): the KEY table keeps the LOWEST row of a key
//                 (atomicMin), the LAST table, keyed by (view, index of the sender in the row's set), the HIGHEST (atomicMax).
//                 Probing is bounded by the slot count, not by a constant: a row that gave up could not fall back without
//                 changing the answer.  With at most n keys in more than n slots a free slot always exists; a row that
//                 exhausts the table nevertheless returns UNPLACED, the kernel raises the error word and the call fails.  A
//                 per-context salt goes into both hashes: nobody outside can aim valid messages at one probe run.
//   is_rep        the row is its key's representative (the key table's slot holds it): representatives, ranked in ascending
//                 row order, number the views.
//   is_stored     the last table's slot holds the row.
//   find_last     the stored row of (view, sender index), or none — how the record step asks for the proposer's PREPARE.
//   view_record   a view's sums → its ibft_wire_view_t, the PREPARE rule (validator_manager.go:99-127) included.  Its SEAL form
//                 (ibft_verify_messages_wire_views; the rows' side: wire_seals_dev.h) reads one more count, the stored rows
//                 that added their power, and marks a COMMIT record pad[SEAL_RULE] = 1.
//
// Everything here is __host__ __device__: csrc/host_wire_views_harness.hip runs it on the CPU against
// tests/wire_views_model.py.  Nothing depends on the table size, the salt or the order rows arrive in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cert_decide_dev.h"
#include "recover_dev.h"
#include "wire_dev.h"
#include "wire_sets_dev.h"

namespace wviews {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;     // a free table word (rows are numbered below 2^31)
constexpr uint32_t UNPLACED = 0xFFFFFFFFu;  // slot of a row: the table was exhausted (an error)
constexpr uint32_t SKIP = 0xFFFFFFFEu;      // slot of a row that is not valid
constexpr int32_t VIEW_NONE = -1, VIEW_OVER = -2;
constexpr uint8_t TYPE_PREPARE = 1, TYPE_COMMIT = 2;

// mirrors ibft_tally_t and ibft_wire_view_t (include/ibftgpu.h)
struct tally_t {
  uint64_t quorum_lo, quorum_hi, power_lo, power_hi;
  uint32_t valid_rows, distinct_senders, has_quorum, shard_overlap, proposer_rows, reserved;
};
struct view_t {
  uint64_t height, round;
  int32_t set;
  uint32_t first_row, rows, stored_rows;
  uint8_t type, hash_len, prepare_rule, pad[5];
  uint8_t proposal_hash[32];
  tally_t tally;
};
static_assert(sizeof(tally_t) == 56 && sizeof(view_t) == 128, "ABI");

// Slots of each table for n rows: a power of two ≥ 2·n (at least 64); hook ≠ 0 (IBFT_WIRE_VIEWS_SLOTS, tests) lowers it to the
// largest power of two ≤ hook, never below the smallest power of two ABOVE n.
__host__ __device__ inline uint32_t table_slots(uint32_t n, uint32_t hook) {
  uint32_t s = 64;
  while (s < 0x80000000u && s < 2ull * n) s <<= 1;
  if (hook) {
    uint32_t floor_ = 1, c = 1;
    while (floor_ <= n) floor_ <<= 1;
    while (c <= hook / 2) c <<= 1;
    if (c < floor_) c = floor_;
    if (c < s) s = c;
  }
  return s;
}

// the columns the tables are keyed by: all written by earlier launches
struct columns {
  const wire::row_info *rows;
  const int32_t *vidx;  // index of the sender in the row's set (valid rows: ≥ 0)
};

__host__ __device__ inline uint32_t mix(uint32_t h, uint32_t w) {
  h = (h ^ w) * 0x85EBCA6Bu;
  return (h << 13) | (h >> 19);
}
__host__ __device__ inline uint32_t finish(uint32_t h) {
  h ^= h >> 16;
  h *= 0xC2B2AE35u;
  return h ^ (h >> 15);
}
__host__ __device__ inline uint32_t view_hash(const wire::row_info &r, uint32_t salt) {
  uint32_t h = 0x9E3779B9u ^ salt;
  h = mix(h, (uint32_t)r.height);
  h = mix(h, (uint32_t)(r.height >> 32));
  h = mix(h, (uint32_t)r.round);
  h = mix(h, (uint32_t)(r.round >> 32));
  return mix(h, r.type);
}
__host__ __device__ inline uint32_t hash_len_of(const wire::row_info &r) { return r.hash_len < 32 ? r.hash_len : 32u; }
__host__ __device__ inline uint32_t key_hash(const wire::row_info &r, uint32_t salt) {
  uint32_t h = view_hash(r, salt);
  const uint32_t len = hash_len_of(r);
  h = mix(h, len);
  for (uint32_t i = 0; i < 32; i += 4) {  // (bytes past hash_len are no part of the key)
    uint32_t w = 0;
    for (uint32_t j = 0; j < 4; j++) w |= (i + j < len ? (uint32_t)r.proposal_hash[i + j] : 0u) << (8 * j);
    h = mix(h, w);
  }
  return finish(h);
}
__host__ __device__ inline uint32_t last_hash(const wire::row_info &r, int32_t si, uint32_t salt) {
  return finish(mix(view_hash(r, salt ^ 0x5BD1E995u), (uint32_t)si));
}
__host__ __device__ inline bool view_equal(const wire::row_info &a, const wire::row_info &b) {
  return a.height == b.height && a.round == b.round && a.type == b.type;
}
__host__ __device__ inline bool key_equal(const wire::row_info &a, const wire::row_info &b) {
  if (!view_equal(a, b) || hash_len_of(a) != hash_len_of(b)) return false;
  uint32_t diff = 0;
  const uint32_t len = hash_len_of(a);
  for (uint32_t i = 0; i < len; i++) diff |= (uint32_t)(a.proposal_hash[i] ^ b.proposal_hash[i]);
  return diff == 0;
}

// The tables' atomics; on the host (one row after the other) plain operations.
__host__ __device__ inline uint32_t slot_claim(uint32_t *slot, uint32_t row) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(slot, EMPTY, row);
#else
  const uint32_t old = *slot;
  if (old == EMPTY) *slot = row;
  return old;
#endif
}
__host__ __device__ inline void slot_lower(uint32_t *slot, uint32_t row) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(slot, row);
#else
  if (row < *slot) *slot = row;
#endif
}
__host__ __device__ inline void slot_raise(uint32_t *slot, uint32_t row) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(slot, row);
#else
  if (row > *slot) *slot = row;
#endif
}
// a table word other workgroups update
__host__ __device__ inline uint32_t slot_read(const uint32_t *slot) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *slot;
#endif
}

// One insert: probe from `start`, claim a free slot or join the slot whose owner has the row's key (same(owner)); → the slot,
// or UNPLACED after `slots` probes.  LOWEST: the slot keeps the lowest row of its key, else the highest.
template <bool LOWEST, class Same>
__host__ __device__ inline uint32_t insert(uint32_t *table, uint32_t slots, uint32_t start, uint32_t row, Same same) {
  const uint32_t slot_mask = slots - 1u;
  uint32_t s = start & slot_mask;
  for (uint32_t probe = 0; probe < slots; probe++, s = (s + 1u) & slot_mask) {
    const uint32_t owner = slot_claim(table + s, row);
    if (owner == EMPTY) return s;
    if (owner == row || same(owner)) {
      if (LOWEST) slot_lower(table + s, row);
      else slot_raise(table + s, row);
      return s;
    }
  }
  return UNPLACED;
}

struct row_slots {
  uint32_t key, last;  // SKIP: the row is not valid; UNPLACED: a table was exhausted
};
__host__ __device__ inline row_slots insert_row(const columns &k, uint32_t row, bool valid, uint32_t *key_table, uint32_t *last_table,
                                                uint32_t slots, uint32_t salt) {
  row_slots r{SKIP, SKIP};
  if (!valid) return r;  // an outsider's garbage creates neither views nor probes
  const wire::row_info &me = k.rows[row];
  const int32_t si = k.vidx[row];
  r.key = insert<true>(key_table, slots, key_hash(me, salt), row, [&](uint32_t o) { return key_equal(k.rows[o], me); });
  // height fixes the set, so the index in the set names the sender
  r.last = insert<false>(last_table, slots, last_hash(me, si, salt), row,
                         [&](uint32_t o) { return view_equal(k.rows[o], me) && k.vidx[o] == si; });
  return r;
}
// after every row has been inserted
__host__ __device__ inline bool is_rep(const uint32_t *key_table, uint32_t slot, uint32_t row) {
  return slot < SKIP && slot_read(key_table + slot) == row;
}
__host__ __device__ inline bool is_stored(const uint32_t *last_table, uint32_t slot, uint32_t row) {
  return slot < SKIP && slot_read(last_table + slot) == row;
}
// the stored row of (the view of `like`, sender index si), EMPTY: none
__host__ __device__ inline uint32_t find_last(const columns &k, const uint32_t *last_table, uint32_t slots, uint32_t salt,
                                              const wire::row_info &like, int32_t si) {
  const uint32_t slot_mask = slots - 1u;
  uint32_t s = last_hash(like, si, salt) & slot_mask;
  for (uint32_t probe = 0; probe < slots; probe++, s = (s + 1u) & slot_mask) {
    const uint32_t owner = slot_read(last_table + s);
    if (owner == EMPTY) return EMPTY;
    if (view_equal(k.rows[owner], like) && k.vidx[owner] == si) return owner;
  }
  return EMPTY;
}
// out_view of a valid row whose key's representative has rank `rank`
__host__ __device__ inline int32_t view_of_rank(uint32_t rank, uint32_t views_cap) { return rank < views_cap ? (int32_t)rank : VIEW_OVER; }

// ---- one view's record ------------------------------------------------------------------------------------------------------
// What the record step knows besides the view's sums.
struct family {
  const int32_t *setidx;     // n_sets × n_union
  const uint2 *set_meta;     // n_sets × {first entry, distinct addresses}
  const uint32_t *vpower32;  // Σ set sizes × n_pieces
  const uint64_t *quorum;    // n_sets × TALLY_SUM_WORDS
  const uint32_t *vtab;      // the union's address table (recover_dev.h: valset_lookup)
  uint32_t vslot_mask, n_union;
  int n_pieces;
};
// acc: the pieces of the powers of the view's stored rows, then rows | stored << 32.  out_view: the rows' views (complete).
// seal_form: the pieces are those of the stored rows that COUNT (wseals::counts: in a COMMIT view the sealed ones), their
// number follows in acc[n_pieces + 1]; a COMMIT record says so in pad[SEAL_RULE].
constexpr int SEAL_RULE = 0;  // IBFT_WIRE_VIEW_SEAL_RULE
__host__ __device__ inline void view_record(view_t &o, uint32_t first_row, const uint64_t *acc, const columns &k, const int32_t *row_set,
                                            const int32_t *out_view, int32_t v, const family &f, const certd::proposer_table &t,
                                            const uint32_t *last_table, uint32_t slots, uint32_t salt, bool seal_form = false) {
  const wire::row_info &me = k.rows[first_row];
  const int32_t set = row_set[first_row];
  const uint32_t len = hash_len_of(me);
  o.height = me.height;
  o.round = me.round;
  o.set = set;
  o.first_row = first_row;
  o.rows = (uint32_t)(acc[f.n_pieces] & 0xFFFFFFFFull);
  o.stored_rows = (uint32_t)(acc[f.n_pieces] >> 32);
  o.type = me.type;
  o.hash_len = (uint8_t)len;
  o.prepare_rule = 0;
  for (int i = 0; i < 5; i++) o.pad[i] = 0;
  if (seal_form && me.type == TYPE_COMMIT) o.pad[SEAL_RULE] = 1;
  const uint32_t counted = seal_form ? (uint32_t)acc[f.n_pieces + 1] : o.stored_rows;
  for (uint32_t i = 0; i < 32; i++) o.proposal_hash[i] = i < len ? me.proposal_hash[i] : 0;
  uint64_t piece[ibftk::TALLY_MAX_PIECES];
  for (int i = 0; i < ibftk::TALLY_MAX_PIECES; i++) piece[i] = i < f.n_pieces ? acc[i] : 0ull;
  uint32_t distinct = counted, proposer_rows = 0;  // stored rows are unique per (view, sender)
  // HasPrepareQuorum: the proposer's seat joins, a stored PREPARE of the proposer voids the quorum
  const uint8_t *p = me.type == TYPE_PREPARE ? certd::table_lookup(t, me.height, me.round) : nullptr;
  if (p) {
    o.prepare_rule = 1;
    uint32_t a[5];
    for (int i = 0; i < 5; i++) a[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
    const int pi = ibftk::valsets_set_index(f.setidx, f.n_union, (uint32_t)set, ibftk::valset_lookup(f.vtab, f.vslot_mask, a));
    if (pi >= 0) {  // (a proposer outside the set has no valid row here and no seat)
      const uint32_t r = find_last(k, last_table, slots, salt, me, pi);
      if (r != EMPTY && out_view[r] == v) {
        proposer_rows = 1;
      } else {
        distinct++;
        const uint32_t entry = f.set_meta[set].x + (uint32_t)pi;
        for (int i = 0; i < f.n_pieces; i++) piece[i] += f.vpower32[(size_t)entry * f.n_pieces + i];
      }
    }
  }
  const uint64_t *q = f.quorum + (size_t)set * ibftk::TALLY_SUM_WORDS;
  uint64_t rec[4];
  ibftk::tally_record(piece, f.n_pieces, 0ull, q, proposer_rows, rec);
  o.tally.quorum_lo = q[0];
  o.tally.quorum_hi = q[1];
  o.tally.power_lo = rec[0];
  o.tally.power_hi = rec[1];
  o.tally.valid_rows = counted;
  o.tally.distinct_senders = distinct;
  o.tally.has_quorum = (uint32_t)rec[3];
  o.tally.shard_overlap = 0;
  o.tally.proposer_rows = proposer_rows;
  o.tally.reserved = 0;
}

}  // namespace wviews
