// cert_dedup_dev.h — the certificate tree's opt-in dedup (IBFT_FLAG_CERT_DEDUP; cert_dedup_kernels.h: cert_dedup_*_kernel): the
// rows of a verdict launch that carry the same (digest, signature, From) are one signature to check.  The row logic lives
// here as __host__ __device__ functions, so that host_cert_dedup_harness.hip runs the exact source on the CPU:
//
//   insert_row    one row into an open-addressing table of 32-bit words in HBM (a power-of-two number of slots, cleared to
//                 EMPTY): linear probing from key_hash; at each slot compare-and-swap EMPTY → row, else compare the owner's
//                 117 key bytes with the row's own — equal: atomicMin(slot, row) and stop, different: next slot.  A slot's
//                 owner only ever changes among rows of EQUAL key, and a slot is never freed, so every row of a key ends at
//                 the same slot whatever the order, and the slot's final value is the LOWEST row of the key.  The columns
//                 were written by earlier kernels: nothing is published through the table but row numbers.
//   MAX_PROBES    after that many slots the row gives up (SLOT_UNPLACED) and is its own representative: correctness never
//                 rests on a match being found, and a batch crafted to collide in the table costs at most MAX_PROBES key
//                 compares per row before it is verified row by row, as without the flag.  128: with at most one key per
//                 two slots and a hash that spreads them, the longest run of occupied slots among 2^20 keys is about
//                 ln n / (α − 1 − ln α) ≈ 72 at α = 1/2 — honest batches never reach the bound (tests/cert_dedup_model.py
//                 checks the run length of every GPU-test input).
//   rep_of        a row's representative: the final value of its slot.  Representatives (rep == row) are compacted in
//                 ascending row order into a dense batch (gather_row), judged by ONE verdict launch, and scatter_bit hands
//                 every row its representative's bit.  Rows with a pre-flag take no part: never inserted, never a
//                 representative, bit 0 — exactly what the verdict kernels give them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cdd {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;          // a free table word (rows are numbered below 2^31)
constexpr uint32_t SLOT_UNPLACED = 0xFFFFFFFFu;  // slot_of[row]: the row gave up after MAX_PROBES slots
constexpr uint32_t SLOT_SKIP = 0xFFFFFFFEu;      // slot_of[row]: the row has a pre-flag
constexpr uint32_t NO_REP = 0xFFFFFFFFu;
constexpr uint32_t MAX_PROBES = 128;
constexpr uint32_t KEY_BYTES = 32 + 65 + 20;

// the verdict columns (d_hash, d_sig, d_signer, d_pre): row r's key is digest32[32r..] ‖ sig65[65r..] ‖ from20[20r..]
struct columns {
  uint8_t *digest32, *sig65, *from20, *pre;
};

// Slots of the table for a launch of `rows` rows: a power of two, at least 2 × rows (at least 64); cap ≠ 0 (the test hook
// IBFT_CERT_DEDUP_SLOTS, rounded down to a power of two, at least 1) bounds it from above.
__host__ __device__ inline uint32_t table_slots(uint32_t rows, uint32_t cap) {
  uint32_t s = 64;
  while (s < 0x80000000u && s < 2ull * rows) s <<= 1;
  if (cap) {
    uint32_t c = 1;
    while (c <= cap / 2) c <<= 1;
    if (c < s) s = c;
  }
  return s;
}

__host__ __device__ inline uint32_t ld32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__host__ __device__ inline uint32_t mix(uint32_t h, uint32_t w) {
  h = (h ^ w) * 0x85EBCA6Bu;
  return (h << 13) | (h >> 19);
}
// Where a key starts probing: every word of the digest AND of the signature (r ‖ s, then v) — whoever crafts rows chooses the
// signature freely for a fixed digest.  From is left to the compare.
__host__ __device__ inline uint32_t key_hash(const columns &k, uint32_t row) {
  const uint8_t *d = k.digest32 + 32ull * row, *s = k.sig65 + 65ull * row;
  uint32_t h = 0x9E3779B9u;
  for (int i = 0; i < 8; i++) h = mix(h, ld32(d + 4 * i));
  for (int i = 0; i < 16; i++) h = mix(h, ld32(s + 4 * i));
  h = mix(h, s[64]);
  h ^= h >> 16;
  h *= 0xC2B2AE35u;
  return h ^ (h >> 15);
}
__host__ __device__ inline bool key_equal(const columns &k, uint32_t a, uint32_t b) {
  const uint8_t *da = k.digest32 + 32ull * a, *db = k.digest32 + 32ull * b;
  const uint8_t *sa = k.sig65 + 65ull * a, *sb = k.sig65 + 65ull * b;
  const uint8_t *fa = k.from20 + 20ull * a, *fb = k.from20 + 20ull * b;
  uint32_t diff = 0;
  for (int i = 0; i < 8; i++) diff |= ld32(da + 4 * i) ^ ld32(db + 4 * i);
  if (diff) return false;  // (most rows that share a slot's neighbourhood differ here)
  for (int i = 0; i < 16; i++) diff |= ld32(sa + 4 * i) ^ ld32(sb + 4 * i);
  diff |= (uint32_t)(sa[64] ^ sb[64]);
  for (int i = 0; i < 5; i++) diff |= ld32(fa + 4 * i) ^ ld32(fb + 4 * i);
  return diff == 0;
}

// The table's two atomics; on the host (one row after the other) plain operations.
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

// → the row's slot, SLOT_SKIP (pre-flagged) or SLOT_UNPLACED (gave up)
__host__ __device__ inline uint32_t insert_row(const columns &k, uint32_t row, uint32_t *table, uint32_t slot_mask) {
  if (k.pre[row] != 0) return SLOT_SKIP;
  uint32_t s = key_hash(k, row) & slot_mask;
  for (uint32_t probe = 0; probe < MAX_PROBES; probe++, s = (s + 1u) & slot_mask) {
    const uint32_t owner = slot_claim(table + s, row);
    if (owner == EMPTY) return s;
    if (key_equal(k, owner, row)) {
      slot_lower(table + s, row);
      return s;
    }
  }
  return SLOT_UNPLACED;
}
// after every row has been inserted
__host__ __device__ inline uint32_t rep_of(const uint32_t *table, uint32_t slot, uint32_t row) {
  return slot == SLOT_SKIP ? NO_REP : slot == SLOT_UNPLACED ? row : table[slot];
}
// what the compaction scans: bit 0 = the row is a representative, bit 31 = it gave up (the two channels of cert_scan_dev.h)
__host__ __device__ inline uint32_t scan_word(const uint32_t *table, uint32_t slot, uint32_t row) {
  return (rep_of(table, slot, row) == row ? 1u : 0u) | (slot == SLOT_UNPLACED ? 0x80000000u : 0u);
}
// representative `row` → row `dst` of the columns (the dense batch lies behind the tree's rows)
__host__ __device__ inline void gather_row(const columns &k, uint32_t row, uint32_t dst) {
  for (int i = 0; i < 32; i++) k.digest32[32ull * dst + i] = k.digest32[32ull * row + i];
  for (int i = 0; i < 65; i++) k.sig65[65ull * dst + i] = k.sig65[65ull * row + i];
  for (int i = 0; i < 20; i++) k.from20[20ull * dst + i] = k.from20[20ull * row + i];
  k.pre[dst] = k.pre[row];
}
// the row's verdict bit: its representative's bit among the dense batch's verdict words
__host__ __device__ inline bool scatter_bit(const uint32_t *table, const uint32_t *slot_of, const uint32_t *dense_pos,
                                            const uint64_t *dense_mask, uint32_t row) {
  const uint32_t rep = rep_of(table, slot_of[row], row);
  if (rep == NO_REP) return false;
  const uint32_t d = dense_pos[rep];
  return (dense_mask[d >> 6] >> (d & 63u)) & 1ull;
}

}  // namespace cdd
