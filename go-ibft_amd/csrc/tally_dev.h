// tally_dev.h — the arithmetic of a tally, once: every tally kernel of kernels.hip.h sums the voting powers of its distinct
// senders as 32-bit PIECES (sums of 32-bit values never overflow a u64 accumulator, and a piece is one atomicAdd), and every
// one of them ends in the same record.
//
//   pieces_to_words     Σ piece_k·2^(32k) → TALLY_SUM_WORDS little-endian words (the carries)
//   words_ge            sum ≥ quorum, from the top word down
//   tally_record        sums → {power_lo, power_hi, valid | distinct << 32, has_quorum}: the ONLY place that compares a power
//                       with a quorum under the proposer rule
//
// Everything here is __host__ __device__: csrc/host_wire_sets_harness.hip runs it on the CPU against Python integers
// (tests/test_dev_wire_sets_host.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ibftk {

constexpr int TALLY_SUM_WORDS = 5;   // 256-bit powers × up to 2^20 validators < 2^276
constexpr int TALLY_MAX_PIECES = 8;  // 2·PW 32-bit pieces

// Σ piece_k·2^(32k) → TALLY_SUM_WORDS little-endian u64 words (pieces are sums of 32-bit values, < 2^60)
__host__ __device__ __forceinline__ void pieces_to_words(const uint64_t *piece, int n_pieces, uint64_t w[TALLY_SUM_WORDS]) {
  uint64_t carry = 0;  // running value >> 32 at each 32-bit position
  uint32_t half[2 * TALLY_SUM_WORDS];
#pragma unroll
  for (int k = 0; k < 2 * TALLY_SUM_WORDS; k++) {
    const uint64_t t = carry + (k < n_pieces ? piece[k] : 0ull);  // < 2^61
    half[k] = (uint32_t)t;
    carry = t >> 32;
  }
#pragma unroll
  for (int i = 0; i < TALLY_SUM_WORDS; i++) w[i] = (uint64_t)half[2 * i] | ((uint64_t)half[2 * i + 1] << 32);
}
__host__ __device__ __forceinline__ bool words_ge(const uint64_t a[TALLY_SUM_WORDS], const uint64_t *b) {
#pragma unroll
  for (int i = TALLY_SUM_WORDS - 1; i >= 0; i--) {
    if (a[i] != b[i]) return a[i] > b[i];
  }
  return true;
}

// The record of a tally.  piece[0 .. n_pieces): the 32-bit pieces of the powers of the distinct senders, summed; counts =
// valid rows | distinct senders << 32; quorum: TALLY_SUM_WORDS words; proposer_rows: valid PREPAREs sent by the proposer —
// any such row voids the quorum, whatever the power (HasPrepareQuorum, core/validator_manager.go:114-121); 0 where the rule
// does not apply.  out[0..3] = {power_lo, power_hi, counts, has_quorum}; w (or null): the power in full.
__host__ __device__ __forceinline__ void tally_record(const uint64_t *piece, int n_pieces, uint64_t counts, const uint64_t *quorum,
                                                      uint64_t proposer_rows, uint64_t out[4], uint64_t *w = nullptr) {
  uint64_t sum[TALLY_SUM_WORDS];
  pieces_to_words(piece, n_pieces, sum);
  out[0] = sum[0];
  out[1] = sum[1];
  out[2] = counts;
  out[3] = (words_ge(sum, quorum) && proposer_rows == 0) ? 1ull : 0ull;
  if (w) {
#pragma unroll
    for (int i = 0; i < TALLY_SUM_WORDS; i++) w[i] = sum[i];
  }
}

}  // namespace ibftk
