// kernels.hip.h — gfx950 kernels of the batch verifier.
//
// Product code.  Rows are go-ibft messages flattened by the host into byte
// columns; each kernel replaces the per-message callback loop of
// /root/reference/messages/messages.go:183-191.
//
//   hash_eq_kernel              a1  IsValidProposalHash   (core/ibft.go:858-861, 938)
//   proposal_hash_kernel            keccak256(raw ‖ BE64(round)), once per batch
//   proposal_digest_kernel<1|64>    n of them in one launch, the round spliced in on the device (chain sync from proposals)
//   ecrecover_lane_kernel       a2  IsValidCommittedSeal  (core/ibft.go:943)      cold path,
//   ecrecover_group_kernel<G>   a3  IsValidValidator      (core/ibft.go:1128)     1 / 2,4,8 lanes per signature
//   ecrecover_wave_kernel           same, one wavefront per signature (limbs spread over lanes, wave_fe_dev.h)
//   ecrecover_wave2_kernel          same, plus a helper wavefront per signature (scalars, u1·G)
//   ecrecover_rows_kernel           same, sixteen lanes (one DPP row) per signature, four signatures per wavefront
//   ecrecover_rows_pair_kernel      same, plus a helper wavefront per four signatures (scalars, u1·G) on the same SIMD
//   verify_known_lane_kernel    a2/a3 against the validator's known key (warm path), 1 lane per signature
//   verify_known_group_kernel<G>    same, G = 2..32 lanes per signature
//   verify_known_wave_kernel        same, one wavefront per signature in the row layout of wave_fe_dev.h
//   envelope_head / _copy / _digest<1|64> / sign_envelope_lane_kernel   f4: PREPREPARE / ROUND_CHANGE envelopes (sign_envelope_dev.h)
//   tally_kernel                a8  HasQuorum             (core/validator_manager.go:77-96)
//   block_head_kernel               chain sync (every block call): the blocks' digests → their rows, seal-digest convention fused
//   block_tally_kernel<PW, THREADS, SETS>   one HasQuorum per block; SETS: under the block's OWN validator set (a family of sets)
//   gtab_build_kernel, qtab_build_kernel, qtab_commit_kernel   one-time fixed-base tables
//   lookup_kernel                   sender → validator index for ibft_tally()
//   wire_parse_kernel, wire_stage_seals_kernel   §8f rank 3: wire bytes → columns on the device (wire_dev.h)
//   wire_recode_kernel                            the same for non-canonical encodings, opt-in (wire_recode_dev.h)
//
// Layout in HBM: one contiguous byte column per field (hash N×32, sig N×65, signer N×20,
// pre_flags N) — structure-of-arrays at field granularity.  The lane kernels stage a block's
// 64 rows through LDS with coalesced dword loads and each lane unpacks its own row into limbs held
// in VGPRs; the group kernels read their row directly (the G lanes of a group share the address).
// The verdict kernels (ecrecover_*, verify_known_*) share their row head (row_sig, row_digest, claimed_signer, row_pre /
// row_done), the warm decision (warm_decide, warm_mark) and the cold verdict tail (cold_tail): below recover_args.  Two of the nine
// still spell their own: ecrecover_lane_kernel (LDS-staged rows, whole verdict words) and verify_known_group_kernel.
// Rule for every kernel here: no call to an outlined device function under a partial EXEC mask
// (see secp256k1_dev.h:wave_any) — idle lanes compute on dummy operands and skip only stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "recover_dev.h"
#include "verify_dev.h"
#include "sign_dev.h"
#include "sign_message_dev.h"
#include "sign_envelope_dev.h"
#include "wave_fe_dev.h"
#include "wire_dev.h"
#include "wire_recode_dev.h"
#include "wire_sets_dev.h"
#include "cert_wave_dev.h"
#include "cert_verdict_dev.h"
#include "cert_decide_dev.h"
#include "wire_views_dev.h"
#include "round_change_dev.h"
#include "wire_seals_dev.h"
#include "cert_dedup_dev.h"

namespace ibftk {

using secp::aff;
using secp::jac;
using secp::u256;

constexpr int ROWS_PER_BLOCK = 64; // one wavefront per block in the lane kernel
static_assert(ROWS_PER_BLOCK == 64, "sign_dev.h: lane_row frames a workgroup of one wavefront");

// (validator table lookup — valset_lookup — and a row's decision once the curve is done — emit_row, claim_row — live in
// recover_dev.h: the CPU harness compiles them too)

// ---- host columns → HBM in one launch --------------------------------------------------------------------
// A batch arrives as 4–9 separate byte columns.  One hipMemcpyAsync per column costs ≈8 µs of host time each and the
// copies run one behind the other (profiles/r02h_seq_*: 134 µs before the first kernel of a COMMIT set).  When the
// caller keeps its columns in ibft_pinned_alloc buffers the device can read them itself: one launch, every segment
// read with 16-byte loads straight over PCIe (≈1.3 MB: ≈25 µs).  Pageable columns keep the per-column copies.
constexpr int GATHER_MAX = 12;
constexpr int GATHER_BLOCK_BYTES = 256 * 16;
constexpr uint32_t GATHER_DIGEST_LDS = 32 * 1024;
struct gather_args {
  const uint8_t *src[GATHER_MAX];
  uint8_t *dst[GATHER_MAX];
  uint32_t bytes[GATHER_MAX];
  uint32_t first_block[GATHER_MAX + 1];  // segment s owns blocks [first_block[s], first_block[s+1])
  uint32_t n;
  // optional digest job (a message set): the PayloadNoSig column is NOT copied — the blocks after the copy blocks read 64
  // rows each from the host column into LDS (coalesced) and write keccak256(row) into the digest column
  const uint8_t *pay_src;   // host (pinned), or null
  const uint32_t *off_src;  // host (pinned): n_rows + 1 offsets
  uint8_t *digest_dst;      // HBM: n_rows × 32
  uint32_t n_rows, pay_bytes;
};
__device__ __forceinline__ void hash_range_dwords(const uint8_t *__restrict__ in, uint32_t len, uint64_t out4[4]);
// DIGEST = true adds the digest blocks (and their 32 KiB of LDS per workgroup) to the launch.
template <bool DIGEST>
__global__ void __launch_bounds__(256) gather_columns_kernel(gather_args a) {
  __shared__ __attribute__((aligned(16))) uint8_t lbuf[DIGEST ? GATHER_DIGEST_LDS + 16 : 16];
  if (DIGEST && blockIdx.x >= a.first_block[a.n]) {
    // ---- digest blocks: 64 rows; all four wavefronts bring the rows into LDS (PCIe reads are latency-bound: many
    // requests in flight), the first one hashes ----
    const uint32_t row0 = (blockIdx.x - a.first_block[a.n]) * 64u, lane = threadIdx.x & 63u;
    if (row0 >= a.n_rows) return;
    const uint32_t cnt = a.n_rows - row0 < 64u ? a.n_rows - row0 : 64u;
    const uint32_t row = row0 + (lane < cnt ? lane : cnt - 1);
    const uint32_t o0 = a.off_src[row], o1 = a.off_src[row + 1];
    const uint32_t first = __shfl(o0, 0, 64), last = __shfl(o1, (int)cnt - 1, 64);
    const uint32_t b0 = first & ~15u;
    const bool staged = last - b0 <= GATHER_DIGEST_LDS && ((reinterpret_cast<uintptr_t>(a.pay_src) & 15u) == 0);  // block-uniform
    if (staged) {
      for (uint32_t i = 16u * threadIdx.x; b0 + i < last; i += 4096u) {  // 16-byte loads over PCIe, never past the column's end
        if (b0 + i + 16u <= a.pay_bytes) {
          *reinterpret_cast<uint4 *>(lbuf + i) = *reinterpret_cast<const uint4 *>(a.pay_src + b0 + i);
        } else {
          for (uint32_t j = 0; b0 + i + j < a.pay_bytes; j++) lbuf[i + j] = a.pay_src[b0 + i + j];
        }
      }
      __syncthreads();
    }
    if (threadIdx.x >= 64) return;
    uint64_t d[4];
    if (staged)
      hash_range_dwords(lbuf + (o0 - b0), o1 - o0, d);  // dword reads may run a few bytes past the row: inside the buffer
    else
      keccak::hash_bytes(a.pay_src + o0, o1 - o0, d);   // rows too long for the buffer: exact byte reads from the host column
    if (lane < cnt) {
      uint4 *o = reinterpret_cast<uint4 *>(a.digest_dst + 32ull * row);
      o[0] = make_uint4((uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32));
      o[1] = make_uint4((uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32));
    }
    return;
  }
  uint32_t s = 0;
#pragma unroll 1
  while (s + 1 < a.n && blockIdx.x >= a.first_block[s + 1]) s++;
  const uint32_t off = (blockIdx.x - a.first_block[s]) * (uint32_t)GATHER_BLOCK_BYTES + threadIdx.x * 16u;
  const uint32_t len = a.bytes[s];
  if (off >= len) return;
  const uint8_t *src = a.src[s] + off;
  uint8_t *dst = a.dst[s] + off;
  const uint32_t take = len - off < 16u ? len - off : 16u;
  if (take == 16u && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
    *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src);
  } else if (take == 16u && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3u) == 0) {
    const uint32_t *sp = reinterpret_cast<const uint32_t *>(src);
    uint32_t *dp = reinterpret_cast<uint32_t *>(dst);
    const uint32_t w0 = sp[0], w1 = sp[1], w2 = sp[2], w3 = sp[3];
    dp[0] = w0; dp[1] = w1; dp[2] = w2; dp[3] = w3;
  } else {
    for (uint32_t i = 0; i < take; i++) dst[i] = src[i];
  }
}

// ---- Keccak-256 of a byte range in HBM, one lane, dword loads ------------------------------------------
// keccak::hash_bytes reads the message a byte at a time (it also runs on the CPU test harness): 136 dependent-
// looking byte loads per block cost more than the permutation itself (payload_digest_kernel: 41 µs for one block
// per lane, profiles/r02g_seq_kernel_stats.csv).  Here a block is 35 aligned dword loads issued together and
// realigned with funnel shifts.  Reads up to 7 bytes past the end of the range: the payload buffers carry 256
// bytes of slack (ibftgpu.hip).
__device__ __forceinline__ void hash_range_dwords(const uint8_t *__restrict__ in, uint32_t len, uint64_t out4[4]) {
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < 25; i++) s[i] = 0;
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(in) & 3u), sh = 8u * mis;
  const uint32_t *p = reinterpret_cast<const uint32_t *>(in - mis);
  for (;;) {
    const uint32_t take = len < 136u ? len : 136u;  // message bytes in this block
    const uint32_t nd = (take + 3u) >> 2;           // dwords that hold them
    uint32_t raw[35];
#pragma unroll
    for (int j = 0; j < 35; j++) raw[j] = (uint32_t)j <= nd ? p[j] : 0u;
    uint32_t w[34];
#pragma unroll
    for (int j = 0; j < 34; j++) {
      const uint32_t v = (uint32_t)(((uint64_t)raw[j + 1] << 32 | raw[j]) >> sh);  // bytes 4j..4j+3 of the block
      const uint32_t have = take > 4u * (uint32_t)j ? take - 4u * (uint32_t)j : 0u;  // how many of them are message bytes
      w[j] = have >= 4u ? v : (have ? (v & ((1u << (8u * have)) - 1u)) : 0u);
      // pad10*1: first bit right after the message … (static register index: no scratch)
      w[j] |= (take < 136u && (take >> 2) == (uint32_t)j) ? 0x01u << (8u * (take & 3u)) : 0u;
    }
#pragma unroll
    for (int i = 0; i < 17; i++) s[i] ^= (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    if (take < 136u) s[16] ^= 0x8000000000000000ULL;               // … last bit at byte 135
    keccak::f1600(s);
    if (take < 136u) break;
    p += 34;
    len -= 136u;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) out4[i] = s[i];
}

// ---- fixed-base table build (entries computed by recover_dev.h:gtab_entry) ----------
__global__ void gtab_build_kernel(uint32_t *__restrict__ gtab) {
  int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= GTAB_WINDOWS * GTAB_ENTRIES) return;
  gtab_entry(tid / GTAB_ENTRIES, tid % GTAB_ENTRIES, gtab + (size_t)GTAB_ENTRY_DWORDS * tid);
}

// ---- f4: signing side, one lane per seal (sign_dev.h) ------------------------------------------------
// Writes the same columns ibft_seals_stage fills (hash32 is already there; sig65 and signer20 are produced
// here), so the batch it signed is a staged batch: ibft_seals_run verifies it without another upload.
struct sign_args {
  const uint32_t *gtab;
  const uint8_t *sk32;     // n × 32, big-endian secret keys
  const uint8_t *hash32;   // n × 32, the proposal hash each row seals
  uint8_t *sig65;          // n × 65 out
  uint8_t *signer20;       // n × 20 out
  uint8_t *ok;             // n out: 1 = signed, 0 = key outside [1, n)
  uint32_t n;
};
// NONCE = SIGN_NONCE_KECCAK is the kernel as it always was; SIGN_NONCE_RFC6979 derives the nonce with the HMAC-SHA-256 DRBG
// (sign_dev.h: rfc6979_drbg) — same arguments, same columns, same stores.
template <int NONCE>
__global__ void __launch_bounds__(ROWS_PER_BLOCK) sign_lane_kernel(sign_args a) {
  const lane_row l(a.n);
  uint8_t sk[32], dg[32];
  load_row32(a.sk32, l.src, sk);
  load_row32(a.hash32, l.src, dg);
  u256 r, s;
  uint32_t v, addr[5];
  const bool ok = sign_row<NONCE>(a.gtab, sk, dg, r, s, v, addr, 0u);
  if (!l.live) return;
  put_sig65(a.sig65 + 65ull * l.row, r, s, v);  // 65-byte rows are not dword aligned: byte stores
  store_addr20(a.signer20, l.row, addr);
  a.ok[l.row] = ok ? 1 : 0;
}

// ---- f4, one layer up: a whole PREPARE / COMMIT message per lane, as wire bytes (sign_message_dev.h) --------------------
// One lane per message, one wavefront per 64 rows, as sign_lane_kernel.  off[] comes from the host (a row's length depends on
// type, height and round only: message_wire_len), so a lane knows where its bytes go without a scan.  The payload is built in
// LDS (152 bytes per lane) and absorbed from there: no private byte array.  Idle lanes of the last wavefront run the last row
// again — sign_core votes across the wavefront — and store nothing.
struct sign_message_args {
  const uint32_t *gtab;
  const uint8_t *sk32;      // n × 32, big-endian secret keys
  const uint8_t *type;      // n: 1 = PREPARE, 2 = COMMIT (checked by the host)
  const uint64_t *height;   // n
  const uint64_t *round;    // n
  const uint8_t *hash32;    // n × 32, the proposal hash each row carries
  const uint32_t *off;      // n + 1: row i is wire[off[i], off[i+1])
  uint8_t *wire;            // out
  uint8_t *from20;          // n × 20 out
  uint8_t *ok;              // n out: 1 = signed, 0 = key outside [1, n)
  uint32_t n;
  uint32_t convert;         // the seal-digest convention: 0 = the seal signs the hash itself
  uint64_t suffix_words[9];
};
template <int NONCE>
__global__ void __launch_bounds__(ROWS_PER_BLOCK) sign_message_lane_kernel(sign_message_args a) {
  __shared__ uint64_t lds[ROWS_PER_BLOCK * SIGN_MESSAGE_BUF_WORDS];
  const lane_row l(a.n);
  uint8_t sk[32], hs[32];
  load_row32(a.sk32, l.src, sk);
  load_row32(a.hash32, l.src, hs);
  uint64_t *buf = lds + (size_t)SIGN_MESSAGE_BUF_WORDS * threadIdx.x;
  const message_row m = sign_message_row<NONCE>(a.gtab, sk, a.type[l.src], a.height[l.src], a.round[l.src], hs, a.convert, a.suffix_words, buf);
  if (!l.live) return;
  const uint32_t at = a.off[l.row];
  const bool fits = a.off[l.row + 1] - at == m.len + SIGN_MESSAGE_SIG_FIELD;  // (the host computed it with the same function)
  if (fits) store_message(a.wire + at, buf, m);
  store_addr20(a.from20, l.row, m.addr);
  a.ok[l.row] = (m.ok && fits) ? 1 : 0;
}

// ---- f4, two layers up: a PREPREPARE / ROUND_CHANGE envelope around a given body, as wire bytes (sign_envelope_dev.h) ------
// A body is any length (≈106 KB for the ROUND_CHANGE of 1 024 validators), so a row is not one lane's work: four launches on one
// stream, each the shape its step wants.  off[], dst_at[] and piece_first[] come from the host (a row's length depends on type,
// height, round and body length only: envelope_wire_len).
//   envelope_head_kernel          a lane per row: From from the key (one fixed-base multiplication), the head built in LDS and
//                                 stored with a zero signature field; no sign_core here
//   envelope_copy_kernel          256 threads per 4 096 bytes of output: the bodies behind their heads (copy_body_piece)
//   envelope_digest_kernel<1|64>  keccak256 of the stored message minus its signature field: a lane per message (wire::hash_pieces),
//                                 or a wavefront per message with the state over 25 lanes (cw::sponge_message) — the verifier's own
//                                 two routines for "bytes minus the signature field"; the host picks as proposal_form does
//   sign_envelope_lane_kernel     a lane per row: sign_core over that digest, the signature into its place — sign_lane_kernel
//                                 without the address, so its code stays below sign_lane_kernel's
// Idle lanes of the last wavefront run the last row again (sign_core votes across the wavefront) and store nothing.
struct sign_envelope_args {
  const uint32_t *gtab;
  const uint8_t *sk32;          // n × 32, big-endian secret keys
  const uint8_t *type;          // n: 0 = PREPREPARE, 3 = ROUND_CHANGE (checked by the host)
  const uint64_t *height;       // n
  const uint64_t *round;        // n
  const uint8_t *body;          // the bodies' buffer (256 bytes of slack behind it)
  const uint32_t *body_at;      // n: row i's body is body[body_at[i], body_at[i] + body_len[i]) — ranges may repeat or overlap
  const uint32_t *body_len;     // n
  const uint32_t *dst_at;       // n: where row i's body goes, off[i] + its head's length
  const uint32_t *piece_first;  // n + 1: row i owns the copy workgroups [piece_first[i], piece_first[i+1])
  const uint32_t *off;          // n + 1: row i is wire[off[i], off[i+1])
  uint8_t *wire;                // out (256 bytes of slack behind it)
  uint8_t *digest32;            // n × 32: keccak256(PayloadNoSig), between the digest and the sign launch
  uint8_t *from20;              // n × 20 out
  uint8_t *ok;                  // n out: 1 = signed, 0 = key outside [1, n)
  uint32_t n;
};
__global__ void __launch_bounds__(ROWS_PER_BLOCK) envelope_head_kernel(sign_envelope_args a) {
  __shared__ uint64_t lds[ROWS_PER_BLOCK * ENVELOPE_HEAD_WORDS];
  const lane_row l(a.n);
  uint8_t sk[32];
  load_row32(a.sk32, l.src, sk);
  u256 d;
  const bool key_ok = sign_key(sk, d);
  uint32_t addr[5];
  sign_address(a.gtab, d, key_ok, addr);
  uint8_t *p = reinterpret_cast<uint8_t *>(lds + (size_t)ENVELOPE_HEAD_WORDS * threadIdx.x);
  const uint32_t body_len = a.body_len[l.src];
  const uint32_t head = envelope_head(p, a.type[l.src], a.height[l.src], a.round[l.src], addr, body_len);
  if (!l.live) return;
  const uint32_t at = a.off[l.row];
  if (a.off[l.row + 1] - at == head + body_len) store_envelope_head(a.wire + at, p, head);  // (the host computed it with the same function)
  store_addr20(a.from20, l.row, addr);
}
__global__ void __launch_bounds__(ENVELOPE_COPY_THREADS) envelope_copy_kernel(sign_envelope_args a) {
  // the row that owns this workgroup: the last one whose first piece is not behind it (rows without a body own none)
  uint32_t lo = 0, hi = a.n;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.piece_first[mid] <= blockIdx.x) lo = mid; else hi = mid;
  }
  copy_body_piece(a.wire, a.body, a.dst_at[lo], a.body_at[lo], a.body_len[lo], blockIdx.x - a.piece_first[lo], threadIdx.x);
}
template <int LANES>
__global__ void __launch_bounds__(64) envelope_digest_kernel(sign_envelope_args a) {
  if constexpr (LANES == 1) {
    const lane_row l(a.n);
    const uint32_t o0 = a.off[l.src], len = a.off[l.src + 1] - o0;
    uint64_t d[4];
    envelope_digest_lane(a.wire + o0, len, envelope_cut(a.height[l.src], a.round[l.src]), l.live, d);  // idle lanes: the empty message
    if (l.live) {
      uint4 *o = reinterpret_cast<uint4 *>(a.digest32 + 32ull * l.row);
      o[0] = make_uint4((uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32));
      o[1] = make_uint4((uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32));
    }
  } else {
    __shared__ uint64_t A[32], B[32];
    const uint32_t row = blockIdx.x, lane = threadIdx.x;  // (grid = n: block-uniform, always a live row)
    const uint32_t o0 = a.off[row], len = a.off[row + 1] - o0;
    const uint64_t word = envelope_digest_wave(a.wire + o0, len, envelope_cut(a.height[row], a.round[row]), lane, A, B);
    if (lane < 4u) *reinterpret_cast<uint64_t *>(a.digest32 + 32ull * row + 8u * lane) = word;
  }
}
template <int NONCE>
__global__ void __launch_bounds__(ROWS_PER_BLOCK) sign_envelope_lane_kernel(sign_envelope_args a) {
  const lane_row l(a.n);
  uint8_t sk[32], dg[32];
  load_row32(a.sk32, l.src, sk);
  load_row32(a.digest32, l.src, dg);
  u256 r, s;
  uint32_t v;
  const bool ok = sign_digest<NONCE>(a.gtab, sk, dg, r, s, v);
  if (!l.live) return;
  const uint32_t row = l.row, at = a.off[row], cut = envelope_cut(a.height[row], a.round[row]);
  const bool fits = a.off[row + 1] - at == envelope_head_len(a.type[row], a.height[row], a.round[row], a.body_len[row]) + a.body_len[row];
  if (fits) put_sig65(a.wire + at + cut + 2u, r, s, v);  // into the field the head left zero
  a.ok[row] = (ok && fits) ? 1 : 0;
}

// ---- proposal hash + a1 ---------------------------------------------------------------
// One sponge is sequential; one wavefront walks it with the state spread over 25 lanes (wave_sponge: ≈5.3 µs per 136-byte
// block; a single lane — scalar 64-bit code, ≈188 operations per round — needed ≈9.4 µs).  The host hands the message over
// already padded (raw ‖ BE64(round) ‖ pad10*1 to a multiple of the rate, 8-byte aligned), so absorbing a block is one 64-bit
// load and XOR in lanes 0…16.
__global__ void __launch_bounds__(64) proposal_hash_kernel(const uint64_t *__restrict__ padded, uint32_t blocks, uint64_t *__restrict__ out4) {
  __shared__ uint64_t A[32], B[32];
  const uint32_t lane = threadIdx.x;
  cw::wave_sponge sp;
  sp.init(lane);
  for (uint32_t b = 0; b < blocks; b++) {
    if (lane < 17u) sp.s ^= padded[17u * b + lane];
    sp.permute(A, B);
  }
  if (lane < 4u) out4[lane] = sp.s;
}

// ---- chain sync from the proposals: n proposal hashes in one launch (ibft_proposal_hashes, the _raw block calls) ----------
// out32[i] = keccak256(raw[raw_off[i], raw_off[i+1]) ‖ BE64(round[i])), straight from the caller's bytes as they were staged:
// nothing is padded or re-packed on the host, the eight bytes of the round are spliced in by the absorb step.  One sponge is
// sequential, n sponges are not — two forms, the same digests:
//   LANES = 1   a lane per proposal (keccak::hash_range_tail_dwords): 64 proposals per wavefront in the time of the longest
//               one, ≈9.4 µs per 136-byte block — the throughput form;
//   LANES = 64  a wavefront per proposal (cw::sponge_message, the state over 25 lanes, ≈5.3 µs per block) — the latency form:
//               one sponge per wavefront, one wavefront per workgroup (the sponge's barrier orders ONE wavefront's LDS accesses).
// The host picks by batch shape (ibftgpu.hip:proposal_form).  Proposals start at any offset mod 4; reads stay inside the staged
// buffer (≤ 7 bytes past a proposal's end, the buffer carries 256 bytes of slack).
struct proposal_digest_args {
  const uint8_t *raw;       // the proposals, concatenated
  const uint32_t *raw_off;  // n + 1 offsets, raw_off[0] = 0, non-decreasing (checked by the host)
  const uint64_t *round;    // n
  uint8_t *out32;           // n × 32
  uint32_t n;
};
template <int LANES>
__global__ void __launch_bounds__(64) proposal_digest_kernel(proposal_digest_args a) {
  if constexpr (LANES == 1) {
    const uint32_t row = blockIdx.x * 64u + threadIdx.x;
    const bool live = row < a.n;
    // idle lanes hash an empty proposal (one block) and store nothing
    const uint32_t o0 = live ? a.raw_off[row] : 0u, o1 = live ? a.raw_off[row + 1] : 0u;
    const uint64_t tail = keccak::round_tail(live ? a.round[row] : 0ull);
    uint64_t d[4];
    keccak::hash_range_tail_dwords(a.raw + o0, o1 - o0, tail, d);
    if (live) {
      uint4 *o = reinterpret_cast<uint4 *>(a.out32 + 32ull * row);
      o[0] = make_uint4((uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32));
      o[1] = make_uint4((uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32));
    }
  } else {
    __shared__ uint64_t A[32], B[32];
    const uint32_t row = blockIdx.x, lane = threadIdx.x;  // (grid = n: block-uniform, always a live row)
    const uint32_t o0 = a.raw_off[row], len = a.raw_off[row + 1] - o0;
    const uint64_t word = cw::sponge_message(a.raw + o0, len, 0u, len + 8u, keccak::round_tail(a.round[row]), true, lane, A, B);
    if (lane < 4u) *reinterpret_cast<uint64_t *>(a.out32 + 32ull * row + 8u * lane) = word;
  }
}

// bit i of mask = (hash_len[i] == 32 && hash32[i] == H); rows are 32 B so each lane
// reads two 16-B vectors; the ballot packs 64 verdicts into one u64 per wavefront.
__global__ void hash_eq_kernel(const uint8_t *__restrict__ hash32, const uint8_t *__restrict__ hash_len,
                               const uint64_t *__restrict__ H4, uint32_t n,
                               uint64_t *__restrict__ mask) {
  uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false;
  if (row < n) {
    const uint4 *p = reinterpret_cast<const uint4 *>(hash32 + 32ull * row);
    uint4 a = p[0], b = p[1];
    const uint32_t *h = reinterpret_cast<const uint32_t *>(H4);
    uint32_t diff = (a.x ^ h[0]) | (a.y ^ h[1]) | (a.z ^ h[2]) | (a.w ^ h[3]) | (b.x ^ h[4]) |
                    (b.y ^ h[5]) | (b.z ^ h[6]) | (b.w ^ h[7]);
    ok = diff == 0 && hash_len[row] == 32;
  }
  uint64_t bal = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && row < n) mask[row >> 6] = bal;
}

// ---- ECDSA recover (cold path), one lane per signature ------------------------------------
struct recover_args {
  const uint8_t *hash32;    // n×32   (seals: per-row proposalHash)
  const uint8_t *sig65;     // n×65
  const uint8_t *signer20;  // n×20
  const uint8_t *pre_flags; // n or null
  const uint8_t *payload;   // senders: concatenated PayloadNoSig
  const uint32_t *off;      // senders: n+1 offsets
  const uint32_t *gtab;     // GTAB_WINDOWS×GTAB_ENTRIES×20 dwords
  const uint32_t *vtab;     // validator table
  uint32_t vslot_mask;
  uint32_t n;
  uint32_t flags;           // IBFT_FLAG_*
  uint64_t *mask;           // ⌈n/64⌉ verdict words
  int32_t *vidx;            // n: validator index of the row's sender (or -1)
  // warm path (null / 0 when the key cache is off)
  uint32_t *pub;            // n_validators × 20 dwords: recovered public keys (affine, 10×26 limbs)
  uint32_t *pub_state;      // n_validators: 0 unknown, 1 key known (claimed by CAS), 2 table built
  uint32_t *learned;        // counter of keys learned (host reads it with the tally)
  const uint32_t *qtab;     // n_validators × 32 × 256 × 20 dwords (wide form) or × 2 176 × 20 (GLV form: verify_dev.h)
  uint8_t *warm_done;       // n: 1 = the warm kernel already produced this row's verdict
  uint32_t dummy_validator; // a SLOT whose table is built (operand for lanes with no work)
  // The key tables belong to the DEVICE, not to a context (every context of a device shares them, a validator keeps its
  // slot — and its table — across validator-set changes): vslot[validator index] = the slot of that validator's
  // address in pub / pub_state / qtab, 0xFFFFFFFF = none (the pool is full: the validator stays on the recover path).
  const uint32_t *vslot;
  uint8_t *signer_out;      // MODE_EMIT: n×20, the address recovered from each row (zeros where there is none)
};
// MODE of the cold kernels.  MODE_SEALS / MODE_SENDERS answer "did signer20[row] sign": digest = the hash32 row / keccak256 of
// the payload row.  MODE_EMIT answers "who signed" for bare seals (digest as MODE_SEALS): no signer20 column is read, the
// recovered address is stored, and membership is that of the RECOVERED address — so only pre_flags and `live` decide whether a
// row needs the curve.  The verify kernels of the warm path know MODE_SEALS and MODE_SENDERS only.
constexpr int MODE_SEALS = 0, MODE_SENDERS = 1, MODE_EMIT = 2;
__device__ __forceinline__ int key_slot(const recover_args &a, int vi) { return (int)a.vslot[vi]; }
// states of a key-cache slot.  0 → WRITING (claimed by one row's compare-and-swap) → KNOWN (the key is in `pub`) → BUILDING
// (claimed by one build pass: keys that become KNOWN while the pass runs wait for the next one) → BUILT (the table is complete)
constexpr uint32_t KEY_UNKNOWN = 0, KEY_KNOWN = 1, KEY_BUILT = 2, KEY_WRITING = 3, KEY_BUILDING = 5;

// ---- warm path: remember a recovered key, exactly once per validator ---------------------------
// Several valid rows of the SAME validator in one cold batch are normal (PREPARE + COMMIT of one
// sender, round-change envelopes + certificate messages): the 0→1 transition of pub_state is claimed
// with a compare-and-swap and only the winner stores the key and counts it, so that `learned` is the
// number of validators with a key — the host compares it with n_validators to drop the cold kernel.
__device__ __forceinline__ void learn_key(const recover_args &a, int vi, const aff &Qa) {
  if (!a.pub_state) return;
  const int sl = key_slot(a, vi);
  if (sl < 0 || a.pub_state[sl] != KEY_UNKNOWN) return;
  if (atomicCAS(a.pub_state + sl, KEY_UNKNOWN, KEY_WRITING) != KEY_UNKNOWN) return;  // another row of this validator won the claim
  // The tables are shared by every context of the device, so a build pass of ANOTHER context (another stream) may scan the
  // states while this kernel runs: the key is published (state KEY_KNOWN, release) only after it has been written.
  store_affine(a.pub + (size_t)GTAB_ENTRY_DWORDS * sl, Qa);
  __hip_atomic_store(a.pub_state + sl, KEY_KNOWN, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(a.learned, 1u);
  a.learned[1] = (uint32_t)sl;  // any learned slot: operand for idle lanes of the warm kernel
}

// MODE_EMIT: one lane of a row stores what emit_row decided — the address column and the validator index; the verdict bit goes
// the way the kernel stores its bits.  Rows past n never come here.
__device__ __forceinline__ void emit_store(const recover_args &a, uint32_t row, const emitted &e) {
  uint32_t *o = reinterpret_cast<uint32_t *>(a.signer_out + 20ull * row);
#pragma unroll
  for (int i = 0; i < 5; i++) o[i] = e.addr[i];
  a.vidx[row] = e.vi;
}
// ... and what a row that never reaches the curve (pre_flags) stores
__device__ __forceinline__ void emit_store_none(const recover_args &a, uint32_t row) {
  const uint32_t none[5] = {0u, 0u, 0u, 0u, 0u};
  emit_store(a, row, emit_row(false, true, none, a.vtab, a.vslot_mask));
}

// ---- what every verdict kernel does around its own arithmetic, written once ------------------------------------------------------
// ROW HEAD: a row's operands straight from the HBM columns (the lane kernels stage theirs through LDS instead: stage_rows).
__device__ __forceinline__ void row_sig(const recover_args &a, uint32_t row, u256 &r, u256 &s) {
  r = secp::from_be32(a.sig65 + 65ull * row);
  s = secp::from_be32(a.sig65 + 65ull * row + 32);
}
__device__ __forceinline__ uint32_t row_recid(const recover_args &a, uint32_t row) { return a.sig65[65ull * row + 64]; }
__device__ __forceinline__ void row_sig(const recover_args &a, uint32_t row, u256 &r, u256 &s, uint32_t &v) {
  row_sig(a, row, r, s);
  v = row_recid(a, row);
}
// the digest the row's signature is over: its hash32 row, or (MODE_SENDERS) keccak256 of its payload row
template <int MODE>
__device__ __forceinline__ u256 row_digest(const recover_args &a, uint32_t row) {
  u256 z;
  if (MODE != MODE_SENDERS) {
    z = secp::from_be32(a.hash32 + 32ull * row);
  } else {
    uint64_t d[4];
    hash_range_dwords(a.payload + a.off[row], a.off[row + 1] - a.off[row], d);
    keccak::digest_to_limbs(d, z.v);
  }
  return z;
}
// the address the row claims (MODE_EMIT claims none: zeros) ...
template <int MODE>
__device__ __forceinline__ void claimed_address(const recover_args &a, uint32_t row, uint32_t want[5]) {
#pragma unroll
  for (int i = 0; i < 5; i++) want[i] = MODE != MODE_EMIT ? reinterpret_cast<const uint32_t *>(a.signer20 + 20ull * row)[i] : 0u;
}
// ... and its index in the validator set: membership is "the signer address is one of the validators" (backend.go:44, 53-54); -1: no
// member (MODE_EMIT: not known before the curve)
template <int MODE>
__device__ __forceinline__ int claimed_signer(const recover_args &a, uint32_t row, uint32_t want[5]) {
  claimed_address<MODE>(a, row, want);
  return MODE != MODE_EMIT ? valset_lookup(a.vtab, a.vslot_mask, want) : -1;
}
// pre: the caller's pre_flags ruled the row out; done: the warm kernel in front already produced its verdict
__device__ __forceinline__ bool row_pre(const recover_args &a, uint32_t row) { return a.pre_flags && a.pre_flags[row] != 0; }
__device__ __forceinline__ bool row_done(const recover_args &a, uint32_t row) { return a.warm_done && a.warm_done[row] != 0; }
// a row that still needs a verdict (need = live && !done) has to go over the curve unless it is pre-flagged or claims a non-member
template <int MODE>
__device__ __forceinline__ bool needs_curve(bool need, bool pre, int vi) {
  return need && !pre && (MODE == MODE_EMIT || vi >= 0);
}
// every kernel but the lane kernels ORs its rows' bits into a mask the host cleaned
__device__ __forceinline__ void verdict_or(const recover_args &a, uint32_t row) {
  atomicOr(reinterpret_cast<unsigned long long *>(a.mask + (row >> 6)), 1ull << (row & 63));
}

// WARM DECISION: decided by the warm kernel are pre-flagged rows and non-members (verdict false) and rows whose validator has a
// table (slot sl); the cold kernel behind it skips the rows marked here.
struct warm_row {
  int vi, sl;
  bool have_table, decided;
};
__device__ __forceinline__ warm_row warm_decide(const recover_args &a, bool pre, const uint32_t want[5]) {
  warm_row w;
  w.vi = valset_lookup(a.vtab, a.vslot_mask, want);
  w.sl = w.vi >= 0 ? key_slot(a, w.vi) : -1;
  w.have_table = w.sl >= 0 && a.pub_state[w.sl] == KEY_BUILT;
  w.decided = pre || w.vi < 0 || w.have_table;
  return w;
}
__device__ __forceinline__ void warm_mark(const recover_args &a, uint32_t row, const warm_row &w) {
  a.warm_done[row] = w.decided ? 1 : 0;
  if (w.decided) a.vidx[row] = w.vi;
}

// VERDICT TAIL of the cold kernels.  rec: the curve gave a key and `got` is its address; report: this lane speaks for the row; need
// false (the warm kernel decided the row, or it lies past n and recomputed row n − 1): no bit and no store.
// cold_decide: the row's bit.  MODE_EMIT: from the recovered address — stored here, its index left in vi (recover_dev.h:
// emit_row); otherwise: got == want of a member (recover_dev.h: claim_row), the index column is the caller's.
template <int MODE>
__device__ __forceinline__ bool cold_decide(const recover_args &a, uint32_t row, bool report, bool rec, bool pre, bool need,
                                            const uint32_t got[5], const uint32_t want[5], int &vi) {
  if (MODE == MODE_EMIT) {
    const emitted e = emit_row(rec, pre, got, a.vtab, a.vslot_mask);
    if (report && need) emit_store(a, row, e);
    vi = e.vi;
    return need && e.bit;
  }
  return claim_row(rec && need, pre, got, want, vi);
}
// ... and what a set bit brings with it: the key (it hashes to a member's address) is remembered for the warm path
template <int MODE>
__device__ __forceinline__ void cold_tail(const recover_args &a, uint32_t row, bool report, bool rec, bool pre, bool need,
                                          const uint32_t got[5], const uint32_t want[5], int vi, const aff &Qa) {
  const bool ok = cold_decide<MODE>(a, row, report, rec, pre, need, got, want, vi);
  if (report && ok) {
    learn_key(a, vi, Qa);
    verdict_or(a, row);
  }
}

// Stage the block's rows through LDS (coalesced dword loads) and unpack this lane's row.
struct row_regs {
  u256 r, s, z;
  uint32_t v;
  uint32_t want[5];
  bool live, pre;
  uint32_t row;
};
template <int MODE>
__device__ __forceinline__ row_regs stage_rows(const recover_args &a, uint8_t *lds) {
  uint8_t *l_sig = lds;
  uint8_t *l_hash = lds + ROWS_PER_BLOCK * 65;
  uint8_t *l_from = l_hash + ROWS_PER_BLOCK * 32;
  const uint32_t row0 = blockIdx.x * ROWS_PER_BLOCK;
  const uint32_t rows = min((uint32_t)ROWS_PER_BLOCK, a.n - row0);
  const uint32_t lane = threadIdx.x;
  {
    // sig: rows*65 bytes starting at 65*row0 (a multiple of 4 because row0 % 64 == 0)
    const uint32_t nb = rows * 65;
    const uint32_t *g = reinterpret_cast<const uint32_t *>(a.sig65 + 65ull * row0);
    for (uint32_t i = lane; i < nb / 4; i += ROWS_PER_BLOCK) reinterpret_cast<uint32_t *>(l_sig)[i] = g[i];
    for (uint32_t i = (nb & ~3u) + lane; i < nb; i += ROWS_PER_BLOCK) l_sig[i] = a.sig65[65ull * row0 + i];
    if (MODE != MODE_EMIT) {
      const uint32_t *gf = reinterpret_cast<const uint32_t *>(a.signer20 + 20ull * row0);
      for (uint32_t i = lane; i < rows * 5; i += ROWS_PER_BLOCK) reinterpret_cast<uint32_t *>(l_from)[i] = gf[i];
    }
    if (MODE != MODE_SENDERS) {
      const uint4 *gh = reinterpret_cast<const uint4 *>(a.hash32 + 32ull * row0);
      for (uint32_t i = lane; i < rows * 2; i += ROWS_PER_BLOCK) reinterpret_cast<uint4 *>(l_hash)[i] = gh[i];
    }
  }
  __syncthreads();
  row_regs q;
  q.row = row0 + lane;
  q.live = lane < rows;
  const uint32_t lrow = q.live ? lane : 0;
  q.pre = q.live && a.pre_flags && a.pre_flags[q.row] != 0;
  q.r = secp::from_be32(l_sig + 65 * lrow);
  q.s = secp::from_be32(l_sig + 65 * lrow + 32);
  q.v = l_sig[65 * lrow + 64];
  if (MODE != MODE_SENDERS) {
    q.z = secp::from_be32(l_hash + 32 * lrow);
  } else {
    uint64_t d[4];
    uint32_t o0 = q.live ? a.off[q.row] : 0u, o1 = q.live ? a.off[q.row + 1] : 0u;
    hash_range_dwords(a.payload + o0, o1 - o0, d);
    keccak::digest_to_limbs(d, q.z.v);
  }
#pragma unroll
  for (int i = 0; i < 5; i++) q.want[i] = MODE != MODE_EMIT ? reinterpret_cast<const uint32_t *>(l_from)[5 * lrow + i] : 0u;
  return q;
}

// MODE: MODE_SEALS / MODE_SENDERS / MODE_EMIT (above recover_args).
// TAB: where the per-lane window table of u2·R lives (recover_dev.h) —
//   TAB_LDS      in the workgroup's LDS (640 B per lane: one wavefront per SIMD, what a batch of ≤ 65 536 rows offers anyway);
//                no private segment at all: the launch moves the rows, the G-table lines and nothing else through HBM;
//   TAB_PRIVATE  in the private segment, read where it is used: 256 registers, TWO resident wavefronts per SIMD — the form for
//                batches that offer more than one wavefront per SIMD (n > 65 536: 15 instead of 18 ns per verify);
//   TAB_PRIVATE_PREFETCH  round 4's form (entries read in front of the doublings, one resident wavefront): kept for the A/B.
constexpr int TAB_LDS = 0, TAB_PRIVATE = 1, TAB_PRIVATE_PREFETCH = 2;
constexpr int STAGE_BYTES = ROWS_PER_BLOCK * (65 + 32 + 20);
template <int MODE, int TAB>
__global__ void __launch_bounds__(ROWS_PER_BLOCK) ecrecover_lane_kernel(recover_args a) {
  // one block of LDS words: first the staging area of the rows, then (TAB_LDS) the window tables — the block is ONE wavefront
  // (ROWS_PER_BLOCK = 64) and its LDS operations execute in order, so the table may overwrite rows already read into registers
  constexpr int LDS_WORDS = TAB == TAB_LDS ? LTAB_WORDS * ROWS_PER_BLOCK : (STAGE_BYTES + 3) / 4;
  static_assert(LTAB_WORDS * ROWS_PER_BLOCK * 4 >= STAGE_BYTES && ROWS_PER_BLOCK == 64, "the table area holds the staging area");
  __shared__ __attribute__((aligned(16))) uint32_t ldsw[LDS_WORDS];
  uint8_t *lds = reinterpret_cast<uint8_t *>(ldsw);
  row_regs q = stage_rows<MODE>(a, lds);
  const uint32_t lane = threadIdx.x;
  // rows the warm kernel already decided keep their bit; a wavefront with nothing left exits
  const bool done = a.warm_done && q.live && a.warm_done[q.row] != 0;
  const bool need = q.live && !done;
  if (!__any(need ? 1 : 0)) return;

  uint32_t got[5];
  aff Qa;
  bool rec;
  if (TAB == TAB_LDS)
    rec = recover_pubkey_with(a.gtab, q.z, q.r, q.s, q.v, a.flags, got, Qa, var_mult_lds<ROWS_PER_BLOCK>{ldsw + lane});
  else
    rec = recover_pubkey_with(a.gtab, q.z, q.r, q.s, q.v, a.flags, got, Qa, var_mult_private<TAB == TAB_PRIVATE_PREFETCH>{});
  bool ok;
  int vi;
  if (MODE == MODE_EMIT) {
    const emitted e = emit_row(rec, q.pre, got, a.vtab, a.vslot_mask);
    if (need) emit_store(a, q.row, e);
    ok = need && e.bit;
    vi = e.vi;
  } else {
    ok = need && !q.pre && rec;
#pragma unroll
    for (int i = 0; i < 5; i++) ok = ok && (got[i] == q.want[i]);
    // membership: "the signer address is one of the validators" (backend.go:44, 53-54)
    vi = valset_lookup(a.vtab, a.vslot_mask, q.want);
    ok = ok && vi >= 0;
    if (need) a.vidx[q.row] = vi;
  }
  // a key that hashes to a member's address is remembered for the warm path
  if (ok) learn_key(a, vi, Qa);
  uint64_t bal = __ballot(ok);
  uint64_t keep = __ballot(done);
  if (lane == 0) {
    uint64_t *w = a.mask + (blockIdx.x * (uint32_t)ROWS_PER_BLOCK >> 6);
    *w = keep ? ((*w & keep) | (bal & ~keep)) : bal;
  }
}

// ---- warm path, one lane per signature ----------------------------------------------------
template <int MODE, int FORM = QTAB_WIDE>
__global__ void __launch_bounds__(ROWS_PER_BLOCK) verify_known_lane_kernel(recover_args a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[ROWS_PER_BLOCK * (65 + 32 + 20)];
  row_regs q = stage_rows<MODE>(a, lds);
  const uint32_t lane = threadIdx.x;
  const warm_row w = warm_decide(a, q.pre, q.want);
  const bool crypto = q.live && !q.pre && w.have_table;
  bool ok = false;
  if (__any(crypto ? 1 : 0)) {  // wave-uniform: every lane runs the arithmetic, idle ones on a dummy table
    const uint32_t tv = crypto ? (uint32_t)w.sl : a.dummy_validator;
    ok = verify_known<FORM>(a.gtab, a.qtab + qtab_slot_dwords<FORM>() * tv, q.z, q.r, q.s, q.v, a.flags) && crypto;
  }
  if (q.live) warm_mark(a, q.row, w);
  uint64_t bal = __ballot(ok);
  if (lane == 0) a.mask[blockIdx.x * (uint32_t)ROWS_PER_BLOCK >> 6] = bal;
}

// ---- warm path, G LANES PER SIGNATURE (G = 64: one wavefront per signature) -------------------
// The 32 window points of u2·Q (validator's table) and the 16 window points of u1·G are dealt
// round-robin to the G lanes of a group; each lane sums its share with mixed additions, then a
// log2(G)-level xor-butterfly of Jacobian additions leaves the total in every lane.  The scalar
// work (s⁻¹ mod n, final Z⁻¹) is replicated across the group.  G is chosen by the host so that a
// batch of n rows yields about one wavefront per SIMD (n·G/64 ≈ 1024): G = 64 up to 1 024 rows,
// 16 at 4 096, 4 at 16 384, and the LDS-staged lane kernel (G = 1) beyond.
__device__ __forceinline__ jac shfl_xor_jac(const jac &p, int off) {
  jac r;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    r.x.n[i] = __shfl_xor(p.x.n[i], off, 64);
    r.y.n[i] = __shfl_xor(p.y.n[i], off, 64);
    r.z.n[i] = __shfl_xor(p.z.n[i], off, 64);
  }
  r.inf = __shfl_xor(p.inf ? 1 : 0, off, 64) != 0;
  return r;
}

template <int MODE, int G, int FORM = QTAB_WIDE>
__global__ void __launch_bounds__(64) verify_known_group_kernel(recover_args a) {
  constexpr int ROWS = 64 / G;                    // signatures per wavefront
  constexpr int POINTS = QTAB_WINDOWS + GTAB_WINDOWS;
  // Round 5: the kernel's CODE has to fit the 64 KB instruction cache — on one lease in four a fetch past it costs 65 % more
  // and a 60 KB kernel ran 0.132 instead of 0.110 ms.  Both point additions inlined (11 + 16 multiplications
  // of 224 instructions) made 60.5 KB; only the one that dominates a lane's work is pasted now — the butterfly for G ≥ 16 (4–5
  // folds of 16 multiplications against 2–3 mixed additions of 11), the mixed addition for G ≤ 8 — and the other one calls the
  // outlined multiply (≈ 25 instructions per call: +2 % of this kernel's instructions).
  constexpr bool INL_FOLD = G >= 16, INL_MADD = !INL_FOLD;
  const uint32_t lane = threadIdx.x;
  const uint32_t sub = lane % G;
  const uint32_t row_raw = blockIdx.x * ROWS + lane / G;
  const bool live = row_raw < a.n;
  const uint32_t row = live ? row_raw : a.n - 1;  // idle groups recompute the last row, store nothing
  const bool pre = a.pre_flags && a.pre_flags[row] != 0;
  u256 r = secp::from_be32(a.sig65 + 65ull * row);
  u256 s = secp::from_be32(a.sig65 + 65ull * row + 32);
  const uint32_t v = a.sig65[65ull * row + 64];
  u256 z;
  if (MODE == MODE_SEALS) {
    z = secp::from_be32(a.hash32 + 32ull * row);
  } else {
    uint64_t d[4];
    hash_range_dwords(a.payload + a.off[row], a.off[row + 1] - a.off[row], d);
    keccak::digest_to_limbs(d, z.v);
  }
  uint32_t want[5];
#pragma unroll
  for (int i = 0; i < 5; i++) want[i] = reinterpret_cast<const uint32_t *>(a.signer20 + 20ull * row)[i];
  const int vi = valset_lookup(a.vtab, a.vslot_mask, want);
  const int sl = vi >= 0 ? key_slot(a, vi) : -1;
  const bool have_table = sl >= 0 && a.pub_state[sl] == KEY_BUILT;
  const bool decided = pre || vi < 0 || have_table;
  const bool crypto = live && !pre && have_table;
  if (live && sub == 0) {
    a.warm_done[row] = decided ? 1 : 0;
    if (decided) a.vidx[row] = vi;
  }
  if (!__any(crypto ? 1 : 0)) return;  // wave-uniform: from here every lane runs the same stream

  bool ok = sig_in_range(r, s, v, a.flags);
  u256 u1, u2;
  // G ≥ 16: a signature owns whole DPP rows, and all their lanes hold the same (z, r, s) — the two inversions (s⁻¹ mod n
  // here, Z⁻¹ mod p at the end) run with the limbs of d, e, f, g over the lanes of the row (wave_fe_dev.h:modinv_wave,
  // ≈9.5 k issue slots) instead of every lane running the whole constant-time safegcd on its own copy (≈15 k): they were
  // 43 % of this kernel at N = 4 096.  Smaller groups share a row between signatures and keep the lane form.
  constexpr bool ROW_INV = G >= 16;
  const wv::wk wkc = wv::wk_init();
  if (ROW_INV) {
    const secp::sc sinv = secp::sc_from_u256(wv::modinv_wave<secp::ModN>(s, wkc));
    u1 = secp::sc_canon(secp::sc_mul(secp::sc_from_u256(z), sinv));
    u2 = secp::sc_canon(secp::sc_mul(secp::sc_from_u256(r), sinv));
  } else {
    verify_scalars(z, r, s, u1, u2);
  }
  const uint32_t *qt = a.qtab + qtab_slot_dwords<FORM>() * (crypto ? (uint32_t)sl : a.dummy_validator);
  jac acc = secp::jac_inf();
  constexpr int STEPS = (POINTS + G - 1) / G;  // wave-uniform trip count
  if constexpr (FORM == QTAB_GLV) {
    // The GLV form (verify_dev.h): points 0…15 the k1 half, 16…31 the k2 half (the same entries, x·β), 32…47 G.  Same deal
    // (point it·G + sub), same pipelining by one.  A step's lanes may be of different classes, so the β product is formed by
    // every lane and selected — but only on steps where some lane of the wavefront needs it (wave_any: a uniform branch).
    const secp::glv_split sp = secp::sc_split_lambda(u2);
    const u256 b1 = qglv_bias(sp.k1), b2 = qglv_bias(sp.k2);
    const secp::fe beta = secp::GLV_CONST(1);
    auto point_of = [&](int it, qglv_operand &op) -> const uint32_t * {
      const int p = it * G + (int)sub;
      const bool has = p < POINTS;
      const int pp = has ? p : 0;
      if (pp < 2 * QGLV_WINDOWS) {
        op = qglv_point(pp, b1, b2, sp.neg1, sp.neg2);
        op.nz = op.nz && has;
        return qt + (size_t)GTAB_ENTRY_DWORDS * op.index;
      }
      const int w = pp - 2 * QGLV_WINDOWS;
      const uint32_t dgt = (u1.v[(w * GTAB_BITS) >> 5] >> ((w * GTAB_BITS) & 31)) & (uint32_t)(GTAB_ENTRIES - 1);
      op.index = dgt;
      op.nz = dgt != 0;
      op.beta = false;
      op.neg = false;
      return a.gtab + (size_t)GTAB_ENTRY_DWORDS * ((size_t)w * GTAB_ENTRIES + dgt);
    };
    qglv_operand op;
    aff cur = load_affine(point_of(0, op));
#pragma unroll 1
    for (int it = 0; it < STEPS; it++) {
      qglv_operand on;
      const aff nxt = load_affine(point_of(it + 1 < STEPS ? it + 1 : it, on));  // (the last step re-reads its own entry)
      secp::fe bx = cur.x;
      if (secp::wave_any(op.beta)) bx = secp::fe_mul(cur.x, beta);
      const aff q = qglv_apply(cur, bx, op.beta, op.neg);
      jac sum = secp::jac_add_aff_t<INL_MADD>(acc, q);
      acc = secp::jac_select(op.nz, sum, acc);
      cur = nxt;
      op = on;
    }
  } else {
  // this lane's table point of step `it` (point it·G + sub of the 48): where it lies, its digit, whether it exists
  auto point_of = [&](int it, uint32_t &dgt, bool &has) -> const uint32_t * {
    const int p = it * G + (int)sub;
    has = p < POINTS;
    const int pp = has ? p : 0;
    if (pp < QTAB_WINDOWS) {
      dgt = (u2.v[pp >> 2] >> (8 * (pp & 3))) & 255u;
      return qt + (size_t)GTAB_ENTRY_DWORDS * (pp * QTAB_ENTRIES + dgt);
    }
    const int w = pp - QTAB_WINDOWS;
    dgt = (u1.v[(w * GTAB_BITS) >> 5] >> ((w * GTAB_BITS) & 31)) & (uint32_t)(GTAB_ENTRIES - 1);
    return a.gtab + (size_t)GTAB_ENTRY_DWORDS * ((size_t)w * GTAB_ENTRIES + dgt);
  };
  // Round 6: software-pipelined by one — the entry of step it + 1 is asked for before the addition of step it runs (a
  // dependent read of a validator's table, far beyond any cache, used to open every step: ≈ 2 µs in front of each addition)
  uint32_t dgt;
  bool has;
  aff cur = load_affine(point_of(0, dgt, has));
#pragma unroll 1
  for (int it = 0; it < STEPS; it++) {
    uint32_t dn;
    bool hasn;
    const aff nxt = load_affine(point_of(it + 1 < STEPS ? it + 1 : it, dn, hasn));  // (the last step re-reads its own entry)
    jac sum = secp::jac_add_aff_t<INL_MADD>(acc, cur);  // (the one inlined copy of the mixed addition: secp256k1_dev.h)
    acc = secp::jac_select(has && dgt != 0, sum, acc);
    cur = nxt;
    dgt = dn;
    has = hasn;
  }
  }
#pragma unroll 1
  for (int off = G / 2; off >= 1; off >>= 1) {
    jac other = shfl_xor_jac(acc, off);
    acc = secp::jac_add_t<INL_FOLD>(acc, other);  // (one inlined copy in the rolled butterfly)
  }
  if (ROW_INV) {
    // The butterfly left the SUM in every lane of the group, but not one REPRESENTATION of it: P + Q and Q + P come out
    // with Z of opposite sign, so the lanes of a group hold (λ²X, λ³Y, λZ) for different λ.  The row-layout inversion
    // takes its limbs from all lanes of a row: give every lane the Z of the group's first lane; that lane then holds a
    // consistent (X, Y, Z) and is the one that reports.
#pragma unroll
    for (int i = 0; i < 10; i++)
      acc.z.n[i] = G == 16 ? wv::row_bcast<0>(acc.z.n[i]) : (uint32_t)__shfl((int)acc.z.n[i], (int)(lane & ~(uint32_t)(G - 1)), 64);
    acc.inf = __shfl(acc.inf ? 1 : 0, (int)(lane & ~(uint32_t)(G - 1)), 64) != 0;
    aff A;
    const bool fin = wv::jac_to_aff_wave(A, acc, wkc);
    const secp::fe rx = secp::fe_from_u256(r);  // r < n < p: canonical limbs
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) diff |= A.x.n[i] ^ rx.n[i];
    ok = fin && diff == 0 && (A.y.n[0] & 1u) == v && ok && crypto;
  } else {
    ok = verify_finish(acc, r, v) && ok && crypto;
  }
  if (sub == 0 && ok) atomicOr(reinterpret_cast<unsigned long long *>(a.mask + (row >> 6)), 1ull << (row & 63));
}

// WAVE_KERNEL_WAVES wavefronts (= signatures) per workgroup: the four wavefronts of a workgroup land on
// the four SIMDs of one CU, so a 1 024-row launch is exactly one wavefront per SIMD by construction
// instead of by the dispatcher's choice.
constexpr int WAVE_KERNEL_WAVES = 4;
// ---- warm path, one wavefront per signature with the limbs spread over lanes (wave_fe_dev.h) ----
// Replaces verify_known_group_kernel<·,64>: same prologue, the point sum runs in the row layout.
template <int MODE, int FORM = QTAB_WIDE>
__global__ void __launch_bounds__(64 * WAVE_KERNEL_WAVES) verify_known_wave_kernel(recover_args a) {
  const uint32_t row = blockIdx.x * WAVE_KERNEL_WAVES + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (row >= a.n) return;  // whole wavefront
  const bool pre = row_pre(a, row);
  u256 r, s;
  uint32_t v, want[5];
  row_sig(a, row, r, s, v);
  const u256 z = row_digest<MODE>(a, row);
  claimed_address<MODE>(a, row, want);
  const warm_row w = warm_decide(a, pre, want);
  if (lane == 0) warm_mark(a, row, w);
  if (pre || !w.have_table) return;  // wave-uniform: the wavefront holds one row
  const bool ok = wv::verify_known_wave<FORM>(a.gtab, a.qtab + qtab_slot_dwords<FORM>() * (uint32_t)w.sl, z, r, s, v, a.flags);
  if (lane == 0 && ok) verdict_or(a, row);
}

// ---- cold path with G = 2, 4 or 8 lanes per signature ----------------------------------------
// The GLV split already yields two independent halves (k1·R, k2·λR); each half is cut into
// P = G/2 pieces of 128/P bits with bases 2^(j·128/P)·R, so a lane does 128/P doublings instead of
// 128 and the pieces are joined by a log2(G)-level butterfly.  Everything that does not split
// (√, r⁻¹, the prefix doublings that produce the bases, the per-lane table, Z⁻¹, Keccak) is
// replicated across the group, so the critical path shrinks from ≈676 k to ≈520 k (G = 2),
// ≈440 k (G = 4), ≈410 k (G = 8) VALU instructions: worth it exactly when the batch is too small
// to fill the chip (host picks G so that n·G/64 ≤ 1024 wavefronts).
template <int MODE, int G, int TAB = TAB_LDS>
__global__ void __launch_bounds__(64) ecrecover_group_kernel(recover_args a) {
  __shared__ uint32_t ldsw[(TAB == TAB_LDS && G != 8) ? LTAB_WORDS * 64 : 1];  // the lanes' window tables (4-bit windows: G = 2, 4)
  constexpr int ROWS = 64 / G;
  constexpr int P = G / 2;            // pieces per GLV half
  constexpr int PIECE_BITS = 128 / P; // 128, 64 or 32 ... (G = 2, 4, 8)
  constexpr int NIBS = PIECE_BITS / 4;
  const uint32_t lane = threadIdx.x;
  const uint32_t sub = lane % G;
  const uint32_t half = sub & 1u;     // 0: k1 on ±R, 1: k2 on λ(±R)
  const uint32_t piece = sub >> 1;    // which 128/P-bit piece of that half
  const uint32_t row_raw = blockIdx.x * ROWS + lane / G;
  const bool live = row_raw < a.n;
  const uint32_t row = live ? row_raw : a.n - 1;
  const bool pre = row_pre(a, row);
  const bool done = row_done(a, row);
  const bool need = live && !done;
  if (!__any(need ? 1 : 0)) return;

  u256 r, s;
  uint32_t v, want[5];
  row_sig(a, row, r, s, v);
  const u256 z = row_digest<MODE>(a, row);
  claimed_address<MODE>(a, row, want);  // (looked up behind the curve: the index is not held in a register across it)

  bool ok = sig_in_range(r, s, v, a.flags);
  // R = (r, y), y² = r³ + 7, parity(y) = v
  secp::fe rx = secp::fe_from_u256(r);
  secp::fe seven = secp::fe_zero();
  seven.n[0] = 7;
  secp::fe rhs = secp::fe_add(secp::fe_mul(secp::fe_sqr(rx), rx), seven);
  secp::fe y = secp::fe_sqrt_candidate(rhs);
  ok = ok && secp::fe_equal(secp::fe_sqr(y), rhs, 2);
  y = secp::fe_normalize(y);
  y = secp::l26_select((y.n[0] & 1u) != v, secp::fe_normalize_weak(secp::fe_neg(y, 1)), y);
  // u1 = −z/r, u2 = s/r, u2 = k1 + k2·λ
  secp::sc rinv = secp::sc_from_u256(secp::modinv_shared<secp::ModN>(r));
  u256 u1 = secp::sc_neg_canon(secp::sc_canon(secp::sc_mul(secp::sc_from_u256(z), rinv)));
  u256 u2 = secp::sc_canon(secp::sc_mul(secp::sc_from_u256(s), rinv));
  secp::glv_split sp = secp::sc_split_lambda(u2);
  // this lane's base: ±R doubled piece·PIECE_BITS times (uniform trip count: every lane runs the
  // longest prefix and keeps the intermediate it needs)
  aff R1;
  R1.x = rx;
  R1.y = secp::l26_select(sp.neg1, secp::fe_normalize_weak(secp::fe_neg(y, 1)), y);
  jac base = secp::jac_from_aff(R1);
  if (P > 1) {
    jac run = base;
#pragma unroll 1
    for (int j = 1; j < P; j++) {
#pragma unroll 1
      for (int d = 0; d < PIECE_BITS; d++) run = secp::jac_dbl(run);
      base = secp::jac_select(piece >= (uint32_t)j && piece == (uint32_t)j, run, base);
    }
  }
  // per-lane window table over the base (Jacobian).  G = 8 (32-bit pieces): 2-bit windows, the three
  // entries {B, 2B, 3B} live in VGPRs and are picked with selects — no scratch traffic at all
  // (the 4-bit table is 1.9 KB per lane in scratch: 16 MB written + re-read per launch at
  // N = 1024, G = 8).  G = 2, 4 (128/64-bit pieces): 4-bit windows, table in scratch.
  constexpr int WBITS = (G == 8) ? 2 : 4;
  constexpr int DIGITS = PIECE_BITS / WBITS;
  const u256 &kk = half ? sp.k2 : sp.k1;
  const bool flip = half && (sp.neg1 != sp.neg2);
  const secp::fe beta = secp::GLV_CONST(1);
  jac acc = secp::jac_inf();
  if (WBITS == 2) {
    const jac b1 = base, b2 = secp::jac_dbl(base), b3 = secp::jac_add(b2, base);
#pragma unroll 1
    for (int dgi = DIGITS - 1; dgi >= 0; dgi--) {
      acc = secp::jac_dbl(secp::jac_dbl(acc));
      const int bit = (int)(piece * PIECE_BITS) + 2 * dgi;
      const uint32_t dg = (kk.v[bit >> 5] >> (bit & 31)) & 3u;
      jac q = secp::jac_select(dg == 1, b1, secp::jac_select(dg == 2, b2, b3));
      secp::fe bx = secp::fe_mul(q.x, beta);
      q.x = secp::l26_select(half != 0, bx, q.x);
      q.y = secp::l26_select(flip, secp::fe_neg(q.y, 1), q.y);
      jac sum = secp::jac_add(acc, q);
      acc = secp::jac_select(dg != 0, sum, acc);
    }
  } else {
    // signed radix-16 windows over a table of the multiples 1…8 of this lane's base brought to one common Z (recover_dev.h:
    // ecmult_table).  The base is Jacobian (X, Y, Z) — the AFFINE point (X, Y) of the isomorphic curve y² = x³ + 7·Z⁶, on
    // which the table is built and the loop runs; Z·Zc goes back into the accumulator's Z at the end.  The λ half uses the
    // entries' β·X, the sign of a digit is a negation of Y.  Digit j of a piece = nibble(k + Σ 8·16^i, piece·NIBS + j) − 8;
    // the half's 33rd digit (the carry, 0 or 1) belongs to its top piece — the other pieces see a zero digit there.
    aff b1;
    b1.x = base.x;
    b1.y = base.y;
    const u256 kb = window_bias(kk);
    if (TAB == TAB_LDS) {
      // the table in LDS (recover_dev.h: ltab): 640 B per lane, β·X multiplied at use — for every lane, the λ half selects it
      // (half differs from lane to lane: no call under divergent control flow)
      ltab<64> lt;
      lt.col = ldsw + lane;
      ecmult_table_lds<64>(b1, lt);
      // this lane's digits — nibbles piece·NIBS … piece·NIBS + NIBS of kb — as a shift register whose current digit is the low
      // nibble of word NW (round 6: nothing indexed by `at`, no select chain per digit, no private segment)
      constexpr int NW = NIBS / 8;  // 4 words (G = 2), 2 (G = 4)
      u256 kr = secp::zero256();
#pragma unroll
      for (int i = 0; i <= NW; i++) {
        kr.v[i] = kb.v[i];
#pragma unroll
        for (int j = 1; j < P; j++) kr.v[i] = piece == (uint32_t)j ? kb.v[i + NW * j] : kr.v[i];
      }
      // Round 6: the window additions and this lane's share of the fixed-base additions are steps of ONE loop around ONE pasted
      // copy of the mixed addition (recover_dev.h: ecmult_var_gen_lds has the reasoning) — the G additions used to go through
      // the outlined multiply in a loop of their own.  u1 is a shift register (this lane's current window in the low bits of
      // word 0: shifted down by GTAB_BITS·sub once, by GTAB_BITS·G per step), the table entry of the next G step is asked for
      // before the addition of this one runs, the first one before the window loop starts.
      constexpr int GSTEPS = (GTAB_WINDOWS + G - 1) / G;
      constexpr int LOG2G = G == 8 ? 3 : (G == 4 ? 2 : 1);
      u256 ug = u1;
      secp::shr_units<GTAB_BITS, LOG2G>(ug, sub);
      uint32_t dg = ug.v[0] & (uint32_t)(GTAB_ENTRIES - 1);
      bool has = (int)sub < GTAB_WINDOWS;
      gtab_raw cur = gtab_load(a.gtab, has ? (int)sub : 0, has ? dg : 0u);
#pragma unroll 1
      for (int st = 0; st <= NIBS + GSTEPS; st++) {
        aff q;
        bool take;
        gtab_raw nxt = cur;
        uint32_t dn = dg;
        bool hasn = has;
        if (st <= NIBS) {  // (wave-uniform) window step: digit NIBS − st of this lane's piece
          const bool mine = st > 0 || piece == (uint32_t)(P - 1);
          const int e = mine ? (int)secp::top_nibble<NW + 1>(kr) - 8 : 0;
          secp::shl4<NW + 1>(kr);
          if (st != 0) {
#pragma unroll 1
            for (int d = 0; d < 4; d++) acc = secp::jac_dbl_t<true>(acc);
          }
          q = window_operand_lds<64>(lt, e, flip);
          q.x = secp::l26_select(half != 0, secp::fe_mul(q.x, beta), q.x);
          take = e != 0;
        } else {           // fixed-base step: window (st − NIBS − 1)·G + sub of u1
          const int it = st - NIBS - 1;
          if (it == 0) acc.z = secp::fe_mul(acc.z, secp::fe_mul(lt.zc, base.z));  // back from the isomorphic curve first
          secp::shr_const<GTAB_BITS * G>(ug);
          const int wn = (it + 1) * G + (int)sub;
          hasn = it + 1 < GSTEPS && wn < GTAB_WINDOWS;
          dn = ug.v[0] & (uint32_t)(GTAB_ENTRIES - 1);
          nxt = gtab_load(a.gtab, hasn ? wn : 0, hasn ? dn : 0u);  // (past the end: entry 0 of window 0, never added)
          q = gtab_point(cur);
          take = has && dg != 0;
        }
        const jac sum = secp::jac_add_aff_t<true>(acc, q);
        acc = secp::jac_select(take, sum, acc);
        if (st > NIBS) {  // (only the fixed-base steps move the pipeline)
          cur = nxt;
          dg = dn;
          has = hasn;
        }
      }
    } else {
      wtab wt;
      ecmult_table(b1, wt);
#pragma unroll 1
      for (int nib = NIBS; nib >= 0; nib--) {
        const int at = (int)(piece * NIBS) + nib;
        const bool mine = nib < NIBS || piece == (uint32_t)(P - 1);
        const int e = mine ? (int)secp::nibble(kb, at) - 8 : 0;
        const aff q = window_operand(wt, e, half != 0, flip);  // read in front of the doublings that cover its latency
        if (nib != NIBS) {
#pragma unroll 1
          for (int d = 0; d < 4; d++) acc = secp::jac_dbl_t<true>(acc);
        }
        acc = window_add_q(acc, q, e);
      }
      acc.z = secp::fe_mul(acc.z, secp::fe_mul(wt.zc, base.z));
    }
  }
  // u1·G: the fixed-base windows are dealt to the lanes of the group — lane `sub` takes windows sub, sub + G, … .  Round 6: u1 is
  // a shift register (this lane's current window in the low bits of word 0: shifted down by GTAB_BITS·sub once, by GTAB_BITS·G
  // per step — nothing indexed), and the table entry of the NEXT step is asked for before the addition of this one runs.
  if (!(WBITS == 4 && TAB == TAB_LDS)) {  // (the LDS-table form has run them as steps of its window loop)
    constexpr int STEPS = (GTAB_WINDOWS + G - 1) / G;
    constexpr int LOG2G = G == 8 ? 3 : (G == 4 ? 2 : 1);
    u256 ug = u1;
    secp::shr_units<GTAB_BITS, LOG2G>(ug, sub);
    uint32_t dg = ug.v[0] & (uint32_t)(GTAB_ENTRIES - 1);
    bool has = (int)sub < GTAB_WINDOWS;
    gtab_raw cur = gtab_load(a.gtab, has ? (int)sub : 0, has ? dg : 0u);
#pragma unroll 1
    for (int it = 0; it < STEPS; it++) {
      secp::shr_const<GTAB_BITS * G>(ug);
      const int wn = (it + 1) * G + (int)sub;
      const bool hasn = it + 1 < STEPS && wn < GTAB_WINDOWS;
      const uint32_t dn = ug.v[0] & (uint32_t)(GTAB_ENTRIES - 1);
      const gtab_raw nxt = gtab_load(a.gtab, hasn ? wn : 0, hasn ? dn : 0u);  // (past the end: entry 0 of window 0, never added)
      const jac sum = secp::jac_add_aff(acc, gtab_point(cur));
      acc = secp::jac_select(has && dg != 0, sum, acc);
      cur = nxt;
      dg = dn;
      has = hasn;
    }
  }
#pragma unroll 1
  for (int off = G / 2; off >= 1; off >>= 1) {
    jac other = shfl_xor_jac(acc, off);
    // (round 5: through the outlined multiply — one to three folds per signature do not pay for 28 KB of pasted code in a
    // kernel that is far over the 64 KB instruction cache already: DESIGN.md §5.8)
    acc = secp::jac_add_t<false>(acc, other);
  }
  aff Qa;
  ok = secp::jac_to_aff_fast(Qa, acc) && ok;
  u256 qx = secp::l26_to_u256(Qa.x), qy = secp::l26_to_u256(Qa.y);
  uint32_t got[5];
  keccak::address_from_xy(qx.v, qy.v, got);
  const int vi = MODE != MODE_EMIT ? valset_lookup(a.vtab, a.vslot_mask, want) : -1;
  if (MODE != MODE_EMIT && sub == 0 && need) a.vidx[row] = vi;
  cold_tail<MODE>(a, row, sub == 0, ok, pre, need, got, want, vi, Qa);
}

// ---- cold path, ONE WAVEFRONT PER SIGNATURE (wave_fe_dev.h) --------------------------------------
// For batches that leave most of the chip idle (n ≤ 2 048: at most two wavefronts per SIMD).  A
// field element is one VGPR spread over the 16 lanes of a DPP row, a multiplication costs ≈86
// instructions for four independent products, and the four rows carry the four 64-bit pieces
// of the GLV-split scalar.  All control flow is uniform: the wavefront holds a single signature.
template <int MODE>
__global__ void __launch_bounds__(64 * WAVE_KERNEL_WAVES) ecrecover_wave_kernel(recover_args a) {
  const uint32_t row = blockIdx.x * WAVE_KERNEL_WAVES + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (row >= a.n) return;                            // whole wavefront
  if (row_done(a, row)) return;                      // decided by the warm kernel
  uint32_t want[5];
  const int vi = claimed_signer<MODE>(a, row, want);
  const bool pre = row_pre(a, row);
  // the wavefront holds ONE row: the index goes out first, and a row that does not need the curve leaves here — its verdict
  // stays 0 (the mask was cleared by the host before the launch), MODE_EMIT stores zeros and -1 for a pre-flagged one
  if (MODE != MODE_EMIT && lane == 0) a.vidx[row] = vi;
  if (!needs_curve<MODE>(true, pre, vi)) {
    if (MODE == MODE_EMIT && lane == 0) emit_store_none(a, row);
    return;
  }
  u256 r, s;
  uint32_t v;
  row_sig(a, row, r, s, v);
  const u256 z = row_digest<MODE>(a, row);
  uint32_t got[5];
  aff Qa;
  __shared__ uint32_t krow_scr[WAVE_KERNEL_WAVES][wv::KROW_SCRATCH_DWORDS];  // the address hash's transposition: wave-private LDS
  const bool rec = wv::recover_pubkey_wave(a.gtab, z, r, s, v, a.flags, got, Qa, krow_scr[threadIdx.x >> 6]);
  cold_tail<MODE>(a, row, lane == 0, rec, false, true, got, want, vi, Qa);
}

// ---- cold path, TWO WAVEFRONTS PER SIGNATURE (n ≤ 512: round 4) ----------------------------------------------------
// Half of the chip's SIMDs idle when n ≤ 512 signatures run one wavefront each.  A workgroup here is PAIRS_PER_BLOCK = 2 pairs
// — four wavefronts, which land on the four SIMDs of ONE compute unit, so 512 rows are exactly one wavefront per SIMD of
// the chip by construction: wavefront w < 2 is the MAIN wavefront of signature slot w (prefix doublings with √, table, main
// loop, joins, Z⁻¹, Keccak), wavefront 2 + w its HELPER (r⁻¹ mod n, u₁, u₂, GLV split; then u₁·G) — the two meet in LDS at two
// workgroup barriers (wave_fe_dev.h: recover_pubkey_wave<…, PAIR>, recover_helper_wave).  Every wavefront of the workgroup
// passes both barriers, whatever its row turns out to be: a pair with nothing to do only synchronises.
constexpr int PAIRS_PER_BLOCK = 2;
template <int MODE>
__global__ void __launch_bounds__(128 * PAIRS_PER_BLOCK) ecrecover_wave2_kernel(recover_args a) {
  __shared__ wv::pair_shared sh[PAIRS_PER_BLOCK];
  __shared__ uint32_t krow_scr[PAIRS_PER_BLOCK][wv::KROW_SCRATCH_DWORDS];  // the main wavefronts' address hash: wave-private LDS
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t slot = w % PAIRS_PER_BLOCK;
  const bool helper = w >= PAIRS_PER_BLOCK;
  const uint32_t row_raw = blockIdx.x * PAIRS_PER_BLOCK + slot;
  const bool live = row_raw < a.n;
  const uint32_t row = live ? row_raw : a.n - 1;
  const bool done = row_done(a, row);
  const bool need = live && !done;
  const bool report = !helper && lane == 0;  // helper wavefronts never store
  uint32_t want[5];
  const int vi = claimed_signer<MODE>(a, row, want);
  const bool pre = row_pre(a, row);
  if (MODE != MODE_EMIT && report && need) a.vidx[row] = vi;
  auto sync = [] { __syncthreads(); };
  // (wave-uniform, the same for both wavefronts of the pair) nothing to recover: keep the workgroup's barrier count
  if (!needs_curve<MODE>(need, pre, vi)) {
    if (MODE == MODE_EMIT && report && need) emit_store_none(a, row);  // (a pre_flags row)
    sync();
    sync();
    return;
  }
  u256 r, s;
  uint32_t v;
  row_sig(a, row, r, s, v);
  const u256 z = row_digest<MODE>(a, row);
  if (helper) {
    wv::recover_helper_wave(a.gtab, z, r, s, &sh[slot], sync);
    return;
  }
  uint32_t got[5];
  aff Qa;
  const bool rec = wv::recover_pubkey_wave<99, true>(a.gtab, z, r, s, v, a.flags, got, Qa, krow_scr[slot], &sh[slot], sync);
  cold_tail<MODE>(a, row, lane == 0, rec, false, true, got, want, vi, Qa);
}

// ---- cold path, SIXTEEN LANES PER SIGNATURE: every row of a wavefront recovers its own signature ------
// (wave_fe_dev.h:recover_pubkey_row).  n = 4 096 is one wavefront per SIMD again; used for
// 4 096 < n ≤ 8 192 (up to 4 096: the pair form below).  Rows beyond n recompute the last row and store nothing.
// waves_per_eu(1, 2): the scheduler may spend registers (up to 256) on interleaving the independent
// multiplications of a doubling — 42 → 9 s_nop per doubling in the main loop, 0.474 → 0.470 ms at 4 096 rows
// (profiles/r02c_sweeps.txt) — while two wavefronts per SIMD (8 192 rows) still fit.
template <int MODE>
__global__ void __launch_bounds__(64 * WAVE_KERNEL_WAVES) __attribute__((amdgpu_waves_per_eu(1, 2))) ecrecover_rows_kernel(recover_args a) {
  const uint32_t wave = blockIdx.x * WAVE_KERNEL_WAVES + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (wave * 4u >= a.n) return;  // whole wavefront
  const uint32_t row_raw = wave * 4u + (lane >> 4);
  const bool live = row_raw < a.n;
  const uint32_t row = live ? row_raw : a.n - 1;
  const bool report = (lane & 15u) == 0;  // the first lane of a DPP row speaks for its signature
  uint32_t want[5];
  const int vi = claimed_signer<MODE>(a, row, want);
  const bool pre = row_pre(a, row);
  const bool done = row_done(a, row);
  const bool need = live && !done;
  if (MODE != MODE_EMIT && report && need) a.vidx[row] = vi;
  if (!__any(needs_curve<MODE>(need, pre, vi) ? 1 : 0)) {  // nothing in this wavefront needs the curve
    if (MODE == MODE_EMIT && report && need) emit_store_none(a, row);  // (every row left is a pre_flags row)
    return;
  }
  u256 r, s;
  uint32_t v;
  row_sig(a, row, r, s, v);
  const u256 z = row_digest<MODE>(a, row);
  uint32_t got[5];
  aff Qa;
  __shared__ uint32_t row_tab[WAVE_KERNEL_WAVES][wv::ROW_TAB_SLOTS * 64];  // the window tables: wave-private LDS
  const bool rec = wv::recover_pubkey_row(a.gtab, z, r, s, v, a.flags, got, Qa, row_tab[threadIdx.x >> 6]);
  // (rows past n recomputed the last row: `need` keeps them from storing it again)
  cold_tail<MODE>(a, row, report, rec, pre, need, got, want, vi, Qa);
}

// ---- the same, TWO WAVEFRONTS PER FOUR SIGNATURES (2 048 < n ≤ 4 096, where the kernel above runs one wavefront per SIMD) --
// A workgroup is four MAIN wavefronts (0…3: R′, tables, main loop, closing chain, Keccak) and their HELPERS (4…7, helper of
// main w is w + 4: r⁻¹ mod n, u1, u2, the GLV split, then u1·G) for the same four rows each (wave_fe_dev.h: rows_pair_shared,
// recover_pubkey_row<…, PAIR>, recover_helper_row).  Wavefronts w and w + 4 of a workgroup share a SIMD
// (tools/simd_placement_probe.hip), so a helper issues in its main wavefront's stalls.  The two meet in LDS twice.
// BARRIER 1 is a barrier of all eight wavefronts: every wavefront passes it, whatever its rows turn out to be, before any
// wavefront of the workgroup ends.  BARRIER 2 is a hand-over (rows_pair_handover): a helper stores u1·G, waits for its own LDS
// stores and ENDS; only the four main wavefronts execute the second s_barrier.  That rests on one documented property of the
// hardware: s_barrier waits for the wavefronts of the workgroup that have NOT ENDED, so the barrier is satisfied once the four
// main wavefronts stand at it and the four helpers are gone — the same whether a helper ended long before the mains arrived
// (its stores were complete before its s_endpgm) or after (the mains are held until the last helper has ended).  `if (row >=
// n) return;` in front of a later __syncthreads() relies on the same property.  A pair with nothing to do only synchronises —
// main: barrier 1, barrier 2; helper: barrier 1, end — and main and helper decide that on the same rows.  n = 17: workgroup 0
// is four working pairs; in workgroup 1 pair 0 works on row 16 (its other three rows repeat it, unreported) and pairs 1…3 are
// idle.  At barrier 1 stand all eight: main 0 behind its tables, helper 0 behind the split, the six idle wavefronts at once.
// The three idle helpers end there; helper 0 adds u1·G, publishes and ends.  At barrier 2 stand main 0 (behind its main loop)
// and the idle mains (at once): it opens when helper 0 has ended, which is all main 0 needs, and the idle mains read nothing.
// WHY the helper leaves: it holds 168 of a SIMD's 512 registers per lane.  Parked at barrier 2 it kept the next pipelined
// pass's workgroup (2 × 168 more per SIMD) off the compute unit for most of this pass; gone, 168 + 336 fit.
// WHERE it does not: a launch that covers only half of the device's compute units leaves idle ones enough to the next pass,
// and there a parked helper is useful — it keeps that pass off this one's SIMDs (2 049 rows: + 0.9 % per step with the
// helpers gone, profiles/r27_helper_leave_ab.txt).  The host picks the instantiation (launch_cold): with STAY the helpers stand at
// barrier 2 as well, as they did before round 27, and the barrier is one of all eight again.
constexpr int ROWS_PAIRS_PER_BLOCK = 4;
template <bool STAY>
struct rows_pair_handover {
  __device__ void operator()() const { __syncthreads(); }  // barrier 1
  // the LDS stores of this wavefront are complete (s_waitcnt lgkmcnt(0)) before the caller's return ends the program
  __device__ void publish_and_leave() const {
    if constexpr (STAY)
      __syncthreads();
    else
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  }
  __device__ void wait() const { __syncthreads(); }  // barrier 2: the main wavefronts (and the helpers that stay)
};
template <int MODE, bool STAY = false>
__global__ void __launch_bounds__(128 * ROWS_PAIRS_PER_BLOCK) ecrecover_rows_pair_kernel(recover_args a) {
  __shared__ uint32_t row_tab[ROWS_PAIRS_PER_BLOCK][wv::ROW_TAB_SLOTS * 64];  // the main wavefronts' window tables
  __shared__ wv::rows_pair_shared sh[ROWS_PAIRS_PER_BLOCK];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t slot = w % ROWS_PAIRS_PER_BLOCK;
  const bool helper = w >= ROWS_PAIRS_PER_BLOCK;
  const uint32_t wave = blockIdx.x * ROWS_PAIRS_PER_BLOCK + slot;
  const uint32_t row_raw = wave * 4u + (lane >> 4);
  const bool live = row_raw < a.n;
  const uint32_t row = live ? row_raw : a.n - 1;
  const bool report = !helper && (lane & 15u) == 0;  // helper wavefronts never store
  uint32_t want[5];
  const int vi = claimed_signer<MODE>(a, row, want);
  const bool pre = row_pre(a, row);
  const bool done = row_done(a, row);
  const bool need = live && !done;
  if (MODE != MODE_EMIT && report && need) a.vidx[row] = vi;
  const rows_pair_handover<STAY> sync;
  // (wave-uniform, the same for both wavefronts of the pair: in MODE_EMIT from pre_flags and `live` alone)
  if (!__any(needs_curve<MODE>(need, pre, vi) ? 1 : 0)) {
    if (MODE == MODE_EMIT && report && need) emit_store_none(a, row);  // (every row left is a pre_flags row)
    sync();
    if (!helper || STAY) sync.wait();  // (an idle helper has nothing to publish: unless it stays, it ends behind barrier 1)
    return;
  }
  u256 r, s;
  row_sig(a, row, r, s);
  if (helper) {  // only the helper needs the digest ...
    wv::recover_helper_row(a.gtab, row_digest<MODE>(a, row), r, s, &sh[slot], sync);
    return;
  }
  const uint32_t v = row_recid(a, row);  // ... and only the main wavefront the recovery id
  uint32_t got[5];
  aff Qa;
  const bool rec = wv::recover_pubkey_row<99, true>(a.gtab, secp::zero256(), r, s, v, a.flags, got, Qa, row_tab[slot], &sh[slot], sync);
  // (rows past n recomputed the last row: `need` keeps them from storing it again)
  cold_tail<MODE>(a, row, (lane & 15u) == 0, rec, pre, need, got, want, vi, Qa);
}

// ---- warm path table build -------------------------------------------------------------------
// Lane ↔ (validator, window): a wavefront holds ONE window index for 64 consecutive validators so
// that the doubling loop's trip count is wave-uniform.
// A build pass is three launches on one stream: claim (KNOWN → BUILDING: the set of slots this pass builds is fixed here,
// whatever other contexts learn meanwhile), build, commit (BUILDING → BUILT).  Passes are serialised by the host (the
// device's mutex).
__global__ void qtab_claim_kernel(uint32_t *__restrict__ pub_state, uint32_t n_slots) {
  uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n_slots && __hip_atomic_load(pub_state + v, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == KEY_KNOWN)
    pub_state[v] = KEY_BUILDING;  // (the acquire pairs with learn_key's release: `pub` of this slot is complete)
}
template <int FORM = QTAB_WIDE>
__global__ void __launch_bounds__(64) qtab_build_kernel(const uint32_t *__restrict__ pub, const uint32_t *__restrict__ pub_state,
                                                        uint32_t *__restrict__ qtab, uint32_t n_validators) {
  constexpr uint32_t WINDOWS = FORM == QTAB_GLV ? QGLV_WINDOWS : QTAB_WINDOWS;  // (the grid: ⌈slots / 64⌉ × WINDOWS workgroups)
  const uint32_t w = blockIdx.x % WINDOWS;
  const uint32_t v = (blockIdx.x / WINDOWS) * 64 + threadIdx.x;
  const bool work = v < n_validators && pub_state[v] == KEY_BUILDING;
  if (!__any(work ? 1 : 0)) return;
  aff Q = work ? load_affine(pub + (size_t)GTAB_ENTRY_DWORDS * v) : secp::generator();
  uint32_t *out = qtab + qtab_slot_dwords<FORM>() * (work ? v : 0u) + qtab_window_dwords<FORM>((int)w);
  qtab_build_window<FORM>(Q, (int)w, out, work);
}
__global__ void qtab_commit_kernel(uint32_t *__restrict__ pub_state, uint32_t n_validators) {
  uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n_validators && pub_state[v] == KEY_BUILDING) pub_state[v] = KEY_BUILT;
}

// ---- §8f rank 3: IbftMessage wire bytes → verifier columns (wire_dev.h) -----------------------------
// One lane per message: canonical-form walk, Keccak of PayloadNoSig, scatter into the columns.
// The 64 messages of a wavefront are contiguous in the batch: they are brought into LDS with coalesced dword loads
// first (a lane walking ≈200 bytes of HBM one dependent byte load at a time made this kernel 75 µs), and every lane
// walks and hashes its message from there.  A wavefront whose messages exceed the buffer reads HBM directly.
constexpr uint32_t WIRE_LDS_BYTES = 32 * 1024;
__global__ void __launch_bounds__(64) wire_parse_kernel(const uint8_t *__restrict__ wire_bytes, const uint32_t *__restrict__ off,
                                                        uint32_t n, wire::row_info *__restrict__ rows,
                                                        uint8_t *__restrict__ digest32, uint8_t *__restrict__ sig65,
                                                        uint8_t *__restrict__ from20, uint8_t *__restrict__ seal65,
                                                        uint8_t *__restrict__ pre_flags) {
  __shared__ __attribute__((aligned(16))) uint8_t lbuf[WIRE_LDS_BYTES + 16];
  const uint32_t row0 = blockIdx.x * 64u, lane = threadIdx.x;
  const uint32_t cnt = n - row0 < 64u ? n - row0 : 64u;
  const uint32_t b0 = off[row0] & ~15u, b1 = off[row0 + cnt];
  const bool staged = b1 - b0 <= WIRE_LDS_BYTES;  // wave-uniform
  if (staged) {
    cw::stage_bytes(lbuf, wire_bytes + b0, b1 - b0, lane);
    __syncthreads();
  }
  const uint32_t row = row0 + lane;
  if (row >= n) return;
  const uint32_t o0 = off[row], o1 = off[row + 1];
  const uint8_t *m = staged ? lbuf + (o0 - b0) : wire_bytes + o0;
  wire::process_row(m, o1 - o0, rows + row, digest32 + 32ull * row, sig65 + 65ull * row, from20 + 20ull * row,
                    seal65 + 65ull * row, pre_flags + row);
}
// IBFT_FLAG_WIRE_RECODE: the second walk, over the rows wire_parse_kernel marked NEEDS_HOST (wire_recode_dev.h).  The same
// grid; a wavefront with no such row leaves after one load per lane and a ballot — that is all a batch of canonical rows
// pays.  Otherwise the wavefront's bytes are staged like above and the flagged lanes decode tolerantly, hash the canonical
// re-encoding and overwrite their row's columns; a row outside the recode class is left as it was.
__global__ void __launch_bounds__(64) wire_recode_kernel(const uint8_t *__restrict__ wire_bytes, const uint32_t *__restrict__ off,
                                                         uint32_t n, wire::row_info *__restrict__ rows,
                                                         uint8_t *__restrict__ digest32, uint8_t *__restrict__ sig65,
                                                         uint8_t *__restrict__ from20, uint8_t *__restrict__ seal65,
                                                         uint8_t *__restrict__ pre_flags) {
  __shared__ __attribute__((aligned(16))) uint8_t lbuf[WIRE_LDS_BYTES + 16];
  const uint32_t row0 = blockIdx.x * 64u, lane = threadIdx.x, row = row0 + lane;
  const bool flagged = row < n && rows[row].status == wire::STATUS_NEEDS_HOST;
  if (!__any(flagged ? 1 : 0)) return;
  const uint32_t cnt = n - row0 < 64u ? n - row0 : 64u;
  const uint32_t b0 = off[row0] & ~15u, b1 = off[row0 + cnt];
  const bool staged = b1 - b0 <= WIRE_LDS_BYTES;  // wave-uniform
  if (staged) {
    cw::stage_bytes(lbuf, wire_bytes + b0, b1 - b0, lane);
    __syncthreads();
  }
  if (!flagged) return;
  const uint32_t o0 = off[row], o1 = off[row + 1];
  const uint8_t *m = staged ? lbuf + (o0 - b0) : wire_bytes + o0;
  wire::recode_row(m, o1 - o0, rows + row, digest32 + 32ull * row, sig65 + 65ull * row, from20 + 20ull * row,
                   seal65 + 65ull * row, pre_flags + row);
}
// After the sender pass: make the COMMIT seals found by wire_parse_kernel the resident seal batch
// (hash column ← proposal hash, signature column ← committed seal, From stays).  Rows that are not
// canonical COMMIT messages with a 32-byte hash and a 65-byte seal are pre-flagged.
__global__ void wire_stage_seals_kernel(const wire::row_info *__restrict__ rows, const uint8_t *__restrict__ seal65,
                                        uint32_t n, uint8_t *__restrict__ hash32, uint8_t *__restrict__ sig65,
                                        uint8_t *__restrict__ pre_flags) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const wire::row_info &ri = rows[row];
  const bool ok = ri.status == wire::STATUS_OK && ri.payload_kind == wire::KIND_COMMIT && ri.type == 2 &&
                  ri.hash_len == 32 && ri.seal_len == 65 && ri.from_len == 20;
  for (int i = 0; i < 32; i++) hash32[32ull * row + i] = ri.proposal_hash[i];
  for (int i = 0; i < 65; i++) sig65[65ull * row + i] = seal65[65ull * row + i];
  pre_flags[row] = ok ? 0 : 1;
}

// ---- a message set in one pass: both signatures of every message in ONE verdict launch ------------------------
// A PREPARE / COMMIT message is checked three times by the reference, at different moments: IsValidValidator when it
// arrives (core/ibft.go:1128), IsValidProposalHash and — COMMIT only — IsValidCommittedSeal when the view is
// handled (:856-862, :932-944).  All three are pure functions of the message bytes and of the validator set, so a
// whole set can be judged at once: the envelope signatures are rows [0, n) of the batch (their digests, Keccak of
// PayloadNoSig, come from payload_digest_kernel), the committed seals are rows [half, half + n) with the hash each
// message carries as digest, half = ⌈n/64⌉·64 — 2n signatures in one launch fill the chip where n alone left
// every SIMD with a single wavefront (n = 4 096: 8 192 rows, two wavefronts per SIMD).
__global__ void payload_digest_kernel(const uint8_t *__restrict__ payload, const uint32_t *__restrict__ off, uint32_t n,
                                      uint8_t *__restrict__ digest32) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = row < n;
  const uint32_t o0 = live ? off[row] : 0u, o1 = live ? off[row + 1] : 0u;
  uint64_t d[4];
  hash_range_dwords(payload + o0, o1 - o0, d);
  if (live) {
    uint4 *o = reinterpret_cast<uint4 *>(digest32 + 32ull * row);
    o[0] = make_uint4((uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32));
    o[1] = make_uint4((uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32));
  }
}
// The same set judged straight from the transport's bytes: wire_parse_kernel has filled the sender rows [0, n)
// (digest of PayloadNoSig, Signature, From) and the seal column; this kernel lays the second group of verdict rows
// [half, half + n) — the hash each message carries as digest, its committed seal as signature, From as signer — and
// decides, per row, everything about the closure that needs no arithmetic: valid_pre ≠ 0 unless the message is a
// canonical COMMIT (type 2, CommitMessage, 65-byte seal) of the view (height, round) with a 20-byte From — a canonical
// PREPARE of the view (type 1, PrepareMessage) is flagged in is_prepare instead: its closure is the hash compare alone (ExtractPrepareHash / ExtractCommitHash / ExtractCommittedSeal return nil
// otherwise, messages/helpers.go).  A PREPARE row's seal row is a zero signature: its verdict is forced below.
__global__ void wire_set_stage_kernel(const wire::row_info *__restrict__ rows, const uint8_t *__restrict__ seal65, uint32_t n,
                                      uint32_t half, uint64_t height, uint64_t round, uint8_t *__restrict__ hash32,
                                      uint8_t *__restrict__ hash_len, uint8_t *__restrict__ sig65,
                                      uint8_t *__restrict__ signer20, uint8_t *__restrict__ pre_flags,
                                      uint8_t *__restrict__ is_prepare, uint8_t *__restrict__ row_class,
                                      uint8_t *__restrict__ host_row_class) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const wire::row_info &ri = rows[row];
  const bool here = ri.status == wire::STATUS_OK && ri.has_view && ri.height == height && ri.round == round && ri.from_len == 20;
  const bool prepare = here && ri.type == 1 && ri.payload_kind == wire::KIND_PREPARE;
  const bool commit = here && ri.type == 2 && ri.payload_kind == wire::KIND_COMMIT && ri.seal_len == 65;
  const uint32_t dst = half + row;
  for (int i = 0; i < 32; i++) hash32[32ull * dst + i] = ri.proposal_hash[i];
  for (int i = 0; i < 65; i++) sig65[65ull * dst + i] = commit ? seal65[65ull * row + i] : 0;
  for (int i = 0; i < 20; i++) signer20[20ull * dst + i] = ri.from[i];
  hash_len[row] = ri.hash_len;
  pre_flags[dst] = commit ? 0 : 1;  // the verdict launch skips every seal row that is not a COMMIT's (whole wavefronts exit)
  is_prepare[row] = prepare ? 1 : 0;
  // what the host needs to route the row, in one byte (include/ibftgpu.h: IBFT_WIRE_CLASS_*): bit 0 = not judged here
  // (stock route), bit 1 = a PREPARE / COMMIT of the asked view, i.e. its valid bit IS the closure's verdict, bits 4.. = type
  const bool in_view = ri.status == wire::STATUS_OK && ri.has_view && ri.height == height && ri.round == round;
  const uint8_t cls = (uint8_t)((ri.status == wire::STATUS_OK ? 0 : 1) | ((in_view && (ri.type == 1 || ri.type == 2)) ? 2 : 0) |
                                ((ri.type & 15u) << 4));
  row_class[row] = cls;
  if (host_row_class) host_row_class[row] = cls;
}

// ---- §8f rank 2 from the transport's bytes: the certificate tree (wire_dev.h, second half) -------------------------
// ibft_verify_certificates_wire: PREPREPARE / ROUND_CHANGE messages carry messages (RoundChangeCertificate,
// PreparedCertificate: core/ibft.go:470-551, 683-788 verify every one of them).  Level by level, rows [lo, hi) of one
// level at a time:
//   cert_parse_kernel       a lane per message: the DEEP walk of its own fields, sender columns, digest of a short message
//                           that has nothing below it; where its nested messages lie goes to cert_span
//   cert_walk_kernel<false> a wavefront per message with a certificate: counts (and checks) the nested messages
//   cert_scan_kernel        exclusive scan of the counts: every row's children become a contiguous row range of the next
//   (cert_scan_tiles/_offsets/_apply for a long level)  level, in order, and the rows whose digest is deferred are listed;
//                           the totals go to the host, which sizes the next level's launches.  The four kernels, the
//                           threshold between the two forms and their launch geometry live in cert_scan_dev.h (included
//                           below, where they stood), so that the test library runs them too
//   cert_walk_kernel<true>  the same walk again, writing the child rows
// then, bottom-up, cert_propagate_kernel (a message with a non-canonical message below it is not canonical either),
// cert_digest_wave_kernel (the deferred digests — messages that carry certificates, long messages — and the proposal hashes:
// one wavefront per sponge, wave_sponge), cert_finish_kernel (final pre-flags and class bits), the verdict launch over all
// rows — or, with the digests on a side stream, over the rows that are not deferred, and a second small one over the deferred
// rows (cert_carrier_stage_kernel, cert_scatter_kernel) —, cert_compare_kernel (hash bits).
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  for (int o = 32; o; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  for (int o = 32; o; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__global__ void __launch_bounds__(64) cert_parse_kernel(const uint8_t *__restrict__ wire_bytes, wire::node_info *__restrict__ nodes,
                                                        uint32_t lo, uint32_t hi, wire::row_info *__restrict__ rows,
                                                        uint2 *__restrict__ cert_span, uint8_t *__restrict__ digest32,
                                                        uint8_t *__restrict__ sig65, uint8_t *__restrict__ from20,
                                                        uint8_t *__restrict__ pre_flags) {
  __shared__ __attribute__((aligned(16))) uint8_t lbuf[WIRE_LDS_BYTES + 16];
  const uint32_t lane = threadIdx.x, row = lo + blockIdx.x * 64u + lane;
  const bool live = row < hi;
  wire::node_info nd{};
  if (live) nd = nodes[row];
  // the 64 messages of a wavefront are usually neighbours in the buffer (children of one certificate): staged in LDS
  // with coalesced dword loads when they span little enough, like wire_parse_kernel
  const uint32_t b0 = wave_min_u32(live ? nd.off : 0xFFFFFFFFu) & ~15u, b1 = wave_max_u32(live ? nd.off + nd.len : 0u);
  const bool staged = b1 >= b0 && b1 - b0 <= WIRE_LDS_BYTES;  // wave-uniform
  if (staged) {
    cw::stage_bytes(lbuf, wire_bytes + b0, b1 - b0, lane);
    __syncthreads();
  }
  if (!live) return;
  const uint8_t *m = staged ? lbuf + (nd.off - b0) : wire_bytes + nd.off;
  uint32_t span[2];
  wire::process_tree_row(m, nd.len, rows + row, &nd, span, digest32 + 32ull * row, sig65 + 65ull * row, from20 + 20ull * row,
                         pre_flags + row);
  nodes[row] = nd;
  cert_span[row] = make_uint2(span[0], span[1]);
}
// A wavefront per message with a certificate lists (FILL) or counts and checks (!FILL) its nested messages: cw::walk_certificate.
template <bool FILL>
__global__ void __launch_bounds__(64) cert_walk_kernel(const uint8_t *__restrict__ wire_bytes, wire::node_info *__restrict__ nodes,
                                                       wire::row_info *__restrict__ rows, const uint2 *__restrict__ cert_span,
                                                       uint32_t lo, uint32_t hi, uint32_t *__restrict__ child_count) {
  __shared__ __attribute__((aligned(16))) uint8_t win[cw::CERT_WIN_BYTES + 16];
  const uint32_t row = lo + blockIdx.x, lane = threadIdx.x;
  if (row >= hi) return;
  const wire::node_info nd = nodes[row];
  const bool has = rows[row].status == wire::STATUS_OK && (nd.flags & wire::TREE_HAS_CERT);
  const uint32_t deferred = rows[row].status == wire::STATUS_OK && wire::tree_deferred(nd) ? 0x80000000u : 0u;
  if (!has || (FILL && nd.n_children == 0)) {
    if (!FILL && lane == 0) child_count[row - lo] = deferred;
    return;
  }
  const bool pc = rows[row].payload_kind == wire::KIND_ROUND_CHANGE;
  const uint2 span = cert_span[row];
  const uint32_t pos = nd.off + span.x;
  bool ok = true;
  uint32_t count = cw::walk_certificate(wire_bytes, pos, pos + span.y, pc, win, lane, ok, [&](uint32_t ordinal, uint32_t off, uint32_t len, uint8_t role) {
    if (!FILL) return;
    wire::node_info c{};
    c.off = off;
    c.len = len;
    c.parent = row;
    c.ordinal = ordinal;
    c.level = (uint8_t)(nd.level + 1);
    c.role = role;
    nodes[nd.first_child + ordinal] = c;
  });
  if (!FILL && lane == 0) {
    if (!ok) {  // a malformed wrapper: the whole message goes the stock route, nothing below it is listed
      rows[row].status = wire::STATUS_NEEDS_HOST;
      count = 0;
    }
    nodes[row].n_children = count;
    child_count[row - lo] = count | (ok ? deferred : 0u);
  }
}
}  // namespace ibftk
// cert_scan_kernel, cert_scan_tiles_kernel, cert_scan_offsets_kernel, cert_scan_apply_kernel and the helper that launches them
#include "cert_scan_dev.h"
namespace ibftk {
__global__ void cert_propagate_kernel(const wire::node_info *__restrict__ nodes, wire::row_info *__restrict__ rows, uint32_t lo,
                                      uint32_t hi) {
  const uint32_t row = lo + blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= hi) return;
  const uint32_t parent = nodes[row].parent;
  if (rows[row].status != wire::STATUS_OK && parent != wire::NO_PARENT) rows[parent].status = wire::STATUS_NEEDS_HOST;
}
// (Keccak by one wavefront: cert_wave_dev.h, cw::sponge_message.)
// One job per wavefront: job 2k hashes PayloadNoSig of deferred row k → digest32[row]; job 2k + 1 hashes the Proposal that row
// carries, keccak(rawProposal ‖ BE64(round)) → prop_digest32[row] (exits at once when there is none).  The message is
// piece A = [a0, a0 + na) followed by piece B = [b0, b0 + nb) of the buffer, then `tail` (≤ 8 bytes, by value).
// mid_state (ibft_decide_certificates_wire; null otherwise): the proposal job of a ROOT (row < mid_roots) also leaves the sponge
// state behind the ⌊raw_len / 136⌋ full blocks of raw, 25 words at mid_state + 25·row — keccak(raw ‖ BE64(another round)) is
// closed from there by cert_decide_proposals_kernel.
__global__ void __launch_bounds__(64) cert_digest_wave_kernel(const uint8_t *__restrict__ wire_bytes, const wire::node_info *__restrict__ nodes,
                                                              const wire::row_info *__restrict__ rows,
                                                              const uint32_t *__restrict__ deferred_rows, uint32_t region,
                                                              uint8_t *__restrict__ digest32, uint8_t *__restrict__ prop_digest32,
                                                              uint64_t *__restrict__ mid_state, uint32_t mid_roots) {
  __shared__ uint64_t A[32], B[32];
  const uint32_t row = deferred_rows[blockIdx.x >> 1], lane = threadIdx.x;
  // region ≠ 0: the deferred rows form a batch of their own at rows [region, region + deferred) of the columns (cert_carrier_stage_kernel)
  const uint32_t digest_row = region ? region + (blockIdx.x >> 1) : row;
  const bool proposal_job = blockIdx.x & 1u;
  const wire::node_info nd = nodes[row];
  if (rows[row].status != wire::STATUS_OK) return;  // block-uniform: not judged here
  const uint8_t *m;
  uint32_t cut0, gap, total;
  uint64_t tail = 0;
  if (!proposal_job) {
    if (nd.len > wire::TREE_DIGEST_MAX_BYTES) return;
    m = wire_bytes + nd.off;
    cut0 = nd.cut0;
    gap = nd.cut1 - nd.cut0;
    total = nd.len - gap;
  } else {
    if (!(nd.flags & wire::TREE_HAS_PROPOSAL) || nd.raw_len > wire::TREE_DIGEST_MAX_BYTES) return;
    m = wire_bytes + nd.raw_off;
    cut0 = nd.raw_len;  // everything before the "cut" is the raw proposal; behind it come the 8 bytes of the round
    gap = 0;
    total = nd.raw_len + 8u;
    for (int k = 0; k < 8; k++) tail |= (uint64_t)((nd.proposal_round >> (8 * (7 - k))) & 0xFFu) << (8 * k);  // BE64 as the bytes lie
  }
  uint64_t *save = mid_state && proposal_job && row < mid_roots ? mid_state + 25ull * row : nullptr;  // block-uniform
  const uint64_t word = cw::sponge_message_from(m, cut0, gap, total, tail, proposal_job, lane, A, B, 0ull, 0u, save, cut0 / 136u * 136u);
  if (lane < 4u) *reinterpret_cast<uint64_t *>((proposal_job ? prop_digest32 + 32ull * row : digest32 + 32ull * digest_row) + 8u * lane) = word;
}
// After the deferred digests: every row's final pre-flag and class bits, and the hash of the Proposal it carries (a lane per row;
// proposals are short next to the messages that carry certificates)
// two_launches: the deferred rows are judged as a batch of their own (cert_carrier_stage_kernel) while the verdict launch over the
// other rows is already running — their pre-flags in the tree's own rows must keep saying "verdict 0".
__global__ void __launch_bounds__(64) cert_finish_kernel(const uint8_t *__restrict__ wire_bytes, wire::node_info *__restrict__ nodes,
                                                         const wire::row_info *__restrict__ rows, uint32_t n,
                                                         uint8_t *__restrict__ digest32, uint8_t *__restrict__ prop_digest32,
                                                         uint8_t *__restrict__ pre_flags, uint32_t two_launches) {
  const uint32_t row = blockIdx.x * 64u + threadIdx.x;
  if (row >= n) return;
  wire::node_info nd = nodes[row];
  // almost every row of a big tree is a PREPARE: not deferred, no Proposal — nothing to do (the proposal-digest column was zeroed)
  if (!wire::tree_deferred(nd) && !(nd.flags & wire::TREE_HAS_PROPOSAL)) return;
  const uint8_t before = nd.flags;
  uint8_t unused = 0;
  wire::tree_digest_row(wire_bytes, rows + row, &nd, digest32 + 32ull * row, prop_digest32 + 32ull * row, two_launches ? &unused : pre_flags + row,
                        false);  // a deferred row's digests are there already
  if (nd.flags != before) nodes[row].flags = nd.flags;
}
// The batch of the deferred rows: signature, From and pre-flag of deferred row k → row region + k of the columns (its digest is
// written there by cert_digest_wave_kernel); after the second verdict launch cert_scatter_kernel brings the bits home.
__global__ void cert_carrier_stage_kernel(const wire::node_info *__restrict__ nodes, const wire::row_info *__restrict__ rows,
                                          const uint32_t *__restrict__ deferred_rows, uint32_t n_deferred, uint32_t region,
                                          uint8_t *__restrict__ sig65, uint8_t *__restrict__ from20, uint8_t *__restrict__ pre_flags) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_deferred) return;
  const uint32_t row = deferred_rows[k], dst = region + k;
  const wire::row_info &ri = rows[row];
  const bool judged = ri.status == wire::STATUS_OK && nodes[row].len <= wire::TREE_DIGEST_MAX_BYTES;
  for (int i = 0; i < 65; i++) sig65[65ull * dst + i] = sig65[65ull * row + i];
  for (int i = 0; i < 20; i++) from20[20ull * dst + i] = from20[20ull * row + i];
  pre_flags[dst] = (uint8_t)((judged ? 0 : 1) | (ri.sig_len == 65 && ri.from_len == 20 ? 0 : 2));
}
__global__ void cert_scatter_kernel(const uint32_t *__restrict__ deferred_rows, uint32_t n_deferred, uint32_t region, uint64_t *__restrict__ mask) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_deferred) return;
  const uint32_t src = region + k, row = deferred_rows[k];
  if ((mask[src >> 6] >> (src & 63u)) & 1ull) atomicOr((unsigned long long *)(mask + (row >> 6)), 1ull << (row & 63u));
}
}  // namespace ibftk
// the five cert_dedup_*_kernels (IBFT_FLAG_CERT_DEDUP, ibft_cert_stats) and the helpers that launch them
#include "cert_dedup_kernels.h"
namespace ibftk {
// hash / self bits and the routing byte of every row (wire::tree_compare_row), one verdict word per wavefront
__global__ void __launch_bounds__(256) cert_compare_kernel(const wire::node_info *__restrict__ nodes, const wire::row_info *__restrict__ rows,
                                                           const uint8_t *__restrict__ prop_digest32, uint32_t n,
                                                           uint64_t *__restrict__ hash_mask, uint64_t *__restrict__ self_mask,
                                                           uint8_t *__restrict__ row_class) {
  const uint32_t row = blockIdx.x * 256u + threadIdx.x;
  bool hash_bit = false, self_bit = false;
  if (row < n) {
    uint8_t cls;
    wire::tree_compare_row(nodes, rows, prop_digest32, row, hash_bit, self_bit, cls);
    row_class[row] = cls;
  }
  const uint64_t hb = __ballot(hash_bit), sb = __ballot(self_bit);
  if ((threadIdx.x & 63u) == 0 && row < n) {
    hash_mask[row >> 6] = hb;
    self_mask[row >> 6] = sb;
  }
}

// ---- a8: weighted quorum tally ------------------------------------------------------------
// HasQuorum (core/validator_manager.go:77-96): Σ power over the DISTINCT member senders of the valid rows
// ≥ ⌊2·total/3⌋+1.  Several workgroups (4 096 rows each) walk the verdict words: a validator's power is
// counted once — a bitmap in HBM updated with device-scope atomicOr gives the Go map's set semantics across
// workgroups —, lanes reduce with wave shuffles, waves through LDS, workgroups with one device-scope
// atomicAdd per 32-bit piece; the workgroup that draws the last ticket recombines the pieces (carries),
// compares with the quorum, delivers the result (also into mapped host memory) and leaves bitmap,
// accumulators and ticket zeroed for the next launch.
//   PW = 64-bit words per voting power: 1 (u64, ibft_set_validators) or 4 (256-bit, ibft_set_validators_u256:
//   GetVotingPowers returns *big.Int, validator_manager.go:17-31).  Sums are TALLY_SUM_WORDS wide.
// out[] (u64 words): [0..1] low 128 bits of the power, [2] valid_rows | distinct << 32, [3] has_quorum,
//   [4] keys learned | a learned validator (written by the recover kernels), [5..9] the power in full,
//   [10] valid rows sent by the proposer (prop_on: any such row voids the quorum, validator_manager.go:114-121),
//   [16..16+2·PW) the raw 32-bit piece sums (what the multi-GPU exchange adds across ranks).
constexpr int TALLY_THREADS = 1024;
constexpr int TALLY_ROWS_PER_BLOCK = 4096;
// (TALLY_SUM_WORDS, TALLY_MAX_PIECES, pieces_to_words, words_ge and tally_record: tally_dev.h, where the CPU harness reaches them)
constexpr int TALLY_OUT_WIDE = 5;        // out[5..10)
constexpr int TALLY_OUT_PIECES = 16;     // out[16..24)
constexpr int TALLY_OUT_WORDS = 24;
constexpr int TALLY_ACC_WORDS = TALLY_MAX_PIECES + 4;  // pieces, valid, distinct, ticket, rows sent by the proposer
constexpr int TALLY_OUT_PROPOSER_ROWS = 10;            // out[10]: valid rows whose sender is the proposer (HasPrepareQuorum)
constexpr int32_t VIDX_PROPOSER_OUTSIDER = -2;         // lookup_kernel: sender == proposer and the proposer is no validator
// bytes of dynamic LDS the distinct-sender bitmap of a tally kernel may take: 393 216 entries; beyond, lds_bitmap = 0
constexpr uint32_t TALLY_BITMAP_LDS_MAX = 48 * 1024;

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- what every tally kernel does around its own rows, written once -------------------------------------------------------------
// (the arithmetic of the record — pieces_to_words, words_ge, tally_record — is tally_dev.h, where the CPU harness reaches it;
// the scan of one value per thread, block_scan_1024, is cert_scan_dev.h)
//
// The distinct-sender claim: a sender's power counts once (a map[string]struct{} in core/validator_manager.go:147-155), so a
// row counts iff it is the one that set the sender's bit.  bm: a bitmap in LDS (workgroup scope) or in HBM (device scope).
__device__ __forceinline__ bool claim_first(uint32_t *bm, uint32_t index) {
  const uint32_t m = 1u << (index & 31);
  return !(atomicOr(&bm[index >> 5], m) & m);
}
// Several workgroups share the set through a bitmap in HBM, but device-scope atomics on one cache line retire at ≈12 ns each —
// one per ROW made tally_kernel 52 µs at 4 096 rows.  So a workgroup claims in its LDS bitmap first and merges that WORD by
// word (one returning atomicOr per non-empty word), keeping per word the bits it was the first to set: a row counts iff it
// was first inside its workgroup (claim_first on lds) AND its workgroup was first for the sender (still_first afterwards).
// The first barrier is behind every row's claim, the second in front of every re-test.
template <int THREADS>
__device__ __forceinline__ void merge_first_bits(uint32_t *lds, uint32_t *hbm, uint32_t words) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < words; i += THREADS) {
    const uint32_t mine = lds[i];
    if (mine) lds[i] = mine & ~atomicOr(&hbm[i], mine);
  }
  __syncthreads();
}
__device__ __forceinline__ bool still_first(const uint32_t *lds, uint32_t index) { return (lds[index >> 5] >> (index & 31)) & 1u; }

// "The last workgroup finishes": every workgroup draws one ticket when its work is done; the one that draws the last knows
// that every other has drawn, and delivers / cleans up for the launch.  True in every thread of that workgroup.
// What it may conclude depends on what the CALLER ordered in front of the call — two disciplines, each sufficient:
//   fence     every thread __threadfence()s, then a barrier (block_tally_kernel<SETS>, wire_sets_tally_kernel,
//             wire_seals_combine_kernel): each thread's earlier stores and atomics are performed device-wide before it passes
//             the barrier, thread 0 draws behind the barrier, so whoever observes the ticket observes them.
//   waitcnt   the threads that issued non-returning device-scope atomics wait for vmcnt(0), then a barrier
//             (tally_kernel<*, true>): a device-scope read-modify-write is performed where it is acknowledged — at the L2,
//             the one point of coherence of the device — so an acknowledged add is in place before the ticket is drawn, and
//             returning atomics (the bitmap's atomicOr) were awaited by their users.  It orders atomics only, no plain stores:
//             enough for tally_kernel, whose workgroups hand each other nothing else, and cheaper than a fence per thread.
// (block_tally_kernel without SETS orders nothing in front: its workgroups only READ what the last one then clears, and a
// load whose value was used has completed.)
// The block and sets tallies let thread 0 fence once more directly in front of its draw, as they always have: that line
// stays at their call sites too, and it is all the plain block tally has.  The last workgroup reads what the others added
// with device-scope atomics.
template <class T>
__device__ __forceinline__ bool draw_last_ticket(T *ticket, uint32_t &last_flag) {
  if (threadIdx.x == 0) {
    T t;
    if constexpr (sizeof(T) == 8) t = (T)atomicAdd(reinterpret_cast<unsigned long long *>(ticket), 1ull);
    else t = atomicAdd(ticket, (T)1);
    last_flag = (t == (T)gridDim.x - (T)1) ? 1u : 0u;
  }
  __syncthreads();
  return last_flag != 0;
}
// … and the last workgroup leaves the ticket zero for the next launch.
template <class T>
__device__ __forceinline__ void reset_ticket(T *ticket) {
  if (threadIdx.x == 0) __hip_atomic_store(ticket, (T)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The verdict kernels accumulate into work_mask (atomicOr / ballot words).  A tally CONSUMES it: word i moves to `mask`, to
// host_mask (mapped pinned host memory) when given, and work_mask is left zero for the next launch.  ATOMIC: under a family
// of sets other workgroups atomic-AND other bits of the same word, so the word is read with a device-scope atomic load.
template <bool ATOMIC>
__device__ __forceinline__ uint64_t verdict_word(const uint64_t *work_mask, uint32_t i) {
  if constexpr (ATOMIC) return __hip_atomic_load(work_mask + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return work_mask[i];
}
__device__ __forceinline__ void hand_over_word(uint64_t *work_mask, uint64_t *mask, uint64_t *host_mask, uint32_t i, uint64_t w) {
  work_mask[i] = 0;
  mask[i] = w;
  if (host_mask) host_mask[i] = w;
}
template <bool ATOMIC, int THREADS>
__device__ __forceinline__ void hand_over_words(uint64_t *work_mask, uint64_t *mask, uint64_t *host_mask, uint32_t words) {
  for (uint32_t i = threadIdx.x; i < words; i += THREADS) hand_over_word(work_mask, mask, host_mask, i, verdict_word<ATOMIC>(work_mask, i));
}

// A workgroup's sums: every wavefront leaves its sum of v in row[wave] (wave_part), and behind a barrier one thread adds the
// wavefronts' parts (parts_total).  on = false (launch-uniform): nobody has anything to add, the part is 0 without the shuffles.
// block_sum / block_totals: the NP power pieces at once; the pieces beyond NP are 0.  block_tally_kernel writes its totals out
// itself: through block_totals its <4, 1024> instantiations (8 × 16 parts) spill, as plain loops in the kernel they do not.
template <int WAVES>
__device__ __forceinline__ void wave_part(uint64_t (&row)[WAVES], uint64_t v, bool on = true) {
  const uint64_t sum = on ? wave_sum_u64(v) : 0ull;
  if ((threadIdx.x & 63u) == 0) row[threadIdx.x >> 6] = sum;
}
template <int WAVES>
__device__ __forceinline__ uint64_t parts_total(const uint64_t (&row)[WAVES]) {
  uint64_t sum = 0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) sum += row[w];
  return sum;
}
template <int NP, int ROWS, int WAVES>
__device__ __forceinline__ void block_sum(uint64_t (&part)[ROWS][WAVES], const uint64_t (&p)[NP]) {
#pragma unroll
  for (int k = 0; k < NP; k++) wave_part(part[k], p[k]);
}
template <int NP, int ROWS, int WAVES>
__device__ __forceinline__ void block_totals(const uint64_t (&part)[ROWS][WAVES], uint64_t (&piece)[TALLY_MAX_PIECES]) {
#pragma unroll
  for (int k = 0; k < TALLY_MAX_PIECES; k++) {
    piece[k] = 0;
    if (k < NP) piece[k] = parts_total(part[k]);
  }
}

// After the verdict launch of a message set: word w of the work mask holds the envelope verdicts of rows 64w.., word
// half/64 + w the seal verdicts of the same messages.  a1 is evaluated here (hash_eq_kernel's compare).  Delivered: sender
// words (IsValidValidator), valid words (a1 ∧ a2 — handlePrepare's / handleCommit's closure; a1 alone without seals);
// the tally goes on with sender ∧ valid, which answers hasQuorumByMsgType for the set.  This runs INSIDE the tally
// kernel (a wavefront per verdict word, lane l judging row 64w + l): as a kernel of its own it cost 4.4 µs plus a
// dependency gap per set.
struct set_args {
  const uint8_t *hash32;    // n × 32: the proposal hash each message carries
  const uint8_t *hash_len;  // n
  const uint64_t *H4;       // keccak256(raw proposal ‖ BE64(round))
  const uint8_t *sender_pre, *valid_pre;  // n each or null: rows the host rejected before any crypto
  const uint8_t *no_seal;   // n or null: rows (PREPAREs of a mixed wire batch) whose valid bit is a1 alone
  uint32_t n, half_words;   // half_words = 0: no seals (PREPARE)
  uint64_t *sender_out, *valid_out;    // device copies (⌈n/64⌉ words each)
  uint64_t *host_sender, *host_valid;  // mapped pinned host memory or null
};
// Per-row part (loads only, no stores: the caller issues several rows' loads before it waits for any of them)
struct set_row_flags {
  bool a1, spre, nos;
};
__device__ __forceinline__ set_row_flags set_row(const set_args &a, uint32_t row) {
  set_row_flags f{false, false, false};
  if (row < a.n) {
    f.spre = a.sender_pre && a.sender_pre[row] != 0;
    f.nos = a.no_seal && a.no_seal[row] != 0;
    const uint4 *p = reinterpret_cast<const uint4 *>(a.hash32 + 32ull * row);
    const uint4 x = p[0], y = p[1];
    const uint32_t *h = reinterpret_cast<const uint32_t *>(a.H4);
    const uint32_t diff = (x.x ^ h[0]) | (x.y ^ h[1]) | (x.z ^ h[2]) | (x.w ^ h[3]) | (y.x ^ h[4]) | (y.y ^ h[5]) |
                          (y.z ^ h[6]) | (y.w ^ h[7]);
    // valid_pre marks a dead seal side; a row flagged no_seal (a PREPARE among raw messages) has no seal side to be dead
    const bool dead = a.valid_pre && a.valid_pre[row] != 0 && !f.nos;
    f.a1 = diff == 0 && a.hash_len[row] == 32 && !dead;
  }
  return f;
}
// Per-word part, called by a whole wavefront with its lanes' flags and the two verdict words already loaded; returns
// sender ∧ valid on every lane, lane 0 delivers the two words
__device__ __forceinline__ uint64_t set_finish_word(const set_args &a, uint64_t *work_mask, uint32_t w, uint32_t lane,
                                                    const set_row_flags &f, uint64_t sender_word, uint64_t seal_word) {
  const uint64_t bal = __ballot(f.a1), sbad = __ballot(f.spre), skip_seal = __ballot(f.nos);
  const uint32_t first = w * 64u;
  const uint32_t left = a.n > first ? a.n - first : 0u;
  const uint64_t tail = left >= 64 ? ~0ull : (left ? (~0ull >> (64 - left)) : 0ull);
  const uint64_t S = sender_word & tail & ~sbad;
  uint64_t V = bal;
  if (a.half_words) V &= seal_word | skip_seal;
  if (lane == 0) {
    if (a.half_words) work_mask[a.half_words + w] = 0;
    a.sender_out[w] = S;
    a.valid_out[w] = V;
    if (a.host_sender) {
      a.host_sender[w] = S;
      a.host_valid[w] = V;
    }
  }
  return S & V;
}

struct tally_args {
  uint64_t *work_mask;      // verdict words accumulated by the verdict kernels; consumed (zeroed) here
  uint64_t *mask;           // verdict words as fetch / export / exchange read them
  const int32_t *vidx;      // n: validator index of the row's sender (−1 = not a member)
  const uint32_t *vpower32; // n_validators × 2·PW little-endian 32-bit pieces
  uint32_t n, n_validators;
  uint32_t *seen;           // ⌈n_validators/32⌉ words, zero between launches
  uint64_t *acc;            // TALLY_ACC_WORDS, zero between launches
  const uint64_t *quorum;   // TALLY_SUM_WORDS
  uint64_t *out;            // TALLY_OUT_WORDS
  uint64_t *host_mask, *host_tally;  // mapped pinned host memory (or null): no device-to-host copy commands
  uint32_t lds_bitmap;      // the launch carries ⌈n_validators/32⌉ words of dynamic LDS for the workgroup's bitmap
  const uint64_t *learned_src;  // or null: {keys learned, a learned slot} of the device's key cache, passed on to the host
  uint32_t *seen_out;       // or null: the launch's distinct-sender bitmap is left here (⌈n_validators/32⌉ words) — what a
                            // sharded batch exchanges, because the SET of senders merges across shards and sums do not
  uint32_t set_on;          // a message set: the verdict words are combined here first (set_combine_word)
  // HasPrepareQuorum (/root/reference/core/validator_manager.go:99-127): the proposer's address joins the sender set
  // (prop_vidx = its validator index, −1 when it is no validator: it then adds nothing, :88-92) and a valid row sent BY
  // the proposer voids the quorum (:114-121).  prop_seat = 0: a rank of a sharded batch only counts the proposer's rows —
  // the seat is added where the shards' bitmaps are merged (exchange_unpack_kernel).
  uint32_t prop_on, prop_seat;
  int32_t prop_vidx;
  set_args set;
};

// MULTI = false: ONE workgroup (n ≤ TALLY_ROWS_PER_BLOCK, the latency-critical sizes): the distinct-sender set is
// a bitmap in LDS (dynamic: ⌈n_validators/32⌉ words) and nothing leaves the workgroup before the result — no
// global atomics, no ticket.  MULTI = true: the bitmap lives in HBM (device-scope atomicOr), workgroups add their
// 32-bit pieces with device-scope atomicAdd and the one that draws the last ticket finishes.
template <int PW, bool MULTI>
__global__ void __launch_bounds__(TALLY_THREADS) tally_kernel(tally_args a) {
  constexpr int NP = 2 * PW;
  constexpr int RPT = TALLY_ROWS_PER_BLOCK / TALLY_THREADS;
  extern __shared__ uint32_t lseen[];  // ⌈n_validators/32⌉ words when a.lds_bitmap
  __shared__ uint64_t wds[TALLY_ROWS_PER_BLOCK / 64];
  __shared__ uint64_t part[NP + 2][TALLY_THREADS / 64];
  __shared__ uint32_t last_flag;
  const uint32_t tid = threadIdx.x;
  const uint32_t row0 = blockIdx.x * (uint32_t)TALLY_ROWS_PER_BLOCK;
  const uint32_t total_words = (a.n + 63) / 64;
  // Two dependent memory round trips instead of four: the validator index of every row of this thread is loaded
  // together with the verdict words, the voting powers right behind them — both speculatively (rows without a
  // verdict bit and repeated senders simply do not use what was loaded).
  int vi[RPT];
#pragma unroll
  for (int j = 0; j < RPT; j++) {
    const uint32_t row = row0 + (uint32_t)j * TALLY_THREADS + tid;
    vi[j] = row < a.n ? a.vidx[row] : -1;
  }
  // the tally consumes the work mask (hand_over_word): every workgroup the words of its own rows
  if (a.set_on) {
    // every wavefront combines its share of the workgroup's verdict words; all loads first, then the ballots and stores
    constexpr int WPW = (TALLY_ROWS_PER_BLOCK / 64) / (TALLY_THREADS / 64);  // words per wavefront
    const uint32_t wv = tid >> 6, ln = tid & 63u;
    set_row_flags fl[WPW];
    uint64_t sw[WPW], lw[WPW];
#pragma unroll
    for (int q = 0; q < WPW; q++) {
      const uint32_t wi = row0 / 64 + wv + (uint32_t)q * (TALLY_THREADS / 64);
      const bool in = wi < total_words;
      fl[q] = set_row(a.set, in ? wi * 64u + ln : 0xFFFFFFFFu);
      sw[q] = in ? a.work_mask[wi] : 0ull;
      lw[q] = (in && a.set.half_words) ? a.work_mask[a.set.half_words + wi] : 0ull;
    }
#pragma unroll
    for (int q = 0; q < WPW; q++) {
      const uint32_t k = wv + (uint32_t)q * (TALLY_THREADS / 64);
      const uint32_t wi = row0 / 64 + k;
      uint64_t w = 0;
      if (wi < total_words) {  // wave-uniform
        w = set_finish_word(a.set, a.work_mask, wi, ln, fl[q], sw[q], lw[q]);
        if (ln == 0) hand_over_word(a.work_mask, a.mask, a.host_mask, wi, w);
      }
      if (ln == 0) wds[k] = w;
    }
  } else if (tid < TALLY_ROWS_PER_BLOCK / 64) {
    const uint32_t wi = row0 / 64 + tid;
    uint64_t w = 0;
    if (wi < total_words) {
      w = a.work_mask[wi];
      hand_over_word(a.work_mask, a.mask, a.host_mask, wi, w);
    }
    wds[tid] = w;
  }
  // the workgroup's own distinct-sender bitmap is always in LDS (a.lds_bitmap = 0 only when a huge validator set
  // does not fit: MULTI then sends every row's bit to the HBM bitmap directly)
  const uint32_t seen_words = (a.n_validators + 31) / 32;
  if (a.lds_bitmap)
    for (uint32_t i = tid; i < seen_words; i += TALLY_THREADS) lseen[i] = 0;
  uint32_t pw[RPT][NP];
#pragma unroll
  for (int j = 0; j < RPT; j++)
#pragma unroll
    for (int k = 0; k < NP; k++) pw[j][k] = vi[j] >= 0 ? a.vpower32[(size_t)vi[j] * NP + k] : 0u;
  __syncthreads();
  bool first[RPT];
  uint64_t valid = 0, distinct = 0;
  uint32_t by_proposer = 0;
#pragma unroll
  for (int j = 0; j < RPT; j++) {
    const uint32_t lr = (uint32_t)j * TALLY_THREADS + tid;
    const bool bit = row0 + lr < a.n && ((wds[lr >> 6] >> (lr & 63)) & 1ull);
    valid += bit;
    first[j] = false;
    if (a.prop_on && bit && ((a.prop_vidx >= 0 && vi[j] == a.prop_vidx) || vi[j] == VIDX_PROPOSER_OUTSIDER)) {
      // HasPrepareQuorum walks PREPARE messages (core/ibft.go:864-871 hands it the PREPAREs of the view): in a batch of raw
      // messages of both types (the wire form marks its PREPAREs: no_seal) a COMMIT of the proposer is no PREPARE of his
      const bool is_prepare = !(a.set_on && a.set.no_seal) || a.set.no_seal[row0 + lr] != 0;
      if (is_prepare) by_proposer++;
    }
    if (bit && vi[j] >= 0)  // unknown senders contribute 0 (validator_manager.go:88-92); HBM: device scope (huge sets only)
      first[j] = a.lds_bitmap ? claim_first(lseen, (uint32_t)vi[j]) : claim_first(a.seen, (uint32_t)vi[j]);
  }
  // the proposer's seat in the sender set: one more "row" of thread 0 of the first workgroup
  bool pfirst = false;
  if (a.prop_on && a.prop_seat && a.prop_vidx >= 0 && blockIdx.x == 0 && tid == 0)
    pfirst = a.lds_bitmap ? claim_first(lseen, (uint32_t)a.prop_vidx) : claim_first(a.seen, (uint32_t)a.prop_vidx);
  if (MULTI && a.lds_bitmap) {  // several workgroups: the set is shared through the bitmap in HBM
    merge_first_bits<TALLY_THREADS>(lseen, a.seen, seen_words);
#pragma unroll
    for (int j = 0; j < RPT; j++)
      first[j] = first[j] && still_first(lseen, first[j] ? (uint32_t)vi[j] : 0u);  // (first[j] implies vi[j] ≥ 0)
    if (pfirst) pfirst = still_first(lseen, (uint32_t)a.prop_vidx);
  }
  uint64_t p[NP];
#pragma unroll
  for (int k = 0; k < NP; k++) p[k] = 0;
  if (pfirst) {
    distinct++;
#pragma unroll
    for (int k = 0; k < NP; k++) p[k] += a.vpower32[(size_t)a.prop_vidx * NP + k];
  }
#pragma unroll
  for (int j = 0; j < RPT; j++) {
    if (!first[j]) continue;
    distinct++;
#pragma unroll
    for (int k = 0; k < NP; k++) p[k] += pw[j][k];
  }
  block_sum(part, p);
  wave_part(part[NP], valid | (distinct << 32));
  wave_part(part[NP + 1], (uint64_t)by_proposer, a.prop_on);
  __syncthreads();
  uint64_t piece[TALLY_MAX_PIECES];
  uint64_t v = 0, d = 0, proposer_rows = 0;
  if (MULTI) {
    if (tid <= NP + 1) {  // thread k adds piece k (thread NP: the two counters, NP + 1: the proposer's rows) of this workgroup to the launch-wide sums
      const uint64_t sum = parts_total(part[tid]);
      if (tid < NP) {
        if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(a.acc + tid), (unsigned long long)sum);
      } else if (tid == NP + 1) {
        if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(a.acc + TALLY_MAX_PIECES + 3), (unsigned long long)sum);
      } else {
        if (sum & 0xFFFFFFFFull) atomicAdd(reinterpret_cast<unsigned long long *>(a.acc + TALLY_MAX_PIECES), (unsigned long long)(sum & 0xFFFFFFFFull));
        if (sum >> 32) atomicAdd(reinterpret_cast<unsigned long long *>(a.acc + TALLY_MAX_PIECES + 1), (unsigned long long)(sum >> 32));
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // draw_last_ticket's "waitcnt" discipline: the adds return nothing
    }
    __syncthreads();  // the bitmap atomics returned values (awaited by their users), the adds were awaited above
    if (!draw_last_ticket(a.acc + TALLY_MAX_PIECES + 2, last_flag)) return;
    // ---- the last workgroup: every other one has added its pieces and set its bits ----
    for (uint32_t i = tid; i < (a.n_validators + 31) / 32; i += TALLY_THREADS) {
      if (a.seen_out) a.seen_out[i] = __hip_atomic_load(a.seen + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.seen + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid != 0) return;
#pragma unroll
    for (int k = 0; k < TALLY_MAX_PIECES; k++)
      piece[k] = k < NP ? (uint64_t)atomicAdd(reinterpret_cast<unsigned long long *>(a.acc + k), 0ull) : 0ull;
    v = (uint64_t)atomicAdd(reinterpret_cast<unsigned long long *>(a.acc + TALLY_MAX_PIECES), 0ull);
    d = (uint64_t)atomicAdd(reinterpret_cast<unsigned long long *>(a.acc + TALLY_MAX_PIECES + 1), 0ull);
    proposer_rows = (uint64_t)atomicAdd(reinterpret_cast<unsigned long long *>(a.acc + TALLY_MAX_PIECES + 3), 0ull);
#pragma unroll
    for (int k = 0; k < TALLY_ACC_WORDS; k++)
      __hip_atomic_store(a.acc + k, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    if (a.seen_out)  // (the barrier above is behind every row's atomicOr)
      for (uint32_t i = tid; i < seen_words; i += TALLY_THREADS) a.seen_out[i] = lseen[i];
    if (tid != 0) return;
    block_totals<NP>(part, piece);
    const uint64_t c = parts_total(part[NP]);
    proposer_rows = parts_total(part[NP + 1]);
    v = c & 0xFFFFFFFFull;
    d = c >> 32;
  }
  uint64_t w[TALLY_SUM_WORDS], rec[4];
  tally_record(piece, NP, (v & 0xFFFFFFFFull) | (d << 32), a.quorum, proposer_rows, rec, w);
  const uint64_t c = rec[2], hq = rec[3];
#pragma unroll
  for (int i = 0; i < 4; i++) a.out[i] = rec[i];
#pragma unroll
  for (int i = 0; i < TALLY_SUM_WORDS; i++) a.out[TALLY_OUT_WIDE + i] = w[i];
#pragma unroll
  for (int k = 0; k < TALLY_MAX_PIECES; k++) a.out[TALLY_OUT_PIECES + k] = piece[k];
  if (a.learned_src) a.out[4] = *a.learned_src;
  a.out[TALLY_OUT_PROPOSER_ROWS] = proposer_rows;
  if (a.host_tally) {
    a.host_tally[TALLY_OUT_PROPOSER_ROWS] = proposer_rows;
    a.host_tally[0] = w[0];
    a.host_tally[1] = w[1];
    a.host_tally[2] = c;
    a.host_tally[3] = hq;
    a.host_tally[4] = a.out[4];  // keys learned | a learned slot (the recover kernels' counter in the device's key cache)
#pragma unroll
    for (int i = 0; i < TALLY_SUM_WORDS; i++) a.host_tally[TALLY_OUT_WIDE + i] = w[i];
  }
}

// ---- chain sync: the committed seals of many finalized blocks in one call (ibft_verify_block_seals …) --------------
// Only the blocks' hashes (n_blocks × 32 B) — or their proposals — and their row offsets cross PCIe; one thread per row finds
// its block by binary search over the offsets and writes the hash the row's seal signs into the row's slot of the hash
// column the verdict kernels read.  The per-row body is recover_dev.h's block_head_row (block_of_row: empty blocks repeat an
// offset, the LAST b with off[b] ≤ row is the one), which tests/test_dev_block_head_host.py drives on the CPU.
// The streamed submits: convert = 1 under a non-identity seal-digest convention — convention and spreading in ONE launch, the
// blocks' digests (computed, or the uploaded hashes) left as they are: they leave for the host on another stream while the
// main stream goes on, so nothing may write them, and one launch less is one dependency gap less per batch; every row hashes
// its block's digest itself (one permutation: nothing next to an ECDSA recover).  The synchronous calls: convert = 0 — they
// converted the digests in place once per BLOCK (seal_digest_kernel) in front, and the row body is a plain copy.
struct block_head_args {
  const uint64_t *digest_words;  // n_blocks × 4: the blocks' digests (proposal_digest_kernel's, or uploaded hashes), read only
  const uint32_t *off;           // n_blocks + 1 row offsets
  uint8_t *hash32;               // n × 32: the hash column the verdict kernels read
  uint32_t n_blocks, n, convert;
  uint64_t suffix_words[9];
};
__global__ void __launch_bounds__(256) block_head_kernel(block_head_args a) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.n) return;
  const block_head_t h = block_head_row(a.digest_words, a.off, a.n_blocks, row, a.convert, a.suffix_words);
  uint4 *d = reinterpret_cast<uint4 *>(a.hash32 + 32ull * row);
  d[0] = make_uint4((uint32_t)h.w[0], (uint32_t)(h.w[0] >> 32), (uint32_t)h.w[1], (uint32_t)(h.w[1] >> 32));
  d[1] = make_uint4((uint32_t)h.w[2], (uint32_t)(h.w[2] >> 32), (uint32_t)h.w[3], (uint32_t)(h.w[3] >> 32));
}

// Segmented HasQuorum: one verdict launch judged the rows of every block, this kernel answers HasQuorum per block against
// the one quorum of the context's validator set (core/validator_manager.go:77-96, 128-136, 147-155) — bit for bit what
// tally_kernel computes for the same rows passed as a batch of their own.  A workgroup takes one block at a time (grid-stride:
// the HBM-bitmap form runs ONE workgroup over all blocks, the bitmap being a single zeroed `seen`): distinct-sender bitmap
// cleared, the block's rows walked, 2·PW 32-bit power pieces reduced through wave_sum_u64 and LDS, thread 0 recombines them
// and writes the block's record {power_lo, power_hi, valid | distinct << 32, has_quorum}.
// The work mask is read by several workgroups (block boundaries do not fall on verdict words), so it is handed over by
// the LAST workgroup to finish (draw_last_ticket on acc[TALLY_MAX_PIECES + 2], left zero again): no word is cleared under a reader.
// THREADS: 256 for blocks of chain-sized seal sets, 1024 when a block has more rows than that (the host picks); a thread
// takes BTALLY_RPT rows per step and issues their loads together (verdict word, validator index, then the powers of the rows
// whose bit is set) — one dependent round trip per step instead of one per row.  Row r of a block belongs to thread
// (r − r0) mod THREADS (STEP is a multiple of THREADS), in the main loop and in the HBM-bitmap clean-up alike.
//
// Under a family of sets: (SETS, ibft_verify_block_seals_sets) the verdict kernels judged every row against the union of the
// family's addresses and left the signer's UNION index; block b is judged under set block_set[b].  Per row one dependent load
// more — setidx[set][union index] → the index in the block's set (recover_dev.h: valsets_row), issued for the BTALLY_RPT rows
// of a step together, in front of the powers.  A row whose signer is in the union but not in the block's set loses its verdict
// bit: an atomic AND on its word of the work mask — other workgroups read other bits of that word (with relaxed atomic loads)
// and never see theirs change — before the row is counted; every thread fences its ANDs before the ticket, and the last
// workgroup then moves the words, which it reads past its compute unit's cache, so no clear of another workgroup is missed.
// The index column is rewritten from union to set index (−1: no member of the block's set), which is what the emitting form
// delivers as out_vidx and ALL the HBM-bitmap clean-up reads: there every thread re-reads the set indices it stored itself
// (the row mapping above), no verdict bit.  Bitmap, powers and quorum are the SET's: powers of set s start at entry
// set_meta[s].x of vpower32, its distinct addresses number set_meta[s].y, its quorum is quorum[s].
constexpr int BTALLY_RPT = 4;
constexpr uint32_t BTALLY_MAX_GRID = 2048;  // workgroups of one launch (each takes blocks b, b + grid, …): few ticket arrivals
struct block_tally_args {
  uint64_t *work_mask;        // verdict words of the launch; consumed (moved to mask / host_mask, zeroed) here
  uint64_t *mask, *host_mask; // host_mask: mapped pinned host memory or null
  int32_t *vidx;              // n: validator index of the row's signer (meaningful where the verdict bit is set), read only;
                              // sets: in — union index, out — index in the block's set or −1
  const uint32_t *vpower32;   // n_validators (sets: Σ set sizes) × 2·PW pieces
  const uint32_t *off;        // n_blocks + 1 row offsets
  uint32_t n, n_blocks, n_validators;  // (sets: n_validators is the union's size)
  uint32_t lds_bitmap;        // ⌈n_validators (sets: largest set)/32⌉ words of dynamic LDS; 0: `seen` in HBM, and the grid is one workgroup
  uint32_t *seen;             // as many words, zero between launches (HBM form only)
  uint64_t *acc;              // TALLY_ACC_WORDS, zero between launches (the ticket)
  const uint64_t *quorum;     // TALLY_SUM_WORDS (sets: n_sets of them)
  uint64_t *out;              // n_blocks × 4 u64 (device memory or mapped pinned host memory)
};
struct block_tally_sets_args : block_tally_args {
  const uint32_t *block_set;  // n_blocks, every entry < n_sets (checked on the host)
  const int32_t *setidx;      // n_sets × n_validators
  const uint2 *set_meta;      // n_sets × {first power entry, distinct addresses}
};
template <int PW, int THREADS, bool SETS>
__global__ void __launch_bounds__(THREADS)
    block_tally_kernel(std::conditional_t<SETS, block_tally_sets_args, block_tally_args> a) {
  constexpr int NP = 2 * PW;
  constexpr int WAVES = THREADS / 64;
  constexpr uint32_t STEP = (uint32_t)THREADS * BTALLY_RPT;
  extern __shared__ uint32_t lseen[];
  __shared__ uint64_t part[NP + 1][WAVES];
  __shared__ uint32_t last_flag;
  const uint32_t tid = threadIdx.x;
  uint32_t *bm = a.lds_bitmap ? lseen : a.seen;
  // does the row add to its block's power?  (the index is only meaningful where the verdict bit is set; valsets_row says −1 elsewhere)
  auto counts = [](const valsets_row_t &s) { return (SETS || s.bit) && s.si >= 0; };
  for (uint32_t b = blockIdx.x; b < a.n_blocks; b += gridDim.x) {
    const uint32_t r0 = a.off[b], r1 = a.off[b + 1];
    uint32_t set = 0, first = 0, members = a.n_validators;  // the block's set: its first power entry, its distinct addresses
    if constexpr (SETS) {
      set = a.block_set[b];
      const uint2 meta = a.set_meta[set];
      first = meta.x;
      members = meta.y;
    }
    if (a.lds_bitmap)
      for (uint32_t i = tid; i < (members + 31) / 32; i += THREADS) lseen[i] = 0;
    __syncthreads();
    uint64_t p[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) p[k] = 0;
    uint64_t valid = 0, distinct = 0;
    for (uint32_t base = r0; base < r1; base += STEP) {
      bool bit[BTALLY_RPT];
      int vi[BTALLY_RPT];
      valsets_row_t sr[BTALLY_RPT];  // what the block's tally makes of the row: its verdict bit, the signer's index in the set
      uint32_t pw[BTALLY_RPT][NP];
#pragma unroll
      for (int j = 0; j < BTALLY_RPT; j++) {
        const uint32_t r = base + (uint32_t)j * THREADS + tid;
        bit[j] = r < r1 && ((verdict_word<SETS>(a.work_mask, r >> 6) >> (r & 63)) & 1ull);
        vi[j] = r < r1 ? a.vidx[r] : -1;
        if constexpr (!SETS) sr[j] = valsets_row_t{vi[j], bit[j], false};  // the one set: the row as the verdict kernel left it
      }
      if constexpr (SETS) {  // union index → index in the block's set: the dependent loads of the step's rows, issued together
#pragma unroll
        for (int j = 0; j < BTALLY_RPT; j++) sr[j] = valsets_row(bit[j], vi[j], a.setidx, a.n_validators, set);
      }
#pragma unroll
      for (int j = 0; j < BTALLY_RPT; j++) {
#pragma unroll
        for (int k = 0; k < NP; k++) pw[j][k] = counts(sr[j]) ? a.vpower32[((size_t)first + (uint32_t)sr[j].si) * NP + k] : 0u;
      }
#pragma unroll
      for (int j = 0; j < BTALLY_RPT; j++) {
        if constexpr (SETS) {
          const uint32_t r = base + (uint32_t)j * THREADS + tid;
          if (r < r1) a.vidx[r] = sr[j].si;
          if (sr[j].clear) atomicAnd(reinterpret_cast<unsigned long long *>(a.work_mask + (r >> 6)), ~(1ull << (r & 63)));
        }
        valid += sr[j].bit;
        if (!counts(sr[j])) continue;  // unknown signers contribute 0 (validator_manager.go:88-92)
        if (!claim_first(bm, (uint32_t)sr[j].si)) continue;  // a signer's power counts once per block (:147-155)
        distinct++;
#pragma unroll
        for (int k = 0; k < NP; k++) p[k] += pw[j][k];
      }
    }
    block_sum(part, p);
    wave_part(part[NP], valid | (distinct << 32));
    __syncthreads();
    if (!a.lds_bitmap)  // the HBM bitmap is left zero for the next block: clear exactly the words this block set
      for (uint32_t r = r0 + tid; r < r1; r += THREADS) {
        bool counted = true;  // (sets: vidx holds set indices, −1 wherever the row set nothing)
        if constexpr (!SETS) counted = (a.work_mask[r >> 6] >> (r & 63)) & 1ull;
        if (counted) {
          const int v = a.vidx[r];
          if (v >= 0) bm[v >> 5] = 0u;
        }
      }
    if (tid == 0) {
      uint64_t piece[TALLY_MAX_PIECES], c = 0;  // (not block_totals: see there)
#pragma unroll
      for (int k = 0; k < TALLY_MAX_PIECES; k++) {
        piece[k] = 0;
        if (k < NP)
          for (int w = 0; w < WAVES; w++) piece[k] += part[k][w];
      }
      for (int w = 0; w < WAVES; w++) c += part[NP][w];
      tally_record(piece, NP, c, a.quorum + (size_t)set * TALLY_SUM_WORDS, 0ull, a.out + 4ull * b);
    }
    __syncthreads();  // part[] and the bitmap are reused by the next block
  }
  // ---- every workgroup has read its rows' verdict words (and cleared what it had to): the last one moves and zeroes them ----
  if constexpr (SETS) {  // draw_last_ticket's "fence" discipline: every thread's atomic ANDs are performed before the ticket is drawn
    __threadfence();
    __syncthreads();
  }
  if (tid == 0) __threadfence();
  if (!draw_last_ticket(a.acc + TALLY_MAX_PIECES + 2, last_flag)) return;
  hand_over_words<SETS, THREADS>(a.work_mask, a.mask, a.host_mask, (a.n + 63) / 64);
  reset_ticket(a.acc + TALLY_MAX_PIECES + 2);
}

// ---- the live route under a family of sets (ibft_verify_senders_wire_sets; the row bodies: wire_sets_dev.h) -----------------
// Behind wire_parse_kernel and the recode walk, in front of the verdict launch: a thread per message looks its decoded height
// up in the height map, writes the row's set and pre-flags the rows that have none — the verdict kernels skip them, so a peer
// that sprays heights of no range buys no ECDSA work.
__global__ void __launch_bounds__(256) wire_row_set_kernel(const wire::row_info *__restrict__ rows, uint32_t n, height_map m,
                                                           int32_t *__restrict__ row_set, uint8_t *__restrict__ pre_flags) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const int32_t s = wire_row_set_row(rows[row], m);
  row_set[row] = s;
  if (s < 0) pre_flags[row] = 1;
}

// HasQuorum per SET over rows whose sets are INTERLEAVED (block_tally_kernel wants a block's rows contiguous): the verdict
// kernels judged every row against the union of the family's addresses and left the signer's union index; this kernel is
// row-parallel — a workgroup takes WSETS_ROWS consecutive rows whatever their sets —, so its work does not depend on how many of the
// family's sets the batch touches (the bound: `work` below).
//   per row      wire_sets_row: the verdict under the row's set (an atomic AND where a member of the union outside the set
//                loses its bit), the index column rewritten from union to set index, the member's entry in the family's
//                packed columns (set_meta[s].x + index).
//   distinct     one bit per (set, member) ENTRY — the bitmap spans the whole family, ⌈Σ set sizes / 32⌉ words: claim_first
//                in LDS, merge_first_bits, still_first.  A family whose bitmap does not fit TALLY_BITMAP_LDS_MAX (more than
//                393 216 entries) sends every counting row's bit to HBM directly (lds_bitmap = 0).
//   sums         a wavefront reduces the rows of one set at a time — every thread first adds up those of its four rows that
//                belong to the turn's set (the set of the first lane that still waits; a receive queue mixes two or three
//                heights, so two or three turns per 256 rows; wire_views_tally_kernel has the same turn with one row per
//                thread and a bounded number of turns — through one helper that kernel takes 12–16 registers more, so the
//                turn is written out in both) — and the leader adds valid | distinct << 32 and, only where a
//                row was first, the 2·PW pieces to the set's accumulators in HBM: NP + 1 words per set.
//   work         O(n + n_sets) for the rows and the records; on top of that every workgroup of the LDS form zeroes and scans
//                the whole bitmap once: ⌈n / 1 024⌉ · ⌈entries / 32⌉ LDS words in all — 7 words per workgroup for two sets of
//                100, 3 200 for 1 024 sets of 100, 12 288 at the LDS cap — and the last workgroup its entries / 32 HBM words.
//   the end      the workgroup that draws the last ticket (draw_last_ticket, "fence" discipline; the ticket is
//                acc[TALLY_MAX_PIECES + 2]) hands the work mask over, turns every set's accumulators into the record
//                (tally_record against the set's quorum) and zeroes them, and zeroes the
//                bitmap — by its words in the LDS form, by the rows' entries (re-read from the rewritten index column) in
//                the HBM form — and the ticket: all scratch is zero again when the kernel ends.
constexpr int WSETS_THREADS = 256, WSETS_RPT = 4;
constexpr uint32_t WSETS_ROWS = WSETS_THREADS * WSETS_RPT;
struct wire_sets_tally_args {
  uint64_t *work_mask;         // verdict words of the launch; consumed (moved to mask / host_mask, zeroed) here
  uint64_t *mask, *host_mask;  // host_mask: mapped pinned host memory or null
  int32_t *vidx;               // n: in — union index (meaningful where the verdict bit is set), out — index in the row's set or −1
  const int32_t *row_set;      // n: the row's set (wire_row_set_kernel), −1: none
  const int32_t *setidx;       // n_sets × n_union
  const uint2 *set_meta;       // n_sets × {first entry, distinct addresses}
  const uint32_t *vpower32;    // Σ set sizes × 2·PW pieces
  const uint64_t *quorum;      // n_sets × TALLY_SUM_WORDS
  uint32_t n, n_sets, n_union;
  uint32_t seen_words;         // ⌈Σ set sizes / 32⌉
  uint32_t lds_bitmap;         // seen_words words of dynamic LDS; 0: every row's bit goes to `seen` directly
  uint32_t *seen;              // seen_words, zero between launches
  uint64_t *set_acc;           // n_sets × (2·PW + 1): pieces, valid | distinct << 32; zero between launches
  uint64_t *acc;               // TALLY_ACC_WORDS, zero between launches (the ticket)
  uint64_t *out;               // n_sets × 4 u64 (device memory or mapped pinned host memory)
};
template <int PW>
__global__ void __launch_bounds__(WSETS_THREADS) wire_sets_tally_kernel(wire_sets_tally_args a) {
  constexpr int NP = 2 * PW;
  extern __shared__ uint32_t wseen[];
  __shared__ uint32_t last_flag;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t row0 = blockIdx.x * WSETS_ROWS;
  if (a.lds_bitmap)
    for (uint32_t i = tid; i < a.seen_words; i += WSETS_THREADS) wseen[i] = 0;
  bool bit[WSETS_RPT];
  int vi[WSETS_RPT];
  int32_t set[WSETS_RPT];
  wire_sets_row_t sr[WSETS_RPT];
  uint32_t pw[WSETS_RPT][NP];
#pragma unroll
  for (int j = 0; j < WSETS_RPT; j++) {
    const uint32_t r = row0 + (uint32_t)j * WSETS_THREADS + tid;
    bit[j] = r < a.n && ((verdict_word<true>(a.work_mask, r >> 6) >> (r & 63)) & 1ull);
    vi[j] = r < a.n ? a.vidx[r] : -1;
    set[j] = r < a.n ? a.row_set[r] : -1;
  }
#pragma unroll
  for (int j = 0; j < WSETS_RPT; j++) sr[j] = wire_sets_row(bit[j], vi[j], set[j], a.setidx, a.n_union, a.set_meta);
#pragma unroll
  for (int j = 0; j < WSETS_RPT; j++) {
#pragma unroll
    for (int k = 0; k < NP; k++) pw[j][k] = sr[j].counts ? a.vpower32[(size_t)sr[j].entry * NP + k] : 0u;
  }
#pragma unroll
  for (int j = 0; j < WSETS_RPT; j++) {
    const uint32_t r = row0 + (uint32_t)j * WSETS_THREADS + tid;
    if (r < a.n) a.vidx[r] = sr[j].si;
    if (sr[j].clear) atomicAnd(reinterpret_cast<unsigned long long *>(a.work_mask + (r >> 6)), ~(1ull << (r & 63)));
  }
  __syncthreads();  // the LDS bitmap is zero
  uint32_t *bm = a.lds_bitmap ? wseen : a.seen;
  bool first[WSETS_RPT];
#pragma unroll
  for (int j = 0; j < WSETS_RPT; j++) {
    first[j] = sr[j].counts && claim_first(bm, sr[j].entry);  // a signer's power counts once per set (validator_manager.go:147-155)
  }
  if (a.lds_bitmap) {  // (launch-uniform)
    merge_first_bits<WSETS_THREADS>(wseen, a.seen, a.seen_words);
#pragma unroll
    for (int j = 0; j < WSETS_RPT; j++) first[j] = first[j] && still_first(wseen, first[j] ? sr[j].entry : 0u);
  }
  // a thread's four rows and a wavefront's 64 threads, one set per turn: the set of the first lane that still holds a valid row
  uint32_t pend = 0;  // the thread's valid rows not yet added
#pragma unroll
  for (int j = 0; j < WSETS_RPT; j++) pend |= sr[j].bit ? 1u << j : 0u;
  for (uint64_t todo = __ballot(pend ? 1 : 0); todo; todo = __ballot(pend ? 1 : 0)) {  // (wave-uniform: every lane takes every turn)
    const int leader = __ffsll((long long)todo) - 1;
    int32_t next = -1;  // the set of this thread's first pending row
#pragma unroll
    for (int j = WSETS_RPT - 1; j >= 0; j--)
      if ((pend >> j) & 1u) next = set[j];
    const int32_t s = __shfl(next, leader, 64);
    uint64_t cnt = 0, p[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) p[k] = 0;
#pragma unroll
    for (int j = 0; j < WSETS_RPT; j++) {
      if (!((pend >> j) & 1u) || set[j] != s) continue;
      pend &= ~(1u << j);
      cnt += 1ull | ((uint64_t)(first[j] ? 1u : 0u) << 32);
      if (first[j]) {
#pragma unroll
        for (int k = 0; k < NP; k++) p[k] += pw[j][k];
      }
    }
    uint64_t *acc = a.set_acc + (size_t)s * (NP + 1);
    cnt = wave_sum_u64(cnt);
    if (cnt >> 32) {  // (wave-uniform) somebody was first: the pieces
#pragma unroll
      for (int k = 0; k < NP; k++) {
        const uint64_t sum = wave_sum_u64(p[k]);
        if ((int)lane == leader && sum) atomicAdd(reinterpret_cast<unsigned long long *>(acc + k), (unsigned long long)sum);
      }
    }
    if ((int)lane == leader) atomicAdd(reinterpret_cast<unsigned long long *>(acc + NP), (unsigned long long)cnt);
  }
  // ---- every workgroup has judged its rows: the last one delivers ----
  __threadfence();  // draw_last_ticket's "fence" discipline: every thread's atomics and index stores
  __syncthreads();
  if (tid == 0) __threadfence();
  if (!draw_last_ticket(a.acc + TALLY_MAX_PIECES + 2, last_flag)) return;
  hand_over_words<true, WSETS_THREADS>(a.work_mask, a.mask, a.host_mask, (a.n + 63) / 64);
  for (uint32_t s = tid; s < a.n_sets; s += WSETS_THREADS) {
    uint64_t *acc = a.set_acc + (size_t)s * (NP + 1);
    uint64_t piece[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) piece[k] = __hip_atomic_load(acc + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t cnt = __hip_atomic_load(acc + NP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cnt) {  // (a set without valid rows added nothing)
#pragma unroll
      for (int k = 0; k <= NP; k++) __hip_atomic_store(acc + k, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    uint64_t rec[4];
    tally_record(piece, NP, cnt, a.quorum + (size_t)s * TALLY_SUM_WORDS, 0ull, rec);
    uint64_t *o = a.out + 4ull * s;
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = rec[i];
  }
  if (a.lds_bitmap) {
    for (uint32_t i = tid; i < a.seen_words; i += WSETS_THREADS)
      if (__hip_atomic_load(a.seen + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_store(a.seen + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {  // by the rows that set a bit: the index column holds set indices now, −1 wherever the row set nothing
    for (uint32_t r = tid; r < a.n; r += WSETS_THREADS) {
      const int32_t s = a.row_set[r];
      const int v = __hip_atomic_load(a.vidx + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (s >= 0 && v >= 0) __hip_atomic_store(a.seen + ((a.set_meta[s].x + (uint32_t)v) >> 5), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  reset_ticket(a.acc + TALLY_MAX_PIECES + 2);
}

// ---- the live route's quorum records (ibft_verify_senders_wire_views; the row bodies: wire_views_dev.h) ---------------------
// Four launches behind wire_sets_tally_kernel on the same stream; each phase that needs every row of the one before it is a
// launch of its own, so nothing here waits for another workgroup.
//   insert   a thread per row: a valid row (final mask bit) goes into the key table (lowest row of its key) and the last table
//            (highest row of its view and sender); its two slots are kept.  A row that exhausts a table raises *err.
//   rank     ONE workgroup: representatives (key_table[slot] == row) ranked in ascending row order — cert_scan_kernel's
//            shape (a run of rows per thread, a scan of the 1 024 sums through LDS); rank_of[rep], first_row[rank] for the
//            views that fit, the number of keys.
//   tally    a thread per row: out_view, the stored bit (one ballot per wavefront is one word of out_stored), and the view's
//            accumulators — rows | stored << 32 and, for stored rows, the member's 2·PW pieces.  A wavefront reduces one view
//            per turn (the view of the first lane that still waits), at most WVIEWS_TURNS turns; whoever still waits then — a
//            hostile batch puts 64 views into a wavefront — adds for itself: O(n) whatever the number of views.
//   records  a thread per view below min(n_views, views_cap): wviews::view_record, then the view's accumulators are zeroed —
//            all scratch but the tables (set to EMPTY, with the call's two words behind them, by one fill in front of every
//            insert) is zero again when the call returns.
// SEALS (ibft_verify_messages_wire_views, behind wire_seals_combine_kernel): tally reads the row's seal bit, a stored row adds
// its pieces only where wseals::counts says so — in a COMMIT view a sealed row — and the rows that did are one more count per
// view, so a view's accumulators are 2·PW + 2 words; records writes wviews::view_record's seal form and zeroes them all.
constexpr int WVIEWS_THREADS = 256, WVIEWS_TURNS = 4;
struct wire_views_args {
  const wire::row_info *rows;
  const int32_t *vidx, *row_set;  // index in the row's set / the row's set, as wire_sets_tally_kernel left them
  const uint64_t *mask;           // the final verdict words
  const uint64_t *seal_mask;      // SEALS: the rows' seal bits
  uint32_t n, views_cap, slots, salt;
  uint32_t *key_table, *last_table;  // slots words each
  uint32_t *slot_key, *slot_last;    // n
  uint32_t *rank_of;                 // n: rank of a representative
  uint32_t *first_row;               // min(n, views_cap): the representative of view v
  uint32_t *words;                   // behind the tables, all-ones like them at the start: [0] ← n_views, [1] ← 0 when a table was exhausted
  int32_t *out_view;                 // n
  uint64_t *out_stored;              // ⌈n / 64⌉
  uint64_t *view_acc;                // min(n, views_cap) × (2·PW + 1; SEALS: + 2), zero between calls
  wviews::view_t *out_views;         // min(n, views_cap)
  wviews::family fam;
  certd::proposer_table table;
};
__global__ void __launch_bounds__(WVIEWS_THREADS) wire_views_insert_kernel(wire_views_args a) {
  const uint32_t row = blockIdx.x * WVIEWS_THREADS + threadIdx.x;
  if (row >= a.n) return;
  const bool valid = (a.mask[row >> 6] >> (row & 63)) & 1ull;
  const wviews::row_slots s = wviews::insert_row(wviews::columns{a.rows, a.vidx}, row, valid, a.key_table, a.last_table, a.slots, a.salt);
  a.slot_key[row] = s.key;
  a.slot_last[row] = s.last;
  if (s.key == wviews::UNPLACED || s.last == wviews::UNPLACED) atomicAnd(a.words + 1, 0u);
}
__global__ void __launch_bounds__(1024) wire_views_rank_kernel(wire_views_args a) {
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x, per = (a.n + 1023u) / 1024u;
  const uint32_t b = t * per < a.n ? t * per : a.n, e = b + per < a.n ? b + per : a.n;
  uint32_t sum = 0;
  for (uint32_t i = b; i < e; i++) sum += wviews::is_rep(a.key_table, a.slot_key[i], i) ? 1u : 0u;
  uint32_t run = block_scan_1024(part, sum) - sum;
  for (uint32_t i = b; i < e; i++) {
    if (!wviews::is_rep(a.key_table, a.slot_key[i], i)) continue;
    a.rank_of[i] = run;
    if (run < a.views_cap) a.first_row[run] = i;
    run++;
  }
  if (t == 1023u) a.words[0] = part[1023];
}
template <int PW, bool SEALS = false>
__global__ void __launch_bounds__(WVIEWS_THREADS) wire_views_tally_kernel(wire_views_args a) {
  constexpr int NP = 2 * PW, STRIDE = NP + 1 + (SEALS ? 1 : 0);
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t row = blockIdx.x * WVIEWS_THREADS + tid;
  const uint32_t sk = row < a.n ? a.slot_key[row] : wviews::SKIP;
  const bool valid = sk < wviews::SKIP;
  int32_t v = wviews::VIEW_NONE;
  bool stored = false;
  if (valid) {
    v = wviews::view_of_rank(a.rank_of[a.key_table[sk]], a.views_cap);
    stored = wviews::is_stored(a.last_table, a.slot_last[row], row);  // a row beyond the cap still supersedes
  }
  if (row < a.n) a.out_view[row] = v;
  const uint64_t sw = __ballot(stored ? 1 : 0);
  if (lane == 0 && (row & ~63u) < a.n) a.out_stored[row >> 6] = sw;
  bool pend = v >= 0;
  uint32_t pw[NP];
  bool counted = stored;  // the row adds its sender's power
  if constexpr (SEALS) {
    const bool sealed = valid && ((a.seal_mask[row >> 6] >> (row & 63)) & 1ull);
    counted = valid && wseals::counts(a.rows[row].type, stored, sealed);
  }
  {
    const bool adds = pend && counted;
    const uint32_t entry = adds ? a.fam.set_meta[a.row_set[row]].x + (uint32_t)a.vidx[row] : 0u;
#pragma unroll
    for (int k = 0; k < NP; k++) pw[k] = adds ? a.fam.vpower32[(size_t)entry * NP + k] : 0u;
  }
  for (int turn = 0; turn < WVIEWS_TURNS; turn++) {  // (wave-uniform: every lane takes every turn)
    const uint64_t todo = __ballot(pend ? 1 : 0);
    if (!todo) break;
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t lv = __shfl(v, leader, 64);
    const bool mine = pend && v == lv;
    uint64_t *acc = a.view_acc + (size_t)lv * STRIDE;
    const uint64_t cnt = wave_sum_u64(mine ? (1ull | ((uint64_t)(stored ? 1u : 0u) << 32)) : 0ull);
    uint64_t adders = cnt >> 32;
    if constexpr (SEALS) {
      if (adders) adders = wave_sum_u64(mine && counted ? 1ull : 0ull);
      if ((int)lane == leader && adders) atomicAdd(reinterpret_cast<unsigned long long *>(acc + NP + 1), (unsigned long long)adders);
    }
    if (adders) {  // (wave-uniform) a stored row that counts among them: the pieces
#pragma unroll
      for (int k = 0; k < NP; k++) {
        const uint64_t sum = wave_sum_u64(mine ? (uint64_t)pw[k] : 0ull);
        if ((int)lane == leader && sum) atomicAdd(reinterpret_cast<unsigned long long *>(acc + k), (unsigned long long)sum);
      }
    }
    if ((int)lane == leader) atomicAdd(reinterpret_cast<unsigned long long *>(acc + NP), (unsigned long long)cnt);
    if (mine) pend = false;
  }
  if (pend) {  // more views in this wavefront than turns: the lane adds for itself
    uint64_t *acc = a.view_acc + (size_t)v * STRIDE;
    if (counted) {
#pragma unroll
      for (int k = 0; k < NP; k++)
        if (pw[k]) atomicAdd(reinterpret_cast<unsigned long long *>(acc + k), (unsigned long long)pw[k]);
      if constexpr (SEALS) atomicAdd(reinterpret_cast<unsigned long long *>(acc + NP + 1), 1ull);
    }
    atomicAdd(reinterpret_cast<unsigned long long *>(acc + NP), 1ull | ((uint64_t)(stored ? 1u : 0u) << 32));
  }
}
template <bool SEALS = false>
__global__ void __launch_bounds__(WVIEWS_THREADS) wire_views_records_kernel(wire_views_args a) {
  const uint32_t v = blockIdx.x * WVIEWS_THREADS + threadIdx.x;
  const uint32_t n_views = a.words[0];
  if (v >= n_views || v >= a.views_cap) return;
  const int words = a.fam.n_pieces + 1 + (SEALS ? 1 : 0);
  uint64_t *acc = a.view_acc + (size_t)v * words;
  wviews::view_t rec;
  wviews::view_record(rec, a.first_row[v], acc, wviews::columns{a.rows, a.vidx}, a.row_set, a.out_view, (int32_t)v, a.fam, a.table, a.last_table,
                      a.slots, a.salt, SEALS);
  a.out_views[v] = rec;
  for (int k = 0; k < words; k++) acc[k] = 0;
}

// ---- the committed seals of the live route's COMMIT records (ibft_verify_messages_wire_views; the row bodies: wire_seals_dev.h)
// Three launches between wire_row_set_kernel and the verdict launch lay the seal rows DENSE behind the sender rows, one
// launch behind wire_sets_tally_kernel turns the seal half's verdict words into the rows' seal bits:
//   mark     a thread per row: wseals::row_flags — is it a COMMIT with a set, is it sealable (the membership lookup included).
//   scan     ONE workgroup (wire_views_rank_kernel's shape): the sealable rows ranked in ascending row order — seal_row[i] = k
//            or NONE, src[k] = i — and the call's two counts: words[0] = sealable rows, words[1] = COMMIT rows with a set;
//            words[2], combine's ticket, is set to zero.
//   stage    a thread per seal row k < n: a live one (k < words[0]) gets the carried hash, the seal and From of src[k] and
//            pre-flag 0; the others a zero signature and pre-flag 1 — the verdict launch covers half + n rows, whole
//            wavefronts of the tail exit at once and the host never waits for the count.
//   combine  a thread per row: wseals::seal_bit from the final sender bit and the verdict bit of the row's seal row; a
//            wavefront's ballot is one word of the seal mask — every word written once, by one wavefront.  The workgroup
//            that draws the last ticket zeroes the seal half's verdict words: the work mask is zero again.
constexpr int WSEALS_THREADS = 256;
struct wire_seals_args {
  const wire::row_info *rows;
  const int32_t *row_set;
  const uint8_t *seal65;  // n × 65: the seals the walks found
  uint32_t n, half;
  wviews::family fam;   // (the lookup fields)
  uint8_t *flags;       // n: wseals::ROW_*
  uint32_t *seal_row;   // n: k of seal row half + k, or NONE
  uint32_t *src;        // n: the row of seal row half + k
  uint32_t *words;      // [0] sealable rows, [1] COMMIT rows with a set, [2] the ticket
  uint8_t *hash32, *sig65, *signer20, *pre_flags;  // the verdict launch's columns (rows [half, half + n) are written)
  const uint64_t *mask;  // the final verdict words of the sender rows
  uint64_t *work_mask;   // the verdict launch's words; those of the seal half are consumed
  uint64_t *seal_mask;   // ⌈n / 64⌉
};
__global__ void __launch_bounds__(WSEALS_THREADS) wire_seals_mark_kernel(wire_seals_args a) {
  const uint32_t row = blockIdx.x * WSEALS_THREADS + threadIdx.x;
  if (row >= a.n) return;
  a.flags[row] = wseals::row_flags(a.rows[row], a.row_set[row], a.fam);
}
__global__ void __launch_bounds__(1024) wire_seals_scan_kernel(wire_seals_args a) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x, per = (a.n + 1023u) / 1024u;
  const uint32_t b = t * per < a.n ? t * per : a.n, e = b + per < a.n ? b + per : a.n;
  uint64_t sum = 0;  // sealable | COMMIT << 32
  for (uint32_t i = b; i < e; i++) {
    const uint8_t f = a.flags[i];
    sum += (uint64_t)((f & wseals::ROW_SEALABLE) ? 1u : 0u) | ((uint64_t)((f & wseals::ROW_COMMIT) ? 1u : 0u) << 32);
  }
  uint32_t run = (uint32_t)(block_scan_1024(part, sum) - sum);
  for (uint32_t i = b; i < e; i++) {
    const bool sealable = a.flags[i] & wseals::ROW_SEALABLE;
    a.seal_row[i] = sealable ? run : wseals::NONE;
    if (sealable) a.src[run++] = i;
  }
  if (t == 1023u) {
    a.words[0] = (uint32_t)part[1023];
    a.words[1] = (uint32_t)(part[1023] >> 32);
    a.words[2] = 0;
  }
}
__global__ void __launch_bounds__(WSEALS_THREADS) wire_seals_stage_kernel(wire_seals_args a) {
  const uint32_t k = blockIdx.x * WSEALS_THREADS + threadIdx.x;
  if (k >= a.n) return;
  const uint32_t dst = a.half + k;
  const bool live = k < a.words[0];
  a.pre_flags[dst] = live ? 0 : 1;
  if (!live) {
    for (int i = 0; i < 65; i++) a.sig65[65ull * dst + i] = 0;
    return;
  }
  const uint32_t r = a.src[k];
  const wire::row_info &ri = a.rows[r];
  for (int i = 0; i < 32; i++) a.hash32[32ull * dst + i] = ri.proposal_hash[i];
  for (int i = 0; i < 65; i++) a.sig65[65ull * dst + i] = a.seal65[65ull * r + i];
  for (int i = 0; i < 20; i++) a.signer20[20ull * dst + i] = ri.from[i];
}
__global__ void __launch_bounds__(WSEALS_THREADS) wire_seals_combine_kernel(wire_seals_args a) {
  __shared__ uint32_t last_flag;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t row = blockIdx.x * WSEALS_THREADS + tid;
  const uint32_t words = (a.n + 63u) / 64u;
  uint64_t *seal_words = a.work_mask + a.half / 64u;
  const bool valid = row < a.n && ((a.mask[row >> 6] >> (row & 63)) & 1ull);
  const bool bit = wseals::seal_bit(valid, row < a.n ? a.seal_row[row] : wseals::NONE, seal_words);
  const uint64_t w = __ballot(bit ? 1 : 0);
  if (lane == 0 && (row >> 6) < words) a.seal_mask[row >> 6] = w;
  // ---- every workgroup has read its seal verdicts: the last one zeroes them ----
  __threadfence();  // draw_last_ticket's "fence" discipline
  __syncthreads();
  if (!draw_last_ticket(a.words + 2, last_flag)) return;
  for (uint32_t i = tid; i < words; i += WSEALS_THREADS) seal_words[i] = 0;
  reset_ticket(a.words + 2);
}

// ---- certificates: one record per carrier (ibft_judge_certificates_wire; the rules: cert_verdict_dev.h) ---------------------
// Records exist for every level-0 row and for every level-1 row of role ROLE_RCC_MESSAGE (the ROUND_CHANGE messages inside a
// root PREPREPARE's RoundChangeCertificate), in ascending row order: record i < n_roots is row i; the records of root i's
// certificate are [rec_base[i], rec_base[i + 1]) — its children are a contiguous row range and share one role.
__device__ __forceinline__ uint32_t cert_rcc_children(const wire::node_info *__restrict__ nodes, uint32_t root, uint32_t rows_bound) {
  const uint32_t lo = nodes[root].first_child, n = nodes[root].n_children;
  if (n == 0 || (uint64_t)lo + n > rows_bound) return 0;
  return nodes[lo].role == wire::ROLE_RCC_MESSAGE ? n : 0;
}
// rec_base[0 .. n_roots]: n_roots + the exclusive prefix count of the roots' certificate children; the record total goes to
// total_dev[2] (and total_host[2]) next to the level totals of cert_scan_kernel.  One workgroup, as cert_scan_kernel: it runs once
// per call, after level 1 has been listed (cert_walk_kernel<true> over level 0 has written the children's roles).
__global__ void __launch_bounds__(1024) cert_record_scan_kernel(const wire::node_info *__restrict__ nodes, uint32_t n_roots, uint32_t rows_bound,
                                                                uint32_t *__restrict__ rec_base, uint32_t *__restrict__ total_dev,
                                                                uint32_t *__restrict__ total_host) {
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x, per = (n_roots + 1023u) / 1024u;
  const uint32_t b = t * per < n_roots ? t * per : n_roots, e = b + per < n_roots ? b + per : n_roots;
  uint32_t sum = 0;
  for (uint32_t i = b; i < e; i++) sum += cert_rcc_children(nodes, i, rows_bound);
  uint32_t run = n_roots + block_scan_1024(part, sum) - sum;
  for (uint32_t i = b; i < e; i++) {
    rec_base[i] = run;
    run += cert_rcc_children(nodes, i, rows_bound);
  }
  if (t == 1023u) {
    const uint32_t total = n_roots + part[1023];
    rec_base[n_roots] = total;
    total_dev[2] = total;
    if (total_host) total_host[2] = total;
  }
}

constexpr uint32_t CERT_JUDGE_MAX_GRID = 1u << 16;  // workgroups of one launch (each takes records r, r + grid, …)
struct cert_judge_args {
  const wire::node_info *nodes;
  const wire::row_info *rows;
  const uint8_t *cls;
  const uint64_t *sender_mask, *hash_mask, *self_mask;  // verdict words over the tree's rows
  const uint32_t *vtab;                                 // the validator table (valset_lookup)
  const uint32_t *vpower32;                             // n_validators × 2·PW pieces
  const uint64_t *quorum;                               // TALLY_SUM_WORDS
  const uint32_t *rec_base;                             // n_roots + 1 (cert_record_scan_kernel); null: no level-1 records
  uint32_t vslot_mask, n_validators;
  uint32_t n_roots, n_rows, n_records;
  uint32_t lds_bitmap;  // ⌈n_validators/32⌉ words of dynamic LDS; 0: `seen` in HBM, and the grid is one workgroup
  uint32_t *seen;       // as many words, zero between launches (HBM form only)
  certv::record *out;
};
__device__ __forceinline__ bool cert_mask_bit(const uint64_t *__restrict__ mask, uint32_t row) { return (mask[row >> 6] >> (row & 63u)) & 1ull; }
__device__ __forceinline__ int cert_row_validator(const cert_judge_args &a, const wire::row_info &w) {
  uint32_t addr[5];
#pragma unroll
  for (int i = 0; i < 5; i++)
    addr[i] = (uint32_t)w.from[4 * i] | ((uint32_t)w.from[4 * i + 1] << 8) | ((uint32_t)w.from[4 * i + 2] << 16) | ((uint32_t)w.from[4 * i + 3] << 24);
  return valset_lookup(a.vtab, a.vslot_mask, addr);
}
// One wavefront per record, the lanes stride over the carrier's children: the flag words of certv::pc_child / rcc_child are
// OR-reduced, the children whose sender bit is set are counted once per validator index through a bitmap (LDS; in HBM when the
// set's bitmap does not fit, one workgroup then walks all records and clears what it set, as block_tally_kernel), their power
// is summed in 2·PW 32-bit pieces and compared with the quorum, the fold gives the verdict.  A root PREPREPARE's rcc still
// lacks its children's pc: cert_judge_children_kernel.
template <int PW>
__global__ void __launch_bounds__(64) cert_judge_kernel(cert_judge_args a) {
  constexpr int NP = 2 * PW;
  extern __shared__ uint32_t jseen[];
  const uint32_t lane = threadIdx.x;
  uint32_t *bm = a.lds_bitmap ? jseen : a.seen;
  const uint32_t bm_words = (a.n_validators + 31u) / 32u;
  for (uint32_t rec = blockIdx.x; rec < a.n_records; rec += gridDim.x) {
    uint32_t row = rec, parent = wire::NO_PARENT;
    if (rec >= a.n_roots) {  // the LAST root whose first record is ≤ rec (roots without such children repeat a base)
      uint32_t lo = 0, hi = a.n_roots - 1;
      while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (a.rec_base[mid] <= rec) lo = mid;
        else hi = mid - 1;
      }
      parent = lo;
      row = a.nodes[lo].first_child + (rec - a.rec_base[lo]);
    }
    const bool root = parent == wire::NO_PARENT;
    const wire::node_info nd = a.nodes[row];
    const wire::row_info &ri = a.rows[row];
    // a root ROUND_CHANGE: its own view, with proposalMatchesCertificate; inside a root PREPREPARE's certificate: the PREPREPARE's view
    const uint64_t height = root ? ri.height : a.rows[parent].height, limit = root ? ri.round : a.rows[parent].round;
    int pc = certv::pc_head(a.nodes, a.rows, a.cls, a.n_rows, row, root);
    int rcc = root ? certv::rcc_head(a.nodes, a.rows, a.cls, a.n_rows, row) : certv::UNDECIDED;
    const bool walk_pc = pc == certv::GO, walk_rcc = rcc == certv::GO;  // never both: one is a ROUND_CHANGE, the other a PREPREPARE
    uint32_t rcc_rows = 0;
    if (walk_pc || walk_rcc) {  // wave-uniform
      const uint32_t lo = nd.first_child, n = nd.n_children;
      if (a.lds_bitmap) {
        for (uint32_t i = lane; i < bm_words; i += 64u) jseen[i] = 0;
        __syncthreads();
      }
      certv::pc_params p{height, limit, 0, nullptr, root};
      if (walk_pc) {
        p.ref_round = a.rows[lo].round;
        p.ref_hash = a.rows[lo].proposal_hash;
      }
      uint32_t flags = 0;
      uint64_t counts = 0;  // distinct validators | rows below << 32
      uint64_t pw[NP];
#pragma unroll
      for (int k = 0; k < NP; k++) pw[k] = 0;
      for (uint32_t c = lo + lane; c < lo + n; c += 64u) {
        const wire::row_info &w = a.rows[c];
        const wire::node_info &cn = a.nodes[c];
        const bool sb = cert_mask_bit(a.sender_mask, c);
        flags |= walk_pc ? certv::pc_child(w, cn, a.cls[c], sb, cert_mask_bit(a.hash_mask, c), c == lo, p)
                         : certv::rcc_child(w, cn, a.cls[c], sb, ri.height, ri.round);
        counts += (uint64_t)(1u + cn.n_children) << 32;
        if (!sb) continue;
        const int vi = cert_row_validator(a, w);
        if (vi < 0 || (uint32_t)vi >= a.n_validators) continue;
        if (!claim_first(bm, (uint32_t)vi)) continue;  // the same validator twice
        counts += 1;
#pragma unroll
        for (int k = 0; k < NP; k++) pw[k] += a.vpower32[(size_t)vi * NP + k];
      }
      __syncthreads();
      if (!a.lds_bitmap) {  // the HBM bitmap is left zero for the next record: clear exactly the words this one set
        for (uint32_t c = lo + lane; c < lo + n; c += 64u) {
          if (!cert_mask_bit(a.sender_mask, c)) continue;
          const int vi = cert_row_validator(a, a.rows[c]);
          if (vi >= 0 && (uint32_t)vi < a.n_validators) bm[vi >> 5] = 0u;
        }
        __syncthreads();
      }
      for (int o = 32; o; o >>= 1) flags |= (uint32_t)__shfl_xor((int)flags, o, 64);
      counts = wave_sum_u64(counts);
      uint64_t piece[TALLY_MAX_PIECES];
#pragma unroll
      for (int k = 0; k < TALLY_MAX_PIECES; k++) piece[k] = 0;
#pragma unroll
      for (int k = 0; k < NP; k++) piece[k] = wave_sum_u64(pw[k]);
      uint64_t wd[TALLY_SUM_WORDS];
      pieces_to_words(piece, NP, wd);
      const bool all_distinct = (uint32_t)counts == n, power_ok = words_ge(wd, a.quorum);
      if (walk_pc) pc = certv::pc_fold(flags, all_distinct, power_ok);
      else {
        rcc = certv::rcc_fold(flags, n, all_distinct, power_ok);
        if (rcc != certv::UNDECIDED) rcc_rows = (uint32_t)(counts >> 32);
      }
    }
    if (lane == 0) {
      certv::record r;
      certv::record_head(r, row, nd, ri, a.cls[row], cert_mask_bit(a.sender_mask, row), cert_mask_bit(a.hash_mask, row),
                         cert_mask_bit(a.self_mask, row));
      r.pc = (int8_t)pc;
      r.rcc = (int8_t)rcc;
      r.rcc_rows = rcc_rows;
      if (root && a.rec_base && a.rec_base[row + 1] != a.rec_base[row]) r.first_child_cert = a.rec_base[row];
      if (pc == certv::VALID) certv::record_pc_proposal(r, a.rows[nd.first_child]);
      a.out[rec] = r;
    }
  }
}
// A root PREPREPARE whose certificate holds (rcc == 1): the prepared certificate of every ROUND_CHANGE message in it must be
// decided — one with pc == −1 leaves rcc undecided (proposalVerdictFromRows returns "not decided" there, after all its other
// clauses).  A wavefront per root; the children's records were written by the launch before this one.
__global__ void __launch_bounds__(64) cert_judge_children_kernel(certv::record *__restrict__ out, uint32_t n_roots) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t root = blockIdx.x; root < n_roots; root += gridDim.x) {
    const certv::record &r = out[root];
    if (r.rcc != certv::VALID || r.first_child_cert == certv::NO_RECORD) continue;  // wave-uniform
    bool undecided = false;
    for (uint32_t k = lane; k < r.n_children; k += 64u) undecided = undecided || out[r.first_child_cert + k].pc == certv::UNDECIDED;
    const int rcc = certv::rcc_with_children(certv::VALID, __any(undecided));
    if (lane == 0 && rcc != certv::VALID) out[root].rcc = (int8_t)rcc;
  }
}

// ---- certificates: one decision per record (ibft_decide_certificates_wire; the rules: cert_decide_dev.h) --------------------
// Behind the two record kernels, with the proposer table of ibft_set_proposers: first a lane per record (valid_pc,
// round_change; everything else of the decision at its "nothing" value), then a wavefront per root for `proposal`.
struct cert_decide_args {
  const wire::node_info *nodes;
  const wire::row_info *rows;
  const certv::record *rec;
  const uint8_t *wire_bytes;
  const uint64_t *mid_state;  // 25 words per root (cert_digest_wave_kernel)
  certd::proposer_table table;
  uint32_t n_roots, n_rows, n_records;
  certd::decision *out;
};
__global__ void __launch_bounds__(256) cert_decide_records_kernel(cert_decide_args a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n_records) return;
  const certv::record &r = a.rec[i];
  const bool root = i < a.n_roots;
  uint64_t height = r.height;
  bool known = true;
  if (!root) {  // a record of a root PREPREPARE's certificate: validPC is asked for the PREPREPARE's height
    const uint32_t parent = r.row < a.n_rows ? a.nodes[r.row].parent : wire::NO_PARENT;
    known = parent < a.n_roots;
    height = known ? a.rec[parent].height : 0ull;
  }
  certd::decision d;
  certd::decide_record(d, r, root, height, known, a.table);
  a.out[i] = d;
}
// One wavefront per workgroup (the wavefront sponge's LDS protocol), roots r, r + grid, …  A root that is no regular PREPREPARE,
// or whose own clauses decide, leaves wave-uniformly; otherwise the lanes stride over the records of its RoundChangeCertificate
// (their valid_pc was written by the launch before this one), the highest prepared round is selected across the lanes, and
// keccak256(raw ‖ BE64(that round)) is closed from the state behind raw's full blocks: one permutation, two when
// raw_len mod 136 ≥ 128 — whatever raw_len is.
__global__ void __launch_bounds__(64) cert_decide_proposals_kernel(cert_decide_args a) {
  __shared__ uint64_t A[32], B[32];
  const uint32_t lane = threadIdx.x;
  for (uint32_t root = blockIdx.x; root < a.n_roots; root += gridDim.x) {
    const certv::record &r = a.rec[root];
    if (r.row != root || root >= a.n_rows) continue;  // (record i < n_roots is row i)
    const wire::row_info &ri = a.rows[root];
    const wire::node_info &nd = a.nodes[root];
    int v = certd::proposal_head(r, ri, nd, true, a.table);  // wave-uniform: every lane reads the same record
    if (v != certd::GO) {
      if (lane == 0) a.out[root].proposal = (int8_t)v;
      continue;
    }
    const uint32_t first = r.first_child_cert, n = r.n_children;
    if (first == certv::NO_RECORD || first < a.n_roots || (uint64_t)first + n > a.n_records) continue;  // stays −1: no such records
    certd::candidate best{0ull, 0u, 0u};
    bool undecided = false;
    for (uint32_t k = lane; k < n; k += 64u) certd::child_step(best, undecided, a.out[first + k].valid_pc, a.rec[first + k].pc_round, k);
    const certd::candidate win = certd::wave_select(best, lane);
    v = certd::proposal_after_children(__any(undecided), win);
    if (v != certd::GO) {
      if (lane == 0) a.out[root].proposal = (int8_t)v;
      continue;
    }
    const uint32_t prepared = first + win.k;  // win.k < n: a child index some lane stepped over
    const certv::record &w = a.rec[prepared];
    const uint32_t raw_len = nd.raw_len, full = raw_len / 136u * 136u;
    const uint64_t word = cw::sponge_message_from(a.wire_bytes + nd.raw_off, raw_len, 0u, raw_len + 8u, keccak::round_tail(w.pc_round), true, lane, A, B,
                                                  a.mid_state[25ull * root + cw::sponge_word(lane)], full, nullptr, 0u);
    uint64_t want = 0;
    if (lane < 4u)
      for (uint32_t b = 0; b < 8u; b++) want |= (uint64_t)w.pc_hash[8u * lane + b] << (8u * b);
    const bool differs = lane < 4u && word != want;
    const bool match = !__any(differs);
    if (lane == 0) {
      certd::decision d = a.out[root];
      certd::record_prepared(d, prepared, w, match);
      a.out[root] = d;
    }
  }
}

// ---- round changes: one quorum record per (height, round), GetExtendedRCC (ibft_decide_round_changes_wire; round_change_dev.h)
// Six launches behind the decision kernels on the same stream, in the shape of the views stage above: each phase that needs
// every row of the one before it is a launch of its own.
//   index    a thread per level-0 row: the sender's validator index of a row that takes part (rcd::row_index), −1 for every
//            other row.  A launch of its own because wviews::insert_row compares the index of OTHER rows: the columns the tables
//            are keyed by must all be written by an earlier launch (wire_views_dev.h: columns).
//   insert   a thread per level-0 row: a row that takes part goes, under that index, into wviews' key table (lowest row of its
//            (height, round)) and last table (highest row of its key and sender).
//   rank     ONE workgroup (wire_views_rank_kernel's shape): the representatives ranked in ascending row order; words[0] = keys,
//            words[2] = the level-0 rows the tree left to the host.
//   tally    a thread per row: out_rc_view, the stored bit (one ballot per wavefront is one word of out_rc_stored) and the key's
//            accumulators (rcd::acc_words).  A wavefront reduces one key per turn, at most RC_TURNS turns; whoever still waits
//            then — one sender's rows of 64 rounds in one wavefront — adds for itself.
//   records  a thread per record slot below min(n, rc_cap): rcd::key_record, then the key's accumulators are zeroed; a slot past
//            the number of keys is zeroed.
//   select   ONE wavefront strides over the records that were written: rcd::record_step, rcd::wave_state, rcd::make_answer.
constexpr int RC_THREADS = 256, RC_TURNS = 4;
struct round_change_args {
  const wire::row_info *rows;       // the tree's rows; level 0 is rows [0, n)
  const certv::record *rec;         // record i < n belongs to row i
  const certd::decision *dec;
  const uint32_t *vtab;             // the validator table (valset_lookup)
  const uint32_t *vpower32;         // n_validators × 2·PW pieces
  const uint64_t *quorum;           // TALLY_SUM_WORDS
  uint32_t vslot_mask, n_validators;
  uint32_t n, cap, slots, salt;     // cap: min(n, rc_cap)
  int n_pieces;
  int32_t *vidx;                    // n: the sender's validator index of a row that takes part, else −1 (index kernel; read-only afterwards)
  uint32_t *key_table, *last_table;  // slots words each
  uint32_t *slot_key, *slot_last;    // n
  uint32_t *rank_of;                 // n: rank of a representative
  uint32_t *first_row;               // cap: the representative of record v
  uint32_t *words;                   // behind the tables, all-ones like them at the start: [0] ← keys, [1] ← 0 when a table was exhausted, [2] ← unjudged rows
  int32_t *out_view;                 // n
  uint64_t *out_stored;              // ⌈n / 64⌉
  uint64_t *acc;                     // cap × rcd::acc_words, zero between calls
  rcd::record *out_rc;               // cap
  rcd::query query;
  rcd::answer *out_answer;
};
__global__ void __launch_bounds__(RC_THREADS) round_change_index_kernel(round_change_args a) {
  const uint32_t row = blockIdx.x * RC_THREADS + threadIdx.x;
  if (row >= a.n) return;
  a.vidx[row] = rcd::row_index(a.rec[row], a.rows[row], a.vtab, a.vslot_mask, a.n_validators);
}
__global__ void __launch_bounds__(RC_THREADS) round_change_insert_kernel(round_change_args a) {
  const uint32_t row = blockIdx.x * RC_THREADS + threadIdx.x;
  if (row >= a.n) return;
  const int32_t *vidx = a.vidx;  // (complete: the launch before this one wrote every entry)
  const wviews::row_slots s = wviews::insert_row(wviews::columns{a.rows, vidx}, row, vidx[row] >= 0, a.key_table, a.last_table, a.slots, a.salt);
  a.slot_key[row] = s.key;
  a.slot_last[row] = s.last;
  if (s.key == wviews::UNPLACED || s.last == wviews::UNPLACED) atomicAnd(a.words + 1, 0u);
}
__global__ void __launch_bounds__(1024) round_change_rank_kernel(round_change_args a) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x, per = (a.n + 1023u) / 1024u;
  const uint32_t b = t * per < a.n ? t * per : a.n, e = b + per < a.n ? b + per : a.n;
  uint64_t sum = 0;  // representatives | unjudged rows << 32
  for (uint32_t i = b; i < e; i++)
    sum += (wviews::is_rep(a.key_table, a.slot_key[i], i) ? 1ull : 0ull) | ((uint64_t)(rcd::unjudged(a.rec[i]) ? 1u : 0u) << 32);
  uint32_t run = (uint32_t)(block_scan_1024(part, sum) - sum);
  for (uint32_t i = b; i < e; i++) {
    if (!wviews::is_rep(a.key_table, a.slot_key[i], i)) continue;
    a.rank_of[i] = run;
    if (run < a.cap) a.first_row[run] = i;
    run++;
  }
  if (t == 1023u) {
    a.words[0] = (uint32_t)part[1023];
    a.words[2] = (uint32_t)(part[1023] >> 32);
  }
}
template <int PW>
__global__ void __launch_bounds__(RC_THREADS) round_change_tally_kernel(round_change_args a) {
  constexpr int NP = 2 * PW, STRIDE = 2 * NP + 2;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t row = blockIdx.x * RC_THREADS + tid;
  const uint32_t sk = row < a.n ? a.slot_key[row] : wviews::SKIP;
  int32_t v = wviews::VIEW_NONE;
  bool stored = false;
  if (sk < wviews::SKIP) {
    v = wviews::view_of_rank(a.rank_of[a.key_table[sk]], a.cap);
    stored = wviews::is_stored(a.last_table, a.slot_last[row], row);  // a row beyond the cap still supersedes
  }
  if (row < a.n) a.out_view[row] = v;
  const uint64_t sw = __ballot(stored ? 1 : 0);
  if (lane == 0 && (row & ~63u) < a.n) a.out_stored[row >> 6] = sw;
  bool pend = v >= 0;
  const int rc = pend && stored ? (int)a.dec[row].round_change : 0;
  const bool yes = rc == certd::YES, open = rc == certd::UNDECIDED;
  uint32_t pw[NP];
  {
    const bool adds = yes || open;
    const uint32_t entry = adds ? (uint32_t)a.vidx[row] : 0u;
#pragma unroll
    for (int k = 0; k < NP; k++) pw[k] = adds ? a.vpower32[(size_t)entry * NP + k] : 0u;
  }
  const uint64_t c0 = 1ull | ((uint64_t)(stored ? 1u : 0u) << 32), c1 = (yes ? 1ull : 0ull) | ((uint64_t)(open ? 1u : 0u) << 32);
  for (int turn = 0; turn < RC_TURNS; turn++) {  // (wave-uniform: every lane takes every turn)
    const uint64_t todo = __ballot(pend ? 1 : 0);
    if (!todo) break;
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t lv = __shfl(v, leader, 64);
    const bool mine = pend && v == lv;
    uint64_t *acc = a.acc + (size_t)lv * STRIDE;
    const uint64_t s0 = wave_sum_u64(mine ? c0 : 0ull), s1 = wave_sum_u64(mine ? c1 : 0ull);
    if (s1 & 0xFFFFFFFFull) {  // (wave-uniform) a yes row among them: its pieces
#pragma unroll
      for (int k = 0; k < NP; k++) {
        const uint64_t sum = wave_sum_u64(mine && yes ? (uint64_t)pw[k] : 0ull);
        if ((int)lane == leader && sum) atomicAdd(reinterpret_cast<unsigned long long *>(acc + k), (unsigned long long)sum);
      }
    }
    if (s1 >> 32) {  // (wave-uniform) an open row among them
#pragma unroll
      for (int k = 0; k < NP; k++) {
        const uint64_t sum = wave_sum_u64(mine && open ? (uint64_t)pw[k] : 0ull);
        if ((int)lane == leader && sum) atomicAdd(reinterpret_cast<unsigned long long *>(acc + NP + k), (unsigned long long)sum);
      }
    }
    if ((int)lane == leader) {
      atomicAdd(reinterpret_cast<unsigned long long *>(acc + 2 * NP), (unsigned long long)s0);
      if (s1) atomicAdd(reinterpret_cast<unsigned long long *>(acc + 2 * NP + 1), (unsigned long long)s1);
    }
    if (mine) pend = false;
  }
  if (pend) {  // more keys in this wavefront than turns: the lane adds for itself
    uint64_t *acc = a.acc + (size_t)v * STRIDE;
    if (yes || open) {
#pragma unroll
      for (int k = 0; k < NP; k++)
        if (pw[k]) atomicAdd(reinterpret_cast<unsigned long long *>(acc + (yes ? 0 : NP) + k), (unsigned long long)pw[k]);
      atomicAdd(reinterpret_cast<unsigned long long *>(acc + 2 * NP + 1), (unsigned long long)c1);
    }
    atomicAdd(reinterpret_cast<unsigned long long *>(acc + 2 * NP), (unsigned long long)c0);
  }
}
__global__ void __launch_bounds__(RC_THREADS) round_change_records_kernel(round_change_args a) {
  const uint32_t v = blockIdx.x * RC_THREADS + threadIdx.x;
  if (v >= a.cap) return;
  rcd::record rec;
  if (v < a.words[0]) {
    const int words = rcd::acc_words(a.n_pieces);
    uint64_t *acc = a.acc + (size_t)v * words;
    const uint32_t first = a.first_row[v];
    rcd::key_record(rec, first, a.rows[first], acc, a.n_pieces, a.quorum);
    for (int k = 0; k < words; k++) acc[k] = 0;
  } else {
    rcd::empty_record(rec);
  }
  a.out_rc[v] = rec;
}
__global__ void __launch_bounds__(64) round_change_select_kernel(round_change_args a) {
  const uint32_t lane = threadIdx.x;
  const uint32_t n_keys = a.words[0], filled = n_keys < a.cap ? n_keys : a.cap;
  rcd::lane_state s = rcd::lane_init();
  for (uint32_t i = lane; i < filled; i += 64u) rcd::record_step(s, a.out_rc[i], i, a.query);
  const rcd::lane_state w = rcd::wave_state(s, lane);
  if (lane == 0) {
    rcd::answer ans;
    rcd::make_answer(ans, w, n_keys, a.cap, a.words[2]);
    *a.out_answer = ans;
  }
}

// ---- multi-GPU: the one exchange step -------------------------------------------------
// Exchange buffer of a sharded batch (u64 slots):
//   [ K × (verdict words of rank 0 | … | rank W−1) | W × ⌈n_validators/64⌉ distinct-sender bitmap words | valid rows ]
// A rank fills its own word range of each of the K verdict arrays (K = 1: a seal / sender batch, K = 2: the sender and
// the valid words of a message set), its own bitmap segment and its count of valid rows; everything else is zero.
// After the all-reduce(SUM) the words are the global verdict masks (disjoint shards: sum ≡ OR) and every rank holds
// every rank's bitmap.  The tally is NOT additive: HasQuorum counts a validator once however many rows it has
// (a map[string]struct{} in core/validator_manager.go:86-92, 147-155), and rows of one sender may lie in two shards —
// so the unpack step ORs the W segments and recomputes power, distinct senders and has_quorum from the merged
// bitmap, exactly what tally_kernel computes from its own bitmap on one device.
struct exchange_pack_args {
  const uint64_t *mask[2];   // this rank's verdict words (my_words each); mask[1] unused when K = 1
  const uint32_t *seen;      // this rank's distinct-sender bitmap (tally_args::seen_out), 2·seen_words 32-bit words
  const uint64_t *tally_out; // this rank's tally (word 2: valid rows | distinct << 32)
  uint64_t *xbuf;
  uint32_t K, world, rank, words_per_rank, my_words, seen_words;
};
__global__ void exchange_pack_kernel(exchange_pack_args a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t total_words = a.words_per_rank * a.world;
  const uint32_t seen_base = a.K * total_words, cnt = seen_base + a.world * a.seen_words;
  if (i < seen_base) {
    const uint32_t k = i / total_words, j = i - k * total_words, off = a.rank * a.words_per_rank;
    a.xbuf[i] = (j >= off && j < off + a.my_words) ? a.mask[k][j - off] : 0ull;
  } else if (i < cnt) {
    const uint32_t r = (i - seen_base) / a.seen_words, j = (i - seen_base) - r * a.seen_words;
    a.xbuf[i] = r == a.rank ? ((uint64_t)a.seen[2 * j] | ((uint64_t)a.seen[2 * j + 1] << 32)) : 0ull;
  } else if (i == cnt) {  // valid rows | valid rows sent by the proposer << 32 (both sum across ranks)
    a.xbuf[i] = (a.tally_out[2] & 0xFFFFFFFFull) | (a.tally_out[TALLY_OUT_PROPOSER_ROWS] << 32);
  }
}

// The collective itself when every rank's buffer is addressable from one device (a group that lists one device
// several times, or peer-mapped devices): out[i] = Σ_r buf_r[i], written back into every rank's buffer — what
// ncclAllReduce(sum, u64) leaves there.
constexpr int XSUM_MAX_RANKS = 64;
struct exchange_sum_args {
  uint64_t *buf[XSUM_MAX_RANKS];
  uint32_t world, slots;
};
__global__ void exchange_sum_kernel(exchange_sum_args a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.slots) return;
  uint64_t s = 0;
  for (uint32_t r = 0; r < a.world; r++) s += a.buf[r][i];
  for (uint32_t r = 0; r < a.world; r++) a.buf[r][i] = s;
}

// merged buffer → [ K·total_words verdict words | TALLY_OUT_WORDS-style tally ] in device memory and, when given,
// mapped host memory.  The last workgroup is the tally over the merged bitmap.
constexpr int XUNPACK_THREADS = 1024;
struct exchange_unpack_args {
  const uint64_t *xbuf;
  const uint32_t *vpower32;  // n_validators × n_pieces 32-bit pieces
  const uint64_t *quorum;
  uint64_t *dst, *host_dst;
  uint32_t K, world, words_per_rank, seen_words, n_pieces, n_validators;
  uint32_t prop_on;    // HasPrepareQuorum: the proposer's seat joins the MERGED bitmap, a valid row of his in any shard voids
  int32_t prop_vidx;
};
__global__ void __launch_bounds__(XUNPACK_THREADS) exchange_unpack_kernel(exchange_unpack_args a) {
  const uint32_t total_words = a.words_per_rank * a.world;
  const uint32_t seen_base = a.K * total_words;
  if (blockIdx.x + 1 < gridDim.x) {
    const uint32_t i = blockIdx.x * XUNPACK_THREADS + threadIdx.x;
    if (i < seen_base) {
      const uint64_t w = a.xbuf[i];
      a.dst[i] = w;
      if (a.host_dst) a.host_dst[i] = w;
    }
    return;
  }
  __shared__ uint64_t part[TALLY_MAX_PIECES + 2][XUNPACK_THREADS / 64];
  const uint32_t tid = threadIdx.x;
  uint64_t p[TALLY_MAX_PIECES];
#pragma unroll
  for (int k = 0; k < TALLY_MAX_PIECES; k++) p[k] = 0;
  uint64_t distinct = 0, overlap = 0;
  for (uint32_t j = tid; j < a.seen_words; j += XUNPACK_THREADS) {
    uint64_t m = 0, per_rank = 0;
    for (uint32_t r = 0; r < a.world; r++) {
      const uint64_t s = a.xbuf[seen_base + r * a.seen_words + j];
      m |= s;
      per_rank += (uint64_t)__popcll(s);
    }
    if (a.prop_on && a.prop_vidx >= 0 && (uint32_t)a.prop_vidx / 64u == j) {  // the proposer's seat
      const uint64_t seat = 1ull << ((uint32_t)a.prop_vidx & 63u);
      if (!(m & seat)) per_rank++;  // (not an overlap: keep per_rank − popcount(m) what it was)
      m |= seat;
    }
    const uint64_t here = (uint64_t)__popcll(m);
    distinct += here;
    overlap += per_rank - here;  // senders with valid rows in more than one shard: counted once
    while (m) {
      const uint32_t b = (uint32_t)__ffsll((long long)m) - 1u;
      m &= m - 1;
      const uint32_t v = 64u * j + b;
      if (v < a.n_validators) {
#pragma unroll
        for (int k = 0; k < TALLY_MAX_PIECES; k++)
          if ((uint32_t)k < a.n_pieces) p[k] += a.vpower32[(size_t)v * a.n_pieces + k];
      }
    }
  }
  block_sum(part, p);
  wave_part(part[TALLY_MAX_PIECES], distinct);
  wave_part(part[TALLY_MAX_PIECES + 1], overlap);
  __syncthreads();
  if (tid != 0) return;
  uint64_t piece[TALLY_MAX_PIECES];
  block_totals<TALLY_MAX_PIECES>(part, piece);
  const uint64_t d = parts_total(part[TALLY_MAX_PIECES]), o = parts_total(part[TALLY_MAX_PIECES + 1]);
  uint64_t t[6 + TALLY_SUM_WORDS];  // the record, the power in full, the overlap, the proposer's rows
  const uint64_t counts = a.xbuf[seen_base + a.world * a.seen_words];
  const uint64_t proposer_rows = a.prop_on ? counts >> 32 : 0ull;
  tally_record(piece, TALLY_MAX_PIECES, (counts & 0xFFFFFFFFull) | (d << 32), a.quorum, proposer_rows, t, t + 4);
  t[4 + TALLY_SUM_WORDS] = o;
  t[5 + TALLY_SUM_WORDS] = proposer_rows;
#pragma unroll
  for (int k = 0; k < 6 + TALLY_SUM_WORDS; k++) {
    a.dst[seen_base + k] = t[k];
    if (a.host_dst) a.host_dst[seen_base + k] = t[k];
  }
}

// ---- the seal-digest convention (ibft_set_seal_digest) --------------------------------------------------
// Backend.IsValidCommittedSeal is "the signature for the proposal hash in the committed seal" (core/backend.go:53-55);
// WHAT is signed is the embedding Backend's business — the 32-byte proposalHash itself (default), or
// keccak256(proposalHash ‖ suffix) (e.g. a COMMIT-type byte appended before hashing).  One lane per row: the carried hash
// is kept (copy32: what a1 compares) and the row's digest replaces it in the column the verdict kernels read.
struct seal_digest_args {
  uint8_t *hash32;        // n × 32: carried hashes in, digests out
  uint8_t *copy32;        // or null: the carried hashes, unchanged
  uint32_t n;
  uint64_t suffix_words[9];  // suffix ‖ 0x01 ‖ 0… as little-endian words (bytes 32..103 of the one Keccak block)
};
__global__ void seal_digest_kernel(seal_digest_args a) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.n) return;
  uint4 *p = reinterpret_cast<uint4 *>(a.hash32 + 32ull * row);
  const uint4 x = p[0], y = p[1];
  if (a.copy32) {
    uint4 *q = reinterpret_cast<uint4 *>(a.copy32 + 32ull * row);
    q[0] = x;
    q[1] = y;
  }
  uint64_t s[4] = {(uint64_t)x.x | ((uint64_t)x.y << 32), (uint64_t)x.z | ((uint64_t)x.w << 32), (uint64_t)y.x | ((uint64_t)y.y << 32),
                   (uint64_t)y.z | ((uint64_t)y.w << 32)};
  seal_digest_words(s, a.suffix_words);
  p[0] = make_uint4((uint32_t)s[0], (uint32_t)(s[0] >> 32), (uint32_t)s[1], (uint32_t)(s[1] >> 32));
  p[1] = make_uint4((uint32_t)s[2], (uint32_t)(s[2] >> 32), (uint32_t)s[3], (uint32_t)(s[3] >> 32));
}

// sender -> validator index, for ibft_tally() on a caller-supplied mask
// proposer5 (or null): HasPrepareQuorum compares From with the proposer's address byte for byte, member or not
// (validator_manager.go:114-115) — a row of a proposer who is no validator is marked VIDX_PROPOSER_OUTSIDER
struct lookup_proposer {
  uint32_t on, a[5];
};
__global__ void lookup_kernel(const uint8_t *__restrict__ signer20, const uint32_t *__restrict__ vtab,
                              uint32_t slot_mask, uint32_t n, int32_t *__restrict__ vidx, lookup_proposer prop) {
  uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  uint32_t a[5];
  const uint32_t *p = reinterpret_cast<const uint32_t *>(signer20 + 20ull * row);
  for (int i = 0; i < 5; i++) a[i] = p[i];
  int v = valset_lookup(vtab, slot_mask, a);
  if (prop.on && v < 0 && a[0] == prop.a[0] && a[1] == prop.a[1] && a[2] == prop.a[2] && a[3] == prop.a[3] && a[4] == prop.a[4])
    v = VIDX_PROPOSER_OUTSIDER;
  vidx[row] = v;
}

// ---- device canary (ibft_issue_probe) ------------------------------------------------------------------------------
// The verdict kernels are bound by VALU issue, so a device that issues slower than its kind (round 5 met one lease in ≈ 35
// whose every throughput-bound kernel ran 1.3–1.45 × slower) shows in ONE number: the time of a plain
// 8-byte VALU instruction that starts on an 8-byte boundary with one resident wavefront per SIMD — 1.89 ns through this
// probe on a healthy MI355X (the bare stream: 1.78 ns = 4.16 cycles at 2.39 GHz, profiles/r06b_ubench_wave.txt).  ISSUE_PROBE_ITERS × 64 independent v_add_u32 per
// wavefront ≈ 0.24 ms per launch; the launch shape is the rows kernel's at N = 4 096 (256 workgroups of four wavefronts).
constexpr int ISSUE_PROBE_ITERS = 2048;
// 96 KB of LDS per workgroup: more than half of a compute unit's 160 KB, so the dispatcher cannot put two of these
// workgroups on one compute unit — 256 workgroups of four wavefronts are ONE wavefront per SIMD on 256 compute units by
// construction.  (A kernel this small — 9 registers, no LDS — is otherwise packed several workgroups to a compute unit, and
// four wavefronts on a SIMD issue a plain instruction every 6.2 cycles each: the first version of this probe read 2.53 ns on a
// healthy device, profiles/r06a_kernel_ab.txt.)
constexpr int ISSUE_PROBE_LDS_WORDS = 96 * 1024 / 4;
__global__ void __launch_bounds__(256) issue_probe_kernel(uint32_t *out, uint32_t seed) {
  __shared__ uint32_t hold[ISSUE_PROBE_LDS_WORDS];
  hold[threadIdx.x] = seed;
  uint32_t a0 = seed + threadIdx.x, a1 = a0 * 3 + 1, a2 = a0 * 5 + 7, a3 = a0 * 7 + 3;
  uint32_t b0 = a0 ^ 0x1234567, b1 = a1 ^ 0x89abcde, b2 = a2 ^ 0x13579bd, b3 = a3 ^ 0x2468ace;
#pragma unroll 1
  for (int i = 0; i < ISSUE_PROBE_ITERS; i++) {
#define IBFT_P8(x) x x x x x x x x
    // (no .p2align here: go-ibft_amd/phase_align.py keeps 8-byte instructions on 8-byte boundaries itself, and an assembler
    // directive that emits padding breaks its instruction count)
    asm volatile(IBFT_P8("v_add_u32_e64 %0, %0, %8\n v_add_u32_e64 %1, %1, %8\n v_add_u32_e64 %2, %2, %8\n"
                                        "v_add_u32_e64 %3, %3, %8\n v_add_u32_e64 %4, %4, %8\n v_add_u32_e64 %5, %5, %8\n"
                                        "v_add_u32_e64 %6, %6, %8\n v_add_u32_e64 %7, %7, %8\n")
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3)
                 : "v"(seed | 1));
#undef IBFT_P8
  }
  if ((a0 ^ a1 ^ a2 ^ a3 ^ b0 ^ b1 ^ b2 ^ b3) == 0x9e3779b9u) out[0] = a0 + hold[(threadIdx.x * 97u) % ISSUE_PROBE_LDS_WORDS];  // keeps the chain (and the LDS block) alive
}

}  // namespace ibftk
