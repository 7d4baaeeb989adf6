// sign_envelope_dev.h — the signing side two layers up: a PREPREPARE / ROUND_CHANGE envelope around a body the caller encoded.
//
// Product code, __host__ __device__ and for simulators only, as sign_dev.h says (tests/test_sign_envelopes_host.py runs this source
// on the CPU).  What the reference's Backend.BuildPrePrepareMessage / BuildRoundChangeMessage do for one validator
// (/root/reference/core/backend.go:12-34).
//
// A row is (sk, type, height, round, body bytes).  Its message is sign_message_dev.h's View ‖ From (put_message_front) and
// signature field, then
//
//     [20 03]                                              Type: absent for PREPREPARE (a zero scalar), 20 03 for ROUND_CHANGE
//     2a | 42  varint(body_len)  <body>                    PrePrepareMessage (field 5) / RoundChangeMessage (field 8), emitted
//                                                          even when the body is empty
//
// Everything in front of the body is the HEAD (at most 121 bytes); the body is any number of bytes — a ROUND_CHANGE that carries
// the PreparedCertificate of 1 024 validators is ≈106 KB.  So the row is not one lane's work from end to end, it is four steps
// (kernels.hip.h wraps each in a kernel):
//   1. envelope_head     a lane per row: From from the key, the head built in LDS and stored with a ZERO signature;
//   2. copy_body_piece   the bodies → behind the heads: a bandwidth copy between byte-granular offsets;
//   3. the digest        keccak256 of the STORED message minus its signature field — the verifier's own code for exactly that:
//                        wire::hash_pieces per lane (envelope_digest_lane) or cw::sponge_message per wavefront;
//   4. sign_digest       sign the digest (sign_dev.h), the signature goes into its place.
// The head is never spliced into a sponge on its own: step 3 reads what steps 1 and 2 stored.
#pragma once
#include "cert_wave_dev.h"
#include "sign_message_dev.h"

namespace ibftk {

constexpr uint32_t MSG_TYPE_PREPREPARE = 0, MSG_TYPE_ROUND_CHANGE = 3;
constexpr uint32_t ENVELOPE_HEAD_MAX = 121;  // View 24 ‖ From 22 ‖ Signature 67 ‖ Type 2 ‖ tag 1 ‖ varint(body_len < 2^32) 5
constexpr int ENVELOPE_HEAD_WORDS = 16;      // 128 bytes of LDS per row
constexpr uint32_t ENVELOPE_COPY_THREADS = 256, ENVELOPE_COPY_PIECE = 16 * ENVELOPE_COPY_THREADS;  // bytes of output per workgroup

// where the signature field starts: behind View and From — a function of height and round alone
__host__ __device__ __forceinline__ uint32_t envelope_cut(uint64_t height, uint64_t round) {
  return 2u + message_view_len(height, round) + 22u;
}
__host__ __device__ __forceinline__ uint32_t envelope_head_len(uint32_t type, uint64_t height, uint64_t round, uint32_t body_len) {
  return envelope_cut(height, round) + SIGN_MESSAGE_SIG_FIELD + (type ? 2u : 0u) + 1u + varint_len(body_len);
}
// the whole row; it depends on nothing but these four (a refused key keeps its row's length)
__host__ __device__ __forceinline__ uint64_t envelope_wire_len(uint32_t type, uint64_t height, uint64_t round, uint32_t body_len) {
  return (uint64_t)envelope_head_len(type, height, round, body_len) + body_len;
}

// 1. The head at p (ENVELOPE_HEAD_WORDS words of the row's own: LDS on the device, never a private byte array), the signature
// zero; returns its length.
__host__ __device__ __forceinline__ uint32_t envelope_head(uint8_t *p, uint32_t type, uint64_t height, uint64_t round,
                                                           const uint32_t addr[5], uint32_t body_len) {
  uint32_t at = put_message_front(p, height, round, addr);
  p[at++] = 0x1a;
  p[at++] = 0x41;
  for (int i = 0; i < 65; i++) p[at + i] = 0;
  at += 65;
  if (type) {
    p[at++] = 0x20;
    p[at++] = (uint8_t)type;
  }
  p[at++] = type == MSG_TYPE_ROUND_CHANGE ? 0x42 : 0x2a;
  return put_varint(p, at, body_len);
}
// byte stores: a row starts wherever the one before it ended
__host__ __device__ __forceinline__ void store_envelope_head(uint8_t *__restrict__ out, const uint8_t *p, uint32_t len) {
  for (uint32_t i = 0; i < len; i++) out[i] = p[i];
}

// 2. The body copy.  Row i's body goes from body[src_at, src_at + len) to wire[dst_at, dst_at + len); both offsets are anything
// mod 4, and rows are packed back to back, so the dword at a row's edge usually belongs to two rows that different wavefronts
// write.  The output is cut into 16-byte aligned segments: a segment that lies inside the row is ONE 16-byte store fed by five
// aligned dword loads realigned with funnel shifts; in the (at most two) segments on a row's edges the dwords that lie inside go
// as dword stores and the bytes of a dword the row shares go as BYTE stores — nothing is read-modify-written.  Loads run up to
// 3 bytes past the body (the body buffer carries 256 bytes of slack); stores never leave [dst_at, dst_at + len).
__host__ __device__ __forceinline__ uint32_t envelope_copy_pieces(uint32_t dst_at, uint32_t len) {
  return len ? ((dst_at & 15u) + len + ENVELOPE_COPY_PIECE - 1u) / ENVELOPE_COPY_PIECE : 0u;
}
// the dword at any address: the aligned dword(s) that hold it, funnel-shifted
__host__ __device__ __forceinline__ uint32_t load_dword_any(const uint8_t *s) {
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3u);
  const uint32_t *q = reinterpret_cast<const uint32_t *>(s - mis);
  const uint32_t d0 = q[0], d1 = mis ? q[1] : 0u;
  return (uint32_t)(((uint64_t)d1 << 32 | d0) >> (8u * mis));
}
// thread t of ENVELOPE_COPY_THREADS, piece `piece` of the row: one 16-byte segment
__host__ __device__ __forceinline__ void copy_body_piece(uint8_t *__restrict__ wire, const uint8_t *__restrict__ body, uint32_t dst_at,
                                                         uint32_t src_at, uint32_t len, uint32_t piece, uint32_t t) {
  const uint32_t lo = dst_at, hi = dst_at + len;
  const uint64_t seg64 = (uint64_t)(lo & ~15u) + 16ull * ((uint64_t)piece * ENVELOPE_COPY_THREADS + t);
  if (seg64 >= hi) return;
  const uint32_t seg = (uint32_t)seg64;
  if (seg >= lo && seg + 16u <= hi) {
    const uint8_t *s = body + src_at + (seg - lo);
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3u), sh = 8u * mis;
    const uint32_t *q = reinterpret_cast<const uint32_t *>(s - mis);
    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = mis ? q[4] : 0u;
    uint4 v;
    v.x = (uint32_t)(((uint64_t)d1 << 32 | d0) >> sh);
    v.y = (uint32_t)(((uint64_t)d2 << 32 | d1) >> sh);
    v.z = (uint32_t)(((uint64_t)d3 << 32 | d2) >> sh);
    v.w = (uint32_t)(((uint64_t)d4 << 32 | d3) >> sh);
    *reinterpret_cast<uint4 *>(wire + seg) = v;
    return;
  }
  for (uint32_t j = 0; j < 4u; j++) {
    const uint32_t x = seg + 4u * j;
    if (x >= lo && x + 4u <= hi) {
      *reinterpret_cast<uint32_t *>(wire + x) = load_dword_any(body + src_at + (x - lo));
    } else {
      for (uint32_t b = 0; b < 4u; b++)
        if (x + b >= lo && x + b < hi) wire[x + b] = body[src_at + (x + b - lo)];
    }
  }
}

// 3. keccak256 of the stored message m[0, len) minus its signature field [cut, cut + 67), by one lane: whole blocks with aligned
// dword loads, the block on the seam and the last one byte by byte (wire_dev.h: hash_pieces — what the certificate path hashes a
// long nested message with).  A lane that is not live hashes the empty message and reads nothing.
__host__ __device__ __forceinline__ void envelope_digest_lane(const uint8_t *m, uint32_t len, uint32_t cut, bool live, uint64_t out4[4]) {
  const uint32_t na = live ? cut : 0u, nb = live ? len - cut - SIGN_MESSAGE_SIG_FIELD : 0u;
  wire::hash_pieces(m, na, m + cut + SIGN_MESSAGE_SIG_FIELD, nb, m, 0u, out4);
}
// the same by the calling wavefront, the state over 25 lanes (cert_wave_dev.h); lanes 0 … 3 return the digest's words
__host__ __device__ __forceinline__ uint64_t envelope_digest_wave(const uint8_t *m, uint32_t len, uint32_t cut, uint32_t lane, uint64_t *A,
                                                                  uint64_t *B) {
  return cw::sponge_message(m, cut, SIGN_MESSAGE_SIG_FIELD, len - SIGN_MESSAGE_SIG_FIELD, 0ull, false, lane, A, B);
}

// 4. The signature over that digest: sign_dev.h's sign_digest, stored by put_sig65 at cut + 2 of the row (the field the head left zero).
}  // namespace ibftk
