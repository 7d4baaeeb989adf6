// sign_message_dev.h — the signing side one layer up: a whole PREPARE / COMMIT message per row, as wire bytes.
//
// Product code, __host__ __device__ and for simulators only, as sign_dev.h says (tests/test_sign_messages_host.py runs this source on
// the CPU).  What the reference's Backend.BuildPrepareMessage / BuildCommitMessage do for one validator
// (/root/reference/core/backend.go:12-34).
//
// A row is (sk, type, height, round, proposal hash).  Its message, in canonical proto3 (fields in field-number order, minimal
// varints, zero scalars omitted, the View always present — messages.proto:24-110, the rules wire_dev.h checks):
//
//     0a <len> [08 varint(height)] [10 varint(round)]      View (field 1), present even when empty     ┐ put_message_front
//     12 14 <From, 20 bytes>                               keccak256(X‖Y)[12..32) of sk·G              ┘
//     1a 41 <signature, 65 bytes>                          ← NOT part of PayloadNoSig
//     20 <type>                                            1 = PREPARE, 2 = COMMIT
//     32 22 0a 20 <hash>                                   PREPARE: PrepareMessage (field 6)
//     3a 65 0a 20 <hash> 12 41 <committed seal>            COMMIT: CommitMessage (field 7)
//
// PayloadNoSig (what the envelope signature signs the Keccak-256 of) is these bytes without the third line: 62 … 84 bytes for
// a PREPARE, 129 … 151 for a COMMIT — so a COMMIT's hash is one Keccak block or two, with the 135-byte case (pad10*1 = the
// single byte 0x81) in between.  The committed seal signs the proposal hash under the seal-digest convention
// (ibft_set_seal_digest), the envelope never does.  The payload is built in a buffer of the caller's (19 words per row: LDS on the
// device, never a private byte array), which also is what the sponge absorbs; the wire form goes out from there with the
// signature spliced in.
#pragma once
#include "sign_dev.h"

namespace ibftk {

constexpr uint32_t MSG_TYPE_PREPARE = 1, MSG_TYPE_COMMIT = 2;
constexpr uint32_t SIGN_MESSAGE_PAYLOAD_MAX = 151;  // COMMIT, height = round = 2^64 − 1
constexpr uint32_t SIGN_MESSAGE_SIG_FIELD = 67;     // 1a 41 ‖ signature
constexpr uint32_t SIGN_MESSAGE_MAX = SIGN_MESSAGE_PAYLOAD_MAX + SIGN_MESSAGE_SIG_FIELD;  // IBFT_SIGN_MESSAGE_MAX
constexpr int SIGN_MESSAGE_BUF_WORDS = 19;          // 152 bytes: the longest payload and the first byte of its padding

__host__ __device__ __forceinline__ uint32_t varint_len(uint64_t v) {
  return (uint32_t)(70 - __builtin_clzll(v | 1u)) / 7u;  // ⌈bits / 7⌉, bits = 1 … 64
}
__host__ __device__ __forceinline__ uint32_t message_view_len(uint64_t height, uint64_t round) {
  return (height ? 1u + varint_len(height) : 0u) + (round ? 1u + varint_len(round) : 0u);
}
// length of PayloadNoSig; it depends on nothing but these three (a refused key keeps its row's length)
__host__ __device__ __forceinline__ uint32_t message_payload_len(uint32_t type, uint64_t height, uint64_t round) {
  return 2u + message_view_len(height, round) + 22u + 2u + 2u + 34u + (type == MSG_TYPE_COMMIT ? 67u : 0u);
}
__host__ __device__ __forceinline__ uint32_t message_wire_len(uint32_t type, uint64_t height, uint64_t round) {
  return message_payload_len(type, height, round) + SIGN_MESSAGE_SIG_FIELD;
}

__host__ __device__ __forceinline__ uint32_t put_varint(uint8_t *p, uint32_t at, uint64_t v) {
  while (v >= 0x80u) {
    p[at++] = (uint8_t)(v | 0x80u);
    v >>= 7;
  }
  p[at++] = (uint8_t)v;
  return at;
}
// The front of every message the signer builds: View ‖ From at p.  Returns the offset behind From, which is where the signature
// field goes on the wire — envelope_cut(height, round) in closed form (sign_envelope_dev.h).
__host__ __device__ __forceinline__ uint32_t put_message_front(uint8_t *p, uint64_t height, uint64_t round, const uint32_t addr[5]) {
  uint32_t at = 0;
  p[at++] = 0x0a;
  p[at++] = (uint8_t)message_view_len(height, round);
  if (height) {
    p[at++] = 0x08;
    at = put_varint(p, at, height);
  }
  if (round) {
    p[at++] = 0x10;
    at = put_varint(p, at, round);
  }
  p[at++] = 0x12;
  p[at++] = 0x14;
#pragma unroll
  for (int i = 0; i < 20; i++) p[at + i] = (uint8_t)(addr[i >> 2] >> (8 * (i & 3)));
  return at + 20;
}

struct message_row {
  uint32_t len;  // bytes of PayloadNoSig in the buffer
  uint32_t cut;  // where field 3 goes: behind From
  u256 r, s;     // the envelope signature
  uint32_t v;
  uint32_t addr[5];
  bool ok;       // false: key outside [1, n) — zero From, zero seal, zero signature, the normal length
};

// One row.  buf: SIGN_MESSAGE_BUF_WORDS words of the row's own; holds PayloadNoSig on return.  convert / suffix_words: the
// seal-digest convention as block_head_row takes it (suffix ‖ 0x01 ‖ 0… as little-endian words).  On the device every lane of a
// wavefront must call this (sign_core votes across the wavefront in both passes): a PREPARE lane next to a COMMIT lane signs
// the seal digest too and drops the result, an idle lane runs a row of its own and stores nothing.
template <int NONCE>
__host__ __device__ __forceinline__ message_row sign_message_row(const uint32_t *__restrict__ gtab, const uint8_t *sk32, uint32_t type,
                                                                 uint64_t height, uint64_t round, const uint8_t *hash32,
                                                                 uint32_t convert, const uint64_t suffix_words[9], uint64_t *buf) {
  message_row m;
  uint8_t *p = reinterpret_cast<uint8_t *>(buf);
  const bool commit = type == MSG_TYPE_COMMIT;
  // a. the address, once
  u256 d;
  const bool key_ok = sign_key(sk32, d);
  sign_address(gtab, d, key_ok, m.addr);
  // c. everything of PayloadNoSig but the seal
#pragma unroll
  for (int i = 0; i < SIGN_MESSAGE_BUF_WORDS; i++) buf[i] = 0;
  uint32_t at = m.cut = put_message_front(p, height, round, m.addr);
  p[at++] = 0x20;
  p[at++] = (uint8_t)type;
  p[at++] = commit ? 0x3a : 0x32;
  p[at++] = commit ? 0x65 : 0x22;
  p[at++] = 0x0a;
  p[at++] = 0x20;
#pragma unroll
  for (int i = 0; i < 32; i++) p[at + i] = hash32[i];
  at += 32;
  const uint32_t seal_at = at;
  m.len = at + (commit ? 67u : 0u);

  // b. what the seal signs: the hash itself, or keccak256(hash ‖ suffix)
  uint8_t dg[32];
#pragma unroll
  for (int i = 0; i < 32; i++) dg[i] = hash32[i];
  if (convert) {
    uint64_t w[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      w[j] = 0;
#pragma unroll
      for (int t = 0; t < 8; t++) w[j] |= (uint64_t)hash32[8 * j + t] << (8 * t);
    }
    seal_digest_words(w, suffix_words);
#pragma unroll
    for (int i = 0; i < 32; i++) dg[i] = (uint8_t)(w[i >> 3] >> (8 * (i & 7)));
  }

  // pass 0 signs the seal digest, pass 1 the digest of PayloadNoSig: ONE copy of sign_core in the instruction stream.  A
  // wavefront without a COMMIT lane has no seal to sign and starts at pass 1 — the WHOLE wavefront does (the vote is
  // wave-uniform), so its lanes still enter sign_core together; one COMMIT lane and every lane runs both passes.
#if defined(__HIP_DEVICE_COMPILE__)
  const bool seal_pass = __ballot(commit) != 0;
#else
  const bool seal_pass = commit;
#endif
  m.ok = false;
  m.r = secp::zero256();
  m.s = secp::zero256();
  m.v = 0;
#pragma unroll 1
  for (int pass = seal_pass ? 0 : 1; pass < 2; pass++) {
    if (pass == 1) {
      if (commit) {
        p[seal_at] = 0x12;
        p[seal_at + 1] = 0x41;
        put_sig65(p + seal_at + 2, m.r, m.s, m.v);
      }
      // d. keccak256(PayloadNoSig): one block below 136 bytes, two from there on; pad10*1 starts right behind the message
      p[m.len] = 0x01;
      uint64_t st[25];
#pragma unroll
      for (int i = 0; i < 25; i++) st[i] = 0;
      const int blocks = m.len >= 136u ? 2 : 1;
#pragma unroll 1
      for (int b = 0; b < blocks; b++) {
        if (b == 0) {
#pragma unroll
          for (int i = 0; i < 17; i++) st[i] ^= buf[i];
        } else {
          st[0] ^= buf[17];
          st[1] ^= buf[18];
        }
        if (b == blocks - 1) st[16] ^= 0x8000000000000000ULL;
        keccak::f1600(st);
      }
      p[m.len] = 0;
#pragma unroll
      for (int i = 0; i < 32; i++) dg[i] = (uint8_t)(st[i >> 3] >> (8 * (i & 7)));
    }
    m.ok = sign_core<NONCE>(gtab, sk32, d, key_ok, dg, m.r, m.s, m.v, 0u);
  }
  return m;
}

// e. the wire message: PayloadNoSig with field 3 spliced in behind From — m.len + 67 bytes at out, byte stores (a row starts
// wherever the one before it ended)
__host__ __device__ __forceinline__ void store_message(uint8_t *__restrict__ out, const uint64_t *buf, const message_row &m) {
  const uint8_t *p = reinterpret_cast<const uint8_t *>(buf);
  for (uint32_t i = 0; i < m.cut; i++) out[i] = p[i];
  out[m.cut] = 0x1a;
  out[m.cut + 1] = 0x41;
  put_sig65(out + m.cut + 2, m.r, m.s, m.v);
  for (uint32_t i = m.cut; i < m.len; i++) out[i + SIGN_MESSAGE_SIG_FIELD] = p[i];
}

}  // namespace ibftk
