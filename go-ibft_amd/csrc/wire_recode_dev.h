// wire_recode_dev.h — PREPARE / COMMIT messages in a NON-canonical protobuf encoding, judged on the device
// (IBFT_FLAG_WIRE_RECODE; kernels.hip.h: wire_recode_kernel).
//
// Product code.  The canonical walk (wire_dev.h) vouches only for bytes that are exactly what proto.Marshal emits, because
// only then is "the bytes minus field 3" the signed PayloadNoSig.  The reference, however, signs and checks
// proto.Marshal(clone with Signature = nil) of whatever proto.Unmarshal DECODED (messages/proto/helper.go:12-27): fields out
// of order, padded varints, explicit defaults and repeated fields all decode, and the signature covers the canonical
// re-encoding.  This walk decodes such a row tolerantly into a small record — values, plus where From, Signature, proposal
// hash and committed seal lie in the source — and hashes the canonical re-encoding without ever building it: Keccak absorbs
// a short list of segments, literal header bytes the lane builds and slices of the source.
//
// THE RECODE CLASS (the same rule at the three levels of a flat message: IbftMessage, View, Prepare / Commit body):
//   * every tag is ONE byte and names a field of that message with that field's wire type — IbftMessage: 1, 2, 3, 6, 7 LEN,
//     4 VARINT; View: 1, 2 VARINT; body: 1 LEN, 2 LEN in a CommitMessage only.  Field 5 or 8 anywhere, any other field
//     number, a wrong wire type, a multi-byte tag: out of class;
//   * varint VALUES are 1 to 10 bytes, LENGTH PREFIXES 1 to 5 bytes, padding allowed; a tenth value byte above 1, an
//     eleventh value byte, a sixth length byte, a length that leaves its enclosing message: out of class;
//   * fields in any order, any number of times: the last scalar / bytes occurrence wins, occurrences of View merge field by
//     field (a present but empty View stays, `0a 00`), an occurrence of the other oneof member discards what the earlier
//     member held, a further occurrence of the same member merges into it;
//   * explicit zero scalars and empty byte strings are defaults: they vanish in the re-encoding (an empty signature is no
//     signature);
//   * after decoding, the canonical walk's own limits: type ≤ 255 (of the decoded 64-bit value), proposal hash ≤ 32 bytes.
// A row outside the class is left exactly as the canonical walk wrote it: NEEDS_HOST.  The restrictions (one-byte tags, no
// 5 / 8, the untruncated type, length prefixes of at most five bytes) are where decoders may differ; unknown fields are out
// because Go re-emits them.
//
// The canonical re-encoding is never longer than the source: each surviving field costs at most what one of its
// occurrences cost (tests/test_wire_recode_model.py asserts it over the corpus).
#pragma once
#include "wire_dev.h"

namespace wire {

// varint of 1 to 10 bytes at m[pos..end), padding allowed; false: truncated, an eleventh byte, a tenth byte above 1
HD bool read_varint_any(const uint8_t *m, uint32_t end, uint32_t &pos, uint64_t &v) {
  v = 0;
  for (int i = 0; i < 10; i++) {
    if (pos >= end) return false;
    const uint8_t b = m[pos++];
    if (i == 9 && b > 1) return false;
    v |= (uint64_t)(b & 0x7Fu) << (7 * i);
    if (!(b & 0x80u)) return true;
  }
  return false;
}
// length prefix of 1 to 5 bytes, padding allowed (no length that fits a message needs more; decoders differ on longer ones:
// upb refuses them, Go's protowire takes ten); false: truncated, a sixth byte, a body that leaves the enclosing message
HD bool read_len_any(const uint8_t *m, uint32_t end, uint32_t &pos, uint32_t &len) {
  uint64_t l = 0;
  for (int i = 0;; i++) {
    if (i == 5 || pos >= end) return false;
    const uint8_t b = m[pos++];
    l |= (uint64_t)(b & 0x7Fu) << (7 * i);
    if (!(b & 0x80u)) break;
  }
  if (l > (uint64_t)(end - pos)) return false;
  len = (uint32_t)l;
  return true;
}

// what a message of the class decodes to; positions are offsets into the source bytes
struct recode_rec {
  uint64_t height, round, type;
  uint32_t from_pos, from_len, sig_pos, sig_len, hash_pos, hash_len, seal_pos, seal_len;
  uint8_t has_view, kind;  // KIND_NONE / KIND_PREPARE / KIND_COMMIT
};

// false: outside the class (or beyond the canonical walk's limits)
HD bool recode_decode(const uint8_t *m, uint32_t n, recode_rec &r) {
  r.height = r.round = r.type = 0;
  r.from_pos = r.from_len = r.sig_pos = r.sig_len = r.hash_pos = r.hash_len = r.seal_pos = r.seal_len = 0;
  r.has_view = 0;
  r.kind = KIND_NONE;
  uint32_t pos = 0;
  while (pos < n) {
    const uint8_t tag = m[pos++];
    const uint32_t f = tag >> 3, wt = tag & 7u;
    if (tag & 0x80u) return false;
    if (f == 4) {
      if (wt != 0 || !read_varint_any(m, n, pos, r.type)) return false;
      continue;
    }
    if (!(f == 1 || f == 2 || f == 3 || f == 6 || f == 7) || wt != 2) return false;
    uint32_t len;
    if (!read_len_any(m, n, pos, len)) return false;
    const uint32_t end = pos + len;
    if (f == 1) {  // View { uint64 height = 1; uint64 round = 2; }: occurrences merge
      r.has_view = 1;
      while (pos < end) {
        const uint8_t t = m[pos++];
        uint64_t v;
        if ((t != 0x08u && t != 0x10u) || !read_varint_any(m, end, pos, v)) return false;
        if (t == 0x08u) r.height = v; else r.round = v;
      }
    } else if (f == 2) {
      r.from_pos = pos;
      r.from_len = len;
    } else if (f == 3) {
      r.sig_pos = pos;
      r.sig_len = len;
    } else {  // PrepareMessage { bytes proposal_hash = 1; }  CommitMessage { …; bytes committed_seal = 2; }
      if (r.kind != f) r.hash_len = r.seal_len = 0;  // another member of the oneof: the earlier one is gone
      r.kind = (uint8_t)f;
      while (pos < end) {
        const uint8_t t = m[pos++];
        uint32_t l;
        if ((t != 0x0Au && !(t == 0x12u && f == 7)) || !read_len_any(m, end, pos, l)) return false;
        if (t == 0x0Au) {
          r.hash_pos = pos;
          r.hash_len = l;
        } else {
          r.seal_pos = pos;
          r.seal_len = l;
        }
        pos += l;
      }
    }
    pos = end;
  }
  return r.type <= 255 && r.hash_len <= 32;
}

// minimal varint of v appended to out; returns the new length
HD uint32_t put_varint(uint8_t *out, uint32_t k, uint64_t v) {
  while (v >= 0x80u) {
    out[k++] = (uint8_t)(v | 0x80u);
    v >>= 7;
  }
  out[k++] = (uint8_t)v;
  return k;
}
HD uint32_t varint_size(uint64_t v) {
  uint32_t k = 1;
  while (v >= 0x80u) {
    v >>= 7;
    k++;
  }
  return k;
}

// PayloadNoSig of the decoded message as six segments, literal and source bytes in turn:
//   lit[0 .. l0)   View, the tag and length of From          m[from)
//   lit[l0 .. l1)  type, the tag and length of the payload, the tag and length of the hash      m[hash)
//   lit[l1 .. l2)  the tag and length of the seal            m[seal)
constexpr int RECODE_SEGS = 6;
constexpr uint32_t RECODE_LIT_BYTES = 64;  // 2 + 22 + 6, 3 + 6 + 2, 6
struct recode_segs {
  const uint8_t *p[RECODE_SEGS];
  uint32_t n[RECODE_SEGS];
  uint32_t total;
};
HD void recode_segments(const uint8_t *m, const recode_rec &r, uint8_t *lit, recode_segs &s) {
  uint32_t k = 0;
  if (r.has_view) {
    lit[k++] = 0x0Au;
    lit[k++] = (uint8_t)((r.height ? 1u + varint_size(r.height) : 0u) + (r.round ? 1u + varint_size(r.round) : 0u));  // ≤ 22
    if (r.height) {
      lit[k++] = 0x08u;
      k = put_varint(lit, k, r.height);
    }
    if (r.round) {
      lit[k++] = 0x10u;
      k = put_varint(lit, k, r.round);
    }
  }
  if (r.from_len) {
    lit[k++] = 0x12u;
    k = put_varint(lit, k, r.from_len);
  }
  const uint32_t l0 = k;
  if (r.type) {
    lit[k++] = 0x20u;
    k = put_varint(lit, k, r.type);
  }
  if (r.kind != KIND_NONE) {
    const uint32_t body = (r.hash_len ? 2u + r.hash_len : 0u) + (r.seal_len ? 1u + varint_size(r.seal_len) + r.seal_len : 0u);
    lit[k++] = (uint8_t)((r.kind << 3) | 2u);
    k = put_varint(lit, k, body);
    if (r.hash_len) {
      lit[k++] = 0x0Au;
      lit[k++] = (uint8_t)r.hash_len;  // ≤ 32
    }
  }
  const uint32_t l1 = k;
  if (r.kind != KIND_NONE && r.seal_len) {
    lit[k++] = 0x12u;
    k = put_varint(lit, k, r.seal_len);
  }
  const uint32_t l2 = k;
  const bool body = r.kind != KIND_NONE;
  s.p[0] = lit;              s.n[0] = l0;
  s.p[1] = m + r.from_pos;   s.n[1] = r.from_len;
  s.p[2] = lit + l0;         s.n[2] = l1 - l0;
  s.p[3] = m + r.hash_pos;   s.n[3] = body ? r.hash_len : 0u;
  s.p[4] = lit + l1;         s.n[4] = l2 - l1;
  s.p[5] = m + r.seal_pos;   s.n[5] = body ? r.seal_len : 0u;
  s.total = 0;
  for (int i = 0; i < RECODE_SEGS; i++) s.total += s.n[i];
}

// Keccak-256 of the concatenation of the segments, consumed in order
HD void hash_segments(const recode_segs &s, uint64_t out4[4]) {
  uint64_t st[25];
#pragma unroll
  for (int i = 0; i < 25; i++) st[i] = 0;
  uint32_t done = 0, k = 0, at = 0;  // segment and position in it of the next byte
  for (;;) {
    const uint32_t left = s.total - done;
    const bool last = left < 136;
    for (int i = 0; i < 17; i++) {
      uint64_t w = 0;
      for (int b = 0; b < 8; b++) {
        const uint32_t off = 8 * i + b;
        uint64_t byte = 0;
        if (off < left) {
          while (at == s.n[k]) {  // (off < left: a byte is still to come, k stays below RECODE_SEGS)
            k++;
            at = 0;
          }
          byte = s.p[k][at++];
        }
        if (last && off == left) byte ^= 0x01u;
        if (last && off == 135) byte ^= 0x80u;
        w |= byte << (8 * b);
      }
      st[i] ^= w;
    }
    keccak::f1600(st);
    if (last) break;
    done += 136;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) out4[i] = st[i];
}

// One row the canonical walk marked NEEDS_HOST.  In the class: every output becomes what process_row writes for the
// canonical re-encoding of the same message (signature kept), but pad[0] = 1 (ibft_wire_row_t: recoded); returns true.
// Outside: nothing is written; returns false.
HD bool recode_row(const uint8_t *m, uint32_t n, row_info *ri_out, uint8_t *digest32, uint8_t *sig65, uint8_t *from20,
                   uint8_t *seal65, uint8_t *pre_flag) {
  recode_rec r;
  if (!recode_decode(m, n, r)) return false;
  row_info ri;
  ri.height = r.height;
  ri.round = r.round;
  ri.status = STATUS_OK;
  ri.type = (uint8_t)r.type;
  ri.payload_kind = r.kind;
  ri.has_view = r.has_view;
  ri.hash_len = (uint8_t)r.hash_len;
  ri.seal_len = r.seal_len > 255 ? 255 : (uint8_t)r.seal_len;
  ri.from_len = r.from_len > 255 ? 255 : (uint8_t)r.from_len;
  ri.sig_len = r.sig_len > 255 ? 255 : (uint8_t)r.sig_len;
  for (uint32_t i = 0; i < 20; i++) ri.from[i] = i < r.from_len ? m[r.from_pos + i] : 0;
  for (uint32_t i = 0; i < 32; i++) ri.proposal_hash[i] = i < r.hash_len ? m[r.hash_pos + i] : 0;
  ri.pad[0] = 1;
  ri.pad[1] = ri.pad[2] = ri.pad[3] = 0;
  *ri_out = ri;
  uint8_t lit[RECODE_LIT_BYTES];
  recode_segs s;
  recode_segments(m, r, lit, s);
  uint64_t d[4];
  hash_segments(s, d);
  for (int j = 0; j < 4; j++)
    for (int b = 0; b < 8; b++) digest32[8 * j + b] = (uint8_t)(d[j] >> (8 * b));
  const bool sig_ok = r.sig_len == 65, from_ok = r.from_len == 20;
  for (int i = 0; i < 65; i++) sig65[i] = sig_ok ? m[r.sig_pos + i] : 0;
  for (int i = 0; i < 20; i++) from20[i] = from_ok ? ri.from[i] : 0;
  const bool seal_ok = r.kind == KIND_COMMIT && r.seal_len == 65;
  for (int i = 0; i < 65; i++) seal65[i] = seal_ok ? m[r.seal_pos + i] : 0;
  *pre_flag = (uint8_t)((sig_ok ? 0 : 2) | (from_ok ? 0 : 2));
  return true;
}

}  // namespace wire
