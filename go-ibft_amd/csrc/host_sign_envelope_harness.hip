// host_sign_envelope_harness.hip — TEST-ONLY: sign_envelope_dev.h (the four steps of ibft_sign_envelopes_wire: head, body copy,
// digest in both forms, signature) on the CPU, so that tests/test_sign_envelopes_host.py can check the exact device source without
// a GPU.  The wavefront form of the digest runs through the 64-coroutine lockstep emulator of wave_emul.h.  Built with hipcc's
// host pass; never linked into libibftgpu.so, never a fallback.
#define IBFT_GTAB_BITS 8  // small table for the CPU harness (see recover_dev.h)
#define IBFT_WAVE_EMUL 1
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sign_envelope_dev.h"
#include "host_gtab.h"

namespace {

// what is LDS on the device: memory shared by the 64 coroutines
alignas(16) uint64_t g_A[32], g_B[32];
struct wave_job {
  const uint8_t *m;
  uint32_t len, cut;
  uint64_t out[4];
};
void lane_digest(void *p) {
  wave_job *j = (wave_job *)p;
  const uint32_t lane = cw::lane_id();
  const uint64_t w = ibftk::envelope_digest_wave(j->m, j->len, j->cut, lane, g_A, g_B);
  if (lane < 4) j->out[lane] = w;
}

}  // namespace

extern "C" {

uint32_t dev_envelope_cut(uint64_t height, uint64_t round) { return ibftk::envelope_cut(height, round); }
// View ‖ From as put_message_front writes them: out holds 46 bytes; returns the offset behind From
uint32_t dev_message_front(uint64_t height, uint64_t round, const uint8_t *addr20, uint8_t *out) {
  uint32_t addr[5];
  memcpy(addr, addr20, 20);
  return ibftk::put_message_front(out, height, round, addr);
}
uint32_t dev_envelope_head_len(uint32_t type, uint64_t height, uint64_t round, uint32_t body_len) {
  return ibftk::envelope_head_len(type, height, round, body_len);
}
uint64_t dev_envelope_wire_len(uint32_t type, uint64_t height, uint64_t round, uint32_t body_len) {
  return ibftk::envelope_wire_len(type, height, round, body_len);
}

// One row as the kernels run it, step by step: the message goes to wire[dst_at, dst_at + its length), the body comes from
// body[src_at, src_at + body_len).  `wire` and `body` must be 16-byte aligned (hipMalloc gives that on the device), body must
// carry 16 readable bytes behind src_at + body_len, wire 16 behind the message.  form: 1 = the lane digest, 64 = the wavefront
// digest.  Returns the row's ok flag; *wire_len the message's length, digest32 what was signed, from20 the address.
int dev_sign_envelope(uint32_t nonce, uint32_t form, const uint8_t *sk32, uint32_t type, uint64_t height, uint64_t round, const uint8_t *body,
                      uint32_t src_at, uint32_t body_len, uint8_t *wire, uint32_t dst_at, uint32_t *wire_len, uint8_t *digest32,
                      uint8_t *from20) {
  gtab_init();
  uint8_t sk[32];
  memcpy(sk, sk32, 32);
  // 1. the head
  ibftk::u256 d;
  const bool key_ok = ibftk::sign_key(sk, d);
  uint32_t addr[5];
  ibftk::sign_address(g_gtab.data(), d, key_ok, addr);
  uint64_t buf[ibftk::ENVELOPE_HEAD_WORDS];
  const uint32_t head = ibftk::envelope_head(reinterpret_cast<uint8_t *>(buf), type, height, round, addr, body_len);
  if (head != ibftk::envelope_head_len(type, height, round, body_len)) return -1;
  ibftk::store_envelope_head(wire + dst_at, reinterpret_cast<const uint8_t *>(buf), head);
  // 2. the body, every thread of every piece in turn
  const uint32_t pieces = ibftk::envelope_copy_pieces(dst_at + head, body_len);
  for (uint32_t p = 0; p < pieces; p++)
    for (uint32_t t = 0; t < ibftk::ENVELOPE_COPY_THREADS; t++) ibftk::copy_body_piece(wire, body, dst_at + head, src_at, body_len, p, t);
  // 3. the digest of what was stored
  const uint32_t len = head + body_len, cut = ibftk::envelope_cut(height, round);
  uint64_t dg[4];
  if (form == 64) {
    wave_job j{wire + dst_at, len, cut, {0, 0, 0, 0}};
    wave_emul::run(lane_digest, &j);
    memcpy(dg, j.out, 32);
  } else {
    ibftk::envelope_digest_lane(wire + dst_at, len, cut, true, dg);
  }
  memcpy(digest32, dg, 32);
  // 4. the signature
  ibftk::u256 r, s;
  uint32_t v;
  const bool ok = nonce == (uint32_t)ibftk::SIGN_NONCE_RFC6979
                      ? ibftk::sign_digest<ibftk::SIGN_NONCE_RFC6979>(g_gtab.data(), sk, digest32, r, s, v)
                      : ibftk::sign_digest<ibftk::SIGN_NONCE_KECCAK>(g_gtab.data(), sk, digest32, r, s, v);
  ibftk::put_sig65(wire + dst_at + cut + 2, r, s, v);
  *wire_len = len;
  memcpy(from20, addr, 20);
  return ok ? 1 : 0;
}

// the two digest forms alone, over any stored message (len bytes at m, signature field at [cut, cut + 67))
void dev_envelope_digest(uint32_t form, const uint8_t *m, uint32_t len, uint32_t cut, uint8_t *out32) {
  uint64_t dg[4];
  if (form == 64) {
    wave_job j{m, len, cut, {0, 0, 0, 0}};
    wave_emul::run(lane_digest, &j);
    memcpy(dg, j.out, 32);
  } else {
    ibftk::envelope_digest_lane(m, len, cut, true, dg);
  }
  memcpy(out32, dg, 32);
}

// the body copy alone (bounds and alignment tests)
void dev_envelope_copy(uint8_t *wire, const uint8_t *body, uint32_t dst_at, uint32_t src_at, uint32_t len) {
  const uint32_t pieces = ibftk::envelope_copy_pieces(dst_at, len);
  for (uint32_t p = 0; p < pieces; p++)
    for (uint32_t t = 0; t < ibftk::ENVELOPE_COPY_THREADS; t++) ibftk::copy_body_piece(wire, body, dst_at, src_at, len, p, t);
}

}  // extern "C"
