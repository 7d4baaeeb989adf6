// host_sign_nonce_harness.hip — TEST-ONLY: sha256_dev.h and the RFC 6979 nonce rule of sign_dev.h on the CPU, so that
// tests/test_sign_rfc6979_host.py can check the exact device source without a GPU: the compression function, HMAC in its
// three message shapes, the DRBG's candidates (the reseed step included) and the whole signing row with its reject_mask
// seam.  Built with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#define IBFT_GTAB_BITS 8  // small table for the CPU harness (see recover_dev.h)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sign_dev.h"
#include "host_gtab.h"

using secp::u256;

static uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
static sha256::state words32(const uint8_t *p) {
  return sha256::state{be32(p), be32(p + 4), be32(p + 8), be32(p + 12), be32(p + 16), be32(p + 20), be32(p + 24), be32(p + 28)};
}
static void bytes32(uint8_t *out, const sha256::state &s) {
  const uint32_t w[8] = {s.a, s.b, s.c, s.d, s.e, s.f, s.g, s.h};
  for (int i = 0; i < 8; i++)
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(w[i] >> (8 * (3 - b)));
}

extern "C" {

// state8: the chaining value H0 … H7 (updated in place); block16: the block as sixteen big-endian words
void dev_sha256_compress(uint32_t *state8, const uint32_t *block16) {
  const uint32_t *m = block16;
  const sha256::state s = sha256::compress(sha256::state{state8[0], state8[1], state8[2], state8[3], state8[4], state8[5], state8[6], state8[7]},
                                           sha256::block{m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11], m[12], m[13], m[14], m[15]});
  state8[0] = s.a, state8[1] = s.b, state8[2] = s.c, state8[3] = s.d, state8[4] = s.e, state8[5] = s.f, state8[6] = s.g, state8[7] = s.h;
}

// HMAC-SHA-256(key32, msg) in the three shapes the device code has: len 32 (V), 33 (V ‖ 0x00: msg[32] must be 0) and
// 97 (V ‖ tag ‖ x ‖ h1: msg[32] must be 0 or 1).  Returns 1, or 0 (out32 untouched) for any other shape.
int dev_hmac32(const uint8_t *key32, const uint8_t *msg, uint32_t len, uint8_t *out32) {
  const sha256::hmac_key k = sha256::hmac_midstates(words32(key32));
  const sha256::state v = words32(msg);
  if (len == 32) {
    bytes32(out32, sha256::hmac_v(k, v));
  } else if (len == 33 && msg[32] == 0) {
    bytes32(out32, sha256::hmac_v_00(k, v));
  } else if (len == 97 && msg[32] <= 1) {
    bytes32(out32, sha256::hmac_v_tag_x_h(k, v, msg[32], words32(msg + 33), words32(msg + 65)));
  } else {
    return 0;
  }
  return 1;
}

// the first m candidates of the DRBG for (sk32, digest32) as sign_row seeds it (h1 = the digest mod n), a reseed between two
// candidates: out = m × 32 big-endian bytes
void dev_rfc6979_candidates(const uint8_t *sk32, const uint8_t *digest32, uint32_t m, uint8_t *out) {
  u256 z = secp::from_be32(digest32);
  secp::sub_const_if(z, secp::geq_const(z, secp::NL()), secp::NL());
  ibftk::rfc6979_drbg g;
  g.init(secp::from_be32(sk32), z);
  for (uint32_t t = 0; t < m; t++) {
    if (t) g.reseed();
    secp::to_be32(out + 32ull * t, g.candidate());
  }
}

// the signing row under the RFC 6979 rule: sig65 = r ‖ s ‖ v and the signer's address; returns 0 (zeros out) for an unusable key.
// reject_mask: bit t set treats candidate t as unusable.
int dev_sign_rfc6979(const uint8_t *sk32, const uint8_t *digest32, uint32_t reject_mask, uint8_t *sig65, uint8_t *addr20) {
  gtab_init();
  u256 r, s;
  uint32_t v, a[5];
  const bool ok = ibftk::sign_row<ibftk::SIGN_NONCE_RFC6979>(g_gtab.data(), sk32, digest32, r, s, v, a, reject_mask);
  ibftk::put_sig65(sig65, r, s, v);
  memcpy(addr20, a, 20);
  return ok ? 1 : 0;
}

}  // extern "C"
