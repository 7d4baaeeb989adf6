// host_sign_message_harness.hip — TEST-ONLY: sign_message_dev.h (the row of sign_message_lane_kernel: encode, hash, sign, store)
// on the CPU, so that tests/test_sign_messages_host.py can check the exact device source without a GPU.  Built with hipcc's
// host pass; never linked into libibftgpu.so, never a fallback.
#define IBFT_GTAB_BITS 8  // small table for the CPU harness (see recover_dev.h)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sign_message_dev.h"
#include "host_gtab.h"

extern "C" {

uint32_t dev_message_payload_len(uint32_t type, uint64_t height, uint64_t round) { return ibftk::message_payload_len(type, height, round); }
uint32_t dev_message_wire_len(uint32_t type, uint64_t height, uint64_t round) { return ibftk::message_wire_len(type, height, round); }

// One row as the kernel runs it.  suffix / suffix_len: the seal-digest convention (suffix = NULL: the identity), turned into
// the nine words exactly as ibft_set_seal_digest does.  out_wire: ≥ 218 bytes, out_payload: ≥ 152 bytes.  Returns the row's ok
// flag; *wire_len and *payload_len the two lengths.
int dev_sign_message(uint32_t nonce, const uint8_t *sk32, uint32_t type, uint64_t height, uint64_t round, const uint8_t *hash32,
                     const uint8_t *suffix, uint32_t suffix_len, uint8_t *out_wire, uint32_t *wire_len, uint8_t *out_payload,
                     uint32_t *payload_len, uint8_t *from20) {
  gtab_init();
  uint8_t block[72] = {0};
  uint64_t words[9];
  if (suffix) {
    if (suffix_len > 64) return -1;
    if (suffix_len) memcpy(block, suffix, suffix_len);
    block[suffix_len] = 0x01;
  }
  memcpy(words, block, sizeof words);
  uint64_t buf[ibftk::SIGN_MESSAGE_BUF_WORDS];
  uint8_t sk[32], hs[32];
  memcpy(sk, sk32, 32);
  memcpy(hs, hash32, 32);
  const ibftk::message_row m =
      nonce == (uint32_t)ibftk::SIGN_NONCE_RFC6979
          ? ibftk::sign_message_row<ibftk::SIGN_NONCE_RFC6979>(g_gtab.data(), sk, type, height, round, hs, suffix ? 1u : 0u, words, buf)
          : ibftk::sign_message_row<ibftk::SIGN_NONCE_KECCAK>(g_gtab.data(), sk, type, height, round, hs, suffix ? 1u : 0u, words, buf);
  ibftk::store_message(out_wire, buf, m);
  memcpy(out_payload, buf, m.len);
  *payload_len = m.len;
  *wire_len = m.len + ibftk::SIGN_MESSAGE_SIG_FIELD;
  memcpy(from20, m.addr, 20);
  return m.ok ? 1 : 0;
}

}  // extern "C"
