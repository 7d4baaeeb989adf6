// host_wire_recode_harness.hip — TEST-ONLY: wire_recode_dev.h (the tolerant walk of IBFT_FLAG_WIRE_RECODE) on the CPU, so that
// tests/test_dev_wire_recode_host.py can check the exact device source without a GPU.  wrh_run does per row what the two
// kernels do one after the other: the canonical walk (wire_parse_kernel), then — for a row it marked NEEDS_HOST — the recode
// walk (wire_recode_kernel).  Built with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "wire_recode_dev.h"

extern "C" {

// Row i is wire[off[i] .. off[i+1]).  Two sets of columns, each n rows of row_info (80 B) / digest (32) / sig (65) / from (20) /
// seal (65) / pre_flag (1): `canon` as the canonical walk leaves them, `out` after the recode walk.  recoded[i] = what
// recode_row returned (0 for a row the canonical walk accepted: it is not called).
void wrh_run(const uint8_t *wire_bytes, const uint32_t *off, uint32_t n, uint8_t *canon_rows, uint8_t *canon_digest, uint8_t *canon_sig,
             uint8_t *canon_from, uint8_t *canon_seal, uint8_t *canon_pre, uint8_t *out_rows, uint8_t *out_digest, uint8_t *out_sig,
             uint8_t *out_from, uint8_t *out_seal, uint8_t *out_pre, uint8_t *recoded) {
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t *m = wire_bytes + off[i];
    const uint32_t len = off[i + 1] - off[i];
    wire::row_info ri;
    wire::process_row(m, len, &ri, canon_digest + 32ull * i, canon_sig + 65ull * i, canon_from + 20ull * i, canon_seal + 65ull * i,
                      canon_pre + i);
    memcpy(canon_rows + 80ull * i, &ri, 80);
    memcpy(out_digest + 32ull * i, canon_digest + 32ull * i, 32);
    memcpy(out_sig + 65ull * i, canon_sig + 65ull * i, 65);
    memcpy(out_from + 20ull * i, canon_from + 20ull * i, 20);
    memcpy(out_seal + 65ull * i, canon_seal + 65ull * i, 65);
    out_pre[i] = canon_pre[i];
    recoded[i] = 0;
    if (ri.status == wire::STATUS_NEEDS_HOST)
      recoded[i] = wire::recode_row(m, len, &ri, out_digest + 32ull * i, out_sig + 65ull * i, out_from + 20ull * i, out_seal + 65ull * i,
                                    out_pre + i)
                       ? 1
                       : 0;
    memcpy(out_rows + 80ull * i, &ri, 80);
  }
}

}  // extern "C"
