// host_qtab_glv_harness.hip — TEST-ONLY: the GLV table form of the warm path (verify_dev.h: qglv_bias, qglv_operand_of,
// qglv_point, qtab_build_window<QTAB_GLV>, verify_known<QTAB_GLV>; wave_fe_dev.h: verify_known_wave<QTAB_GLV>) on the CPU, so
// that tests/test_qtab_glv_host.py and tests/test_dev_warm_glv_edges_host.py can check the exact device source without a GPU.
// The lane form runs as plain host code, the wavefront form through the 64-coroutine lockstep emulator of wave_emul.h.
// Built with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#define IBFT_GTAB_BITS 8
#define IBFT_WAVE_EMUL 1
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "wave_fe_dev.h"

using secp::u256;

static std::vector<uint32_t> g_gtab;

namespace {

struct vk_job {
  const uint32_t *qtab;
  const uint8_t *hash32, *sig65;
  uint32_t flags;
  int *ok;  // [64]
};
void lane_vk(void *vp) {
  vk_job *j = (vk_job *)vp;
  u256 z = secp::from_be32(j->hash32), r = secp::from_be32(j->sig65), s = secp::from_be32(j->sig65 + 32);
  bool ok = wv::verify_known_wave<ibftk::QTAB_GLV>(g_gtab.data(), j->qtab, z, r, s, j->sig65[64], j->flags);
  j->ok[wave_emul::lane()] = ok ? 1 : 0;
}

// a 128-bit (or, biased, 129-bit) value as five little-endian dwords
u256 from_words5(const uint32_t *w) {
  u256 k = secp::zero256();
  for (int i = 0; i < 5; i++) k.v[i] = w[i];
  return k;
}

}  // namespace

extern "C" {

int qgh_gtab_bits(void) { return ibftk::GTAB_BITS; }
uint32_t qgh_slot_dwords(void) { return (uint32_t)ibftk::qtab_slot_dwords<ibftk::QTAB_GLV>(); }
uint32_t qgh_points(void) { return ibftk::QGLV_POINTS; }

void qgh_init_gtab(void) {
  if (!g_gtab.empty()) return;
  g_gtab.resize((size_t)ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES * ibftk::GTAB_ENTRY_DWORDS);
  for (int t = 0; t < ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES; t++)
    ibftk::gtab_entry(t / ibftk::GTAB_ENTRIES, t % ibftk::GTAB_ENTRIES, g_gtab.data() + (size_t)ibftk::GTAB_ENTRY_DWORDS * t);
}

// the split the kernels run on u2 (32 BE bytes, < n): the halves' magnitudes as 16 LE bytes each, the signs
void qgh_split(const uint8_t *u2_be32, uint8_t *k1_le16, uint8_t *k2_le16, int *neg) {
  const secp::glv_split sp = secp::sc_split_lambda(secp::from_be32(u2_be32));
  memcpy(k1_le16, sp.k1.v, 16);
  memcpy(k2_le16, sp.k2.v, 16);
  neg[0] = sp.neg1 ? 1 : 0;
  neg[1] = sp.neg2 ? 1 : 0;
  neg[2] = (sp.k1.v[4] | sp.k1.v[5] | sp.k1.v[6] | sp.k1.v[7] | sp.k2.v[4] | sp.k2.v[5] | sp.k2.v[6] | sp.k2.v[7]) ? 1 : 0;  // a half ≥ 2^128
}

// The recoding of a half k < 2^128 (16 LE bytes), read out BOTH ways the kernels read it: by position (qglv_point, the group
// and wavefront forms) and from a shift register (the lane form).  Per window w: digit[w] (signed; the top one unsigned),
// index[w] (entry of the table), flags[w] = nz | beta << 1 | neg << 2.  `lambda`: recode as the k2 half; half_neg its sign.
// Returns 0 when the two readings agree everywhere.
int qgh_recode(const uint8_t *k_le16, int lambda, int half_neg, int32_t *digit, uint32_t *index, uint32_t *flags) {
  uint32_t w4[5] = {0, 0, 0, 0, 0};
  memcpy(w4, k_le16, 16);
  const u256 k = from_words5(w4);
  const u256 b = ibftk::qglv_bias(k);
  const u256 zero = secp::zero256();
  u256 sh = b;
  int bad = 0;
  for (int w = 0; w < ibftk::QGLV_WINDOWS; w++) {
    const ibftk::qglv_operand byp = lambda ? ibftk::qglv_point(ibftk::QGLV_WINDOWS + w, zero, b, false, half_neg != 0)
                                           : ibftk::qglv_point(w, b, zero, half_neg != 0, false);
    const ibftk::qglv_operand bys = ibftk::qglv_operand_of(w, sh.v[0], half_neg != 0, lambda != 0);
    if (byp.index != bys.index || byp.nz != bys.nz || byp.beta != bys.beta || byp.neg != bys.neg) bad = 1;
    secp::shr_bits<8>(sh);
    const uint32_t mag = byp.nz ? byp.index - (uint32_t)(w * ibftk::QGLV_ENTRIES) + 1u : 0u;
    digit[w] = (byp.neg != (half_neg != 0)) ? -(int32_t)mag : (int32_t)mag;
    index[w] = byp.index;
    flags[w] = (byp.nz ? 1u : 0u) | (byp.beta ? 2u : 0u) | (byp.neg ? 4u : 0u);
  }
  return bad;
}

// the GLV table of the public key X‖Y (64 BE bytes): qgh_slot_dwords() dwords
void qgh_build_qtab(const uint8_t *pub64, uint32_t *qtab) {
  secp::aff Q;
  Q.x = secp::fe_from_u256(secp::from_be32(pub64));
  Q.y = secp::fe_from_u256(secp::from_be32(pub64 + 32));
  for (int w = 0; w < ibftk::QGLV_WINDOWS; w++)
    ibftk::qtab_build_window<ibftk::QTAB_GLV>(Q, w, qtab + ibftk::qtab_window_dwords<ibftk::QTAB_GLV>(w), true);
}
// entry m (1 …) of window w as X‖Y
void qgh_entry(const uint32_t *qtab, int w, int m, uint8_t *out64) {
  const secp::aff a = ibftk::load_affine(qtab + ibftk::qtab_window_dwords<ibftk::QTAB_GLV>(w) + (size_t)ibftk::GTAB_ENTRY_DWORDS * (m - 1));
  secp::to_be32(out64, secp::fe_to_u256(a.x));
  secp::to_be32(out64 + 32, secp::fe_to_u256(a.y));
}

int qgh_verify_lane(const uint32_t *qtab, const uint8_t *hash32, const uint8_t *sig65, uint32_t flags) {
  return ibftk::verify_known<ibftk::QTAB_GLV>(g_gtab.data(), qtab, secp::from_be32(hash32), secp::from_be32(sig65),
                                              secp::from_be32(sig65 + 32), sig65[64], flags)
             ? 1
             : 0;
}
void qgh_verify_wave(const uint32_t *qtab, const uint8_t *hash32, const uint8_t *sig65, uint32_t flags, int *ok64) {
  vk_job j{qtab, hash32, sig65, flags, ok64};
  wave_emul::run(lane_vk, &j);
}

}  // extern "C"
