// verify_dev.h — the "warm" path: ECDSA verification against per-validator fixed-base tables.
//
// Product code.  IsValidCommittedSeal / IsValidValidator ask "was this signed by the key whose
// address is msg.From?" (/root/reference/core/backend.go:41-45, 53-55).  The cold path answers
// by recovering the key (recover_dev.h): one square root, a 128-doubling variable-base
// multiplication and two inversions — ≈676 k VALU instructions, inherently sequential.  But a
// validator set is small and stable: once a validator's public key Q has been recovered ONCE
// (and hashed to its address), every later signature (z, r, s, v) from it can be checked as
//
//     R' = (z/s)·G + (r/s)·Q ,   accept  ⇔  R' ≠ ∞  ∧  R'.x = r  ∧  parity(R'.y) = v
//
// which gives the same verdict as recover-and-compare: accept ⇔ the recovered key equals Q
// (a different key with the same address would be a Keccak collision).  Both bases are now
// FIXED, so with per-validator tables Q·e·2^(8w) (32 windows × 256 affine points = 655 KB per
// validator; 1 024 validators = 0.67 GB, 65 536 = 43 GB of the 288 GB HBM) there are no
// doublings at all: 32 + 16 table points are summed.  That sum is a reduction, so several lanes
// can share one signature: G lanes fetch their share of the points and a log2(G)-level butterfly of
// point additions finishes it (verify_known_group_kernel, kernels.hip.h); with one wavefront per
// signature the sum runs in the row layout of wave_fe_dev.h (verify_known_wave); the lane-per-
// signature form below is used when there are enough rows to fill the chip anyway.
#pragma once
#include "recover_dev.h"

namespace ibftk {

constexpr int QTAB_WINDOWS = 32;  // 8-bit windows over u2
constexpr int QTAB_ENTRIES = 256;
constexpr size_t QTAB_DWORDS_PER_VALIDATOR = (size_t)QTAB_WINDOWS * QTAB_ENTRIES * GTAB_ENTRY_DWORDS;

// ---- the GLV table form (opt-in: IBFT_QTAB_FORM=glv) ---------------------------------------------------------------------
// With u2 = ±k1 ± k2·λ (secp::sc_split_lambda, |k1|, |k2| < 2^128) and λ·(x, y) = (β·x, y), the λ half needs no table of
// its own: u2·Q = ±Σ d1_j·2^(8j)·Q ± Σ d2_j·2^(8j)·λQ reads the SAME entries, x multiplied by β for the second sum.  So 16
// windows over 128 bits replace 32 over 256, and signed digits halve a window.  A half k < 2^128 is recoded without a carry
// chain: b = k + Σ_{i<15} 128·256^i; digit i = byte i of b, minus 128, in [−128, 127] for i < 15; the top digit is b >> 120 in
// [0, 256], unsigned.  Then k = Σ_{i<15} d_i·256^i + top·2^120.
// Entries: windows 0…14 hold m·2^(8w)·Q for m = 1…128, window 15 holds m·2^120·Q for m = 1…256 — 15·128 + 256 = 2 176
// affine points = 174 080 B per validator (the wide form: 655 360 B).  No entry is ∞.  A signature still sums 48 table
// points: 16 of the k1 half, 16 of the k2 half, 16 of G.
// (The split rounds to the nearest lattice point, so a half of a scalar below n stays below 2^127.4 and its top digit below
// 164: entries 164 … 256 of window 15 — 93 points, 4.3 % of the slot — are built and read by no signature.  The layout follows
// the recoding's range, which is what qglv_operand_of can be handed.)
constexpr int QTAB_WIDE = 0, QTAB_GLV = 1;
constexpr int QGLV_WINDOWS = 16;        // 8-bit windows over a 128-bit half
constexpr int QGLV_ENTRIES = 128;       // |digit| of windows 0…14
constexpr int QGLV_TOP_ENTRIES = 256;   // the unsigned top digit
constexpr int QGLV_POINTS = (QGLV_WINDOWS - 1) * QGLV_ENTRIES + QGLV_TOP_ENTRIES;
constexpr size_t QGLV_DWORDS_PER_VALIDATOR = (size_t)QGLV_POINTS * GTAB_ENTRY_DWORDS;
static_assert(QGLV_DWORDS_PER_VALIDATOR * 4 == 174080, "15·128 + 256 affine points of 80 B");
template <int FORM>
__host__ __device__ constexpr size_t qtab_slot_dwords() {
  return FORM == QTAB_GLV ? QGLV_DWORDS_PER_VALIDATOR : QTAB_DWORDS_PER_VALIDATOR;
}
// k + Σ_{i<15} 128·256^i (k < 2^128): 129 bits
__host__ __device__ __forceinline__ u256 qglv_bias(const u256 &k) {
  u256 r = secp::zero256();
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) r.v[i] = secp::addc(i < 4 ? k.v[i] : 0u, i < 3 ? 0x80808080u : (i == 3 ? 0x00808080u : 0u), c);
  return r;
}
// THE helper of the form: one table point of a half as the kernels need it.  `field` holds the bits of the biased half from
// bit 8w on (nine of them are looked at), `half_neg` the sign of the half, `lambda` whether it is the k2 half.
struct qglv_operand {
  uint32_t index;  // entry of the validator's table (|d| = 0: entry of m = 1 of the window, a dummy operand)
  bool nz;         // d ≠ 0: the point is added
  bool beta;       // multiply x by β
  bool neg;        // negate y
};
__host__ __device__ __forceinline__ qglv_operand qglv_operand_of(int w, uint32_t field, bool half_neg, bool lambda) {
  const bool top = w == QGLV_WINDOWS - 1;
  const int d = top ? (int)(field & 511u) : (int)(field & 255u) - 128;
  uint32_t mag = (uint32_t)(d < 0 ? -d : d);
  mag = mag > (uint32_t)QGLV_TOP_ENTRIES ? (uint32_t)QGLV_TOP_ENTRIES : mag;  // (a half below 2^128 never gets here: no index leaves the slot)
  qglv_operand o;
  o.nz = mag != 0;
  o.index = (uint32_t)(w * QGLV_ENTRIES) + (o.nz ? mag : 1u) - 1u;
  o.beta = lambda;
  o.neg = (d < 0) != half_neg;
  return o;
}
// point p of the 32 of u2·Q (0…15: window p of the k1 half, 16…31: window p − 16 of the k2 half), read from the two biased
// halves by position (the lane form shifts its halves instead and calls qglv_operand_of on the low bits)
__host__ __device__ __forceinline__ qglv_operand qglv_point(int p, const u256 &b1, const u256 &b2, bool neg1, bool neg2) {
  const bool lambda = p >= QGLV_WINDOWS;
  const int w = p & (QGLV_WINDOWS - 1);
  const int word = w >> 2, sh = 8 * (w & 3);
  // (p differs from lane to lane: the two words are picked with selects, not by indexing — an indexed half would be laid
  // into the private segment)
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    lo = word == i ? (lambda ? b2.v[i] : b1.v[i]) : lo;
    hi = word == i ? (lambda ? b2.v[i + 1] : b1.v[i + 1]) : hi;
  }
  const uint32_t field = sh == 24 ? (lo >> 24) | (hi << 8) : lo >> sh;
  return qglv_operand_of(w, field, lambda ? neg2 : neg1, lambda);
}
// the operand itself: the loaded entry, x·β for the k2 half (the callers multiply where the step is uniform), y negated
__host__ __device__ __forceinline__ aff qglv_apply(const aff &e, const secp::fe &bx, bool beta, bool neg) {
  aff q;
  q.x = secp::l26_select(beta, bx, e.x);
  q.y = secp::l26_select(neg, secp::fe_neg(e.y, 1), e.y);  // magnitude ≤ 2
  return q;
}

__host__ __device__ __forceinline__ aff load_affine(const uint32_t *__restrict__ e20) {
  const uint4 *e = reinterpret_cast<const uint4 *>(e20);
  uint4 t0 = e[0], t1 = e[1], t2 = e[2], t3 = e[3], t4 = e[4];
  aff q;
  q.x.n[0] = t0.x; q.x.n[1] = t0.y; q.x.n[2] = t0.z; q.x.n[3] = t0.w;
  q.x.n[4] = t1.x; q.x.n[5] = t1.y; q.x.n[6] = t1.z; q.x.n[7] = t1.w;
  q.x.n[8] = t2.x; q.x.n[9] = t2.y; q.y.n[0] = t2.z; q.y.n[1] = t2.w;
  q.y.n[2] = t3.x; q.y.n[3] = t3.y; q.y.n[4] = t3.z; q.y.n[5] = t3.w;
  q.y.n[6] = t4.x; q.y.n[7] = t4.y; q.y.n[8] = t4.z; q.y.n[9] = t4.w;
  return q;
}
__host__ __device__ __forceinline__ void store_affine(uint32_t *__restrict__ e20, const aff &a) {
  for (int i = 0; i < 10; i++) {
    e20[i] = a.x.n[i];
    e20[10 + i] = a.y.n[i];
  }
}

// signature range checks shared by both paths (same list as oracle/secp256k1.c:orc_ecrecover)
__host__ __device__ __forceinline__ bool sig_in_range(const u256 &r, const u256 &s, uint32_t v, uint32_t flags) {
  bool ok = v <= 1;
  ok = ok && !secp::is_zero(r) && !secp::geq_const(r, secp::NL());
  ok = ok && !secp::is_zero(s) && !secp::geq_const(s, secp::NL());
  if (flags & 1u) {
    u256 sm1;
    secp::sub256(sm1, s, secp::one256());
    ok = ok && !secp::geq_const(sm1, secp::NHL());
  }
  return ok;
}

// u1 = z/s, u2 = r/s (mod n), canonical
__host__ __device__ __forceinline__ void verify_scalars(const u256 &z_raw, const u256 &r, const u256 &s, u256 &u1,
                                                        u256 &u2) {
  secp::sc sinv = secp::sc_from_u256(secp::modinv_shared<secp::ModN>(s));
  u1 = secp::sc_canon(secp::sc_mul(secp::sc_from_u256(z_raw), sinv));
  u2 = secp::sc_canon(secp::sc_mul(secp::sc_from_u256(r), sinv));
}

// final check on R' = u1·G + u2·Q
__host__ __device__ __forceinline__ bool verify_finish(const jac &Rp, const u256 &r, uint32_t v) {
  aff A;
  bool fin = secp::jac_to_aff_fast(A, Rp);
  secp::fe rx = secp::fe_from_u256(r);  // r < n < p: canonical limbs
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) diff |= A.x.n[i] ^ rx.n[i];
  return fin && diff == 0 && (A.y.n[0] & 1u) == v;
}

// lane-per-signature form: 32 + GTAB_WINDOWS mixed additions, no doublings
template <int FORM = QTAB_WIDE>
__host__ __device__ __forceinline__ bool verify_known(const uint32_t *__restrict__ gtab,
                                                      const uint32_t *__restrict__ qtab_v, const u256 &z_raw,
                                                      const u256 &r, const u256 &s, uint32_t v, uint32_t flags) {
  bool ok = sig_in_range(r, s, v, flags);
  u256 u1, u2;
  verify_scalars(z_raw, r, s, u1, u2);
  jac acc = secp::jac_inf();
  if constexpr (FORM == QTAB_GLV) {
    // The GLV form: 16 points of the k1 half, 16 of the k2 half, 16 of G, in that order.  Same loop shape as below: the
    // biased halves and u1 are shift registers, the entry of step w + 1 is asked for before the addition of step w runs; the
    // β multiplication and the negation are applied to the entry when its step begins (the load has had an addition's time).
    const secp::glv_split sp = secp::sc_split_lambda(u2);
    u256 b1 = qglv_bias(sp.k1), b2 = qglv_bias(sp.k2), k1 = u1;
    const secp::fe beta = secp::GLV_CONST(1);
    constexpr int POINTS = 2 * QGLV_WINDOWS + GTAB_WINDOWS;
    qglv_operand op = qglv_operand_of(0, b1.v[0], sp.neg1, false);
    const uint32_t *entry = qtab_v + (size_t)GTAB_ENTRY_DWORDS * op.index;
    aff cur = load_affine(entry);
#pragma unroll 1
    for (int w = 0; w < POINTS; w++) {
      qglv_operand on = op;               // (the last step re-reads its own entry)
      const int wn = w + 1;
      if (wn < QGLV_WINDOWS) {            // (wave-uniform)
        secp::shr_bits<8>(b1);
        on = qglv_operand_of(wn, b1.v[0], sp.neg1, false);
        entry = qtab_v + (size_t)GTAB_ENTRY_DWORDS * on.index;
      } else if (wn < 2 * QGLV_WINDOWS) {
        if (wn > QGLV_WINDOWS) secp::shr_bits<8>(b2);
        on = qglv_operand_of(wn - QGLV_WINDOWS, b2.v[0], sp.neg2, true);
        entry = qtab_v + (size_t)GTAB_ENTRY_DWORDS * on.index;
      } else if (wn < POINTS) {
        const int g = wn - 2 * QGLV_WINDOWS;
        if (g > 0) secp::shr_bits<GTAB_BITS>(k1);
        const uint32_t dn = k1.v[0] & (uint32_t)(GTAB_ENTRIES - 1);
        on.index = dn;
        on.nz = dn != 0;
        on.beta = false;
        on.neg = false;
        entry = gtab + (size_t)GTAB_ENTRY_DWORDS * ((size_t)g * GTAB_ENTRIES + dn);
      }
      const aff nxt = load_affine(entry);
      secp::fe bx = cur.x;
      if (w >= QGLV_WINDOWS && w < 2 * QGLV_WINDOWS) bx = secp::fe_mul(cur.x, beta);  // (wave-uniform: w is the loop counter)
      const aff q = qglv_apply(cur, bx, op.beta, op.neg);
      jac sum = secp::jac_add_aff_t<true>(acc, q);
      acc = secp::jac_select(op.nz, sum, acc);
      cur = nxt;
      op = on;
    }
    return verify_finish(acc, r, v) && ok;
  }
  // ONE rolled loop over the 32 + GTAB_WINDOWS table points (one inlined copy of the mixed addition: secp256k1_dev.h).
  // Round 6: software-pipelined by one — the entry of step w + 1 is asked for before the addition of step w runs.  Every step
  // used to open with a dependent read of a table far beyond any cache (655 KB per validator: 43 GB at 65 536 validators;
  // ≈ 2 µs with one resident wavefront per SIMD) in front of a 4.4 µs addition: a third of this kernel's time was that wait.
  // The scalars are shift registers (the current window in the low bits of word 0): nothing is indexed by w, nothing lives
  // in the private segment (the 80 B of scratch this kernel had were u1 and u2).
  u256 k2 = u2, k1 = u1;
  uint32_t dgt = k2.v[0] & 255u;
  const uint32_t *entry = qtab_v + (size_t)GTAB_ENTRY_DWORDS * dgt;
  aff cur = load_affine(entry);
  constexpr int POINTS = QTAB_WINDOWS + GTAB_WINDOWS;
#pragma unroll 1
  for (int w = 0; w < POINTS; w++) {
    uint32_t dn = dgt;                  // (the last step re-reads its own entry)
    const int wn = w + 1;
    if (wn < QTAB_WINDOWS) {            // (wave-uniform)
      secp::shr_bits<8>(k2);
      dn = k2.v[0] & 255u;
      entry = qtab_v + (size_t)GTAB_ENTRY_DWORDS * (wn * QTAB_ENTRIES + dn);
    } else if (wn < POINTS) {
      const int g = wn - QTAB_WINDOWS;
      if (g > 0) secp::shr_bits<GTAB_BITS>(k1);
      dn = k1.v[0] & (uint32_t)(GTAB_ENTRIES - 1);
      entry = gtab + (size_t)GTAB_ENTRY_DWORDS * ((size_t)g * GTAB_ENTRIES + dn);
    }
    const aff nxt = load_affine(entry);
    jac sum = secp::jac_add_aff_t<true>(acc, cur);
    acc = secp::jac_select(dgt != 0, sum, acc);
    cur = nxt;
    dgt = dn;
  }
  return verify_finish(acc, r, v) && ok;
}

// ---- table build: one (validator, window) per lane, 16 entries per Montgomery batch ------------
// Wide form: writes qtab[v][w][e] = e·2^(8w)·Q_v for e = 1..255 (entry 0 zeroed).  GLV form: window w holds m·2^(8w)·Q_v for
// m = 1..128 (w < 15) or 1..256 (w = 15), entry m − 1 of the window, nothing zeroed.  Every lane of a wavefront executes the
// same instruction stream (same w, uniform trip counts); lanes with nothing to build run on the generator and skip only the
// stores — no call sits under a partial EXEC mask.
constexpr int QTAB_CHUNK = 16;

template <int FORM = QTAB_WIDE>
__host__ __device__ inline void qtab_build_window(const aff &Q, int w, uint32_t *__restrict__ out, bool do_store) {
  constexpr bool GLV = FORM == QTAB_GLV;
  constexpr int FIRST = GLV ? 1 : 0;  // the multiple of the window's entry 0
  // base = 2^(8w)·Q, affine
  jac b = secp::jac_from_aff(Q);
  for (int k = 0; k < 8 * w; k++) b = secp::jac_dbl(b);
  aff B;
  secp::jac_to_aff_fast(B, b);
  if (!GLV && do_store)
    for (int i = 0; i < GTAB_ENTRY_DWORDS; i++) out[i] = 0;
  const int entries = GLV ? (w == QGLV_WINDOWS - 1 ? QGLV_TOP_ENTRIES : QGLV_ENTRIES) : QTAB_ENTRIES;
  jac run = secp::jac_inf();
  for (int c = 0; c < entries / QTAB_CHUNK; c++) {
    jac buf[QTAB_CHUNK];
    secp::fe pre[QTAB_CHUNK];  // pre[i] = Z_0·…·Z_i over the finite entries of the chunk
    secp::fe acc = secp::fe_one();
    for (int i = 0; i < QTAB_CHUNK; i++) {
      const int e = c * QTAB_CHUNK + i + FIRST;
      if (e > 0) run = secp::jac_add_aff(run, B);  // e = 0 stays ∞ (uniform: e is lane-independent)
      buf[i] = run;
      secp::fe z = secp::l26_select(run.inf, secp::fe_one(), run.z);
      acc = secp::fe_mul(acc, z);
      pre[i] = acc;
    }
    secp::fe inv = secp::fe_inv_safegcd(acc);
    for (int i = QTAB_CHUNK - 1; i >= 0; i--) {
      const int e = c * QTAB_CHUNK + i + FIRST;
      secp::fe z = secp::l26_select(buf[i].inf, secp::fe_one(), buf[i].z);
      secp::fe zi = i > 0 ? secp::fe_mul(inv, pre[i - 1]) : inv;
      inv = secp::fe_mul(inv, z);
      secp::fe zi2 = secp::fe_sqr(zi);
      aff a;
      a.x = secp::fe_normalize(secp::fe_mul(buf[i].x, zi2));
      a.y = secp::fe_normalize(secp::fe_mul(buf[i].y, secp::fe_mul(zi2, zi)));
      if (do_store && e > 0) store_affine(out + (size_t)GTAB_ENTRY_DWORDS * (e - FIRST), a);
    }
  }
}
// where window w of a validator's table begins
template <int FORM>
__host__ __device__ constexpr size_t qtab_window_dwords(int w) {
  return (size_t)GTAB_ENTRY_DWORDS * (FORM == QTAB_GLV ? QGLV_ENTRIES : QTAB_ENTRIES) * w;
}

}  // namespace ibftk
