// sign_dev.h — the signing side: one committed seal per row.
//
// Product code (__host__ __device__ like recover_dev.h, so tests can run the identical source on
// the CPU; the shipped library only runs it on gfx950).  The reference produces a committed seal
// inside Backend.BuildCommitMessage (/root/reference/core/backend.go:12-34, called from
// core/ibft.go:898-909 sendCommitMessage); a real validator signs ONE seal per round with ITS key,
// which is not a batch problem.  The batch exists for simulators, load generators and test rigs
// that play thousands of validators in one process (the shape of the reference's own
// core/consensus_test.go clusters) — that is the only use this entry point is meant for: the keys
// cross PCIe in the clear and sit in HBM for the duration of the call.
//
// The signature is plain ECDSA over secp256k1 with the low-s rule and v = parity(R.y) (flipped when
// s is negated), i.e. what ibft_verify_seals accepts under every flag.  The nonce is deterministic
// and is the one the CPU oracle uses (oracle/secp256k1.c:orc_sign):
//     k = keccak256(sk32 ‖ digest32 ‖ LE32(ctr)) mod n,   ctr = 0, 1, … until (k, r, s) are all usable
// so that a device signature can be compared byte for byte with the oracle's.  That rule (SIGN_NONCE_KECCAK) is this
// repository's own and stays the default.  The second rule, SIGN_NONCE_RFC6979, is RFC 6979 §3.2 with HMAC-SHA-256 at
// hlen = qlen = 256 and bits2octets(h1) = h1 mod n (rfc6979_drbg below, the restatement of oracle/secp256k1.c:
// orc_sign_rfc6979): what btcec, bitcoinjs and the published secp256k1 vectors use, so a seal signed under it can be re-derived
// by third-party tools.  The candidate rules are the same under both: 0 < k < n, r = R.x with 0 < r < n (R.x ≥ n would need
// recovery id ≥ 2: the next candidate is taken instead), s ≠ 0.  Nothing on the verify side depends on how k was chosen.
#pragma once
#include "recover_dev.h"
#include "sha256_dev.h"

namespace ibftk {

constexpr uint32_t SIGN_MAX_TRIES = 1024;  // same bound as the oracle; a retry has probability ≈2^-128
constexpr int SIGN_NONCE_KECCAK = 0;       // IBFT_SIGN_NONCE_KECCAK
constexpr int SIGN_NONCE_RFC6979 = 1;      // IBFT_SIGN_NONCE_RFC6979

// keccak256 of the 68-byte nonce preimage, as a 256-bit big-endian integer
__host__ __device__ __forceinline__ u256 sign_nonce_hash(const uint8_t *sk32, const uint8_t *digest32, uint32_t ctr) {
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < 25; i++) s[i] = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint64_t a = 0, b = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) {
      a |= (uint64_t)sk32[8 * j + t] << (8 * t);
      b |= (uint64_t)digest32[8 * j + t] << (8 * t);
    }
    s[j] = a;
    s[4 + j] = b;
  }
  // bytes 64..67 = ctr (the oracle writes two counter bytes and two zeros; ctr < 1024), byte 68 = 0x01 pad
  s[8] = (uint64_t)(ctr & 0xFFFFu) | (0x01ULL << 32);
  s[16] ^= 0x8000000000000000ULL;
  keccak::f1600(s);
  u256 k;
  keccak::digest_to_limbs(s, k.v);
  return k;
}

// RFC 6979 §3.2 (b)–(h), HMAC-SHA-256, for one signature.  Of K only the two pad midstates are kept (sha256_dev.h: every
// HMAC under K starts from them); they and V are 24 words in registers and never stored.  A signature whose first candidate
// is usable costs 16 compressions: 2 × (3 for K = HMAC_K(V ‖ tag ‖ x ‖ h1) + 2 for the new K's midstates + 2 for V = HMAC_K(V))
// + 2 for the candidate (the midstates of the initial all-zero K are constants).
struct rfc6979_drbg {
  sha256::hmac_key K;
  sha256::state V;

  __host__ __device__ static __forceinline__ sha256::state words(const u256 &a) {  // 32 big-endian bytes as words
    return sha256::state{a.v[7], a.v[6], a.v[5], a.v[4], a.v[3], a.v[2], a.v[1], a.v[0]};
  }
  // x = int2octets(secret key), h1 = bits2octets(digest) = the digest mod n
  __host__ __device__ __forceinline__ void init(const u256 &x, const u256 &h1) {
    const sha256::state xs = words(x), hs = words(h1);
    K = sha256::hmac_midstates_zero_key();                                                       // (c) K = 0x00 …
    V = sha256::state{0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};  // (b)
#pragma unroll 1
    for (uint32_t tag = 0; tag < 2; tag++) {                                                     // (d) (e), then (f) (g)
      K = sha256::hmac_midstates(sha256::hmac_v_tag_x_h(K, V, tag, xs, hs));
      V = sha256::hmac_v(K, V);
    }
  }
  // (h.2) with tlen = qlen after one block: V = HMAC_K(V), the candidate is V as a big-endian integer
  __host__ __device__ __forceinline__ u256 candidate() {
    V = sha256::hmac_v(K, V);
    u256 k;
    k.v[7] = V.a, k.v[6] = V.b, k.v[5] = V.c, k.v[4] = V.d, k.v[3] = V.e, k.v[2] = V.f, k.v[1] = V.g, k.v[0] = V.h;
    return k;
  }
  // (h.3) after an unusable candidate: K = HMAC_K(V ‖ 0x00), V = HMAC_K(V)
  __host__ __device__ __forceinline__ void reseed() {
    K = sha256::hmac_midstates(sha256::hmac_v_00(K, V));
    V = sha256::hmac_v(K, V);
  }
};

// One signature under the key d (sign_key: key_ok says whether it lies in [1, n); sk32 are its bytes, for the nonce).  Returns
// false (and writes zeros) for a key outside [1, n) or when no nonce was usable.
// The retry loop keeps a wavefront convergent: its body is executed by every lane until all lanes of the wavefront are done
// (on the device: EVERY lane of a wavefront must call this, lanes with nothing to sign included), lanes that finished
// discard the extra attempts.
// NONCE: SIGN_NONCE_KECCAK (the rule above) or SIGN_NONCE_RFC6979.  reject_mask is a test seam of the RFC 6979 rule: bit t set
// treats candidate t as unusable, which is the only way to reach the reseed step (a real retry has probability ≈2^-128); the
// kernels pass the constant 0 and the seam folds away.
template <int NONCE = SIGN_NONCE_KECCAK>
__host__ __device__ __forceinline__ bool sign_core(const uint32_t *__restrict__ gtab, const uint8_t *sk32, const u256 &d, bool key_ok,
                                                   const uint8_t *digest32, u256 &r_out, u256 &s_out, uint32_t &v_out,
                                                   uint32_t reject_mask = 0) {
  static_assert(NONCE == SIGN_NONCE_KECCAK || NONCE == SIGN_NONCE_RFC6979, "unknown nonce rule");
  u256 z = secp::from_be32(digest32);
  secp::sub_const_if(z, secp::geq_const(z, secp::NL()), secp::NL());  // z mod n (z < 2^256 < 2n)
  const secp::sc d_sc = secp::sc_from_u256(d);

  rfc6979_drbg drbg;
  if constexpr (NONCE == SIGN_NONCE_RFC6979) drbg.init(d, z);

  bool done = !key_ok, ok = false;
  r_out = secp::zero256();
  s_out = secp::zero256();
  v_out = 0;
  for (uint32_t ctr = 0; ctr < SIGN_MAX_TRIES; ctr++) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (__ballot(!done) == 0) break;
#else
    if (done) break;
#endif
    u256 k;
    bool good;
    if constexpr (NONCE == SIGN_NONCE_RFC6979) {
      if (ctr) drbg.reseed();  // (uniform: every lane of the wavefront is in the same attempt)
      k = drbg.candidate();
      good = !secp::is_zero(k) && !secp::geq_const(k, secp::NL());
      good = good && !(ctr < 32u && ((reject_mask >> ctr) & 1u));
    } else {
      k = sign_nonce_hash(sk32, digest32, ctr);
      secp::sub_const_if(k, secp::geq_const(k, secp::NL()), secp::NL());
      good = !secp::is_zero(k);
    }
    const u256 k_safe = secp::select(good, k, secp::one256());  // keep the inversion's precondition
    // R = k·G
    jac R = ecmult_gen(gtab, k_safe, secp::jac_inf());
    aff Ra;
    good = secp::jac_to_aff_fast(Ra, R) && good;
    const u256 rx = secp::l26_to_u256(Ra.x), ry = secp::l26_to_u256(Ra.y);
    good = good && !secp::geq_const(rx, secp::NL()) && !secp::is_zero(rx);  // r = x would need v ≥ 2: next nonce
    // s = k⁻¹ (z + r·d) mod n
    const secp::sc kinv = secp::sc_from_u256(secp::modinv<secp::ModN>(k_safe));
    const u256 rd = secp::sc_canon(secp::sc_mul(secp::sc_from_u256(rx), d_sc));
    const u256 t = secp::add_mod_n(rd, z);
    u256 s = secp::sc_canon(secp::sc_mul(kinv, secp::sc_from_u256(t)));
    good = good && !secp::is_zero(s);
    uint32_t v = ry.v[0] & 1u;
    // low-s: s > (n−1)/2  ⇔  s − 1 ≥ (n−1)/2
    u256 sm1;
    secp::sub256(sm1, s, secp::one256());
    const bool high = !secp::is_zero(s) && secp::geq_const(sm1, secp::NHL());
    s = secp::select(high, secp::sc_neg_canon(s), s);
    v ^= high ? 1u : 0u;
    if (!done && good) {
      r_out = rx;
      s_out = s;
      v_out = v;
      ok = true;
      done = true;
    }
  }
  return ok;
}

// The secret key as a number, and whether it lies in [1, n)
__host__ __device__ __forceinline__ bool sign_key(const uint8_t *sk32, u256 &d) {
  d = secp::from_be32(sk32);
  return !secp::is_zero(d) && !secp::geq_const(d, secp::NL());
}

// The signer's address, keccak256(X‖Y)[12..32) of d·G — what the validator set is keyed by; zeros for a key outside [1, n).
__host__ __device__ __forceinline__ void sign_address(const uint32_t *__restrict__ gtab, const u256 &d, bool key_ok, uint32_t addr[5]) {
  jac Q = ecmult_gen(gtab, secp::select(key_ok, d, secp::one256()), secp::jac_inf());
  aff Qa;
  (void)secp::jac_to_aff_fast(Qa, Q);
  const u256 qx = secp::l26_to_u256(Qa.x), qy = secp::l26_to_u256(Qa.y);
  keccak::address_from_xy(qx.v, qy.v, addr);
  if (!key_ok) {
#pragma unroll
    for (int i = 0; i < 5; i++) addr[i] = 0;
  }
}

// One signature over a digest under the key sk32: sign_key + sign_core.  What the envelope kernel and the CPU harnesses call;
// sign_message_row keeps the two apart (one key, two digests).  On the device every lane of a wavefront must call it.
template <int NONCE = SIGN_NONCE_KECCAK>
__host__ __device__ __forceinline__ bool sign_digest(const uint32_t *__restrict__ gtab, const uint8_t *sk32, const uint8_t *digest32,
                                                     u256 &r_out, u256 &s_out, uint32_t &v_out, uint32_t reject_mask = 0) {
  u256 d;
  const bool key_ok = sign_key(sk32, d);
  return sign_core<NONCE>(gtab, sk32, d, key_ok, digest32, r_out, s_out, v_out, reject_mask);
}

// One row of ibft_sign_seals: the signature and the signer's address — sign_digest, then sign_address under the same key.  Spelled
// with the key derived once: composed from the two calls it is derived twice, and sign_lane_kernel, which sits just below the
// 64 KB of the instruction cache, pays 7 registers and 0.3 KB for that.
template <int NONCE = SIGN_NONCE_KECCAK>
__host__ __device__ __forceinline__ bool sign_row(const uint32_t *__restrict__ gtab, const uint8_t *sk32,
                                                  const uint8_t *digest32, u256 &r_out, u256 &s_out, uint32_t &v_out,
                                                  uint32_t addr[5], uint32_t reject_mask = 0) {
  u256 d;
  const bool key_ok = sign_key(sk32, d);
  const bool ok = sign_core<NONCE>(gtab, sk32, d, key_ok, digest32, r_out, s_out, v_out, reject_mask);
  sign_address(gtab, d, key_ok, addr);
  return ok;
}

// ---- the row frame of the signer's lane kernels (kernels.hip.h): one lane per row, one wavefront per workgroup ----------------
// Idle lanes of the last wavefront run the last row again (sign_core votes across the wavefront) and store nothing: `src` is the row
// a lane reads, `row` the one it may write when `live`.
struct lane_row {
  uint32_t row, src;
  bool live;
  __device__ explicit lane_row(uint32_t n) : row(blockIdx.x * 64u + threadIdx.x), src(row < n ? row : n - 1), live(row < n) {}
};
// row `src` of a column of 32-byte entries as a private byte array: dword loads, unpacked
__host__ __device__ __forceinline__ void load_row32(const uint8_t *__restrict__ col, uint32_t src, uint8_t out[32]) {
  const uint32_t *w = reinterpret_cast<const uint32_t *>(col + 32ull * src);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t x = w[i];
#pragma unroll
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(x >> (8 * b));
  }
}
// an address into row `row` of a column of 20-byte entries
__host__ __device__ __forceinline__ void store_addr20(uint8_t *__restrict__ col, uint32_t row, const uint32_t addr[5]) {
  uint32_t *ad = reinterpret_cast<uint32_t *>(col + 20ull * row);
#pragma unroll
  for (int i = 0; i < 5; i++) ad[i] = addr[i];
}
// r ‖ s ‖ v (big-endian; the 0x41-byte body of a signature field, or a 65-byte seal) at p — byte stores: p is anywhere
__host__ __device__ __forceinline__ void put_sig65(uint8_t *p, const u256 &r, const u256 &s, uint32_t v) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
      p[4 * (7 - i) + b] = (uint8_t)(r.v[i] >> (8 * (3 - b)));
      p[32 + 4 * (7 - i) + b] = (uint8_t)(s.v[i] >> (8 * (3 - b)));
    }
  }
  p[64] = (uint8_t)v;
}

}  // namespace ibftk
