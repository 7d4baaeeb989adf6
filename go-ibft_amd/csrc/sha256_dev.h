// sha256_dev.h — SHA-256's compression function and HMAC-SHA-256 in the three shapes RFC 6979 §3.2 needs at
// hlen = qlen = 256 (sign_dev.h: rfc6979_drbg), one lane per signature.
//
// __host__ __device__ like the rest of csrc/, so tests run the identical source on the CPU.  Written for gfx950 registers:
// the state, the chaining values and the 16-word rolling message schedule are named 32-bit words and every round is spelled
// out, so nothing is indexed at run time and nothing goes to the private segment; rotates are funnel shifts (v_alignbit_b32),
// Ch and Maj are bit selects (v_bfi_b32).  There are no byte arrays: a block is sixteen big-endian words composed in
// registers, and the padding words of the three fixed message shapes are constants.
//
// HMAC here always has a 32-byte key, and its message is one of
//     V ‖ 0x00|0x01 ‖ x ‖ h1   97 bytes (two inner blocks; x and h1 sit one byte off word alignment)
//     V ‖ 0x00                 33 bytes
//     V                        32 bytes
// The inner and the outer pad block depend on the key alone: their midstates are computed once per key (hmac_midstates) and
// every HMAC under that key starts from them, which leaves 2 compressions for the 32- and 33-byte shapes and 3 for the 97-byte
// one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sha256 {

struct state {  // a chaining value: H0 … H7
  uint32_t a, b, c, d, e, f, g, h;
};
struct block {  // one 64-byte block as big-endian words
  uint32_t w0, w1, w2, w3, w4, w5, w6, w7, w8, w9, w10, w11, w12, w13, w14, w15;
};

__host__ __device__ __forceinline__ uint32_t rotr(uint32_t x, uint32_t n) { return __builtin_rotateright32(x, n); }
// bit select: mask ? x : y
__host__ __device__ __forceinline__ uint32_t bsel(uint32_t mask, uint32_t x, uint32_t y) { return y ^ (mask & (x ^ y)); }
__host__ __device__ __forceinline__ uint32_t ch(uint32_t e, uint32_t f, uint32_t g) { return bsel(e, f, g); }
__host__ __device__ __forceinline__ uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return bsel(a ^ b, c, b); }
__host__ __device__ __forceinline__ uint32_t bsig0(uint32_t x) { return rotr(x, 2) ^ rotr(x, 13) ^ rotr(x, 22); }
__host__ __device__ __forceinline__ uint32_t bsig1(uint32_t x) { return rotr(x, 6) ^ rotr(x, 11) ^ rotr(x, 25); }
__host__ __device__ __forceinline__ uint32_t ssig0(uint32_t x) { return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3); }
__host__ __device__ __forceinline__ uint32_t ssig1(uint32_t x) { return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10); }

__host__ __device__ __forceinline__ state iv() {
  return state{0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
}

// one round; the eight working variables rotate by renaming, not by moving
#define SHA256_RND(a, b, c, d, e, f, g, h, k, w)                         \
  {                                                                      \
    const uint32_t t1 = h + bsig1(e) + ch(e, f, g) + (k) + (w);          \
    const uint32_t t2 = bsig0(a) + maj(a, b, c);                         \
    d += t1;                                                             \
    h = t1 + t2;                                                         \
  }
// eight rounds on schedule words x0 … x7
#define SHA256_RND8(x0, x1, x2, x3, x4, x5, x6, x7, k0, k1, k2, k3, k4, k5, k6, k7) \
  SHA256_RND(a, b, c, d, e, f, g, h, k0, x0)                                        \
  SHA256_RND(h, a, b, c, d, e, f, g, k1, x1)                                        \
  SHA256_RND(g, h, a, b, c, d, e, f, k2, x2)                                        \
  SHA256_RND(f, g, h, a, b, c, d, e, k3, x3)                                        \
  SHA256_RND(e, f, g, h, a, b, c, d, k4, x4)                                        \
  SHA256_RND(d, e, f, g, h, a, b, c, k5, x5)                                        \
  SHA256_RND(c, d, e, f, g, h, a, b, k6, x6)                                        \
  SHA256_RND(b, c, d, e, f, g, h, a, k7, x7)
// the rolling schedule: W[t] overwrites W[t − 16]
#define SHA256_EXP(x0, x1, x9, x14) x0 += ssig1(x14) + x9 + ssig0(x1);
#define SHA256_EXP16                                                                          \
  SHA256_EXP(w0, w1, w9, w14) SHA256_EXP(w1, w2, w10, w15) SHA256_EXP(w2, w3, w11, w0)        \
  SHA256_EXP(w3, w4, w12, w1) SHA256_EXP(w4, w5, w13, w2) SHA256_EXP(w5, w6, w14, w3)         \
  SHA256_EXP(w6, w7, w15, w4) SHA256_EXP(w7, w8, w0, w5) SHA256_EXP(w8, w9, w1, w6)           \
  SHA256_EXP(w9, w10, w2, w7) SHA256_EXP(w10, w11, w3, w8) SHA256_EXP(w11, w12, w4, w9)       \
  SHA256_EXP(w12, w13, w5, w10) SHA256_EXP(w13, w14, w6, w11) SHA256_EXP(w14, w15, w7, w12)   \
  SHA256_EXP(w15, w0, w8, w13)

// the compression function: the chaining value after block m
__host__ __device__ __forceinline__ state compress_inl(const state &s, const block &m) {
  uint32_t a = s.a, b = s.b, c = s.c, d = s.d, e = s.e, f = s.f, g = s.g, h = s.h;
  uint32_t w0 = m.w0, w1 = m.w1, w2 = m.w2, w3 = m.w3, w4 = m.w4, w5 = m.w5, w6 = m.w6, w7 = m.w7;
  uint32_t w8 = m.w8, w9 = m.w9, w10 = m.w10, w11 = m.w11, w12 = m.w12, w13 = m.w13, w14 = m.w14, w15 = m.w15;
  SHA256_RND8(w0, w1, w2, w3, w4, w5, w6, w7, 0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u)
  SHA256_RND8(w8, w9, w10, w11, w12, w13, w14, w15, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u)
  SHA256_EXP16
  SHA256_RND8(w0, w1, w2, w3, w4, w5, w6, w7, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau)
  SHA256_RND8(w8, w9, w10, w11, w12, w13, w14, w15, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u)
  SHA256_EXP16
  SHA256_RND8(w0, w1, w2, w3, w4, w5, w6, w7, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u)
  SHA256_RND8(w8, w9, w10, w11, w12, w13, w14, w15, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u)
  SHA256_EXP16
  SHA256_RND8(w0, w1, w2, w3, w4, w5, w6, w7, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u)
  SHA256_RND8(w8, w9, w10, w11, w12, w13, w14, w15, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u)
  return state{s.a + a, s.b + b, s.c + c, s.d + d, s.e + e, s.f + f, s.g + g, s.h + h};
}
#undef SHA256_EXP16
#undef SHA256_EXP
#undef SHA256_RND8
#undef SHA256_RND
// On the device every call site shares ONE outlined copy (as secp256k1_dev.h does for fe_mul / sc_mul): the 64 rounds are ≈11 KB
// of straight-line code, a signature runs them 16 times, and 16 inlined copies would stream ≈170 KB through a 64 KB instruction
// cache once per wavefront.  State and block travel as 24 scalar arguments, i.e. in registers.
#if defined(__HIP_DEVICE_COMPILE__)
static __device__ __attribute__((noinline)) state compress_fn(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e, uint32_t f, uint32_t g,
                                                              uint32_t h, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4,
                                                              uint32_t w5, uint32_t w6, uint32_t w7, uint32_t w8, uint32_t w9, uint32_t w10,
                                                              uint32_t w11, uint32_t w12, uint32_t w13, uint32_t w14, uint32_t w15) {
  return compress_inl(state{a, b, c, d, e, f, g, h}, block{w0, w1, w2, w3, w4, w5, w6, w7, w8, w9, w10, w11, w12, w13, w14, w15});
}
__device__ __forceinline__ state compress(const state &s, const block &m) {
  return compress_fn(s.a, s.b, s.c, s.d, s.e, s.f, s.g, s.h, m.w0, m.w1, m.w2, m.w3, m.w4, m.w5, m.w6, m.w7, m.w8, m.w9, m.w10, m.w11, m.w12,
                     m.w13, m.w14, m.w15);
}
#else
__host__ __device__ __forceinline__ state compress(const state &s, const block &m) { return compress_inl(s, m); }
#endif

// ---- HMAC-SHA-256, 32-byte key ----------------------------------------------------------------------------------------
struct hmac_key {  // the chaining values after (key ⊕ ipad) and after (key ⊕ opad): all an HMAC under this key needs of it
  state inner, outer;
};

__host__ __device__ __forceinline__ hmac_key hmac_midstates(const state &key) {  // key = its 32 bytes as big-endian words
  constexpr uint32_t I = 0x36363636u, O = 0x5c5c5c5cu;
  hmac_key k;
  k.inner = compress(iv(), block{key.a ^ I, key.b ^ I, key.c ^ I, key.d ^ I, key.e ^ I, key.f ^ I, key.g ^ I, key.h ^ I, I, I, I, I, I, I, I, I});
  k.outer = compress(iv(), block{key.a ^ O, key.b ^ O, key.c ^ O, key.d ^ O, key.e ^ O, key.f ^ O, key.g ^ O, key.h ^ O, O, O, O, O, O, O, O, O});
  return k;
}
// the midstates of the all-zero key (RFC 6979 §3.2 step c): compress(IV, 0x36 × 64) and compress(IV, 0x5c × 64)
__host__ __device__ __forceinline__ hmac_key hmac_midstates_zero_key() {
  hmac_key k;
  k.inner = state{0xf454deadu, 0x9725214fu, 0x90daf2a0u, 0xdf1228eau, 0x64e5750fu, 0xa3924181u, 0x824a932bu, 0xf8e04e32u};
  k.outer = state{0xd385480fu, 0x7abb6477u, 0x37c9c538u, 0x5dd82467u, 0x8e043a72u, 0x753434b0u, 0xdeb82818u, 0x361d45a6u};
  return k;
}

// outer hash: opad block ‖ the 32-byte inner digest — one block of 64 + 32 bytes, 768 bits
__host__ __device__ __forceinline__ state hmac_finish(const hmac_key &k, const state &in) {
  return compress(k.outer, block{in.a, in.b, in.c, in.d, in.e, in.f, in.g, in.h, 0x80000000u, 0, 0, 0, 0, 0, 0, 768u});
}
// HMAC_K(V), 32 bytes: (64 + 32) · 8 = 768 bits
__host__ __device__ __forceinline__ state hmac_v(const hmac_key &k, const state &v) {
  return hmac_finish(k, compress(k.inner, block{v.a, v.b, v.c, v.d, v.e, v.f, v.g, v.h, 0x80000000u, 0, 0, 0, 0, 0, 0, 768u}));
}
// HMAC_K(V ‖ 0x00), 33 bytes: the zero byte and the padding's 0x80 share word 8; (64 + 33) · 8 = 776 bits
__host__ __device__ __forceinline__ state hmac_v_00(const hmac_key &k, const state &v) {
  return hmac_finish(k, compress(k.inner, block{v.a, v.b, v.c, v.d, v.e, v.f, v.g, v.h, 0x00800000u, 0, 0, 0, 0, 0, 0, 776u}));
}
// HMAC_K(V ‖ tag ‖ x ‖ h1), 97 bytes (tag = 0x00 or 0x01; x, h1 = 32 bytes each as big-endian words).  Behind the tag byte
// every word takes one byte of its left neighbour and three of its own: shifts by 24 and 8 only.  The second block ends
// h1's last byte ‖ 0x80 ‖ zeros ‖ (64 + 97) · 8 = 1288 bits.
__host__ __device__ __forceinline__ state hmac_v_tag_x_h(const hmac_key &k, const state &v, uint32_t tag, const state &x, const state &h) {
  const state s1 = compress(k.inner, block{v.a, v.b, v.c, v.d, v.e, v.f, v.g, v.h,
                                           (tag << 24) | (x.a >> 8), (x.a << 24) | (x.b >> 8), (x.b << 24) | (x.c >> 8), (x.c << 24) | (x.d >> 8),
                                           (x.d << 24) | (x.e >> 8), (x.e << 24) | (x.f >> 8), (x.f << 24) | (x.g >> 8), (x.g << 24) | (x.h >> 8)});
  const state s2 = compress(s1, block{(x.h << 24) | (h.a >> 8), (h.a << 24) | (h.b >> 8), (h.b << 24) | (h.c >> 8), (h.c << 24) | (h.d >> 8),
                                      (h.d << 24) | (h.e >> 8), (h.e << 24) | (h.f >> 8), (h.f << 24) | (h.g >> 8), (h.g << 24) | (h.h >> 8),
                                      (h.h << 24) | 0x00800000u, 0, 0, 0, 0, 0, 0, 1288u});
  return hmac_finish(k, s2);
}

}  // namespace sha256
