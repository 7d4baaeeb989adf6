// keccak_row_dev.h — Keccak-256 of one 64-byte public key per ROW of sixteen lanes: the address of the recovered key.
//
// Product code; included by wave_fe_dev.h (namespace wv, behind its cross-lane primitives), which is also how the host
// tests run it under wave_emul.h.  keccak::address_from_xy is lane-layout code: called by a row kernel, each of the
// sixteen lanes of a row runs the same permutation of the same 64 bytes, ≈290 VALU instructions per round, and one main
// wavefront per SIMD pays for every instruction it issues.  Here the 25 state words of a row's hash are spread over
// five of its lanes instead — PLANE PER LANE: lane y (0 … 4) of a row holds A[0 … 4][y] in ten VGPRs —
//   θ   column parities: three row_shr xors per dword leave the sum of lanes 0 … 4 in lane 4, which works out D;
//       every lane folds row_bcast<4>(D) in as a DPP operand
//   ρ   a 64-bit rotation by a per-lane amount: two selects (swap the halves for ≥ 32), two v_alignbit
//   π   B[y][2x + 3y] = A[x][y]: new word X of lane Y is old word (X + 3Y) mod 5 of lane X — every lane of a row reads a
//       DIFFERENT register of ONE lane, which DPP cannot do without five selects per dword.  It goes through wave-private
//       LDS: the ten dwords go out at one address + immediate offsets (three LDS writes), five two-dword reads at
//       addresses computed once.  A lane touches only locations of its own row and the LDS serves a wavefront's accesses
//       in order: no barrier
//   χ   in-lane, one v_bitop3_b32 per dword
//   ι   in-lane, under a mask that is all ones in lane 0
// The gfx950 round loop (rolled) is 96 VALU instructions — 52 v_xor, 20 v_alignbit, 12 v_cndmask, 10 v_bitop3, 2 v_mov —
// and 8 LDS instructions (DESIGN.md §9 has the count and the measurements).
// Lanes 5 … 15 of a row execute the same instructions on junk: their LDS traffic goes to
// slots of their own behind the row's 25 words, nothing of theirs is ever read by lanes 0 … 4 (row_shr only looks down,
// the broadcast reads lane 4), and the result is handed out by row_bcast<0>.  Control flow is wave-uniform throughout
// (the RULE of wave_fe_dev.h): every row goes through the same 24 rounds whatever its verdict.
#pragma once
#include "keccak_dev.h"

namespace wv {

// wave-private scratch of address_from_xy_row, in dwords: per row 25 state words + 31 words that take the idle lanes' writes
constexpr int KROW_ROW_QWORDS = 56;
constexpr int KROW_SCRATCH_DWORDS = 4 * KROW_ROW_QWORDS * 2;

// Between a wavefront's LDS writes and its reads of what OTHER lanes wrote.  The hardware needs nothing (one wavefront, LDS
// operations in order); the fence keeps the compiler from moving a read across the writes, and the emulator's coroutine
// lanes — which run one after the other between two cross-lane operations — meet here.
HD void wave_lds_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#elif defined(IBFT_WAVE_EMUL)
  (void)wave_emul::xchg(0u, wave_emul::lane(), 0x700u);
#endif
}

// ({a, b} >> (s & 31)) as 32 bits: v_alignbit_b32
HD uint32_t krow_alignbit(uint32_t a, uint32_t b, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(a, b, s);
#else
  return (uint32_t)((((uint64_t)a << 32) | b) >> (s & 31u));
#endif
}

// rotate-RIGHT amounts (64 − ρ offset) mod 64 of plane y, word x in bits 6x … 6x + 5
HD constexpr uint32_t krow_rot_pack(int a0, int a1, int a2, int a3, int a4) {
  return (uint32_t)((64 - a0) & 63) | (uint32_t)((64 - a1) & 63) << 6 | (uint32_t)((64 - a2) & 63) << 12 |
         (uint32_t)((64 - a3) & 63) << 18 | (uint32_t)((64 - a4) & 63) << 24;
}

// Keccak-256 of X‖Y (two field elements, normalized, the same in every lane of a row — what rows_finish_deferred and
// jac_to_aff_wave hand back): the low 20 bytes of the digest as keccak::address_from_xy returns them, the same in every
// lane of the row.  scr: KROW_SCRATCH_DWORDS dwords of wave-private scratch (LDS in the kernels).
WVF void address_from_xy_row(const fe &X, const fe &Y, uint32_t addr[5], uint32_t *scr) {
  const u256 qx = secp::l26_to_u256(X), qy = secp::l26_to_u256(Y);
  const uint32_t lane = lane_id(), li = lane & 15u, row = lane >> 4;
  const bool l0 = li == 0, l1 = li == 1;
  // state word x + 5y = message bytes 8(x + 5y) …, little-endian; the message is X‖Y big-endian, then 0x01 at byte 64 and
  // 0x80 at byte 135: lane 0 holds X and the first word of Y, lane 1 the rest of Y and the first pad byte, lane 3 the last
  uint32_t lo[5], hi[5];
#pragma unroll
  for (int x = 0; x < 5; x++) {
    // (x = 4: lane 0 takes Y's first word; lane 1's words 3, 4 are padding)
    const uint32_t a_lo = x < 4 ? qx.v[7 - 2 * x] : qy.v[7], a_hi = x < 4 ? qx.v[6 - 2 * x] : qy.v[6];
    const uint32_t b_lo = x < 3 ? qy.v[5 - 2 * x] : 0u, b_hi = x < 3 ? qy.v[4 - 2 * x] : 0u;
    lo[x] = keccak::bswap32(l0 ? a_lo : (l1 ? b_lo : 0u));
    hi[x] = keccak::bswap32(l0 ? a_hi : (l1 ? b_hi : 0u));
  }
  lo[3] |= l1 ? 0x01u : 0u;
  hi[1] |= li == 3 ? 0x80000000u : 0u;
  // per-lane constants: the ρ amounts of this lane's plane, the ι mask, the LDS places
  const uint32_t R0 = krow_rot_pack(0, 1, 62, 28, 27), R1 = krow_rot_pack(36, 44, 6, 55, 20),
                 R2 = krow_rot_pack(3, 10, 43, 25, 39), R3 = krow_rot_pack(41, 45, 15, 21, 8),
                 R4 = krow_rot_pack(18, 2, 61, 56, 14);
  const uint32_t rot = l0 ? R0 : (l1 ? R1 : (li == 2 ? R2 : (li == 3 ? R3 : R4)));
  uint32_t rs[5];
  bool swp[5];
#pragma unroll
  for (int x = 0; x < 5; x++) {
    rs[x] = rot >> (6 * x);  // v_alignbit looks at five bits
    swp[x] = (rot >> (6 * x + 5) & 1u) != 0;
  }
  const uint32_t m0 = l0 ? 0xFFFFFFFFu : 0u;
  // places, in two-dword units: word x of plane y at 5x + y; an idle lane writes (and reads back) slots 20 + li + 5x
  const bool plane = li < 5;
  const uint32_t rbase = row * (uint32_t)KROW_ROW_QWORDS;
  const uint32_t wr = rbase + li + (plane ? 0u : 20u);
  const uint32_t y3 = (0x24130u >> (4u * (li & 7u))) & 7u;  // 3·li mod 5 for li < 5
  uint32_t rd[5];
#pragma unroll
  for (int x = 0; x < 5; x++) {
    const uint32_t t = (uint32_t)x + y3, src = t >= 5u ? t - 5u : t;  // (X + 3Y) mod 5
    rd[x] = plane ? rbase + 5u * src + (uint32_t)x : wr + 5u * (uint32_t)x;
  }
#pragma unroll 1
  for (int round = 0; round < 24; round++) {
    // θ
    uint32_t cl[5], ch[5];
#pragma unroll
    for (int x = 0; x < 5; x++) {
      uint32_t a = lo[x], b = hi[x];
      a ^= row_shr<1>(a);
      b ^= row_shr<1>(b);
      a ^= row_shr<2>(a);
      b ^= row_shr<2>(b);
      a ^= row_shr<4>(a);
      b ^= row_shr<4>(b);
      cl[x] = a;  // lane 4: the parity of column x
      ch[x] = b;
    }
#pragma unroll
    for (int x = 0; x < 5; x++) {
      const int p = (x + 4) % 5, n = (x + 1) % 5;
      const uint32_t dl = cl[p] ^ krow_alignbit(cl[n], ch[n], 31u);  // C[x − 1] ^ rotl(C[x + 1], 1)
      const uint32_t dh = ch[p] ^ krow_alignbit(ch[n], cl[n], 31u);
      lo[x] ^= row_bcast<4>(dl);
      hi[x] ^= row_bcast<4>(dh);
    }
    // ρ, then π through the scratch
#pragma unroll
    for (int x = 0; x < 5; x++) {
      const uint32_t a = swp[x] ? hi[x] : lo[x], b = swp[x] ? lo[x] : hi[x];
      scr[2u * (wr + 5u * (uint32_t)x)] = krow_alignbit(b, a, rs[x]);
      scr[2u * (wr + 5u * (uint32_t)x) + 1u] = krow_alignbit(a, b, rs[x]);
    }
    wave_lds_sync();
    uint32_t bl[5], bh[5];
#pragma unroll
    for (int x = 0; x < 5; x++) {
      bl[x] = scr[2u * rd[x]];
      bh[x] = scr[2u * rd[x] + 1u];
    }
    wave_lds_sync();
    // χ, ι
#pragma unroll
    for (int x = 0; x < 5; x++) {
      lo[x] = bl[x] ^ (~bl[(x + 1) % 5] & bl[(x + 2) % 5]);
      hi[x] = bh[x] ^ (~bh[(x + 1) % 5] & bh[(x + 2) % 5]);
    }
    const uint64_t rc = keccak::rc(round);
    lo[0] ^= (uint32_t)rc & m0;
    hi[0] ^= (uint32_t)(rc >> 32) & m0;
  }
  // digest bytes 12 … 31: the upper half of word 1, words 2 and 3 — all of plane 0
  addr[0] = row_bcast<0>(hi[1]);
  addr[1] = row_bcast<0>(lo[2]);
  addr[2] = row_bcast<0>(hi[2]);
  addr[3] = row_bcast<0>(lo[3]);
  addr[4] = row_bcast<0>(hi[3]);
}

}  // namespace wv
