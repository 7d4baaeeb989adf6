// cert_dedup_kernels.h — the kernels of the certificate tree's opt-in dedup (IBFT_FLAG_CERT_DEDUP; the row logic:
// cert_dedup_dev.h) and of ibft_cert_stats, with the helpers that launch them: cert_dedup_front_launch,
// cert_dedup_scatter_launch and cert_dedup_count_launch are the only places that know their geometry.  The kernels need
// nothing but byte columns and the tile scan of cert_scan_dev.h, so the test library (devtest.hip: devtest_cert_dedup) runs
// them on key columns of its own (tests/test_gpu_cert_dedup_kernels.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cert_dedup_dev.h"
#include "cert_scan_dev.h"

namespace ibftk {

// In place of the verdict launch over rows [0, n): cert_dedup_insert_kernel (every row without a pre-flag into the table),
// cert_dedup_mark_kernel (bit 0: the row is its key's lowest row, bit 31: it gave up — the count words the tiled scan of
// cert_scan_dev.h takes: cert_scan_tiles_kernel, cert_scan_offsets_kernel), cert_dedup_apply_kernel (every representative's
// position in the dense batch, ascending, and its columns gathered there), the verdict launch over the dense batch (the host
// reads its size), cert_dedup_scatter_kernel (whole verdict words of the tree).
__global__ void __launch_bounds__(256) cert_dedup_insert_kernel(cdd::columns k, uint32_t n, uint32_t *__restrict__ table, uint32_t slot_mask,
                                                                uint32_t *__restrict__ slot_of) {
  const uint32_t row = blockIdx.x * 256u + threadIdx.x;
  if (row < n) slot_of[row] = cdd::insert_row(k, row, table, slot_mask);
}
__global__ void __launch_bounds__(256) cert_dedup_mark_kernel(const uint32_t *__restrict__ table, const uint32_t *__restrict__ slot_of, uint32_t n,
                                                              uint32_t *__restrict__ scan_word) {
  const uint32_t row = blockIdx.x * 256u + threadIdx.x;
  if (row < n) scan_word[row] = cdd::scan_word(table, slot_of[row], row);
}
// tile_off[tile].x: representatives in the tiles before this one (cert_scan_offsets_kernel with base 0)
__global__ void __launch_bounds__(1024) cert_dedup_apply_kernel(const uint32_t *__restrict__ scan_word, uint32_t n, const uint2 *__restrict__ tile_off,
                                                                cdd::columns k, uint32_t dense_base, uint32_t *__restrict__ dense_pos) {
  __shared__ uint32_t a[1024];
  const uint32_t t = threadIdx.x, i = blockIdx.x * 1024u + t;
  const uint32_t rep = i < n ? scan_word[i] & 1u : 0u;
  const uint32_t incl = block_scan_1024(a, rep);
  if (!rep) return;
  const uint32_t d = tile_off[blockIdx.x].x + incl - 1u;
  dense_pos[i] = d;
  cdd::gather_row(k, i, dense_base + d);
}
// dense_mask: the verdict words of the dense batch; mask: those of the tree's rows [0, n), every one of them stored whole
__global__ void __launch_bounds__(256) cert_dedup_scatter_kernel(const uint32_t *__restrict__ table, const uint32_t *__restrict__ slot_of,
                                                                 const uint32_t *__restrict__ dense_pos, const uint64_t *__restrict__ dense_mask,
                                                                 uint32_t n, uint64_t *__restrict__ mask) {
  const uint32_t row = blockIdx.x * 256u + threadIdx.x;
  const bool bit = row < n && cdd::scatter_bit(table, slot_of, dense_pos, dense_mask, row);
  const uint64_t word = __ballot(bit);
  if ((threadIdx.x & 63u) == 0 && row < n) mask[row >> 6] = word;
}
// ibft_cert_stats: the rows without a pre-flag among pre_a[0, n_a) (the tree's rows) and pre_b[0, n_b) (the batch of the deferred
// rows) → out[0], out[1] (device, and the mapped host words when not null).  acc: three words that are zero between launches —
// the workgroup that draws the last ticket delivers the sums and zeroes them again.
constexpr uint32_t CERT_DEDUP_COUNT_GRID = 64;
__global__ void __launch_bounds__(256) cert_dedup_count_kernel(const uint8_t *__restrict__ pre_a, uint32_t n_a, const uint8_t *__restrict__ pre_b,
                                                               uint32_t n_b, uint32_t *__restrict__ acc, uint32_t *__restrict__ out_dev,
                                                               uint32_t *__restrict__ out_host) {
  // at most CERT_DEDUP_COUNT_GRID workgroups stride the rows and add ONE pair of sums each (a device-scope atomic per wavefront
  // of a grid over all rows — 7 300 on one address at 467 172 rows — took 0.15 ms)
  __shared__ uint32_t part[2];
  if (threadIdx.x < 2u) part[threadIdx.x] = 0;
  __syncthreads();
  uint32_t ca = 0, cb = 0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_a + n_b; i += gridDim.x * 256u) {
    if (i < n_a) ca += pre_a[i] == 0;
    else cb += pre_b[i - n_a] == 0;
  }
  for (int o = 32; o; o >>= 1) {
    ca += (uint32_t)__shfl_xor((int)ca, o, 64);
    cb += (uint32_t)__shfl_xor((int)cb, o, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicAdd(part, ca);
    atomicAdd(part + 1, cb);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (part[0]) atomicAdd(acc, part[0]);
  if (part[1]) atomicAdd(acc + 1, part[1]);
  __threadfence();
  if (atomicAdd(acc + 2, 1u) != gridDim.x - 1u) return;
  __threadfence();
  const uint32_t sa = atomicExch(acc, 0u), sb = atomicExch(acc + 1, 0u);
  atomicExch(acc + 2, 0u);
  out_dev[0] = sa;
  out_dev[1] = sb;
  if (out_host) {
    out_host[0] = sa;
    out_host[1] = sb;
  }
}

// The dedup's front over rows [0, rows) of `cols` on `stream`: the table (`slots` words, cdd::table_slots) cleared to EMPTY,
// every row inserted (→ slot_of), marked (→ scan_word, `rows` words), the marks scanned over tiles (d_tiles: cert_scan_tiles(rows)
// cells) and every representative's position → dense_pos, its columns → row dense_base + position.  {representatives, rows
// that gave up} → stat_dev[0..1] and, when not null, stat_host[0..1].  Returns the status of the table's clear; the caller
// checks hipGetLastError() for the launches.
inline hipError_t cert_dedup_front_launch(hipStream_t stream, const cdd::columns &cols, uint32_t rows, uint32_t slots, uint32_t dense_base,
                                          uint32_t *d_table, uint32_t *d_slot_of, uint32_t *d_scan_word, uint2 *d_tiles, uint32_t *d_dense_pos,
                                          uint32_t *stat_dev, uint32_t *stat_host) {
  const uint32_t tiles = cert_scan_tiles(rows);
  const dim3 grid((rows + 255u) / 256u), group(256), tile_group(CERT_SCAN_TILE_ROWS);
  const hipError_t e = hipMemsetAsync(d_table, 0xFF, (size_t)slots * 4, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cert_dedup_insert_kernel, grid, group, 0, stream, cols, rows, d_table, slots - 1u, d_slot_of);
  hipLaunchKernelGGL(cert_dedup_mark_kernel, grid, group, 0, stream, (const uint32_t *)d_table, (const uint32_t *)d_slot_of, rows, d_scan_word);
  hipLaunchKernelGGL(cert_scan_tiles_kernel, dim3(tiles), tile_group, 0, stream, (const uint32_t *)d_scan_word, rows, d_tiles);
  hipLaunchKernelGGL(cert_scan_offsets_kernel, dim3(1), tile_group, 0, stream, d_tiles, tiles, 0u, 0u, stat_dev, stat_host);
  hipLaunchKernelGGL(cert_dedup_apply_kernel, dim3(tiles), tile_group, 0, stream, (const uint32_t *)d_scan_word, rows, (const uint2 *)d_tiles, cols,
                     dense_base, d_dense_pos);
  return hipSuccess;
}
// After the verdict launch over the dense batch (its words: d_dense_mask): every verdict word of rows [0, rows) → d_mask.
inline void cert_dedup_scatter_launch(hipStream_t stream, const uint32_t *d_table, const uint32_t *d_slot_of, const uint32_t *d_dense_pos,
                                      const uint64_t *d_dense_mask, uint32_t rows, uint64_t *d_mask) {
  hipLaunchKernelGGL(cert_dedup_scatter_kernel, dim3((rows + 255u) / 256u), dim3(256), 0, stream, d_table, d_slot_of, d_dense_pos, d_dense_mask, rows,
                     d_mask);
}
// Workgroups of the count over n_a + n_b (> 0) flag bytes: one per 256 of them, at most CERT_DEDUP_COUNT_GRID.
inline uint32_t cert_dedup_count_grid(uint32_t n_a, uint32_t n_b) { return std::min(CERT_DEDUP_COUNT_GRID, (n_a + n_b + 255u) / 256u); }
inline void cert_dedup_count_launch(hipStream_t stream, const uint8_t *d_pre_a, uint32_t n_a, const uint8_t *d_pre_b, uint32_t n_b, uint32_t *d_acc,
                                    uint32_t *out_dev, uint32_t *out_host) {
  hipLaunchKernelGGL(cert_dedup_count_kernel, dim3(cert_dedup_count_grid(n_a, n_b)), dim3(256), 0, stream, d_pre_a, n_a, d_pre_b, n_b, d_acc, out_dev,
                     out_host);
}

}  // namespace ibftk
