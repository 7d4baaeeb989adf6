// cert_scan_dev.h — the level scans of the certificate tree (kernels.hip.h §8f; ibft_verify_certificates_wire expands the
// tree one level at a time): after cert_walk_kernel<false> has counted every row's nested messages, a scan turns the counts
// of rows [lo, hi) into each row's first_child, the ordered list of the rows whose digest is deferred, and the two totals the
// host reads to size the next level's launches.  Two forms, one workgroup or three launches over tiles of 1 024 rows;
// cert_scan_launch is the only place that picks between them and the only place that knows their geometry.  The kernels
// need nothing but wire::node_info, so the test library (devtest.hip: devtest_cert_scan) runs them on count columns of its
// own (tests/test_gpu_cert_scan.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_dev.h"

namespace ibftk {

// A level of at most this many rows is scanned by one workgroup (at most 8 rows per thread); a longer one by tiles.
constexpr uint32_t CERT_SCAN_ONE_GROUP_MAX = 8192;
constexpr uint32_t CERT_SCAN_TILE_ROWS = 1024;  // rows per tile = threads per workgroup of all four kernels

// The inclusive scan of one value per thread across a workgroup of 1 024 threads (Hillis–Steele through LDS: ten steps, each
// read of a neighbour's sum between two barriers).  value[k] of thread t becomes Σ value[k] of threads 0 … t; the total is
// part[k][1023].  Every thread of the workgroup calls it; part[k] is 1 024 cells and free again behind a barrier of the
// caller's.  N values are scanned in the same ten steps (the level scans carry a count and a deferred flag).
template <int N, class T>
__device__ __forceinline__ void block_scan_1024_n(T *const (&part)[N], T (&value)[N]) {
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; k++) part[k][t] = value[k];
  __syncthreads();
  for (uint32_t o = 1; o < 1024u; o <<= 1) {
    T v[N];
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = t >= o ? part[k][t - o] : (T)0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) part[k][t] += v[k];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < N; k++) value[k] = part[k][t];
}
// one value (T: uint32_t, or a uint64_t that packs two counts): returns the thread's inclusive sum
template <class T>
__device__ __forceinline__ T block_scan_1024(T *part, T value) {
  T *const p[1] = {part};
  T v[1] = {value};
  block_scan_1024_n(p, v);
  return v[0];
}
// a pair of values: they come back as the thread's inclusive sums
template <class T>
__device__ __forceinline__ void block_scan_1024(T *part, T *part2, T &value, T &value2) {
  T *const p[2] = {part, part2};
  T v[2] = {value, value2};
  block_scan_1024_n(p, v);
  value = v[0];
  value2 = v[1];
}

// first_child of rows [lo, hi) = base + exclusive prefix sum of their child counts; the sum → total[0] (device and host).
// The rows whose digest is deferred (wire::tree_deferred: they carry a certificate, or are long) are listed the same way:
// deferred_rows[slot_base + rank] = row, their count → total[1].  child_count[i] bit 31 = row lo + i is deferred.
__global__ void __launch_bounds__(1024) cert_scan_kernel(const uint32_t *__restrict__ child_count, wire::node_info *__restrict__ nodes,
                                                         uint32_t lo, uint32_t hi, uint32_t base, uint32_t slot_base,
                                                         uint32_t *__restrict__ deferred_rows, uint32_t *__restrict__ total_dev,
                                                         uint32_t *__restrict__ total_host) {
  __shared__ uint32_t part[1024], part2[1024];
  const uint32_t n = hi - lo, t = threadIdx.x, per = (n + 1023u) / 1024u;
  const uint32_t b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
  uint32_t sum = 0, sum2 = 0;
  for (uint32_t i = b; i < e; i++) {
    const uint32_t c = child_count[i];
    sum += c & 0x7FFFFFFFu;
    sum2 += c >> 31;
  }
  uint32_t incl = sum, incl2 = sum2;
  block_scan_1024(part, part2, incl, incl2);
  uint32_t run = base + incl - sum, run2 = slot_base + incl2 - sum2;
  for (uint32_t i = b; i < e; i++) {
    const uint32_t c = child_count[i];
    nodes[lo + i].first_child = run;
    run += c & 0x7FFFFFFFu;
    if (c >> 31) deferred_rows[run2++] = lo + i;
  }
  if (t == 1023u) {
    total_dev[0] = part[1023];
    total_dev[1] = part2[1023];
    if (total_host) {
      total_host[0] = part[1023];
      total_host[1] = part2[1023];
    }
  }
}
// The same scan for a long level (the single workgroup above walks n/1024 rows per thread: 0.8 ms at 467 k rows): (A) per-tile
// sums of 1 024 rows, (B) one workgroup scans the tile sums (≤ 1 024 tiles per pass of its loop) and delivers the totals, (C) every
// tile scans its own rows and adds its offset.
__global__ void __launch_bounds__(1024) cert_scan_tiles_kernel(const uint32_t *__restrict__ child_count, uint32_t n, uint2 *__restrict__ tile_sum) {
  __shared__ uint32_t a[1024], b[1024];
  const uint32_t t = threadIdx.x, i = blockIdx.x * 1024u + t;
  const uint32_t c = i < n ? child_count[i] : 0u;
  a[t] = c & 0x7FFFFFFFu;
  b[t] = c >> 31;
  __syncthreads();
  for (uint32_t o = 512u; o; o >>= 1) {
    if (t < o) {
      a[t] += a[t + o];
      b[t] += b[t + o];
    }
    __syncthreads();
  }
  if (t == 0) tile_sum[blockIdx.x] = make_uint2(a[0], b[0]);
}
__global__ void __launch_bounds__(1024) cert_scan_offsets_kernel(uint2 *__restrict__ tile_sum, uint32_t tiles, uint32_t base, uint32_t slot_base,
                                                                 uint32_t *__restrict__ total_dev, uint32_t *__restrict__ total_host) {
  __shared__ uint32_t a[1024], b[1024];
  const uint32_t t = threadIdx.x;
  uint32_t run = 0, run2 = 0;  // sums of the passes before this one (the same in every thread)
  for (uint32_t t0 = 0; t0 < tiles; t0 += 1024u) {
    const uint2 v = t0 + t < tiles ? tile_sum[t0 + t] : make_uint2(0, 0);
    uint32_t x = v.x, y = v.y;
    block_scan_1024(a, b, x, y);
    if (t0 + t < tiles) tile_sum[t0 + t] = make_uint2(base + run + x - v.x, slot_base + run2 + y - v.y);  // exclusive, with the bases
    run += a[1023];
    run2 += b[1023];
    __syncthreads();
  }
  if (t == 0) {
    total_dev[0] = run;
    total_dev[1] = run2;
    if (total_host) {
      total_host[0] = run;
      total_host[1] = run2;
    }
  }
}
__global__ void __launch_bounds__(1024) cert_scan_apply_kernel(const uint32_t *__restrict__ child_count, wire::node_info *__restrict__ nodes,
                                                               uint32_t lo, uint32_t n, const uint2 *__restrict__ tile_off,
                                                               uint32_t *__restrict__ deferred_rows) {
  __shared__ uint32_t a[1024], b[1024];
  const uint32_t t = threadIdx.x, i = blockIdx.x * 1024u + t;
  const uint32_t c = i < n ? child_count[i] : 0u, cnt = c & 0x7FFFFFFFu, def = c >> 31;
  uint32_t x = cnt, y = def;
  block_scan_1024(a, b, x, y);
  if (i >= n) return;
  const uint2 off = tile_off[blockIdx.x];
  nodes[lo + i].first_child = off.x + x - cnt;
  if (def) deferred_rows[off.y + y - 1u] = lo + i;
}

// Tiles of a level of cnt rows: the tiled form needs that many uint2 cells at d_tiles.
inline uint32_t cert_scan_tiles(uint32_t cnt) { return (cnt + CERT_SCAN_TILE_ROWS - 1u) / CERT_SCAN_TILE_ROWS; }
// The scan of rows [lo, lo + cnt) on `stream`: child_count[0, cnt) → nodes[lo, lo + cnt).first_child (from `base`),
// deferred_rows[slot_base, …), total_dev[0..1] and, when not null, total_host[0..1].  one_group: cert_scan_kernel, else the
// three tile kernels (d_tiles is not touched by the former).  The caller checks hipGetLastError().
inline void cert_scan_launch(hipStream_t stream, bool one_group, const uint32_t *d_count, wire::node_info *d_nodes, uint32_t lo, uint32_t cnt,
                             uint32_t base, uint32_t slot_base, uint32_t *d_deferred_rows, uint2 *d_tiles, uint32_t *d_total,
                             uint32_t *total_host) {
  const dim3 group(CERT_SCAN_TILE_ROWS);
  if (one_group) {
    hipLaunchKernelGGL(cert_scan_kernel, dim3(1), group, 0, stream, d_count, d_nodes, lo, lo + cnt, base, slot_base, d_deferred_rows, d_total,
                       total_host);
  } else {  // a long level: per-tile sums, their scan, per-tile scans
    const uint32_t tiles = cert_scan_tiles(cnt);
    hipLaunchKernelGGL(cert_scan_tiles_kernel, dim3(tiles), group, 0, stream, d_count, cnt, d_tiles);
    hipLaunchKernelGGL(cert_scan_offsets_kernel, dim3(1), group, 0, stream, d_tiles, tiles, base, slot_base, d_total, total_host);
    hipLaunchKernelGGL(cert_scan_apply_kernel, dim3(tiles), group, 0, stream, d_count, d_nodes, lo, cnt, (const uint2 *)d_tiles, d_deferred_rows);
  }
}

}  // namespace ibftk
