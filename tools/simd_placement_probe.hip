// tools/simd_placement_probe.hip — which SIMD of its compute unit each wavefront of a 512-thread workgroup lands on.
//
// ecrecover_rows_pair_kernel pairs main wavefront w (0…3) of a workgroup with helper wavefront w + 4 and counts on the two
// sharing a SIMD, with every SIMD holding one main wavefront and one helper.  This probe launches the same shape (512
// threads, one workgroup per compute unit: 81 KB of LDS make a second one not fit) and lets lane 0 of every wavefront read
// HW_ID (SIMD_ID = bits 5:4, CU_ID = bits 11:8, SH_ID bit 12, SE_ID bits 15:13) and XCC_ID, written out with an ordinary
// vector store.  It prints, for each wavefront index, how often it landed on each SIMD, and whether waves w and w + 4 shared one.
//
//   hipcc --offload-arch=gfx950 -O2 -o tools/simd_placement_probe tools/simd_placement_probe.hip && tools/simd_placement_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

constexpr int WAVES = 8, BLOCKS = 1024;
constexpr int LDS_WORDS = 81 * 1024 / 4;

__global__ void __launch_bounds__(64 * WAVES) placement_kernel(uint32_t *out) {
  __shared__ uint32_t pad[LDS_WORDS];
  uint32_t hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  const uint32_t w = threadIdx.x >> 6;
  pad[threadIdx.x] = hw;  // (the LDS is allocated, not needed)
  __syncthreads();
  if ((threadIdx.x & 63u) == 0) {
    out[2 * (blockIdx.x * WAVES + w)] = pad[threadIdx.x];
    out[2 * (blockIdx.x * WAVES + w) + 1] = xcc;
  }
}

#define CHK(x)                                                        \
  do {                                                                \
    hipError_t e_ = (x);                                              \
    if (e_ != hipSuccess) {                                           \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));         \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  const size_t words = 2ull * BLOCKS * WAVES;
  uint32_t *d = nullptr;
  CHK(hipMalloc(&d, words * 4));
  CHK(hipMemset(d, 0xFF, words * 4));
  hipLaunchKernelGGL(placement_kernel, dim3(BLOCKS), dim3(64 * WAVES), 0, 0, d);
  CHK(hipGetLastError());
  CHK(hipDeviceSynchronize());
  std::vector<uint32_t> h(words);
  CHK(hipMemcpy(h.data(), d, words * 4, hipMemcpyDeviceToHost));
  CHK(hipFree(d));
  int hist[WAVES][4] = {};
  int pair_same[4] = {}, mains_cover = 0, helpers_cover = 0;
  for (int b = 0; b < BLOCKS; b++) {
    int simd[WAVES];
    for (int w = 0; w < WAVES; w++) {
      simd[w] = (h[2 * (b * WAVES + w)] >> 4) & 3;
      hist[w][simd[w]]++;
    }
    int m = 0, hm = 0;
    for (int w = 0; w < 4; w++) {
      pair_same[w] += simd[w] == simd[w + 4];
      m |= 1 << simd[w];
      hm |= 1 << simd[w + 4];
    }
    mains_cover += m == 15;
    helpers_cover += hm == 15;
  }
  printf("workgroups: %d of %d threads (one per compute unit)\n", BLOCKS, 64 * WAVES);
  printf("wave  SIMD0 SIMD1 SIMD2 SIMD3\n");
  for (int w = 0; w < WAVES; w++) printf("%4d  %5d %5d %5d %5d\n", w, hist[w][0], hist[w][1], hist[w][2], hist[w][3]);
  for (int w = 0; w < 4; w++) printf("waves %d and %d on the same SIMD: %d / %d workgroups\n", w, w + 4, pair_same[w], BLOCKS);
  printf("waves 0-3 on four different SIMDs: %d / %d; waves 4-7: %d / %d\n", mains_cover, BLOCKS, helpers_cover, BLOCKS);
  printf("first workgroups (HW_ID, XCC_ID of waves 0-7):\n");
  for (int b = 0; b < 4; b++) {
    for (int w = 0; w < WAVES; w++) printf(" %08x/%u", h[2 * (b * WAVES + w)], h[2 * (b * WAVES + w) + 1]);
    printf("\n");
  }
  return 0;
}
