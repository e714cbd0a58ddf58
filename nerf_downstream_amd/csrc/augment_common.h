// Device helpers shared by the scene-augmentation programs (augment.hip: MINK_AUG_*, seg_augment.hip: MINK_SEGAUG_*).
#pragma once
#include "common.h"

namespace mink {
namespace {

constexpr int kBlock = 256;

struct Philox {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return {c0, c1, c2, c3};
}

__device__ __forceinline__ float u01(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }  // [0,1), exact

__device__ __forceinline__ int scene_of(const int *__restrict__ scene_offsets, int n_scenes, int64_t i) {
  int lo = 0, hi = n_scenes;  // scene b with scene_offsets[b] <= i < scene_offsets[b+1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)scene_offsets[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// order-preserving float <-> uint (for atomicMax)
__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// row i of a [n][4] coordinate array that is float32 or (as_int) int32, e.g. straight from mink_decode_plenoxel
__device__ __forceinline__ float4 load_coord(const void *__restrict__ coords, int64_t i, bool as_int) {
  if (as_int) {
    const int4 v = *reinterpret_cast<const int4 *>((const int *)coords + 4 * i);
    return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
  }
  return *reinterpret_cast<const float4 *>((const float *)coords + 4 * i);
}

// one block: exclusive scan of block_counts[nb] -> block_offsets[nb], total -> *n_kept
__global__ __launch_bounds__(kBlock) void augment_scan_kernel(const int *__restrict__ block_counts, int nb,
                                                              int *__restrict__ block_offsets, int *__restrict__ n_kept) {
  __shared__ int s[kBlock];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += kBlock) {
    const int j = base + threadIdx.x;
    const int v = j < nb ? block_counts[j] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {  // Hillis-Steele inclusive scan
      const int add = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    if (j < nb) block_offsets[j] = carry + s[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == kBlock - 1) carry += s[kBlock - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_kept = carry;
}

constexpr int kDraws = MINK_AUG_MAX_CHANNELS / 4;  // Philox draws that can carry feature noise

struct RawCols {
  int inv[MINK_AUG_MAX_CHANNELS];  // feature column of every raw-layout column, -1 = not selected
  int raw[MINK_AUG_MAX_CHANNELS];  // raw-layout column of every feature column (CO3D: [xyzs 0:3 | density 3 | sh 4:31], co3d.py:205-214;
                                   // ScanNet: [xyzs 0:3 | dists 3 | density 4 | sh 5:32]), -1 = none
};

}  // namespace
}  // namespace mink
