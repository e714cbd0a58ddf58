// What the bandwidth-bound row passes over a feature matrix x[n][C] share (norm.hip, pool.hip, interp.hip, field.hip).
//
// The convention: a thread owns one column group of one row, and the group is VEC wide -- VEC = 4 (one 16-byte access) when
// C % 4 == 0 and every pointer and row pitch involved is a multiple of 16 bytes, VEC = 1 (one dword) otherwise.  The host
// decides with aligned16() and launches the <4> or the <1> instantiation of the kernel; the kernel moves rows with ldv / stv.
// Flat passes walk the rows * C / VEC column groups with a grid from flat_grid().  Per-sample reductions cut every sample
// b = rows [off[b], off[b + 1]) into the same number G = sample_chunks(n, B) of row chunks on a grid (G, B, channel slabs)
// (ChunkLaunch on the host, chunk_lane() in the kernel), so the launch shape depends on n and B alone.
#pragma once
#include <algorithm>

#include "common.h"

namespace mink {

// ---- device side ----------------------------------------------------------------------------------------------------
template <typename T> struct Vec4;
template <> struct Vec4<float> { using type = float4; };
template <> struct Vec4<int> { using type = int4; };

template <int VEC, typename T>
__device__ __forceinline__ void ldv(const T *__restrict__ p, T (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const typename Vec4<T>::type t = *reinterpret_cast<const typename Vec4<T>::type *>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
template <int VEC, typename T>
__device__ __forceinline__ void stv(T *__restrict__ p, const T (&v)[VEC]) {
  if constexpr (VEC == 4)
    *reinterpret_cast<typename Vec4<T>::type *>(p) = typename Vec4<T>::type{v[0], v[1], v[2], v[3]};
  else
    p[0] = v[0];
}

// rows [lo, hi) of sample b, clamped into [0, n] (offsets that do not describe x cannot send a load out of bounds)
__device__ __forceinline__ void sample_range(const int *__restrict__ off, int b, int64_t n, int64_t &lo, int64_t &hi) {
  lo = off[b], hi = off[b + 1];
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < lo ? lo : (hi > n ? n : hi);
}

// the sample that owns `row`: the largest b in [0, B) with off[b] <= row (an empty sample shares its offset with the next
// one and is never the answer for a row inside it)
__device__ __forceinline__ int sample_of(const int *__restrict__ off, int B, int64_t row) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)off[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

// This thread's share of chunk blockIdx.x (of gridDim.x) of sample blockIdx.y: the chunk is rows [r0, r1); the thread owns
// column group cg (ncg = C / VEC of them, tprb per workgroup, blockIdx.z walks further slabs of W = tprb * VEC channels) as
// column lane cl and the rows r0 + rl, r0 + rl + rlanes, ... as row lane rl.  Threads with rl >= rlanes or cg >= ncg idle.
struct ChunkLane {
  int64_t r0, r1;
  int ncg, rlanes, W, cl, rl, cg;
};
template <int VEC, int THREADS>
__device__ __forceinline__ ChunkLane chunk_lane(const int *__restrict__ off, int64_t n, int C, int tprb) {
  const int G = gridDim.x, g = blockIdx.x;
  int64_t lo, hi;
  sample_range(off, blockIdx.y, n, lo, hi);
  const int64_t len = hi - lo;
  ChunkLane t;
  t.r0 = lo + len * g / G, t.r1 = lo + len * (g + 1) / G;
  t.ncg = C / VEC, t.rlanes = THREADS / tprb, t.W = tprb * VEC;
  t.cl = threadIdx.x % tprb, t.rl = threadIdx.x / tprb;
  t.cg = blockIdx.z * tprb + t.cl;
  return t;
}

// a query row (b, x, y, z): false for NaN / infinite / far outside the key space (integers are exact in fp32 below 65536)
__device__ __forceinline__ bool query_in_range(const float4 q) {
  if (!(fabsf(q.x) < 65536.f && fabsf(q.y) < 65536.f && fabsf(q.z) < 65536.f && fabsf(q.w) < 65536.f)) return false;
  return true;  // (an early return, as the callers had it: a plain `return a && b && c && d` orders one s_and differently)
}

// ---- host side ------------------------------------------------------------------------------------------------------
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }  // (an absent, NULL operand counts as aligned)

static inline unsigned flat_grid(int64_t work, int threads, int64_t cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(work, threads), cap));
}

constexpr int kSampleMaxBlocks = 2048;  // B * G stays near this
static inline int sample_chunks(int64_t n, int B) {
  const int64_t cap = std::max<int64_t>(1, kSampleMaxBlocks / std::max(B, 1));
  return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 256), cap));
}

// launch geometry of a per-sample chunked reduction; its dynamic LDS is rlanes * W elements of the kernel's own partial type
struct ChunkLaunch {
  int tprb, rlanes, W;
  dim3 grid;
  ChunkLaunch(int64_t n, int C, int B, int VEC, int threads)
      : tprb(std::min(C / VEC, threads)), rlanes(threads / tprb), W(tprb * VEC),
        grid((unsigned)sample_chunks(n, B), (unsigned)B, (unsigned)cdiv(C / VEC, tprb)) {}
};

#define MINK_REQUIRE_WORKSPACE(name, bytes, need, ptr)                                                                   \
  MINK_REQUIRE((bytes) >= (need) && ((uintptr_t)(ptr) & 7) == 0, name ": workspace of %lld bytes, %lld needed (8-byte aligned)", \
               (long long)(bytes), (long long)(need))

#define MINK_REQUIRE_ROWS_C(name, rows, max_rows, C)                                                                     \
  MINK_REQUIRE((rows) >= 0 && (rows) <= (max_rows) && (C) >= 1 && (C) <= 4096, name ": bad shape (rows=%lld, C=%d; 1 <= C <= 4096)", \
               (long long)(rows), (int)(C))

}  // namespace mink
