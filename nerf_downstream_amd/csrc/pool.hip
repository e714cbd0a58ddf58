// The sparse pooling family on gfx950: local average / sum / max pooling over a neighbour table whose windows may overlap
// (ME.MinkowskiAvgPooling, MinkowskiSumPooling beyond kernel_size == stride, MinkowskiMaxPooling) and the segmented global
// max / sum pooling over the batch offsets (ME.MinkowskiGlobalMaxPooling, MinkowskiGlobalSumPooling) -- the row-pass
// family, in the anonymous namespace -- and, behind it in namespace mink proper, the three pools of the classification
// networks: the non-overlapping sum pooling of the ResNet stem (mink_pool_sum_*), the max pooling of the dense 2-D
// baseline (mink_pool_max_*) and the global average (mink_global_avg_*).  Those three take C % 4 == 0 and 16-byte aligned
// pointers only (16-byte lanes, ld4 / st4 of ew_common.h) and have no dword form.  The stem's sum pool fused with its
// batch norm and ReLU is in batchnorm.hip.
//
// The row-pass family: all of them are bandwidth-bound row passes over x[n][C] (row pitch ldx >= C): a thread owns one column group of one row,
// 16 bytes wide when C % 4 == 0 and every pointer is 16-byte aligned (and ldx % 4 == 0), one dword otherwise (C = 1, 3, 70).
//
// Local pools.  nbr[n_out][K] holds the input row of output o at kernel offset k, or -1.  Forward walks k = 0 .. K-1 in
// order and skips the empty entries; backward gathers through the transposed table nbr_t[n_in][K] (nbr_t[i][k] = o iff
// nbr[o][k] = i, the windows that contain row i), again k ascending: one owner per element, no atomics, a fixed order.
//   average: y[o] = (sum of the present rows) / cnt[o], cnt[o] = number of present entries -- NOT the kernel volume; one true
//            fp32 division per element (dx[i] = sum of dy[o] / cnt[o], the same division per term)
//   max    : the first present entry in offset order wins a tie (only a larger value replaces); arg[o][c] = its input row.
//            A row with no present entry gets y = 0, arg = -1.  A NaN replaces a number and is never replaced, so the
//            first NaN in offset order is the result and the arg: torch's rule (the value of max_pool1d / amax, the
//            index of max(dim)).
//
// Global pools.  Sample b owns rows [off[b], off[b+1]) (the manager's device-resident offsets; never read by the host).  The
// launch shape is the per-sample chunked reduction of rowpass.h: grid (G, B, channel slabs), every sample cut into the same
// number G of row chunks chosen from n and B alone, one partial per workgroup, then one wave per (sample, channel) combines
// the G partials -- lane l takes partials l, l + 64, ... in order, then a fixed butterfly.  Two launches forward, one
// backward, whatever B is.  An empty sample finds an empty range: y = 0, arg = -1.
//   max: the combine rule is a total order (a NaN above every number as in torch, then the larger value, then the lower
//        row), so arg[b][c] is the LOWEST row attaining the maximum -- the first NaN of the sample if it has one -- however
//        the rows were spread over threads.  Backward is one pass over the rows of dx that compares the row
//        index with arg: dx[i][c] = arg[b][c] == i ? dy[b][c] : 0 -- no scatter.
//   sum: accumulated in DOUBLE from the first add on and rounded to fp32 once; backward dx[i] = dy[b].
// Determinism: rows -> threads -> partials -> results is a fixed assignment in a fixed order: two runs are bitwise equal.
#include <algorithm>

#include "ew_common.h"
#include "rowpass.h"

namespace mink {
namespace {

constexpr int PB = 256;  // threads per workgroup

// ------------------------------------------------------------------------------------------------ local pools
enum { kSum = 0, kAvg = 1 };

template <int VEC, int MODE>
__global__ __launch_bounds__(PB) void pool_local_fwd_kernel(const float *__restrict__ x, int ldx, int C, const int *__restrict__ nbr,
                                                            int64_t n_out, int K, float *__restrict__ y, int *__restrict__ cnt) {
  const int ncg = C / VEC;
  const int64_t total = n_out * ncg;
  for (int64_t idx = (int64_t)blockIdx.x * PB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * PB) {
    const int64_t o = idx / ncg;
    const int c = (int)(idx - o * ncg) * VEC;
    const int *__restrict__ row = nbr + o * K;
    float s[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = 0.f;
    int m = 0;
    for (int k = 0; k < K; ++k) {
      const int i = row[k];
      if (i >= 0) {
        float v[VEC];
        ldv<VEC>(x + (int64_t)i * ldx + c, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] += v[j];
        ++m;
      }
    }
    if (MODE == kAvg && m > 0) {
      const float d = (float)m;
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] = s[j] / d;
    }
    stv<VEC>(y + o * C + c, s);
    if (cnt && c == 0) cnt[o] = m;
  }
}

template <int VEC, int MODE>
__global__ __launch_bounds__(PB) void pool_local_bwd_kernel(const float *__restrict__ dy, int C, const int *__restrict__ nbr_t,
                                                            int64_t n_in, int K, const int *__restrict__ cnt,
                                                            float *__restrict__ dx) {
  const int ncg = C / VEC;
  const int64_t total = n_in * ncg;
  for (int64_t idx = (int64_t)blockIdx.x * PB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * PB) {
    const int64_t i = idx / ncg;
    const int c = (int)(idx - i * ncg) * VEC;
    const int *__restrict__ row = nbr_t + i * K;
    float s[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = 0.f;
    for (int k = 0; k < K; ++k) {
      const int o = row[k];
      if (o >= 0) {
        float g[VEC];
        ldv<VEC>(dy + (int64_t)o * C + c, g);
        if (MODE == kAvg) {
          const float d = (float)cnt[o];  // (>= 1: window o contains row i)
#pragma unroll
          for (int j = 0; j < VEC; ++j) g[j] = g[j] / d;
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] += g[j];
      }
    }
    stv<VEC>(dx + i * C + c, s);
  }
}

template <int VEC>
__global__ __launch_bounds__(PB) void pool_local_max_fwd_kernel(const float *__restrict__ x, int ldx, int C,
                                                                const int *__restrict__ nbr, int64_t n_out, int K,
                                                                float *__restrict__ y, int *__restrict__ arg) {
  const int ncg = C / VEC;
  const int64_t total = n_out * ncg;
  for (int64_t idx = (int64_t)blockIdx.x * PB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * PB) {
    const int64_t o = idx / ncg;
    const int c = (int)(idx - o * ncg) * VEC;
    const int *__restrict__ row = nbr + o * K;
    float m[VEC];
    int a[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) m[j] = 0.f, a[j] = -1;
    for (int k = 0; k < K; ++k) {
      const int i = row[k];
      if (i >= 0) {
        float v[VEC];
        ldv<VEC>(x + (int64_t)i * ldx + c, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (a[j] < 0 || max_replaces(v[j], m[j])) m[j] = v[j], a[j] = i;  // (the lowest k wins a tie)
      }
    }
    stv<VEC>(y + o * C + c, m);
    stv<VEC>(arg + o * C + c, a);
  }
}

template <int VEC>
__global__ __launch_bounds__(PB) void pool_local_max_bwd_kernel(const float *__restrict__ dy, const int *__restrict__ arg, int C,
                                                                const int *__restrict__ nbr_t, int64_t n_in, int K,
                                                                float *__restrict__ dx) {
  const int ncg = C / VEC;
  const int64_t total = n_in * ncg;
  for (int64_t idx = (int64_t)blockIdx.x * PB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * PB) {
    const int64_t i = idx / ncg;
    const int c = (int)(idx - i * ncg) * VEC;
    const int *__restrict__ row = nbr_t + i * K;
    float s[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = 0.f;
    for (int k = 0; k < K; ++k) {
      const int o = row[k];
      if (o >= 0) {
        float g[VEC];
        int a[VEC];
        ldv<VEC>(dy + (int64_t)o * C + c, g);
        ldv<VEC>(arg + (int64_t)o * C + c, a);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] += a[j] == (int)i ? g[j] : 0.f;
      }
    }
    stv<VEC>(dx + i * C + c, s);
  }
}

// ------------------------------------------------------------------------------------------------ global pools
// (m, a) <- the better of (m, a) and (v, r): a present candidate (r >= 0) beats an absent one, then a NaN beats a number,
// then the larger value, then the lower row (also between two NaNs).  A total order, so both sides of a butterfly exchange
// end with the same pair, NaN or not.
__device__ __forceinline__ void max_take(float &m, int &a, float v, int r) {
  const bool tie = v == m || (v != v && m != m);
  if (r >= 0 && (a < 0 || max_replaces(v, m) || (tie && r < a))) m = v, a = r;
}

// Chunk g of sample b -> pval / parg [b][g][C].  A thread owns VEC channels (column group cg) and the rows rl, rl + rlanes,
// ... of the chunk, ascending; tprb column groups per workgroup, blockIdx.z walks further slabs of tprb groups.
template <int VEC>
__global__ __launch_bounds__(PB) void gmax_partial_kernel(const float *__restrict__ x, int ldx, const int *__restrict__ off,
                                                          int64_t n, int C, int tprb, float *__restrict__ pval,
                                                          int *__restrict__ parg) {
  extern __shared__ __align__(16) unsigned char s_raw[];  // [rlanes][W] float, then [rlanes][W] int
  const int b = blockIdx.y, G = gridDim.x, g = blockIdx.x;
  const auto [r0, r1, ncg, rlanes, W, cl, rl, cg] = chunk_lane<VEC, PB>(off, n, C, tprb);
  float *s_val = reinterpret_cast<float *>(s_raw);
  int *s_arg = reinterpret_cast<int *>(s_raw) + rlanes * W;
  float m[VEC];
  int a[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) m[k] = 0.f, a[k] = -1;
  if (rl < rlanes && cg < ncg) {
    const int c = cg * VEC;
#pragma unroll 4
    for (int64_t row = r0 + rl; row < r1; row += rlanes) {
      float v[VEC];
      ldv<VEC>(x + row * ldx + c, v);
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        if (a[k] < 0 || max_replaces(v[k], m[k])) m[k] = v[k], a[k] = (int)row;
    }
  }
  if (rl < rlanes) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) s_val[rl * W + cl * VEC + k] = m[k], s_arg[rl * W + cl * VEC + k] = a[k];
  }
  __syncthreads();
  const int64_t base = ((int64_t)b * G + g) * C;
  for (int e = threadIdx.x; e < W; e += PB) {
    const int c = blockIdx.z * W + e;
    if (c >= C) continue;
    float bm = s_val[e];
    int ba = s_arg[e];
    for (int r = 1; r < rlanes; ++r) max_take(bm, ba, s_val[r * W + e], s_arg[r * W + e]);
    pval[base + c] = bm;
    parg[base + c] = ba;
  }
}

// grid (ceil(C / 4), B): one wave per (sample, channel) combines the G chunk partials
__global__ __launch_bounds__(PB) void gmax_finalize_kernel(const float *__restrict__ pval, const int *__restrict__ parg, int G, int C,
                                                           float *__restrict__ y, int *__restrict__ arg) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (c >= C) return;  // whole wave
  const int lane = threadIdx.x & 63;
  const int64_t base = (int64_t)b * G * C + c;
  float m = 0.f;
  int a = -1;
  for (int j = lane; j < G; j += 64) max_take(m, a, pval[base + (int64_t)j * C], parg[base + (int64_t)j * C]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(a, o, 64);
    max_take(m, a, ov, oa);
  }
  if (lane == 0) {
    y[(int64_t)b * C + c] = a < 0 ? 0.f : m;
    arg[(int64_t)b * C + c] = a;
  }
}

template <int VEC>
__global__ __launch_bounds__(PB) void gsum_partial_kernel(const float *__restrict__ x, int ldx, const int *__restrict__ off,
                                                          int64_t n, int C, int tprb, double *__restrict__ partial) {
  extern __shared__ __align__(16) unsigned char s_raw[];  // [rlanes][W] double
  double *s_red = reinterpret_cast<double *>(s_raw);
  const int b = blockIdx.y, G = gridDim.x, g = blockIdx.x;
  const auto [r0, r1, ncg, rlanes, W, cl, rl, cg] = chunk_lane<VEC, PB>(off, n, C, tprb);
  double s[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) s[k] = 0.0;
  if (rl < rlanes && cg < ncg) {
    const int c = cg * VEC;
#pragma unroll 4
    for (int64_t row = r0 + rl; row < r1; row += rlanes) {
      float v[VEC];
      ldv<VEC>(x + row * ldx + c, v);
#pragma unroll
      for (int k = 0; k < VEC; ++k) s[k] += (double)v[k];
    }
  }
  if (rl < rlanes) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) s_red[rl * W + cl * VEC + k] = s[k];
  }
  __syncthreads();
  const int64_t base = ((int64_t)b * G + g) * C;
  for (int e = threadIdx.x; e < W; e += PB) {
    const int c = blockIdx.z * W + e;
    if (c >= C) continue;
    double t = 0.0;
    for (int r = 0; r < rlanes; ++r) t += s_red[r * W + e];
    partial[base + c] = t;
  }
}

__global__ __launch_bounds__(PB) void gsum_finalize_kernel(const double *__restrict__ partial, int G, int C, float *__restrict__ y) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (c >= C) return;  // whole wave
  const int lane = threadIdx.x & 63;
  const int64_t base = (int64_t)b * G * C + c;
  double s = 0.0;
  for (int j = lane; j < G; j += 64) s += partial[base + (int64_t)j * C];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) y[(int64_t)b * C + c] = (float)s;  // the one rounding
}

// MAX: dx[i][c] = arg[b][c] == i ? dy[b][c] : 0;  !MAX: dx[i][c] = dy[b][c].  Flat over the n * C / VEC column groups.
template <int VEC, bool MAX>
__global__ __launch_bounds__(PB) void gpool_bwd_kernel(const float *__restrict__ dy, const int *__restrict__ arg, int64_t n, int C,
                                                       const int *__restrict__ off, int B, float *__restrict__ dx) {
  const int ncg = C / VEC;
  const int64_t total = n * ncg;
  int b = 0;
  int64_t lo = 0, hi = 0;  // the cached sample's rows: empty until the first search
  for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < total; i += (int64_t)gridDim.x * PB) {
    const int64_t row = i / ncg;
    const int c = (int)(i - row * ncg) * VEC;
    if (row < lo || row >= hi) {
      b = sample_of(off, B, row);
      lo = off[b], hi = off[b + 1];
    }
    float g[VEC];
    ldv<VEC>(dy + (int64_t)b * C + c, g);
    if (MAX) {
      int a[VEC];
      ldv<VEC>(arg + (int64_t)b * C + c, a);
#pragma unroll
      for (int k = 0; k < VEC; ++k) g[k] = a[k] == (int)row ? g[k] : 0.f;
    }
    stv<VEC>(dx + i * VEC, g);
  }
}

}  // namespace

// ------------------------------------------------------------------------- pooling
__global__ __launch_bounds__(EB) void pool_sum_fwd_kernel(const float *__restrict__ x, int ldx, int C4,
                                                          const int *__restrict__ nbr, int64_t n_out, int K,
                                                          float *__restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (idx >= n_out * C4) return;
  const int64_t o = idx / C4;
  const int c = (int)(idx - o * C4) * 4;
  float4 s = make_float4(0, 0, 0, 0);
  for (int k = 0; k < K; ++k) {
    const int i = nbr[o * K + k];
    if (i >= 0) {
      const float4 v = ld4(x + (int64_t)i * ldx + c);
      s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
    }
  }
  st4(y + o * (int64_t)(4 * C4) + c, s);
}

__global__ __launch_bounds__(EB) void pool_sum_bwd_kernel(const float *__restrict__ dy, int C4,
                                                          const int *__restrict__ in2out, int64_t n_in,
                                                          float *__restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (idx >= n_in * C4) return;
  const int64_t i = idx / C4;
  const int c = (int)(idx - i * C4) * 4;
  st4(dx + i * (int64_t)(4 * C4) + c, ld4(dy + (int64_t)in2out[i] * (4 * C4) + c));
}

// Max pooling over a neighbour table (overlapping windows allowed: the dense 2-D baseline's 3x3 stride-2 pooling).
// arg[o][c] = input row holding the maximum (the first one in offset order, as torch's window scan picks it).
__global__ __launch_bounds__(EB) void pool_max_fwd_kernel(const float *__restrict__ x, int C4, const int *__restrict__ nbr,
                                                          int64_t n_out, int K, float *__restrict__ y, int *__restrict__ arg) {
  const int64_t idx = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (idx >= n_out * C4) return;
  const int64_t o = idx / C4;
  const int c = (int)(idx - o * C4) * 4;
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  int4 a = make_int4(-1, -1, -1, -1);
  for (int k = 0; k < K; ++k) {
    const int i = nbr[o * K + k];
    if (i >= 0) {
      const float4 v = ld4(x + (int64_t)i * (4 * C4) + c);
      if (a.x < 0 || max_replaces(v.x, m.x)) m.x = v.x, a.x = i;  // (torch's rule: the first NaN of the window wins, else
      if (a.y < 0 || max_replaces(v.y, m.y)) m.y = v.y, a.y = i;  //  the first of the largest numbers)
      if (a.z < 0 || max_replaces(v.z, m.z)) m.z = v.z, a.z = i;
      if (a.w < 0 || max_replaces(v.w, m.w)) m.w = v.w, a.w = i;
    }
  }
  st4(y + o * (int64_t)(4 * C4) + c, m);
  *reinterpret_cast<int4 *>(arg + o * (int64_t)(4 * C4) + c) = a;
}

// dx[i][c] = sum of dy[o][c] over the windows o that contain i and chose it (gathered through the transposed table:
// no atomics, one owner per element)
__global__ __launch_bounds__(EB) void pool_max_bwd_kernel(const float *__restrict__ dy, const int *__restrict__ arg, int C4,
                                                          const int *__restrict__ nbr_t, int64_t n_in, int K,
                                                          float *__restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (idx >= n_in * C4) return;
  const int64_t i = idx / C4;
  const int c = (int)(idx - i * C4) * 4;
  float4 s = make_float4(0, 0, 0, 0);
  for (int k = 0; k < K; ++k) {
    const int o = nbr_t[i * K + k];
    if (o >= 0) {
      const int4 a = *reinterpret_cast<const int4 *>(arg + (int64_t)o * (4 * C4) + c);
      const float4 g = ld4(dy + (int64_t)o * (4 * C4) + c);
      s.x += a.x == (int)i ? g.x : 0.f, s.y += a.y == (int)i ? g.y : 0.f;
      s.z += a.z == (int)i ? g.z : 0.f, s.w += a.w == (int)i ? g.w : 0.f;
    }
  }
  st4(dx + i * (int64_t)(4 * C4) + c, s);
}

// one workgroup per (batch, 64-channel slab): 16 float4 columns x 16 row lanes
__global__ __launch_bounds__(EB) void global_avg_fwd_kernel(const float *__restrict__ x, int C,
                                                            const int *__restrict__ boff, float *__restrict__ y) {
  __shared__ float4 s_red[EB];
  const int b = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 15) * 4, rl = threadIdx.x >> 4;
  const int beg = boff[b], end = boff[b + 1];
  float4 s = make_float4(0, 0, 0, 0);
  if (c < C)
    for (int r = beg + rl; r < end; r += 16) {
      const float4 v = ld4(x + (int64_t)r * C + c);
      s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
    }
  s_red[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int r = 1; r < 16; ++r) {
      const float4 v = s_red[r * 16 + (threadIdx.x & 15)];
      s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
    }
    const float inv = end > beg ? 1.f / (float)(end - beg) : 0.f;
    st4(y + (int64_t)b * C + c, make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv));
  }
}

__global__ __launch_bounds__(EB) void global_avg_bwd_kernel(const float *__restrict__ dy, int C4,
                                                            const int *__restrict__ boff, int B, int64_t n,
                                                            float *__restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (idx >= n * C4) return;
  const int64_t i = idx / C4;
  const int c = (int)(idx - i * C4) * 4;
  int lo = 0, hi = B;  // largest b with boff[b] <= i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (boff[mid] <= i) lo = mid;
    else hi = mid;
  }
  const float inv = 1.f / (float)(boff[lo + 1] - boff[lo]);
  const float4 g = ld4(dy + (int64_t)lo * (4 * C4) + c);
  st4(dx + i * (int64_t)(4 * C4) + c, make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv));
}

}  // namespace mink

using namespace mink;

extern "C" {

int mink_pool_local_fwd(const float *x, int32_t ldx, int32_t C, const int32_t *nbr, int64_t n_out, int32_t K, int32_t mode,
                        float *y, int32_t *cnt, void *stream) {
  MINK_REQUIRE_ROWS_C("pool_local_fwd", n_out, 0x7fffffffLL, C);
  MINK_REQUIRE(K >= 1 && K <= 81 && ldx >= C && (mode == kSum || mode == kAvg), "pool_local_fwd: bad arguments (K=%d, ldx=%d, mode=%d)", K,
               ldx, mode);
  if (n_out == 0) return MINK_OK;
  MINK_REQUIRE(x && nbr && y && (mode == kSum || cnt), "pool_local_fwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C & 3) == 0 && (ldx & 3) == 0 && aligned16(x) && aligned16(y);
  const unsigned grid = flat_grid(n_out * (vec ? C / 4 : C), PB, 1 << 16);
  if (mode == kAvg) {
    if (vec) pool_local_fwd_kernel<4, kAvg><<<dim3(grid), PB, 0, st>>>(x, ldx, C, nbr, n_out, K, y, cnt);
    else pool_local_fwd_kernel<1, kAvg><<<dim3(grid), PB, 0, st>>>(x, ldx, C, nbr, n_out, K, y, cnt);
  } else {
    if (vec) pool_local_fwd_kernel<4, kSum><<<dim3(grid), PB, 0, st>>>(x, ldx, C, nbr, n_out, K, y, cnt);
    else pool_local_fwd_kernel<1, kSum><<<dim3(grid), PB, 0, st>>>(x, ldx, C, nbr, n_out, K, y, cnt);
  }
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_pool_local_bwd(const float *dy, int32_t C, const int32_t *nbr_t, int64_t n_in, int32_t K, int32_t mode,
                        const int32_t *cnt, float *dx, void *stream) {
  MINK_REQUIRE_ROWS_C("pool_local_bwd", n_in, 0x7fffffffLL, C);
  MINK_REQUIRE(K >= 1 && K <= 81 && (mode == kSum || mode == kAvg), "pool_local_bwd: bad arguments (K=%d, mode=%d)", K, mode);
  if (n_in == 0) return MINK_OK;
  MINK_REQUIRE(dy && nbr_t && dx && (mode == kSum || cnt), "pool_local_bwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C & 3) == 0 && aligned16(dy) && aligned16(dx);
  const unsigned grid = flat_grid(n_in * (vec ? C / 4 : C), PB, 1 << 16);
  if (mode == kAvg) {
    if (vec) pool_local_bwd_kernel<4, kAvg><<<dim3(grid), PB, 0, st>>>(dy, C, nbr_t, n_in, K, cnt, dx);
    else pool_local_bwd_kernel<1, kAvg><<<dim3(grid), PB, 0, st>>>(dy, C, nbr_t, n_in, K, cnt, dx);
  } else {
    if (vec) pool_local_bwd_kernel<4, kSum><<<dim3(grid), PB, 0, st>>>(dy, C, nbr_t, n_in, K, cnt, dx);
    else pool_local_bwd_kernel<1, kSum><<<dim3(grid), PB, 0, st>>>(dy, C, nbr_t, n_in, K, cnt, dx);
  }
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_pool_local_max_fwd(const float *x, int32_t ldx, int32_t C, const int32_t *nbr, int64_t n_out, int32_t K, float *y,
                            int32_t *arg, void *stream) {
  MINK_REQUIRE_ROWS_C("pool_local_max_fwd", n_out, 0x7fffffffLL, C);
  MINK_REQUIRE(K >= 1 && K <= 81 && ldx >= C, "pool_local_max_fwd: bad arguments (K=%d, ldx=%d)", K, ldx);
  if (n_out == 0) return MINK_OK;
  MINK_REQUIRE(x && nbr && y && arg, "pool_local_max_fwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C & 3) == 0 && (ldx & 3) == 0 && aligned16(x) && aligned16(y) && aligned16(arg);
  const unsigned grid = flat_grid(n_out * (vec ? C / 4 : C), PB, 1 << 16);
  if (vec) pool_local_max_fwd_kernel<4><<<dim3(grid), PB, 0, st>>>(x, ldx, C, nbr, n_out, K, y, arg);
  else pool_local_max_fwd_kernel<1><<<dim3(grid), PB, 0, st>>>(x, ldx, C, nbr, n_out, K, y, arg);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_pool_local_max_bwd(const float *dy, const int32_t *arg, int32_t C, const int32_t *nbr_t, int64_t n_in, int32_t K,
                            float *dx, void *stream) {
  MINK_REQUIRE_ROWS_C("pool_local_max_bwd", n_in, 0x7fffffffLL, C);
  MINK_REQUIRE(K >= 1 && K <= 81, "pool_local_max_bwd: bad arguments (K=%d)", K);
  if (n_in == 0) return MINK_OK;
  MINK_REQUIRE(dy && arg && nbr_t && dx, "pool_local_max_bwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C & 3) == 0 && aligned16(dy) && aligned16(arg) && aligned16(dx);
  const unsigned grid = flat_grid(n_in * (vec ? C / 4 : C), PB, 1 << 16);
  if (vec) pool_local_max_bwd_kernel<4><<<dim3(grid), PB, 0, st>>>(dy, arg, C, nbr_t, n_in, K, dx);
  else pool_local_max_bwd_kernel<1><<<dim3(grid), PB, 0, st>>>(dy, arg, C, nbr_t, n_in, K, dx);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int64_t mink_global_pool_workspace_bytes(int64_t n, int32_t C, int32_t B) {
  if (n < 0 || C < 1 || B < 1) return 0;
  return (int64_t)B * sample_chunks(n, B) * C * (int64_t)sizeof(double);  // max: (float, int32) per partial; sum: one double
}

#define GPOOL_ARGS(name)                                                                                                           \
  MINK_REQUIRE_ROWS_C(name, n, 0x7fffffffLL, C);                                                                                   \
  MINK_REQUIRE(B >= 1 && B <= 65535, name ": bad batch size %d (1 <= B <= 65535)", B)

int mink_global_max_fwd(const float *x, int64_t n, int32_t ldx, int32_t C, const int32_t *batch_offsets, int32_t B, float *y,
                        int32_t *arg, void *workspace, int64_t workspace_bytes, void *stream) {
  GPOOL_ARGS("global_max_fwd");
  MINK_REQUIRE(ldx >= C && batch_offsets && y && arg && workspace && (n == 0 || x), "global_max_fwd: NULL pointer or ldx < C");
  MINK_REQUIRE_WORKSPACE("global_max_fwd", workspace_bytes, mink_global_pool_workspace_bytes(n, C, B), workspace);
  hipStream_t st = (hipStream_t)stream;
  const int G = sample_chunks(n, B);
  float *pval = (float *)workspace;
  int *parg = (int *)(pval + (int64_t)B * G * C);
  const bool vec = (C & 3) == 0 && (ldx & 3) == 0 && aligned16(x);
  const ChunkLaunch l(n, C, B, vec ? 4 : 1, PB);
  const size_t shm = (size_t)l.rlanes * l.W * (sizeof(float) + sizeof(int));
  if (vec) gmax_partial_kernel<4><<<l.grid, PB, shm, st>>>(x, ldx, batch_offsets, n, C, l.tprb, pval, parg);
  else gmax_partial_kernel<1><<<l.grid, PB, shm, st>>>(x, ldx, batch_offsets, n, C, l.tprb, pval, parg);
  MINK_CHECK_LAUNCH();
  gmax_finalize_kernel<<<dim3((unsigned)cdiv(C, 4), (unsigned)B), PB, 0, st>>>(pval, parg, G, C, y, arg);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_global_max_bwd(const float *dy, const int32_t *arg, int64_t n, int32_t C, const int32_t *batch_offsets, int32_t B,
                        float *dx, void *stream) {
  GPOOL_ARGS("global_max_bwd");
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(dy && arg && batch_offsets && dx, "global_max_bwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C & 3) == 0 && aligned16(dy) && aligned16(arg) && aligned16(dx);
  if (vec) gpool_bwd_kernel<4, true><<<dim3(flat_grid(n * (C / 4), PB, 1 << 16)), PB, 0, st>>>(dy, arg, n, C, batch_offsets, B, dx);
  else gpool_bwd_kernel<1, true><<<dim3(flat_grid(n * C, PB, 1 << 16)), PB, 0, st>>>(dy, arg, n, C, batch_offsets, B, dx);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_global_sum_fwd(const float *x, int64_t n, int32_t ldx, int32_t C, const int32_t *batch_offsets, int32_t B, float *y,
                        void *workspace, int64_t workspace_bytes, void *stream) {
  GPOOL_ARGS("global_sum_fwd");
  MINK_REQUIRE(ldx >= C && batch_offsets && y && workspace && (n == 0 || x), "global_sum_fwd: NULL pointer or ldx < C");
  MINK_REQUIRE_WORKSPACE("global_sum_fwd", workspace_bytes, mink_global_pool_workspace_bytes(n, C, B), workspace);
  hipStream_t st = (hipStream_t)stream;
  const int G = sample_chunks(n, B);
  const bool vec = (C & 3) == 0 && (ldx & 3) == 0 && aligned16(x);
  const ChunkLaunch l(n, C, B, vec ? 4 : 1, PB);
  const size_t shm = (size_t)l.rlanes * l.W * sizeof(double);
  if (vec) gsum_partial_kernel<4><<<l.grid, PB, shm, st>>>(x, ldx, batch_offsets, n, C, l.tprb, (double *)workspace);
  else gsum_partial_kernel<1><<<l.grid, PB, shm, st>>>(x, ldx, batch_offsets, n, C, l.tprb, (double *)workspace);
  MINK_CHECK_LAUNCH();
  gsum_finalize_kernel<<<dim3((unsigned)cdiv(C, 4), (unsigned)B), PB, 0, st>>>((const double *)workspace, G, C, y);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_global_sum_bwd(const float *dy, int64_t n, int32_t C, const int32_t *batch_offsets, int32_t B, float *dx, void *stream) {
  GPOOL_ARGS("global_sum_bwd");
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(dy && batch_offsets && dx, "global_sum_bwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C & 3) == 0 && aligned16(dy) && aligned16(dx);
  if (vec) gpool_bwd_kernel<4, false><<<dim3(flat_grid(n * (C / 4), PB, 1 << 16)), PB, 0, st>>>(dy, nullptr, n, C, batch_offsets, B, dx);
  else gpool_bwd_kernel<1, false><<<dim3(flat_grid(n * C, PB, 1 << 16)), PB, 0, st>>>(dy, nullptr, n, C, batch_offsets, B, dx);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_pool_sum_fwd(const float *x, int32_t ldx, int32_t C, const int32_t *nbr, int64_t n_out, int32_t K, float *y,
                      void *stream) {
  REQ_C4(C, "pool_sum_fwd");
  MINK_REQUIRE(n_out >= 0 && K >= 1 && (ldx & 3) == 0 && ldx >= C, "pool_sum_fwd: bad shape");
  if (n_out == 0) return MINK_OK;
  MINK_REQUIRE(x && nbr && y, "pool_sum_fwd: NULL pointer");
  REQ_A16(x, "pool_sum_fwd");
  REQ_A16(y, "pool_sum_fwd");
  pool_sum_fwd_kernel<<<dim3((unsigned)cdiv(n_out * (C >> 2), EB)), EB, 0, (hipStream_t)stream>>>(x, ldx, C >> 2, nbr,
                                                                                                 n_out, K, y);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_pool_sum_bwd(const float *dy, int32_t C, const int32_t *in2out, int64_t n_in, float *dx, void *stream) {
  REQ_C4(C, "pool_sum_bwd");
  MINK_REQUIRE(n_in >= 0, "pool_sum_bwd: bad n");
  if (n_in == 0) return MINK_OK;
  MINK_REQUIRE(dy && in2out && dx, "pool_sum_bwd: NULL pointer");
  REQ_A16(dy, "pool_sum_bwd");
  REQ_A16(dx, "pool_sum_bwd");
  pool_sum_bwd_kernel<<<dim3((unsigned)cdiv(n_in * (C >> 2), EB)), EB, 0, (hipStream_t)stream>>>(dy, C >> 2, in2out,
                                                                                                n_in, dx);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_pool_max_fwd(const float *x, int32_t C, const int32_t *nbr, int64_t n_out, int32_t K, float *y, int32_t *arg,
                      void *stream) {
  REQ_C4(C, "pool_max_fwd");
  MINK_REQUIRE(n_out >= 0 && K >= 1, "pool_max_fwd: bad shape");
  if (n_out == 0) return MINK_OK;
  MINK_REQUIRE(x && nbr && y && arg, "pool_max_fwd: NULL pointer");
  REQ_A16(x, "pool_max_fwd");
  REQ_A16(y, "pool_max_fwd");
  REQ_A16(arg, "pool_max_fwd");
  pool_max_fwd_kernel<<<dim3((unsigned)cdiv(n_out * (C >> 2), EB)), EB, 0, (hipStream_t)stream>>>(x, C >> 2, nbr, n_out, K, y, arg);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_pool_max_bwd(const float *dy, const int32_t *arg, int32_t C, const int32_t *nbr_t, int64_t n_in, int32_t K, float *dx,
                      void *stream) {
  REQ_C4(C, "pool_max_bwd");
  MINK_REQUIRE(n_in >= 0 && K >= 1, "pool_max_bwd: bad shape");
  if (n_in == 0) return MINK_OK;
  MINK_REQUIRE(dy && arg && nbr_t && dx, "pool_max_bwd: NULL pointer");
  REQ_A16(dy, "pool_max_bwd");
  REQ_A16(dx, "pool_max_bwd");
  REQ_A16(arg, "pool_max_bwd");
  pool_max_bwd_kernel<<<dim3((unsigned)cdiv(n_in * (C >> 2), EB)), EB, 0, (hipStream_t)stream>>>(dy, arg, C >> 2, nbr_t, n_in, K, dx);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_global_avg_fwd(const float *x, int32_t C, const int32_t *batch_offsets, int32_t B, float *y, void *stream) {
  REQ_C4(C, "global_avg_fwd");
  MINK_REQUIRE(B >= 1 && x && batch_offsets && y, "global_avg_fwd: bad arguments");
  REQ_A16(x, "global_avg_fwd");
  REQ_A16(y, "global_avg_fwd");
  global_avg_fwd_kernel<<<dim3((unsigned)B, (unsigned)cdiv(C, 64)), EB, 0, (hipStream_t)stream>>>(x, C, batch_offsets, y);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_global_avg_bwd(const float *dy, int32_t C, const int32_t *batch_offsets, int32_t B, int64_t n, float *dx,
                        void *stream) {
  REQ_C4(C, "global_avg_bwd");
  MINK_REQUIRE(B >= 1 && n >= 0, "global_avg_bwd: bad arguments");
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(dy && batch_offsets && dx, "global_avg_bwd: NULL pointer");
  REQ_A16(dy, "global_avg_bwd");
  REQ_A16(dx, "global_avg_bwd");
  global_avg_bwd_kernel<<<dim3((unsigned)cdiv(n * (C >> 2), EB)), EB, 0, (hipStream_t)stream>>>(dy, C >> 2,
                                                                                               batch_offsets, B, n, dx);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
