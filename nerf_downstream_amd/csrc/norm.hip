// Per-sample and per-row normalisation of the feature matrix on gfx950: MinkowskiInstanceNorm (statistics over the rows of
// one batch sample, per channel) and MinkowskiLayerNorm (statistics over the channels of one row), each with the optional
// residual add and ReLU of the batch-norm kernels (batchnorm.hip) fused into the same pass.
//
// Both are bandwidth-bound passes over x[n][C]; the figure of merit is bytes moved per element against the minimum:
//   instance norm forward : read x (statistics), read x + write y (apply)             12 B / element  (+4 residual)
//   instance norm backward: read dy, x [, y] (sums), read dy, x [, y] + write dx      20 B / element  (+8 relu, +4 dresidual)
//   layer norm forward    : read x, write y -- the row stays in registers between the two passes   8 B / element
//   layer norm backward   : read dy, x [, y], write dx; dgamma / dbeta out of the same pass        12 B / element
// 16-byte accesses per lane when C % 4 == 0 and the matrices are 16-byte aligned, dword accesses otherwise (C = 3, 5, ...).
//
// Instance norm.  Sample b owns rows [off[b], off[b+1]) (CoordinateManager.batch_offsets, on the device; never read by the
// host).  The grid is (G, B, channel slabs): every sample is cut into the same number G of row chunks, G chosen from n and
// B alone, so the launch shape -- and the number of launches: 3 forward, 4 backward -- does not depend on how the rows are
// spread over the samples; an empty sample's workgroups find an empty range.  The apply passes are flat over the n rows and
// find a row's sample by a binary search in the B + 1 offsets (cached; re-done only when the row leaves the sample).
//
// Statistics.  sum x and sum x^2 are accumulated in DOUBLE from the first add on (per thread, across the row lanes of a
// workgroup through LDS in lane order, across the G chunks by a fixed butterfly of one wave): var = E[x^2] - mean^2 then loses
// log2(mean^2 / var) of 53 bits, not of 24, so activations far from zero (mean 50, sd 1) keep full fp32 accuracy, and a
// channel that is constant within a sample gets mean == x exactly and y == beta.  Layer norm is two-pass over the row held
// in registers: mean first, then sum (x - mean)^2.
// Determinism: no floating-point atomics; rows -> threads -> partials -> sums is a fixed assignment and a fixed order, so
// two runs are bitwise equal.
#include <algorithm>

#include "rowpass.h"

namespace mink {

constexpr int NB = 256;            // threads per workgroup
constexpr int kLnMaxC = 512;
constexpr int kLnRedBlocks = 1024;  // workgroups (= partial rows) of the layer-norm backward

// Two column sums over `count` partial rows (`stride` doubles apart) by one wave: lane l adds rows l, l + 64, ... in order,
// then a fixed butterfly; every lane returns the sums.
__device__ __forceinline__ void wave_sum2(const double *__restrict__ p0, const double *__restrict__ p1, int count, int64_t stride,
                                          double &s, double &ss) {
  const int lane = threadIdx.x & 63;
  double a = 0.0, b = 0.0;
  for (int j = lane; j < count; j += 64) a += p0[j * stride], b += p1[j * stride];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64), b += __shfl_xor(b, o, 64);
  s = a, ss = b;
}

// ------------------------------------------------------------------------------------------------ instance norm
// Column sums of chunk g of sample b: partial[b][g][2][C] (double).
//   !BWD: (sum x, sum x^2) of a = x          BWD: (sum g, sum g * xhat), g = a = dy masked by yrelu > 0
// A thread owns VEC channels (column group cg) and the rows rl, rl + rlanes, ... of the chunk; tprb column groups per
// workgroup, blockIdx.z walks further slabs of tprb groups.
template <int VEC, bool BWD>
__global__ __launch_bounds__(NB) void in_reduce_kernel(const float *__restrict__ a, const float *__restrict__ x,
                                                       const float *__restrict__ yrelu, const int *__restrict__ off, int64_t n,
                                                       int C, int tprb, const float *__restrict__ mean,
                                                       const float *__restrict__ invstd, double *__restrict__ partial) {
  extern __shared__ __align__(16) double s_red[];  // [rlanes][2][W]
  const int b = blockIdx.y, G = gridDim.x, g = blockIdx.x;
  const auto [r0, r1, ncg, rlanes, W, cl, rl, cg] = chunk_lane<VEC, NB>(off, n, C, tprb);
  double s0[VEC], s1[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) s0[k] = 0.0, s1[k] = 0.0;
  if (rl < rlanes && cg < ncg) {
    const int c = cg * VEC;
    float mu[VEC], is[VEC];
    if (BWD) ldv<VEC>(mean + (int64_t)b * C + c, mu), ldv<VEC>(invstd + (int64_t)b * C + c, is);
#pragma unroll 4
    for (int64_t row = r0 + rl; row < r1; row += rlanes) {
      const int64_t o = row * C + c;
      float v[VEC];
      ldv<VEC>(a + o, v);
      if (!BWD) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) s0[k] += (double)v[k], s1[k] += (double)v[k] * (double)v[k];
      } else {
        float xv[VEC];
        ldv<VEC>(x + o, xv);
        if (yrelu) {
          float yv[VEC];
          ldv<VEC>(yrelu + o, yv);
#pragma unroll
          for (int k = 0; k < VEC; ++k) v[k] = yv[k] > 0.f ? v[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float xh = (xv[k] - mu[k]) * is[k];
          s0[k] += (double)v[k], s1[k] += (double)v[k] * (double)xh;
        }
      }
    }
  }
  if (rl < rlanes) {
    double *d = s_red + (int64_t)rl * 2 * W + cl * VEC;
#pragma unroll
    for (int k = 0; k < VEC; ++k) d[k] = s0[k], d[W + k] = s1[k];
  }
  __syncthreads();
  double *out = partial + ((int64_t)b * G + g) * 2 * C;
  for (int e = threadIdx.x; e < 2 * W; e += NB) {
    const int q = e / W, c = blockIdx.z * W + (e - q * W);
    if (c >= C) continue;
    double s = 0.0;
    for (int r = 0; r < rlanes; ++r) s += s_red[(int64_t)r * 2 * W + e];
    out[(int64_t)q * C + c] = s;
  }
}

// grid (ceil(C / 4), B): one wave per (sample, channel) sums the G chunk partials.
//   !BWD: mean[b][c], invstd[b][c] (an empty sample: 0, 0 -- no row reads them)
//   BWD : o0 = sum g / n_b, o1 = sum g xhat / n_b (fp32, what the apply pass subtracts) and dsum[b][2][C] (double) for dgamma / dbeta
template <bool BWD>
__global__ __launch_bounds__(NB) void in_finalize_kernel(const double *__restrict__ partial, int G, const int *__restrict__ off,
                                                         int64_t n, int C, float eps, float *__restrict__ o0,
                                                         float *__restrict__ o1, double *__restrict__ dsum) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (c >= C) return;  // whole wave
  const double *p = partial + (int64_t)b * G * 2 * C + c;
  double s, ss;
  wave_sum2(p, p + C, G, 2 * (int64_t)C, s, ss);
  if ((threadIdx.x & 63) != 0) return;
  int64_t lo, hi;
  sample_range(off, b, n, lo, hi);
  const double nb = (double)(hi - lo);
  const int64_t i = (int64_t)b * C + c;
  if (!BWD) {
    if (hi == lo) {
      o0[i] = 0.f, o1[i] = 0.f;
    } else {
      const double m = s / nb;
      double var = ss / nb - m * m;
      var = var < 0.0 ? 0.0 : var;
      o0[i] = (float)m;
      o1[i] = (float)(1.0 / sqrt(var + (double)eps));
    }
  } else {
    o0[i] = hi == lo ? 0.f : (float)(s / nb);
    o1[i] = hi == lo ? 0.f : (float)(ss / nb);
    dsum[((int64_t)b * 2) * C + c] = s;
    dsum[((int64_t)b * 2 + 1) * C + c] = ss;
  }
}

// dbeta[c] = sum_b sum g, dgamma[c] = sum_b sum g xhat, samples added in index order
__global__ __launch_bounds__(NB) void in_param_grad_kernel(const double *__restrict__ dsum, int B, int C, float *__restrict__ dgamma,
                                                           float *__restrict__ dbeta) {
  const int c = blockIdx.x * NB + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, ss = 0.0;
  for (int b = 0; b < B; ++b) s += dsum[((int64_t)b * 2) * C + c], ss += dsum[((int64_t)b * 2 + 1) * C + c];
  dbeta[c] = (float)s;
  dgamma[c] = (float)ss;
}

// y = [relu]( (x - mean_b) * invstd_b * gamma + beta [+ residual] ), flat over the n * C / VEC column groups
template <int VEC>
__global__ __launch_bounds__(NB) void in_apply_kernel(const float *__restrict__ x, int64_t n, int C, const int *__restrict__ off,
                                                      int B, const float *__restrict__ mean, const float *__restrict__ invstd,
                                                      const float *__restrict__ gamma, const float *__restrict__ beta,
                                                      const float *__restrict__ residual, int relu, float *__restrict__ y) {
  const int ncg = C / VEC;
  const int64_t total = n * ncg;
  int b = 0;
  int64_t lo = 0, hi = 0;  // the cached sample's rows: empty until the first search
  for (int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x; i < total; i += (int64_t)gridDim.x * NB) {
    const int64_t row = i / ncg;
    const int c = (int)(i - row * ncg) * VEC;
    if (row < lo || row >= hi) {
      b = sample_of(off, B, row);
      lo = off[b], hi = off[b + 1];
    }
    float v[VEC], mu[VEC], is[VEC], ga[VEC], be[VEC];
    ldv<VEC>(x + i * VEC, v);
    ldv<VEC>(mean + (int64_t)b * C + c, mu), ldv<VEC>(invstd + (int64_t)b * C + c, is);
    ldv<VEC>(gamma + c, ga), ldv<VEC>(beta + c, be);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = (v[k] - mu[k]) * is[k] * ga[k] + be[k];
    if (residual) {
      float r[VEC];
      ldv<VEC>(residual + i * VEC, r);
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] += r[k];
    }
    if (relu) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = relu_keep_nan(v[k]);
    }
    stv<VEC>(y + i * VEC, v);
  }
}

// dx = gamma * invstd_b * (g - mean_b(g) - xhat * mean_b(g xhat)); dresidual = g (dy masked by y > 0)
template <int VEC>
__global__ __launch_bounds__(NB) void in_bwd_apply_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                          const float *__restrict__ yrelu, int64_t n, int C,
                                                          const int *__restrict__ off, int B, const float *__restrict__ mean,
                                                          const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                          const float *__restrict__ gmean, const float *__restrict__ gxmean,
                                                          float *__restrict__ dx, float *__restrict__ dres) {
  const int ncg = C / VEC;
  const int64_t total = n * ncg;
  int b = 0;
  int64_t lo = 0, hi = 0;
  for (int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x; i < total; i += (int64_t)gridDim.x * NB) {
    const int64_t row = i / ncg;
    const int c = (int)(i - row * ncg) * VEC;
    if (row < lo || row >= hi) {
      b = sample_of(off, B, row);
      lo = off[b], hi = off[b + 1];
    }
    float g[VEC], v[VEC], mu[VEC], is[VEC], ga[VEC], gm[VEC], gxm[VEC];
    ldv<VEC>(dy + i * VEC, g);
    if (yrelu) {
      float yv[VEC];
      ldv<VEC>(yrelu + i * VEC, yv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
    }
    if (dres) stv<VEC>(dres + i * VEC, g);
    ldv<VEC>(x + i * VEC, v);
    const int64_t s = (int64_t)b * C + c;
    ldv<VEC>(mean + s, mu), ldv<VEC>(invstd + s, is), ldv<VEC>(gmean + s, gm), ldv<VEC>(gxmean + s, gxm);
    ldv<VEC>(gamma + c, ga);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = ga[k] * is[k] * (g[k] - gm[k] - (v[k] - mu[k]) * is[k] * gxm[k]);
    stv<VEC>(dx + i * VEC, v);
  }
}

// ------------------------------------------------------------------------------------------------ layer norm
// gs lanes (a power of two <= 64) own one row, 64 / gs rows per wave; lane `sub` of the group holds the column groups sub,
// sub + gs, ... (at most MAXI of them: C <= 512) in registers between the passes.
template <int VEC>
struct LnShape {
  static constexpr int MAXI = VEC == 4 ? 2 : 8;
};

__device__ __forceinline__ float group_sum(float v, int gs) {
  for (int o = gs >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int VEC>
__global__ __launch_bounds__(NB) void ln_fwd_kernel(const float *__restrict__ x, int64_t n, int C, int gs, float eps,
                                                    const float *__restrict__ gamma, const float *__restrict__ beta,
                                                    const float *__restrict__ residual, int relu, float *__restrict__ y,
                                                    float *__restrict__ mean, float *__restrict__ invstd) {
  constexpr int MAXI = LnShape<VEC>::MAXI;
  const int lane = threadIdx.x & 63, sub = lane & (gs - 1), rw = lane / gs, rpw = 64 / gs;
  const int ncg = C / VEC, items = (ncg + gs - 1) / gs;
  const float inv_c = 1.f / (float)C;
  float ga[MAXI][VEC], be[MAXI][VEC];
#pragma unroll
  for (int i = 0; i < MAXI; ++i) {
    const int cg = sub + i * gs;
#pragma unroll
    for (int k = 0; k < VEC; ++k) ga[i][k] = 0.f, be[i][k] = 0.f;
    if (i < items && cg < ncg) ldv<VEC>(gamma + cg * VEC, ga[i]), ldv<VEC>(beta + cg * VEC, be[i]);
  }
  const int64_t wave = (int64_t)blockIdx.x * (NB / 64) + (threadIdx.x >> 6), step = (int64_t)gridDim.x * (NB / 64) * rpw;
  for (int64_t row0 = wave * rpw; row0 < n; row0 += step) {  // (wave-uniform trip count: the shuffles below see all 64 lanes)
    const int64_t row = row0 + rw;
    const bool live = row < n;
    float v[MAXI][VEC];
    double s = 0.0;  // (the mean of a row far from zero must not lose bits to the sum: 512 x 50 in fp32 would)
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int cg = sub + i * gs;
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[i][k] = 0.f;
      if (i < items && live && cg < ncg) ldv<VEC>(x + row * C + cg * VEC, v[i]);
#pragma unroll
      for (int k = 0; k < VEC; ++k) s += (double)v[i][k];
    }
    for (int o = gs >> 1; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mu = (float)(s / (double)C);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int cg = sub + i * gs;
      if (i < items && cg < ncg) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) q += (v[i][k] - mu) * (v[i][k] - mu);
      }
    }
    const float is = 1.f / sqrtf(group_sum(q, gs) * inv_c + eps);
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int cg = sub + i * gs;
      if (i < items && live && cg < ncg) {
        const int64_t o = row * C + cg * VEC;
        float r[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) r[k] = (v[i][k] - mu) * is * ga[i][k] + be[i][k];
        if (residual) {
          float t[VEC];
          ldv<VEC>(residual + o, t);
#pragma unroll
          for (int k = 0; k < VEC; ++k) r[k] += t[k];
        }
        if (relu) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) r[k] = relu_keep_nan(r[k]);
        }
        stv<VEC>(y + o, r);
      }
    }
    if (live && sub == 0) mean[row] = mu, invstd[row] = is;
  }
}

// dx[r] = invstd_r * (gh - mean_c(gh) - xhat * mean_c(gh xhat)), gh = g * gamma, g = dy masked by y > 0; dresidual = g; and
// this workgroup's share of (sum_r g, sum_r g xhat) per channel -> partial[blk][2][C] (double), row slots added in slot order
template <int VEC>
__global__ __launch_bounds__(NB) void ln_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                    const float *__restrict__ yrelu, int64_t n, int C, int gs,
                                                    const float *__restrict__ mean, const float *__restrict__ invstd,
                                                    const float *__restrict__ gamma, float *__restrict__ dx,
                                                    float *__restrict__ dres, double *__restrict__ partial) {
  constexpr int MAXI = LnShape<VEC>::MAXI;
  extern __shared__ __align__(16) double s_red[];  // [slots][2][Wp], Wp = gs * items * VEC >= C
  const int lane = threadIdx.x & 63, sub = lane & (gs - 1), rw = lane / gs, rpw = 64 / gs;
  const int ncg = C / VEC, items = (ncg + gs - 1) / gs;
  const float inv_c = 1.f / (float)C;
  float ga[MAXI][VEC];
  double a0[MAXI][VEC], a1[MAXI][VEC];
#pragma unroll
  for (int i = 0; i < MAXI; ++i) {
    const int cg = sub + i * gs;
#pragma unroll
    for (int k = 0; k < VEC; ++k) ga[i][k] = 0.f, a0[i][k] = 0.0, a1[i][k] = 0.0;
    if (i < items && cg < ncg) ldv<VEC>(gamma + cg * VEC, ga[i]);
  }
  const int64_t wave = (int64_t)blockIdx.x * (NB / 64) + (threadIdx.x >> 6), step = (int64_t)gridDim.x * (NB / 64) * rpw;
  for (int64_t row0 = wave * rpw; row0 < n; row0 += step) {
    const int64_t row = row0 + rw;
    const bool live = row < n;
    const float mu = live ? mean[row] : 0.f, is = live ? invstd[row] : 0.f;
    float g[MAXI][VEC], xh[MAXI][VEC];
    float s = 0.f, sx = 0.f;
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int cg = sub + i * gs;
#pragma unroll
      for (int k = 0; k < VEC; ++k) g[i][k] = 0.f, xh[i][k] = 0.f;
      if (i < items && live && cg < ncg) {
        const int64_t o = row * C + cg * VEC;
        ldv<VEC>(dy + o, g[i]);
        ldv<VEC>(x + o, xh[i]);
        if (yrelu) {
          float yv[VEC];
          ldv<VEC>(yrelu + o, yv);
#pragma unroll
          for (int k = 0; k < VEC; ++k) g[i][k] = yv[k] > 0.f ? g[i][k] : 0.f;
        }
        if (dres) stv<VEC>(dres + o, g[i]);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          xh[i][k] = (xh[i][k] - mu) * is;
          const float gh = g[i][k] * ga[i][k];
          s += gh, sx += gh * xh[i][k];
          a0[i][k] += (double)g[i][k], a1[i][k] += (double)g[i][k] * (double)xh[i][k];
        }
      }
    }
    const float m1 = group_sum(s, gs) * inv_c, m2 = group_sum(sx, gs) * inv_c;
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int cg = sub + i * gs;
      if (i < items && live && cg < ncg) {
        float r[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) r[k] = is * (g[i][k] * ga[i][k] - m1 - xh[i][k] * m2);
        stv<VEC>(dx + row * C + cg * VEC, r);
      }
    }
  }
  const int Wp = gs * items * VEC, slots = (NB / 64) * rpw, slot = (threadIdx.x >> 6) * rpw + rw;
#pragma unroll
  for (int i = 0; i < MAXI; ++i) {
    if (i < items) {
      double *d = s_red + (int64_t)slot * 2 * Wp + (sub + i * gs) * VEC;
#pragma unroll
      for (int k = 0; k < VEC; ++k) d[k] = a0[i][k], d[Wp + k] = a1[i][k];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * C; e += NB) {
    const int q = e >= C, c = e - q * C;
    double t = 0.0;
    for (int r = 0; r < slots; ++r) t += s_red[(int64_t)r * 2 * Wp + q * Wp + c];
    partial[(int64_t)blockIdx.x * 2 * C + e] = t;
  }
}

// one wave per channel: dbeta[c], dgamma[c] from the nblk workgroup partials
__global__ __launch_bounds__(NB) void ln_param_grad_kernel(const double *__restrict__ partial, int nblk, int C,
                                                           float *__restrict__ dgamma, float *__restrict__ dbeta) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;  // whole wave
  double s, ss;
  wave_sum2(partial + c, partial + C + c, nblk, 2 * (int64_t)C, s, ss);
  if ((threadIdx.x & 63) == 0) dbeta[c] = (float)s, dgamma[c] = (float)ss;
}

// ------------------------------------------------------------------------------------------------ host side
struct InWorkspace {
  double *partial, *dsum;
  float *gmean, *gxmean;
};
static inline int64_t in_ws_layout(int64_t n, int C, int B, void *base, InWorkspace *w) {
  const int64_t np = (int64_t)B * sample_chunks(n, B) * 2 * C, nd = (int64_t)B * 2 * C, nf = (int64_t)B * C;
  if (w) {
    w->partial = (double *)base;
    w->dsum = w->partial + np;
    w->gmean = (float *)(w->dsum + nd);
    w->gxmean = w->gmean + nf;
  }
  return (np + nd) * (int64_t)sizeof(double) + 2 * nf * (int64_t)sizeof(float);
}

template <int VEC, bool BWD>
static void launch_in_reduce(const float *a, const float *x, const float *yr, const int *off, int64_t n, int C, int B,
                             const float *mean, const float *invstd, double *partial, hipStream_t st) {
  const ChunkLaunch l(n, C, B, VEC, NB);
  const size_t shm = (size_t)l.rlanes * 2 * l.W * sizeof(double);
  in_reduce_kernel<VEC, BWD><<<l.grid, NB, shm, st>>>(a, x, yr, off, n, C, l.tprb, mean, invstd, partial);
}

static inline int ln_group(int ncg) {
  int gs = 1;
  while (gs < ncg && gs < 64) gs <<= 1;
  return gs;
}

}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_in_workspace_bytes(int64_t n, int32_t C, int32_t B) {
  if (n < 0 || C < 1 || B < 1) return 0;
  return in_ws_layout(n, C, B, nullptr, nullptr);
}

int mink_in_fwd(const float *x, int64_t n, int32_t C, const int32_t *batch_offsets, int32_t B, float eps, const float *gamma,
                const float *beta, const float *residual, int32_t relu, float *y, float *mean, float *invstd, void *workspace,
                int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(n >= 0 && n <= 0x7fffffffLL && C >= 1 && C <= 4096 && B >= 1 && B <= 65535, "in_fwd: bad shape (n=%lld, C=%d, B=%d)",
               (long long)n, C, B);
  MINK_REQUIRE(batch_offsets && gamma && beta && mean && invstd && workspace && (n == 0 || (x && y)), "in_fwd: NULL pointer");
  MINK_REQUIRE_WORKSPACE("in_fwd", workspace_bytes, mink_in_workspace_bytes(n, C, B), workspace);
  hipStream_t st = (hipStream_t)stream;
  InWorkspace w;
  in_ws_layout(n, C, B, workspace, &w);
  const bool vec = (C & 3) == 0 && aligned16(x) && aligned16(y) && aligned16(residual) && aligned16(mean) && aligned16(invstd) &&
                   aligned16(gamma) && aligned16(beta);
  if (vec)
    launch_in_reduce<4, false>(x, nullptr, nullptr, batch_offsets, n, C, B, nullptr, nullptr, w.partial, st);
  else
    launch_in_reduce<1, false>(x, nullptr, nullptr, batch_offsets, n, C, B, nullptr, nullptr, w.partial, st);
  MINK_CHECK_LAUNCH();
  in_finalize_kernel<false><<<dim3((unsigned)cdiv(C, 4), (unsigned)B), NB, 0, st>>>(w.partial, sample_chunks(n, B), batch_offsets, n, C, eps,
                                                                                 mean, invstd, nullptr);
  MINK_CHECK_LAUNCH();
  if (n == 0) return MINK_OK;
  if (vec)
    in_apply_kernel<4><<<dim3(flat_grid(n * (C / 4), NB, 4096)), NB, 0, st>>>(x, n, C, batch_offsets, B, mean, invstd, gamma, beta, residual, relu, y);
  else
    in_apply_kernel<1><<<dim3(flat_grid(n * C, NB, 4096)), NB, 0, st>>>(x, n, C, batch_offsets, B, mean, invstd, gamma, beta, residual, relu, y);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_in_bwd(const float *dy, const float *x, const float *y, int64_t n, int32_t C, const int32_t *batch_offsets, int32_t B,
                const float *mean, const float *invstd, const float *gamma, int32_t relu, float *dx, float *dresidual,
                float *dgamma, float *dbeta, void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(n >= 0 && n <= 0x7fffffffLL && C >= 1 && C <= 4096 && B >= 1 && B <= 65535, "in_bwd: bad shape (n=%lld, C=%d, B=%d)",
               (long long)n, C, B);
  MINK_REQUIRE(batch_offsets && gamma && mean && invstd && dgamma && dbeta && workspace && (n == 0 || (dy && x && dx)),
               "in_bwd: NULL pointer");
  MINK_REQUIRE(!relu || n == 0 || y, "in_bwd: fused ReLU needs the forward output");
  MINK_REQUIRE_WORKSPACE("in_bwd", workspace_bytes, mink_in_workspace_bytes(n, C, B), workspace);
  hipStream_t st = (hipStream_t)stream;
  InWorkspace w;
  in_ws_layout(n, C, B, workspace, &w);
  const float *yr = relu ? y : nullptr;
  const bool vec = (C & 3) == 0 && aligned16(dy) && aligned16(x) && aligned16(yr) && aligned16(dx) && aligned16(dresidual) &&
                   aligned16(mean) && aligned16(invstd) && aligned16(gamma);  // (gmean / gxmean: 8-byte base + whole doubles before them, B * C * 4 apart)
  const bool ws16 = aligned16(w.gmean) && aligned16(w.gxmean);
  if (vec && ws16)
    launch_in_reduce<4, true>(dy, x, yr, batch_offsets, n, C, B, mean, invstd, w.partial, st);
  else
    launch_in_reduce<1, true>(dy, x, yr, batch_offsets, n, C, B, mean, invstd, w.partial, st);
  MINK_CHECK_LAUNCH();
  in_finalize_kernel<true><<<dim3((unsigned)cdiv(C, 4), (unsigned)B), NB, 0, st>>>(w.partial, sample_chunks(n, B), batch_offsets, n, C, 0.f,
                                                                                w.gmean, w.gxmean, w.dsum);
  MINK_CHECK_LAUNCH();
  in_param_grad_kernel<<<dim3((unsigned)cdiv(C, NB)), NB, 0, st>>>(w.dsum, B, C, dgamma, dbeta);
  MINK_CHECK_LAUNCH();
  if (n == 0) return MINK_OK;
  if (vec && ws16)
    in_bwd_apply_kernel<4><<<dim3(flat_grid(n * (C / 4), NB, 4096)), NB, 0, st>>>(dy, x, yr, n, C, batch_offsets, B, mean, invstd, gamma, w.gmean,
                                                                       w.gxmean, dx, dresidual);
  else
    in_bwd_apply_kernel<1><<<dim3(flat_grid(n * C, NB, 4096)), NB, 0, st>>>(dy, x, yr, n, C, batch_offsets, B, mean, invstd, gamma, w.gmean, w.gxmean,
                                                                 dx, dresidual);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int64_t mink_ln_workspace_bytes(int64_t n, int32_t C) {
  if (n < 0 || C < 1) return 0;
  return (int64_t)kLnRedBlocks * 2 * C * (int64_t)sizeof(double);
}

static inline unsigned ln_grid(int64_t n, int gs, int cap) {
  const int64_t rows_per_block = (int64_t)(NB / 64) * (64 / gs);
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, rows_per_block), cap));
}

int mink_ln_fwd(const float *x, int64_t n, int32_t C, float eps, const float *gamma, const float *beta, const float *residual,
                int32_t relu, float *y, float *mean, float *invstd, void *stream) {
  MINK_REQUIRE(n >= 0 && n <= 0x7fffffffLL && C >= 1 && C <= kLnMaxC, "ln_fwd: bad shape (n=%lld, C=%d; 1 <= C <= %d)", (long long)n, C,
               kLnMaxC);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(x && gamma && beta && y && mean && invstd, "ln_fwd: NULL pointer");
  const bool vec = (C & 3) == 0 && aligned16(x) && aligned16(y) && aligned16(residual) && aligned16(gamma) && aligned16(beta);
  hipStream_t st = (hipStream_t)stream;
  if (vec) {
    const int gs = ln_group(C / 4);
    ln_fwd_kernel<4><<<dim3(ln_grid(n, gs, 4096)), NB, 0, st>>>(x, n, C, gs, eps, gamma, beta, residual, relu, y, mean, invstd);
  } else {
    const int gs = ln_group(C);
    ln_fwd_kernel<1><<<dim3(ln_grid(n, gs, 4096)), NB, 0, st>>>(x, n, C, gs, eps, gamma, beta, residual, relu, y, mean, invstd);
  }
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_ln_bwd(const float *dy, const float *x, const float *y, int64_t n, int32_t C, const float *mean, const float *invstd,
                const float *gamma, int32_t relu, float *dx, float *dresidual, float *dgamma, float *dbeta, void *workspace,
                int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(n >= 0 && n <= 0x7fffffffLL && C >= 1 && C <= kLnMaxC, "ln_bwd: bad shape (n=%lld, C=%d; 1 <= C <= %d)", (long long)n, C,
               kLnMaxC);
  MINK_REQUIRE(gamma && dgamma && dbeta && workspace && (n == 0 || (dy && x && mean && invstd && dx)), "ln_bwd: NULL pointer");
  MINK_REQUIRE(!relu || n == 0 || y, "ln_bwd: fused ReLU needs the forward output");
  MINK_REQUIRE_WORKSPACE("ln_bwd", workspace_bytes, mink_ln_workspace_bytes(n, C), workspace);
  hipStream_t st = (hipStream_t)stream;
  const float *yr = relu ? y : nullptr;
  const bool vec = (C & 3) == 0 && aligned16(dy) && aligned16(x) && aligned16(yr) && aligned16(dx) && aligned16(dresidual) && aligned16(gamma);
  const int VEC = vec ? 4 : 1, ncg = C / VEC, gs = ln_group(ncg), items = (int)cdiv(ncg, gs);
  const unsigned nblk = ln_grid(n, gs, kLnRedBlocks);
  const size_t shm = (size_t)(NB / 64) * (64 / gs) * 2 * gs * items * VEC * sizeof(double);
  if (vec)
    ln_bwd_kernel<4><<<dim3(nblk), NB, shm, st>>>(dy, x, yr, n, C, gs, mean, invstd, gamma, dx, dresidual, (double *)workspace);
  else
    ln_bwd_kernel<1><<<dim3(nblk), NB, shm, st>>>(dy, x, yr, n, C, gs, mean, invstd, gamma, dx, dresidual, (double *)workspace);
  MINK_CHECK_LAUNCH();
  ln_param_grad_kernel<<<dim3((unsigned)cdiv(C, 4)), NB, 0, st>>>((const double *)workspace, (int)nblk, C, dgamma, dbeta);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
