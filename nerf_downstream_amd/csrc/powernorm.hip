// PowerNorm (MinkowskiPowerNorm) of the feature matrix x[n][C] on gfx950: a per-row group scaling by the root of the group's
// second moment, then a per-channel division by the root of the batch's (warm-up) or the running (after warm-up) second moment
// of the scaled rows, an affine map, and the optional residual add and ReLU of the other norm layers.  No mean is subtracted.
//
//   r[row][g] = 1 / sqrt(mean_{c in group g} x^2 + 1e-5)      xh = x * r          (G groups of Cg = C / G channels)
//   var[c]    = mean_rows xh^2                                 z  = xh * s[c]      s = 1/sqrt(var + eps) | 1/sqrt(phi + eps)
//   y         = [relu]( weight * z + bias [+ residual] )
// Backward is PowerNorm's approximate derivative with its running state ema_gz, then the exact derivative of the group scaling:
//   g = dy (masked by y > 0) * weight     a = g - (1 - alpha_bkw) * ema_gz * z     ema_gz += mean_rows (a * z)
//   dxh = a / sqrt(var + eps)             dx = r * (dxh - xh * mean_{group} (dxh * xh))
//
// Passes (all bandwidth-bound; B / element of x, fp32):
//   forward, training : group pass (read x -> r)  4 | column pass (read x, r -> partials)  4 | apply (read x, write y)  8
//   forward, eval     : group pass  4 | apply  8
//   backward          : column pass (read dy, x [, y])  8..12 | group pass (read dy, x [, y] twice, the second time from cache;
//                       write dx [, dresidual])  12..20
// What is kept for backward beside x (and y under a fused ReLU): r[n][G] -- n floats with the default G = 1 -- and two [C] vectors.
//
// The step counter, the warm-up branch, both running_phi updates and the ema_gz update are decided and done on the device:
// the group pass of the forward bumps iters[0] (one lane), the one-wave-per-channel finalize kernel that follows reads it.
// ema_gz is read by the backward column pass and by the group pass in its state BEFORE the step: the finalize kernel between
// them copies it aside (workspace) and writes the updated value, so the order of reads and the update is that of the formulas.
//
// Sums: every sum of squares / products is accumulated in DOUBLE from the first add on (per lane, across the lanes of a group
// by a fixed butterfly, across the row lanes of a workgroup through LDS in lane order, across the chunks by one wave in a fixed
// order), and rounded to fp32 once.  No floating-point atomics: two runs are bitwise equal.
#include <algorithm>

#include "rowpass.h"

namespace mink {

constexpr int PNB = 256;           // threads per workgroup
constexpr int kPnMaxC = MINK_PN_MAX_C;  // the widest registered layer is 2048 (the Bottleneck nets)
constexpr double kPnGroupEps = 1e-5;  // the group scaling's own epsilon (added in double); the module's eps does not reach it

// per-channel vectors ([C], any alignment: weight, bias, workspace slices): dword loads, they stay in cache
template <int VEC>
__device__ __forceinline__ void ldc(const float *__restrict__ p, float (&v)[VEC]) {
#pragma unroll
  for (int k = 0; k < VEC; ++k) v[k] = p[k];
}

__device__ __forceinline__ double group_sum_d(double v, int gs) {
  for (int o = gs >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One (row, group) item per gs lanes (a power of two <= 64), 64 / gs items per wave; lane `sub` of the item owns the column
// groups sub, sub + gs, ... of the Cg / VEC the group has.
struct PnItem {
  int gs, sub, iw, ipw;
  int64_t first, step;
};
__device__ __forceinline__ PnItem pn_item(int gs) {
  PnItem t;
  const int lane = threadIdx.x & 63;
  t.gs = gs, t.sub = lane & (gs - 1), t.iw = lane / gs, t.ipw = 64 / gs;
  t.first = ((int64_t)blockIdx.x * (PNB / 64) + (threadIdx.x >> 6)) * t.ipw;
  t.step = (int64_t)gridDim.x * (PNB / 64) * t.ipw;
  return t;
}

// ------------------------------------------------------------------------------------------------ group pass, forward
// r[row][g] = 1 / sqrt(mean of the group's x^2 + 1e-5); with `iters` (training) lane 0 of the grid bumps the step counter.
template <int VEC>
__global__ __launch_bounds__(PNB) void pn_rscale_kernel(const float *__restrict__ x, int ldx, int64_t n, int C, int G, int gs,
                                                        float *__restrict__ r, int64_t *__restrict__ iters) {
  if (iters && blockIdx.x == 0 && threadIdx.x == 0) iters[0] += 1;
  const PnItem t = pn_item(gs);
  const int Cg = C / G, ncg = Cg / VEC;
  const int64_t items = n * G;
  for (int64_t i0 = t.first; i0 < items; i0 += t.step) {  // (wave-uniform trip count: the shuffles see all 64 lanes)
    const int64_t item = i0 + t.iw;
    const bool live = item < items;
    double s = 0.0;
    if (live) {
      const int64_t row = item / G;
      const float *p = x + row * ldx + (int64_t)(item - row * G) * Cg;
      for (int cg = t.sub; cg < ncg; cg += gs) {
        float v[VEC];
        ldv<VEC>(p + cg * VEC, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) s += (double)v[k] * (double)v[k];
      }
    }
    s = group_sum_d(s, gs);
    if (live && t.sub == 0) r[item] = (float)(1.0 / sqrt(s / (double)Cg + kPnGroupEps));
  }
}

// ------------------------------------------------------------------------------------------------ column pass
// Column sums of row chunk blockIdx.x (of gridDim.x): partial[chunk][NS][C] (double).  A thread owns VEC channels (column
// group cg; tprb of them per workgroup, blockIdx.y walks further slabs) and the rows rl, rl + rlanes, ... of the chunk.
//   !BWD (NS = 1): sum xh^2, xh = x * r
//   BWD  (NS = 3): sum dym * z, sum dym, sum a * z;  dym = dy masked by yrelu > 0, z = x * r * s, a = dym * w - kema * z
template <int VEC, bool BWD>
__global__ __launch_bounds__(PNB) void pn_colsum_kernel(const float *__restrict__ a, const float *__restrict__ x, int ldx,
                                                        const float *__restrict__ yrelu, const float *__restrict__ r, int64_t n,
                                                        int C, int G, int tprb, const float *__restrict__ s,
                                                        const float *__restrict__ w, const float *__restrict__ ema, float k1,
                                                        double *__restrict__ partial) {
  constexpr int NS = BWD ? 3 : 1;
  extern __shared__ __align__(16) double s_red[];  // [rlanes][NS][W]
  const int nchunk = gridDim.x, chunk = blockIdx.x;
  const int64_t r0 = n * chunk / nchunk, r1 = n * (chunk + 1) / nchunk;
  const int ncg = C / VEC, rlanes = PNB / tprb, W = tprb * VEC;
  const int cl = threadIdx.x % tprb, rl = threadIdx.x / tprb, cg = blockIdx.y * tprb + cl;
  double acc[NS][VEC];
#pragma unroll
  for (int q = 0; q < NS; ++q)
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[q][k] = 0.0;
  if (rl < rlanes && cg < ncg) {
    const int c = cg * VEC, grp = c / (C / G);
    float sv[VEC], wv[VEC], ke[VEC];
    if (BWD) {
      ldc<VEC>(s + c, sv), ldc<VEC>(w + c, wv), ldc<VEC>(ema + c, ke);
#pragma unroll
      for (int k = 0; k < VEC; ++k) ke[k] *= k1;
    }
#pragma unroll 4
    for (int64_t row = r0 + rl; row < r1; row += rlanes) {
      const int64_t o = row * C + c;
      const float rr = r[row * G + grp];
      float xv[VEC];
      ldv<VEC>(x + row * ldx + c, xv);
      if (!BWD) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float xh = xv[k] * rr;
          acc[0][k] += (double)xh * (double)xh;
        }
      } else {
        float g[VEC];
        ldv<VEC>(a + o, g);
        if (yrelu) {
          float yv[VEC];
          ldv<VEC>(yrelu + o, yv);
#pragma unroll
          for (int k = 0; k < VEC; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float z = xv[k] * rr * sv[k];
          const float av = g[k] * wv[k] - ke[k] * z;
          acc[0][k] += (double)g[k] * (double)z, acc[1][k] += (double)g[k], acc[2][k] += (double)av * (double)z;
        }
      }
    }
  }
  if (rl < rlanes) {
    double *d = s_red + (int64_t)rl * NS * W + cl * VEC;
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
      for (int k = 0; k < VEC; ++k) d[q * W + k] = acc[q][k];
  }
  __syncthreads();
  double *out = partial + (int64_t)chunk * NS * C;
  for (int e = threadIdx.x; e < NS * W; e += PNB) {
    const int q = e / W, c = blockIdx.y * W + (e - q * W);
    if (c >= C) continue;
    double t = 0.0;
    for (int j = 0; j < rlanes; ++j) t += s_red[(int64_t)j * NS * W + e];
    out[(int64_t)q * C + c] = t;
  }
}

// NS column sums over `count` chunk partials by one wave: lane l adds chunks l, l + 64, ... in order, then a fixed butterfly
template <int NS>
__device__ __forceinline__ void wave_sums(const double *__restrict__ p, int count, int C, double (&out)[NS]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < NS; ++q) out[q] = 0.0;
  for (int j = lane; j < count; j += 64)
#pragma unroll
    for (int q = 0; q < NS; ++q) out[q] += p[((int64_t)j * NS + q) * C];
#pragma unroll
  for (int q = 0; q < NS; ++q)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) out[q] += __shfl_xor(out[q], o, 64);
}

// grid ceil(C / 4): one wave per channel.  it = iters[0], already bumped by the group pass.
//   var = sum / n;  s = it <= warmup ? 1/sqrt(var + eps) : 1/sqrt(phi + eps) (phi before this step's update);
//   it < warmup: phi = phi (it - 1) / it + var / it;   always: phi = afwd phi + (1 - afwd) var
__global__ __launch_bounds__(PNB) void pn_fwd_finalize_kernel(const double *__restrict__ partial, int nchunk, int64_t n, int C,
                                                              float eps, float afwd, int64_t warmup,
                                                              const int64_t *__restrict__ iters, float *__restrict__ phi,
                                                              float *__restrict__ var, float *__restrict__ s) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;  // whole wave
  double sum[1];
  wave_sums<1>(partial + c, nchunk, C, sum);
  if ((threadIdx.x & 63) != 0) return;
  const int64_t it = iters[0];
  const float v = (float)(sum[0] / (double)n);
  const float p0 = phi[c];
  var[c] = v;
  s[c] = (float)(1.0 / sqrt((double)(it <= warmup ? v : p0) + (double)eps));
  double p = (double)p0;
  if (it < warmup) p = p * (double)(it - 1) / (double)it + (double)v / (double)it;
  p = (double)afwd * p + (1.0 - (double)afwd) * (double)v;
  phi[c] = (float)p;
}

// eval: s = 1 / sqrt(phi + eps)
__global__ __launch_bounds__(PNB) void pn_eval_scale_kernel(const float *__restrict__ phi, int C, float eps, float *__restrict__ s) {
  const int c = blockIdx.x * PNB + threadIdx.x;
  if (c < C) s[c] = (float)(1.0 / sqrt((double)phi[c] + (double)eps));
}

// y = [relu]( w * (x * r * s) + b [+ residual] ), flat over the n * C / VEC column groups
template <int VEC>
__global__ __launch_bounds__(PNB) void pn_apply_kernel(const float *__restrict__ x, int ldx, const float *__restrict__ r, int64_t n, int C,
                                                       int G, const float *__restrict__ s, const float *__restrict__ w,
                                                       const float *__restrict__ b, const float *__restrict__ residual, int relu,
                                                       float *__restrict__ y) {
  const int ncg = C / VEC, Cg = C / G;
  const int64_t total = n * ncg;
  for (int64_t i = (int64_t)blockIdx.x * PNB + threadIdx.x; i < total; i += (int64_t)gridDim.x * PNB) {
    const int64_t row = i / ncg;
    const int c = (int)(i - row * ncg) * VEC;
    const float rr = r[row * G + c / Cg];
    float v[VEC], sv[VEC], wv[VEC], bv[VEC];
    ldv<VEC>(x + row * ldx + c, v);
    ldc<VEC>(s + c, sv), ldc<VEC>(w + c, wv), ldc<VEC>(b + c, bv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = wv[k] * (v[k] * rr * sv[k]) + bv[k];
    if (residual) {
      float t[VEC];
      ldv<VEC>(residual + i * VEC, t);
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] += t[k];
    }
    if (relu) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = relu_keep_nan(v[k]);
    }
    stv<VEC>(y + i * VEC, v);
  }
}

// ------------------------------------------------------------------------------------------------ backward
// one wave per channel: dweight = sum dym z, dbias = sum dym; training: ema_old = ema (kept for the group pass),
// ema += sum a z / n, isv = 1 / sqrt(var + eps); eval: ema_old = 0, isv = s.
__global__ __launch_bounds__(PNB) void pn_bwd_finalize_kernel(const double *__restrict__ partial, int nchunk, int64_t n, int C,
                                                              float eps, int training, const float *__restrict__ var,
                                                              const float *__restrict__ s, float *__restrict__ ema,
                                                              float *__restrict__ ema_old, float *__restrict__ isv,
                                                              float *__restrict__ dweight, float *__restrict__ dbias) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;  // whole wave
  double sum[3];
  wave_sums<3>(partial + c, nchunk, C, sum);
  if ((threadIdx.x & 63) != 0) return;
  dweight[c] = (float)sum[0];
  dbias[c] = (float)sum[1];
  if (training) {
    const float e = ema[c];
    ema_old[c] = e;
    ema[c] = (float)((double)e + sum[2] / (double)n);
    isv[c] = (float)(1.0 / sqrt((double)var[c] + (double)eps));
  } else {
    ema_old[c] = 0.f;
    isv[c] = s[c];
  }
}

// group pass: dxh = (dym w - k1 ema_old z) isv, t = mean over the group of dxh xh, dx = r (dxh - xh t); dresidual = dym.
// Two sweeps over the group's channels: the second one finds the row in cache.
template <int VEC>
__global__ __launch_bounds__(PNB) void pn_bwd_group_kernel(const float *__restrict__ dy, const float *__restrict__ x, int ldx,
                                                           const float *__restrict__ yrelu, const float *__restrict__ r, int64_t n,
                                                           int C, int G, int gs, const float *__restrict__ s,
                                                           const float *__restrict__ w, const float *__restrict__ ema_old,
                                                           const float *__restrict__ isv, float k1, float *__restrict__ dx,
                                                           float *__restrict__ dres) {
  const PnItem t = pn_item(gs);
  const int Cg = C / G, ncg = Cg / VEC;
  const int64_t items = n * G;
  for (int64_t i0 = t.first; i0 < items; i0 += t.step) {
    const int64_t item = i0 + t.iw;
    const bool live = item < items;
    const int64_t row = live ? item / G : 0;
    const int c0 = live ? (int)(item - row * G) * Cg : 0;
    const int64_t base = row * C + c0, xbase = row * ldx + c0;
    const float rr = live ? r[item] : 0.f;
    double acc = 0.0;
    for (int sweep = 0; sweep < 2; ++sweep) {
      const float tm = (float)(acc / (double)Cg);  // (sweep 1 only)
      if (live) {
        for (int cg = t.sub; cg < ncg; cg += gs) {
          const int64_t o = base + cg * VEC;
          const int c = c0 + cg * VEC;
          float g[VEC], xv[VEC], sv[VEC], wv[VEC], ev[VEC], iv[VEC];
          ldv<VEC>(dy + o, g);
          ldv<VEC>(x + xbase + cg * VEC, xv);
          if (yrelu) {
            float yv[VEC];
            ldv<VEC>(yrelu + o, yv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
          }
          ldc<VEC>(s + c, sv), ldc<VEC>(w + c, wv), ldc<VEC>(ema_old + c, ev), ldc<VEC>(isv + c, iv);
          float out[VEC];
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const float xh = xv[k] * rr;
            const float z = xh * sv[k];
            const float dxh = (g[k] * wv[k] - (k1 * ev[k]) * z) * iv[k];
            if (sweep == 0)
              acc += (double)dxh * (double)xh;
            else
              out[k] = rr * (dxh - xh * tm);
          }
          if (sweep == 1) {
            stv<VEC>(dx + o, out);
            if (dres) stv<VEC>(dres + o, g);
          }
        }
      }
      if (sweep == 0) acc = group_sum_d(acc, gs);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
static inline int pn_chunks(int64_t n) { return sample_chunks(n, 1); }

struct PnWorkspace {
  double *partial;  // [chunks][3][C]
  float *v0, *v1;   // [C] each: eval forward s | backward ema_old, isv
};
static inline int64_t pn_ws_layout(int64_t n, int C, void *base, PnWorkspace *w) {
  const int64_t np = (int64_t)pn_chunks(n) * 3 * C;
  if (w) {
    w->partial = (double *)base;
    w->v0 = (float *)(w->partial + np);
    w->v1 = w->v0 + C;
  }
  return np * (int64_t)sizeof(double) + 2 * (int64_t)C * (int64_t)sizeof(float);
}

static inline int pn_group_lanes(int ncg) {
  int gs = 1;
  while (gs < ncg && gs < 64) gs <<= 1;
  return gs;
}
static inline unsigned pn_item_grid(int64_t items, int gs) {
  const int64_t per_block = (int64_t)(PNB / 64) * (64 / gs);
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(items, per_block), 8192));
}

struct PnColLaunch {
  int tprb, rlanes, W;
  dim3 grid;
  PnColLaunch(int64_t n, int C, int VEC) : tprb(std::min(C / VEC, PNB)), rlanes(PNB / tprb), W(tprb * VEC),
                                           grid((unsigned)pn_chunks(n), (unsigned)cdiv(C / VEC, tprb)) {}
};

static inline bool pn_shape_ok(int64_t n, int C, int G) { return n >= 0 && n <= 0x7fffffffLL && C >= 1 && C <= kPnMaxC && G >= 1 && G <= C && C % G == 0; }

#define MINK_REQUIRE_PN_SHAPE(name, n, C, G)                                                                                       \
  MINK_REQUIRE(pn_shape_ok(n, C, G), name ": bad shape (n=%lld, C=%d, groups=%d; 1 <= C <= %d, groups must divide C)", (long long)(n), \
               (int)(C), (int)(G), kPnMaxC)

static void pn_launch_rscale(bool vec, const float *x, int ldx, int64_t n, int C, int G, float *r, int64_t *iters, hipStream_t st) {
  const int gs = pn_group_lanes(C / G / (vec ? 4 : 1));
  const unsigned grid = pn_item_grid(n * G, gs);
  if (vec)
    pn_rscale_kernel<4><<<dim3(grid), PNB, 0, st>>>(x, ldx, n, C, G, gs, r, iters);
  else
    pn_rscale_kernel<1><<<dim3(grid), PNB, 0, st>>>(x, ldx, n, C, G, gs, r, iters);
}

static void pn_launch_apply(bool vec, const float *x, int ldx, const float *r, int64_t n, int C, int G, const float *s, const float *w,
                            const float *b, const float *res, int relu, float *y, hipStream_t st) {
  if (vec)
    pn_apply_kernel<4><<<dim3(flat_grid(n * (C / 4), PNB, 4096)), PNB, 0, st>>>(x, ldx, r, n, C, G, s, w, b, res, relu, y);
  else
    pn_apply_kernel<1><<<dim3(flat_grid(n * C, PNB, 4096)), PNB, 0, st>>>(x, ldx, r, n, C, G, s, w, b, res, relu, y);
}

}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_pn_workspace_bytes(int64_t n, int32_t C, int32_t groups) {
  if (!pn_shape_ok(n, C, groups)) return 0;
  return pn_ws_layout(n, C, nullptr, nullptr);
}

int mink_pn_fwd(const float *x, int32_t ldx, int64_t n, int32_t C, int32_t groups, float eps, float alpha_fwd, int64_t warmup_iters,
                const float *weight, const float *bias, const float *residual, int32_t relu, float *y, float *rscale, float *var,
                float *scale, float *running_phi, int64_t *iters, void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE_PN_SHAPE("pn_fwd", n, C, groups);
  MINK_REQUIRE(ldx >= C, "pn_fwd: row pitch ldx=%d below C=%d", ldx, C);
  MINK_REQUIRE(n >= 1, "pn_fwd: no rows (the batch second moment of an empty batch is undefined; running_phi would become NaN)");
  MINK_REQUIRE(x && weight && bias && y && rscale && var && scale && running_phi && iters && workspace, "pn_fwd: NULL pointer");
  MINK_REQUIRE(((uintptr_t)iters & 7) == 0, "pn_fwd: iters must be 8-byte aligned");
  MINK_REQUIRE_WORKSPACE("pn_fwd", workspace_bytes, mink_pn_workspace_bytes(n, C, groups), workspace);
  hipStream_t st = (hipStream_t)stream;
  PnWorkspace ws;
  pn_ws_layout(n, C, workspace, &ws);
  const bool vec = ((C / groups) & 3) == 0 && (ldx & 3) == 0 && aligned16(x) && aligned16(y) && aligned16(residual);
  pn_launch_rscale(vec, x, ldx, n, C, groups, rscale, iters, st);
  MINK_CHECK_LAUNCH();
  const PnColLaunch l(n, C, vec ? 4 : 1);
  const size_t shm = (size_t)l.rlanes * l.W * sizeof(double);
  if (vec)
    pn_colsum_kernel<4, false><<<l.grid, PNB, shm, st>>>(nullptr, x, ldx, nullptr, rscale, n, C, groups, l.tprb, nullptr, nullptr, nullptr, 0.f, ws.partial);
  else
    pn_colsum_kernel<1, false><<<l.grid, PNB, shm, st>>>(nullptr, x, ldx, nullptr, rscale, n, C, groups, l.tprb, nullptr, nullptr, nullptr, 0.f, ws.partial);
  MINK_CHECK_LAUNCH();
  pn_fwd_finalize_kernel<<<dim3((unsigned)cdiv(C, 4)), PNB, 0, st>>>(ws.partial, pn_chunks(n), n, C, eps, alpha_fwd, warmup_iters, iters,
                                                                  running_phi, var, scale);
  MINK_CHECK_LAUNCH();
  pn_launch_apply(vec, x, ldx, rscale, n, C, groups, scale, weight, bias, residual, relu, y, st);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_pn_apply(const float *x, int32_t ldx, int64_t n, int32_t C, int32_t groups, float eps, const float *running_phi, const float *weight,
                  const float *bias, const float *residual, int32_t relu, float *y, float *rscale, float *scale, void *stream) {
  MINK_REQUIRE_PN_SHAPE("pn_apply", n, C, groups);
  MINK_REQUIRE(ldx >= C, "pn_apply: row pitch ldx=%d below C=%d", ldx, C);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(x && running_phi && weight && bias && y && rscale && scale, "pn_apply: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = ((C / groups) & 3) == 0 && (ldx & 3) == 0 && aligned16(x) && aligned16(y) && aligned16(residual);
  pn_launch_rscale(vec, x, ldx, n, C, groups, rscale, nullptr, st);
  MINK_CHECK_LAUNCH();
  pn_eval_scale_kernel<<<dim3((unsigned)cdiv(C, PNB)), PNB, 0, st>>>(running_phi, C, eps, scale);
  MINK_CHECK_LAUNCH();
  pn_launch_apply(vec, x, ldx, rscale, n, C, groups, scale, weight, bias, residual, relu, y, st);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_pn_bwd(const float *dy, const float *x, int32_t ldx, const float *y, int64_t n, int32_t C, int32_t groups, float eps, float alpha_bkw,
                int32_t training, const float *rscale, const float *var, const float *scale, const float *weight, int32_t relu,
                float *ema_gz, float *dx, float *dresidual, float *dweight, float *dbias, void *workspace, int64_t workspace_bytes,
                void *stream) {
  MINK_REQUIRE_PN_SHAPE("pn_bwd", n, C, groups);
  MINK_REQUIRE(ldx >= C, "pn_bwd: row pitch ldx=%d below C=%d", ldx, C);
  MINK_REQUIRE(n >= 1, "pn_bwd: no rows");
  MINK_REQUIRE(dy && x && rscale && scale && weight && dx && dweight && dbias && workspace, "pn_bwd: NULL pointer");
  MINK_REQUIRE(!training || (var && ema_gz), "pn_bwd: the training-mode backward needs var and ema_gz");
  MINK_REQUIRE(!relu || y, "pn_bwd: fused ReLU needs the forward output");
  MINK_REQUIRE_WORKSPACE("pn_bwd", workspace_bytes, mink_pn_workspace_bytes(n, C, groups), workspace);
  hipStream_t st = (hipStream_t)stream;
  PnWorkspace ws;
  pn_ws_layout(n, C, workspace, &ws);
  const float *yr = relu ? y : nullptr;
  const float k1 = training ? 1.f - alpha_bkw : 0.f;
  const float *ema_in = training ? ema_gz : scale;  // (eval: multiplied by k1 = 0 -- any finite [C] vector)
  const bool vec = ((C / groups) & 3) == 0 && (ldx & 3) == 0 && aligned16(dy) && aligned16(x) && aligned16(yr) && aligned16(dx) && aligned16(dresidual);
  const PnColLaunch l(n, C, vec ? 4 : 1);
  const size_t shm = (size_t)l.rlanes * 3 * l.W * sizeof(double);
  if (vec)
    pn_colsum_kernel<4, true><<<l.grid, PNB, shm, st>>>(dy, x, ldx, yr, rscale, n, C, groups, l.tprb, scale, weight, ema_in, k1, ws.partial);
  else
    pn_colsum_kernel<1, true><<<l.grid, PNB, shm, st>>>(dy, x, ldx, yr, rscale, n, C, groups, l.tprb, scale, weight, ema_in, k1, ws.partial);
  MINK_CHECK_LAUNCH();
  pn_bwd_finalize_kernel<<<dim3((unsigned)cdiv(C, 4)), PNB, 0, st>>>(ws.partial, pn_chunks(n), n, C, eps, training, var, scale, ema_gz, ws.v0,
                                                                  ws.v1, dweight, dbias);
  MINK_CHECK_LAUNCH();
  const int gs = pn_group_lanes(C / groups / (vec ? 4 : 1));
  const unsigned grid = pn_item_grid(n * groups, gs);
  if (vec)
    pn_bwd_group_kernel<4><<<dim3(grid), PNB, 0, st>>>(dy, x, ldx, yr, rscale, n, C, groups, gs, scale, weight, ws.v0, ws.v1, k1, dx, dresidual);
  else
    pn_bwd_group_kernel<1><<<dim3(grid), PNB, 0, st>>>(dy, x, ldx, yr, rscale, n, C, groups, gs, scale, weight, ws.v0, ws.v1, k1, dx, dresidual);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
