// Dynamic graph layers of DGCNN (reference co3d_3d/src/models/mink/dgcnn.py:8-38,81-85) on the rows of a field: the
// k-nearest-neighbour graph of every sample in feature space, and the edge convolution over it fused with its batch norm,
// LeakyReLU(0.2) and the maximum over the k edges.  Neither ever forms an n x n or an edge-sized (n x k x C) tensor.
//
//   mink_knn        : one workgroup per tile of 32 query rows of ONE sample (the tile -> sample search walks the device
//                     offsets, so nothing is read back); the sample's rows stream through LDS 128 at a time, the inner
//                     products run on v_mfma_f32_32x32x2_f32 (exact fp32: a fused multiply-add chain, k ascending), the score
//                     ||x_j||^2 - 2 x_i.x_j ranks as the squared distance does.  Every wave keeps the running top-k of 8
//                     queries sorted across its lanes (lane l = the l-th nearest so far, k <= 64): a candidate is first
//                     tested against the k-th entry, and only a survivor is inserted (one ballot, one lane shift).
//   mink_knn_cross  : the same tile loop with the queries in one matrix and the candidates in another (per-sample offsets on
//                     both sides), and an epilogue that recomputes the squared distance of every chosen pair by direct
//                     differences, accumulated in double and rounded once (query from the LDS tile, candidate row from memory; a -1
//                     slot is never followed)
//   mink_edge_stats : per-channel sum / sum of squares of e[i][j] = P[idx[i][j]] + Q[i] over the n k edges, as the double
//                     column partials [rows][2][C] that mink_bn_stats_from_partials consumes
//   mink_edge_fwd   : y[i][c] = max_j lrelu(gamma (e - mean) invstd + beta), arg = the lowest slot attaining it
//   mink_edge_bwd   : three launches (g + column partials; finalize; dP and dQ), every sum in a fixed order, no atomics
#include <limits.h>

#include "common.h"

namespace mink {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ---------------------------------------------------------------------------------------------- kNN
constexpr int KQ = 32, KC = 128, KK = 32;  // query rows / candidate rows / channels per LDS chunk
constexpr int KLQ = KQ + 1, KLC = KC + 1;  // k-major LDS pitches (odd: the two half-waves of an MFMA operand read apart)
constexpr int KQW = KQ / 4;                // queries owned by one of the four waves

__device__ __forceinline__ bool knn_before(float d, int j, float dk, int jk) { return d < dk || (d == dk && j < jk); }

// The tile loop both entry points share.  Queries are rows qs0 .. qs1 of q (sample b of qoff), candidates rows cs0 .. cs1 of c
// (sample b of coff); CROSS = false is mink_knn, instantiated with q = c and qoff = coff, where the two ranges are one.
template <bool CROSS>
__device__ __forceinline__ void knn_body(const float *__restrict__ q, int64_t ldq, int64_t nq, const float *__restrict__ c, int64_t ldc,
                                         int64_t nc, int C, const int *__restrict__ qoff, const int *__restrict__ coff, int B, int k,
                                         int *__restrict__ idx, float *__restrict__ dist) {
  extern __shared__ float sQ[];    // [Cpad][KLQ]: the query tile, k-major, zero-padded to a multiple of KK channels
  __shared__ float sB[KK * KLC];   // a candidate chunk [KK][KLC], k-major; then the score tile [KQ][KLC]
  __shared__ float sN[KC];         // ||x_j||^2 of the candidate tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Cpad = (C + KK - 1) / KK * KK;
  // the sample and the tile of this workgroup: tiles are numbered sample by sample
  int blk = blockIdx.x, b = 0, qs0 = 0, qs1 = 0;
  for (; b < B; ++b) {
    qs0 = qoff[b], qs1 = qoff[b + 1];
    if (CROSS) qs0 = qs0 < 0 ? 0 : qs0, qs1 = qs1 > nq ? (int)nq : qs1;  // (never outside q, whatever the offsets hold)
    const int t = qs1 > qs0 ? (qs1 - qs0 + KQ - 1) / KQ : 0;
    if (blk < t) break;
    blk -= t;
  }
  if (b == B) return;  // (the grid is the upper bound n / KQ + B)
  int cs0 = qs0, cs1 = qs1;
  if (CROSS) {
    cs0 = coff[b], cs1 = coff[b + 1];
    cs0 = cs0 < 0 ? 0 : cs0, cs1 = cs1 > nc ? (int)nc : cs1;
  }
  const int q0 = qs0 + blk * KQ;
  for (int e = tid; e < KQ * Cpad; e += 256) {
    const int r = e / Cpad, ch = e - r * Cpad;
    sQ[ch * KLQ + r] = (q0 + r < qs1 && ch < C) ? q[(int64_t)(q0 + r) * ldq + ch] : 0.f;
  }
  float bd[KQW];
  int bj[KQW];
#pragma unroll
  for (int qi = 0; qi < KQW; ++qi) bd[qi] = __builtin_inff(), bj[qi] = INT_MAX;

  for (int c0 = cs0; c0 < cs1; c0 += KC) {
    f32x16 acc = (f32x16){0};
    float nrm = 0.f;
    for (int k0 = 0; k0 < Cpad; k0 += KK) {
      __syncthreads();  // sB is free: the previous chunk's MFMAs / the previous tile's selection are done (and sQ is written)
      for (int e = tid; e < KC * KK; e += 256) {
        const int r = e >> 5, kk = e & 31;
        sB[kk * KLC + r] = (c0 + r < cs1 && k0 + kk < C) ? c[(int64_t)(c0 + r) * ldc + k0 + kk] : 0.f;
      }
      __syncthreads();
      if (tid < KC) {
#pragma unroll 8
        for (int kk = 0; kk < KK; ++kk) {
          const float v = sB[kk * KLC + tid];
          nrm = fmaf(v, v, nrm);
        }
      }
      const float *a = sQ + (k0 + (lane >> 5)) * KLQ + (lane & 31), *bb = sB + (lane >> 5) * KLC + wave * 32 + (lane & 31);
#pragma unroll
      for (int kk = 0; kk < KK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk * KLQ], bb[kk * KLC], acc, 0, 0, 0);
    }
    __syncthreads();  // every wave has read its last chunk
    if (tid < KC) sN[tid] = nrm;
    __syncthreads();
    {
      const int col = wave * 32 + (lane & 31);
      const float nj = sN[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        sB[row * KLC + col] = fmaf(-2.f, acc[r], nj);
      }
    }
    __syncthreads();
    // selection: wave w owns queries 8 w .. 8 w + 7; candidates ascend, so among equal scores the lower row stays ahead
#pragma unroll
    for (int qi = 0; qi < KQW; ++qi) {
      const int qr = wave * KQW + qi;
      if (q0 + qr >= qs1) continue;  // (uniform)
      float dk = __shfl(bd[qi], k - 1, 64);
      int jk = __shfl(bj[qi], k - 1, 64);
#pragma unroll
      for (int half = 0; half < KC / 64; ++half) {
        const int cand = c0 + half * 64 + lane;
        const float s = sB[qr * KLC + half * 64 + lane];
        unsigned long long mask = __ballot(cand < cs1 && knn_before(s, cand, dk, jk));
        while (mask) {
          const int src = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          const float ns = __shfl(s, src, 64);
          const int nj = c0 + half * 64 + src;
          if (!knn_before(ns, nj, dk, jk)) continue;  // (the k-th entry moved since the ballot)
          const int pos = __popcll(__ballot(knn_before(bd[qi], bj[qi], ns, nj)));  // the list is sorted: a prefix
          const float ud = __shfl_up(bd[qi], 1, 64);
          const int uj = __shfl_up(bj[qi], 1, 64);
          if (lane == pos) bd[qi] = ns, bj[qi] = nj;
          else if (lane > pos) bd[qi] = ud, bj[qi] = uj;
          dk = __shfl(bd[qi], k - 1, 64);
          jk = __shfl(bj[qi], k - 1, 64);
        }
      }
    }
  }
#pragma unroll
  for (int qi = 0; qi < KQW; ++qi) {
    const int row = q0 + wave * KQW + qi;
    if (row < qs1 && lane < k) idx[(int64_t)row * k + lane] = bj[qi] == INT_MAX ? -1 : bj[qi];  // -1: fewer than k comparable rows
    if (CROSS && dist && row < qs1 && lane < k) {
      // the squared distance of the chosen pair by direct differences (the ranking score is not reused: it cancels); the
      // query from the LDS tile (one address per wave: a broadcast), the candidate row from memory; a -1 slot is not followed.
      // Differences and the fused multiply-add chain in double, rounded to fp32 once: an fp32 chain rounds every difference
      // as well and is off by up to (C + 2) u, measured 3.15 u at C = 3 against the C u the callers are promised.
      float d = __builtin_inff();
      if (bj[qi] != INT_MAX) {
        const float *cr = c + (int64_t)bj[qi] * ldc;
        const float *qr = sQ + wave * KQW + qi;
        double acc = 0.0;
        for (int ch = 0; ch < C; ++ch) {
          const double t = (double)qr[ch * KLQ] - (double)cr[ch];
          acc = fma(t, t, acc);
        }
        d = (float)acc;
      }
      dist[(int64_t)row * k + lane] = d;
    }
  }
}

__global__ __launch_bounds__(256) void knn_kernel(const float *__restrict__ x, int64_t ldx, int C, const int *__restrict__ boff, int B,
                                                  int k, int *__restrict__ idx) {
  knn_body<false>(x, ldx, 0, x, ldx, 0, C, boff, boff, B, k, idx, nullptr);
}

__global__ __launch_bounds__(256) void knn_cross_kernel(const float *__restrict__ q, int64_t ldq, int64_t nq, const float *__restrict__ c,
                                                        int64_t ldc, int64_t nc, int C, const int *__restrict__ qoff,
                                                        const int *__restrict__ coff, int B, int k, int *__restrict__ idx,
                                                        float *__restrict__ dist) {
  knn_body<true>(q, ldq, nq, c, ldc, nc, C, qoff, coff, B, k, idx, dist);
}

// ---------------------------------------------------------------------------------------------- edge convolution
constexpr int EC = 64, ER = 4;  // a workgroup: 64 channels x 4 row lanes

// the two lines every edge kernel shares: the backward must see the normalised edge and the sign the forward saw
__device__ __forceinline__ float edge_xhat(float p, float q, float mu, float is) {
#pragma clang fp contract(off)
  return ((p + q) - mu) * is;
}
__device__ __forceinline__ float edge_z(float xh, float g, float b) {
#pragma clang fp contract(off)
  return g * xh + b;
}
__device__ __forceinline__ int64_t edge_row(const int *__restrict__ idx, int64_t e, int64_t n) {  // (never outside P, whatever idx holds)
  const int64_t r = idx[e];
  return r < 0 ? 0 : (r >= n ? n - 1 : r);
}

// sum over the row lanes in lane order, then one partial row [2][C] per workgroup row
__device__ __forceinline__ void edge_write_partials(double s, double ss, int c, int C, double *__restrict__ partial) {
  __shared__ double sh[2][ER][EC];
  const int cl = threadIdx.x & (EC - 1), rl = threadIdx.x / EC;
  sh[0][rl][cl] = s, sh[1][rl][cl] = ss;
  __syncthreads();
  if (rl == 0 && c < C) {
    double a = sh[0][0][cl], b = sh[1][0][cl];
#pragma unroll
    for (int r = 1; r < ER; ++r) a += sh[0][r][cl], b += sh[1][r][cl];
    partial[((int64_t)blockIdx.x * 2) * C + c] = a;
    partial[((int64_t)blockIdx.x * 2 + 1) * C + c] = b;
  }
}

__global__ __launch_bounds__(256) void edge_stats_kernel(const float *__restrict__ P, const float *__restrict__ Q,
                                                         const int *__restrict__ idx, int64_t n, int k, int C, int64_t chunk,
                                                         double *__restrict__ partial) {
  const int c = blockIdx.y * EC + (threadIdx.x & (EC - 1)), rl = threadIdx.x / EC;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
  double s = 0.0, ss = 0.0;
  if (c < C)
    for (int64_t i = r0 + rl; i < r1; i += ER) {
      const float q = Q[i * C + c];
      for (int j = 0; j < k; ++j) {
        const float e = P[edge_row(idx, i * k + j, n) * C + c] + q;
        s += (double)e, ss += (double)e * (double)e;
      }
    }
  edge_write_partials(s, ss, c, C, partial);
}

__global__ __launch_bounds__(256) void edge_fwd_kernel(const float *__restrict__ P, const float *__restrict__ Q,
                                                       const int *__restrict__ idx, int64_t n, int k, int C,
                                                       const float *__restrict__ mean, const float *__restrict__ invstd,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       float *__restrict__ y, uint8_t *__restrict__ arg) {
  const int c = blockIdx.y * EC + (threadIdx.x & (EC - 1));
  const int64_t i = (int64_t)blockIdx.x * ER + threadIdx.x / EC;
  if (c >= C || i >= n) return;
  const float q = Q[i * C + c], mu = mean[c], is = invstd[c], g = gamma[c], bt = beta[c];
  float best = edge_z(edge_xhat(P[edge_row(idx, i * k, n) * C + c], q, mu, is), g, bt);
  int at = 0;
  for (int j = 1; j < k; ++j) {
    const float z = edge_z(edge_xhat(P[edge_row(idx, i * k + j, n) * C + c], q, mu, is), g, bt);
    if (max_replaces(z, best)) best = z, at = j;  // (LeakyReLU is increasing: the maximum of z is the maximum of lrelu(z);
                                                  //  the first NaN wins, as in torch)
  }
  y[i * C + c] = best > 0.f ? best : 0.2f * best;
  arg[i * C + c] = (uint8_t)at;
}

// g = dy * lrelu'(z at the arg slot), kept for the second pass; column partials of (g, g * xhat at the arg slot)
__global__ __launch_bounds__(256) void edge_bwd_g_kernel(const float *__restrict__ dy, const float *__restrict__ P,
                                                         const float *__restrict__ Q, const int *__restrict__ idx,
                                                         const uint8_t *__restrict__ arg, int64_t n, int k, int C, int64_t chunk,
                                                         const float *__restrict__ mean, const float *__restrict__ invstd,
                                                         const float *__restrict__ gamma, const float *__restrict__ beta,
                                                         float *__restrict__ gbuf, double *__restrict__ partial) {
  const int c = blockIdx.y * EC + (threadIdx.x & (EC - 1)), rl = threadIdx.x / EC;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
  double s = 0.0, ss = 0.0;
  if (c < C) {
    const float mu = mean[c], is = invstd[c], g = gamma[c], bt = beta[c];
    for (int64_t i = r0 + rl; i < r1; i += ER) {
      int a = arg[i * C + c];
      a = a < k ? a : k - 1;
      const float xh = edge_xhat(P[edge_row(idx, i * k + a, n) * C + c], Q[i * C + c], mu, is);
      const float gg = dy[i * C + c] * (edge_z(xh, g, bt) > 0.f ? 1.f : 0.2f);
      gbuf[i * C + c] = gg;
      s += (double)gg, ss += (double)gg * (double)xh;
    }
  }
  edge_write_partials(s, ss, c, C, partial);
}

__global__ void edge_bwd_finalize_kernel(const double *__restrict__ partial, int rows, int C, float *__restrict__ dgamma,
                                         float *__restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, ss = 0.0;
  for (int r = 0; r < rows; ++r) s += partial[((int64_t)r * 2) * C + c], ss += partial[((int64_t)r * 2 + 1) * C + c];
  dbeta[c] = (float)s, dgamma[c] = (float)ss;
}

// dQ[i] = the sum of de over the k edges leaving row i; dP[r] = the sum over the edges arriving at row r (members / seg: the
// flat edge ids i k + j grouped by idx, ascending inside a segment)
__global__ __launch_bounds__(256) void edge_bwd_pq_kernel(const float *__restrict__ gbuf, const float *__restrict__ P,
                                                          const float *__restrict__ Q, const int *__restrict__ idx,
                                                          const uint8_t *__restrict__ arg, int64_t n, int k, int C,
                                                          const float *__restrict__ mean, const float *__restrict__ invstd,
                                                          const float *__restrict__ gamma, const float *__restrict__ dgamma,
                                                          const float *__restrict__ dbeta, int training, float inv_m,
                                                          const int *__restrict__ members, const int *__restrict__ seg,
                                                          float *__restrict__ dP, float *__restrict__ dQ) {
#pragma clang fp contract(off)
  const int c = blockIdx.y * EC + (threadIdx.x & (EC - 1));
  const int64_t row = (int64_t)blockIdx.x * ER + threadIdx.x / EC;
  if (c >= C || row >= n) return;
  const float mu = mean[c], is = invstd[c], scale = gamma[c] * is;
  const float db = training ? dbeta[c] * inv_m : 0.f, dg = training ? dgamma[c] * inv_m : 0.f;
  const float q = Q[row * C + c], p = P[row * C + c];
  float sx = 0.f;
  if (training)
    for (int j = 0; j < k; ++j) sx += edge_xhat(P[edge_row(idx, row * k + j, n) * C + c], q, mu, is);
  dQ[row * C + c] = scale * (gbuf[row * C + c] - (float)k * db - sx * dg);
  const int e0 = seg[row], e1 = seg[row + 1];
  float G = 0.f, tx = 0.f;
  for (int e = e0; e < e1; ++e) {
    const int m = members[e];
    const int64_t i = m / k;
    const int j = m - (int)i * k;
    if (i < 0 || i >= n) continue;  // (never outside the buffers, whatever the lists hold)
    if (training) tx += edge_xhat(p, Q[i * C + c], mu, is);
    if (arg[i * C + c] == j) G += gbuf[i * C + c];
  }
  dP[row * C + c] = scale * (G - (float)(e1 - e0) * db - tx * dg);
}

int edge_args(const char *what, int64_t n, int32_t k, int32_t C) {
  MINK_REQUIRE(n >= 0 && k >= 1 && k <= MINK_KNN_MAX_K && C >= 1 && n * (int64_t)k < ((int64_t)1 << 31),
               "%s: bad shape (n %lld, k %d of 1..%d, C %d, n k < 2^31)", what, (long long)n, k, MINK_KNN_MAX_K, C);
  return MINK_OK;
}

int edge_rows(int64_t n) {
  const int64_t r = cdiv(n, 4 * ER);
  return (int)(r < 1 ? 1 : (r > 256 ? 256 : r));
}

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int mink_knn(const float *x, int64_t n, int64_t ldx, int32_t C, const int32_t *batch_offsets, int32_t B, int32_t k, int32_t *idx,
             void *stream) {
  MINK_REQUIRE(k >= 1 && k <= MINK_KNN_MAX_K, "knn: k = %d outside 1..%d", k, MINK_KNN_MAX_K);
  MINK_REQUIRE(C >= 1 && C <= MINK_KNN_MAX_C, "knn: C = %d outside 1..%d", C, MINK_KNN_MAX_C);
  MINK_REQUIRE(n >= 0 && B >= 1 && ldx >= C && n * (int64_t)k < ((int64_t)1 << 31), "knn: bad shape (n %lld, B %d, ldx %lld, n k < 2^31)",
               (long long)n, B, (long long)ldx);
  MINK_REQUIRE(batch_offsets && (n == 0 || (x && idx)), "knn: NULL pointer");
  if (n == 0) return MINK_OK;
  const int Cpad = (int)align_up(C, KK);
  knn_kernel<<<dim3((unsigned)(cdiv(n, KQ) + B)), 256, (size_t)Cpad * KLQ * sizeof(float), (hipStream_t)stream>>>(x, ldx, C, batch_offsets,
                                                                                                                 B, k, idx);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_knn_cross(const float *q, int64_t nq, int64_t ldq, const float *c, int64_t nc, int64_t ldc, int32_t C,
                   const int32_t *q_offsets, const int32_t *c_offsets, int32_t B, int32_t k, int32_t *idx, float *dist, void *stream) {
  MINK_REQUIRE(k >= 1 && k <= MINK_KNN_MAX_K, "knn_cross: k = %d outside 1..%d", k, MINK_KNN_MAX_K);
  MINK_REQUIRE(C >= 1 && C <= MINK_KNN_MAX_C, "knn_cross: C = %d outside 1..%d", C, MINK_KNN_MAX_C);
  MINK_REQUIRE(nq >= 0 && nc >= 0 && nc < ((int64_t)1 << 31) && B >= 1 && ldq >= C && ldc >= C && nq * (int64_t)k < ((int64_t)1 << 31),
               "knn_cross: bad shape (nq %lld, nc %lld, B %d, ldq %lld, ldc %lld, nq k < 2^31)", (long long)nq, (long long)nc, B,
               (long long)ldq, (long long)ldc);
  MINK_REQUIRE(q_offsets && c_offsets && (nq == 0 || (q && idx)) && (nc == 0 || c), "knn_cross: NULL pointer");
  if (nq == 0) return MINK_OK;
  const int Cpad = (int)align_up(C, KK);
  knn_cross_kernel<<<dim3((unsigned)(cdiv(nq, KQ) + B)), 256, (size_t)Cpad * KLQ * sizeof(float), (hipStream_t)stream>>>(
      q, ldq, nq, c, ldc, nc, C, q_offsets, c_offsets, B, k, idx, dist);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int32_t mink_edge_stats_rows(int64_t n) { return edge_rows(n > 0 ? n : 0); }

int mink_edge_stats(const float *P, const float *Q, const int32_t *idx, int64_t n, int32_t k, int32_t C, double *partial,
                    int64_t partial_bytes, void *stream) {
  if (int rc = edge_args("edge_stats", n, k, C)) return rc;
  MINK_REQUIRE(n >= 1 && P && Q && idx && partial, "edge_stats: NULL pointer or no rows");
  const int rows = edge_rows(n);
  MINK_REQUIRE(partial_bytes >= (int64_t)rows * 2 * C * 8, "edge_stats: workspace of %lld bytes, %lld needed", (long long)partial_bytes,
               (long long)rows * 2 * C * 8);
  edge_stats_kernel<<<dim3(rows, (unsigned)cdiv(C, EC)), 256, 0, (hipStream_t)stream>>>(P, Q, idx, n, k, C, cdiv(n, rows), partial);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_edge_fwd(const float *P, const float *Q, const int32_t *idx, int64_t n, int32_t k, int32_t C, const float *mean,
                  const float *invstd, const float *gamma, const float *beta, float *y, uint8_t *arg, void *stream) {
  if (int rc = edge_args("edge_fwd", n, k, C)) return rc;
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(P && Q && idx && mean && invstd && gamma && beta && y && arg, "edge_fwd: NULL pointer");
  edge_fwd_kernel<<<dim3((unsigned)cdiv(n, ER), (unsigned)cdiv(C, EC)), 256, 0, (hipStream_t)stream>>>(P, Q, idx, n, k, C, mean, invstd,
                                                                                                       gamma, beta, y, arg);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int64_t mink_edge_bwd_workspace_bytes(int64_t n, int32_t C) {
  if (n < 0 || C < 1) return 0;
  return align_up(n * C * 4, 256) + align_up((int64_t)edge_rows(n) * 2 * C * 8, 256);
}

int mink_edge_bwd(const float *dy, const float *P, const float *Q, const int32_t *idx, const uint8_t *arg, int64_t n, int32_t k,
                  int32_t C, const float *mean, const float *invstd, const float *gamma, const float *beta, int32_t training,
                  const int32_t *members, const int32_t *seg, float *dP, float *dQ, float *dgamma, float *dbeta, void *workspace,
                  int64_t workspace_bytes, void *stream) {
  if (int rc = edge_args("edge_bwd", n, k, C)) return rc;
  MINK_REQUIRE(n >= 1 && dy && P && Q && idx && arg && mean && invstd && gamma && beta && members && seg && dP && dQ && dgamma &&
                   dbeta && workspace,
               "edge_bwd: NULL pointer or no rows");
  MINK_REQUIRE(workspace_bytes >= mink_edge_bwd_workspace_bytes(n, C) && ((uintptr_t)workspace & 7) == 0,
               "edge_bwd: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)workspace_bytes,
               (long long)mink_edge_bwd_workspace_bytes(n, C));
  hipStream_t st = (hipStream_t)stream;
  float *gbuf = (float *)workspace;
  double *partial = (double *)((char *)workspace + align_up(n * C * 4, 256));
  const int rows = edge_rows(n);
  const unsigned cy = (unsigned)cdiv(C, EC);
  edge_bwd_g_kernel<<<dim3(rows, cy), 256, 0, st>>>(dy, P, Q, idx, arg, n, k, C, cdiv(n, rows), mean, invstd, gamma, beta, gbuf, partial);
  MINK_CHECK_LAUNCH();
  edge_bwd_finalize_kernel<<<dim3((unsigned)cdiv(C, 64)), 64, 0, st>>>(partial, rows, C, dgamma, dbeta);
  MINK_CHECK_LAUNCH();
  const float inv_m = (float)(1.0 / ((double)n * (double)k));
  edge_bwd_pq_kernel<<<dim3((unsigned)cdiv(n, ER), cy), 256, 0, st>>>(gbuf, P, Q, idx, arg, n, k, C, mean, invstd, gamma, dgamma, dbeta,
                                                                      training != 0, inv_m, members, seg, dP, dQ);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
