// PAConv (reference co3d_3d/src/models/paconv: feat_trans_* + assign_score_withk*) on the rows of a field, rearranged so
// that the neighbour sum runs in INPUT space and the weight bank meets it in one dense GEMM:
//
//   A[i][m][:] = sum_j s[i][j][m] x[idx[i][j]][:]      S[i][m] = sum_j s[i][j][m]      CX[i][m][:] = S[i][m] x[i][:]
//   y[i] = sum_m (A[i][m] Wn_m - CX[i][m] Wc_m)                                         (the GEMM, outside this file)
//
// No [n][M][O] and no [n][k][.][O] tensor exists, forward or backward; every sum has a fixed order and nothing is atomic.
//
//   mink_paconv_gather      : a group of G lanes (G = 4 .. 64, the power of two covering the row's column groups) owns a row
//                             and a chunk of G * VEC channels; a lane holds M accumulators per channel, walks the k slots in
//                             ascending order (an fp32 fma chain) and reads the slot's M scores, the same for the whole group
//   mink_paconv_score_bwd   : one lane per edge (i, j): M dot products over the channels, ascending, no cross-lane sum
//   mink_paconv_scatter_bwd : the gather's layout over the incoming-edge lists (edges ascending, then the centre term)
#include "rowpass.h"

namespace mink {
namespace {

constexpr int PT = 256;  // threads of a workgroup

// the M scores of one slot into registers: 16-byte loads when the host found M % 4 == 0 and s aligned
template <int MB>
__device__ __forceinline__ void load_scores(const float *__restrict__ p, int M, bool vec, float (&sc)[MB]) {
  if constexpr (MB >= 4) {
    if (vec) {
#pragma unroll
      for (int m = 0; m < MB; m += 4)
        if (m < M) {
          const float4 t = *reinterpret_cast<const float4 *>(p + m);
          sc[m] = t.x, sc[m + 1] = t.y, sc[m + 2] = t.z, sc[m + 3] = t.w;
        }
      return;
    }
  }
#pragma unroll
  for (int m = 0; m < MB; ++m)
    if (m < M) sc[m] = p[m];
}

// this lane's row and first channel: groups of G lanes, PT / G rows per workgroup, blockIdx.y walks chunks of G * VEC channels
template <int VEC>
__device__ __forceinline__ bool group_lane(int G, int64_t n, int C, int64_t &row, int &c0) {
  const int gl = threadIdx.x & (G - 1);
  row = (int64_t)blockIdx.x * (PT / G) + threadIdx.x / G;
  c0 = (blockIdx.y * G + gl) * VEC;
  return row < n && c0 < C;
}

template <int VEC, int MB>
__global__ __launch_bounds__(PT) void paconv_gather_kernel(const float *__restrict__ x, const float *__restrict__ s,
                                                           const int *__restrict__ idx, int64_t n, int k, int M, int C, int G,
                                                           bool vec_s, float *__restrict__ A, float *__restrict__ CX, int64_t ldz,
                                                           float *__restrict__ S) {
  int64_t i;
  int c0;
  if (!group_lane<VEC>(G, n, C, i, c0)) return;
  float acc[MB][VEC], sum[MB], sc[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    sum[m] = 0.f, sc[m] = 0.f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[m][v] = 0.f;
  }
  for (int j = 0; j < k; ++j) {
    const int64_t e = i * k + j, r = idx[e];
    if (r < 0 || r >= n) continue;  // contributes nothing, never followed
    float xv[VEC];
    ldv<VEC>(x + r * C + c0, xv);
    load_scores<MB>(s + e * M, M, vec_s, sc);
#pragma unroll
    for (int m = 0; m < MB; ++m)
      if (m < M) {
        sum[m] += sc[m];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[m][v] = fmaf(sc[m], xv[v], acc[m][v]);
      }
  }
  float xi[VEC];
  ldv<VEC>(x + i * C + c0, xi);
#pragma unroll
  for (int m = 0; m < MB; ++m)
    if (m < M) {
      stv<VEC>(A + i * ldz + (int64_t)m * C + c0, acc[m]);
      if (CX) {
        float cv[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) cv[v] = sum[m] * xi[v];
        stv<VEC>(CX + i * ldz + (int64_t)m * C + c0, cv);
      }
      if (S && c0 == 0) S[i * M + m] = sum[m];
    }
}

template <int VEC, int MB>
__global__ __launch_bounds__(PT) void paconv_score_bwd_kernel(const float *__restrict__ dA, const float *__restrict__ dCX, int64_t ldz,
                                                              const float *__restrict__ x, const int *__restrict__ idx, int64_t n,
                                                              int k, int M, int C, float *__restrict__ ds) {
  const int64_t e = (int64_t)blockIdx.x * PT + threadIdx.x;
  if (e >= n * k) return;
  const int64_t i = e / k, r = idx[e];
  float acc[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) acc[m] = 0.f;
  if (r >= 0 && r < n) {
    const float *__restrict__ xj = x + r * C, *__restrict__ xi = x + i * C;
    const float *__restrict__ a = dA + i * ldz, *__restrict__ b = dCX + i * ldz;
    for (int c = 0; c < C; c += VEC) {
      float vj[VEC], vi[VEC];
      ldv<VEC>(xj + c, vj);
      ldv<VEC>(xi + c, vi);
#pragma unroll
      for (int m = 0; m < MB; ++m)
        if (m < M) {
          float va[VEC], vb[VEC];
          ldv<VEC>(a + (int64_t)m * C + c, va);
          ldv<VEC>(b + (int64_t)m * C + c, vb);
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[m] = fmaf(vb[v], vi[v], fmaf(va[v], vj[v], acc[m]));
        }
    }
  }
#pragma unroll
  for (int m = 0; m < MB; ++m)
    if (m < M) ds[e * M + m] = acc[m];  // (a slot that is not followed gets 0)
}

template <int VEC, int MB>
__global__ __launch_bounds__(PT) void paconv_scatter_bwd_kernel(const float *__restrict__ dA, const float *__restrict__ dCX, int64_t ldz,
                                                                const float *__restrict__ s, const float *__restrict__ S,
                                                                const int *__restrict__ members, const int *__restrict__ seg,
                                                                int64_t n, int k, int M, int C, int G, bool vec_s,
                                                                float *__restrict__ dx) {
  int64_t row;
  int c0;
  if (!group_lane<VEC>(G, n, C, row, c0)) return;
  const int64_t ne = n * k;
  int64_t e0 = seg[row], e1 = seg[row + 1];
  e0 = e0 < 0 ? 0 : (e0 > ne ? ne : e0);  // (never outside the lists, whatever seg holds)
  e1 = e1 < e0 ? e0 : (e1 > ne ? ne : e1);
  float acc[VEC], sc[MB];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
#pragma unroll
  for (int m = 0; m < MB; ++m) sc[m] = 0.f;
  for (int64_t t = e0; t < e1; ++t) {
    const int64_t e = members[t];
    if (e < 0 || e >= ne) continue;
    const int64_t i = e / k;
    load_scores<MB>(s + e * M, M, vec_s, sc);
    const float *__restrict__ a = dA + i * ldz + c0;
#pragma unroll
    for (int m = 0; m < MB; ++m)
      if (m < M) {
        float va[VEC];
        ldv<VEC>(a + (int64_t)m * C, va);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(sc[m], va[v], acc[v]);
      }
  }
  load_scores<MB>(S + row * M, M, vec_s, sc);
  const float *__restrict__ b = dCX + row * ldz + c0;
#pragma unroll
  for (int m = 0; m < MB; ++m)
    if (m < M) {
      float vb[VEC];
      ldv<VEC>(b + (int64_t)m * C, vb);
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = fmaf(sc[m], vb[v], acc[v]);
    }
  stv<VEC>(dx + row * C + c0, acc);
}

int paconv_args(const char *what, int64_t n, int32_t k, int32_t M, int32_t C, int64_t ldz) {
  MINK_REQUIRE(M >= 1 && M <= MINK_PACONV_MAX_M, "%s: M = %d outside 1..%d", what, M, MINK_PACONV_MAX_M);
  MINK_REQUIRE(k >= 1 && k <= MINK_KNN_MAX_K, "%s: k = %d outside 1..%d", what, k, MINK_KNN_MAX_K);
  MINK_REQUIRE(n >= 0 && C >= 1 && n * (int64_t)k < ((int64_t)1 << 31) && ldz >= (int64_t)M * C,
               "%s: bad shape (n %lld, Cin %d >= 1, ldz %lld >= M Cin, n k < 2^31)", what, (long long)n, C, (long long)ldz);
  return MINK_OK;
}

// the lanes of a group: the power of two in 4 .. 64 that covers the row's column groups
int group_lanes(int ncg) {
  int G = 4;
  while (G < ncg && G < 64) G *= 2;
  return G;
}

int bucket(int M) { return M <= 1 ? 1 : (M <= 4 ? 4 : (M <= 8 ? 8 : 16)); }

// launch f<VEC, MB> for the runtime (vec, M)
#define PACONV_DISPATCH(vec, M, CALL)          \
  do {                                         \
    const int mb_ = bucket(M);                 \
    if (vec) {                                 \
      if (mb_ == 1) { CALL(4, 1); }            \
      else if (mb_ == 4) { CALL(4, 4); }       \
      else if (mb_ == 8) { CALL(4, 8); }       \
      else { CALL(4, 16); }                    \
    } else {                                   \
      if (mb_ == 1) { CALL(1, 1); }            \
      else if (mb_ == 4) { CALL(1, 4); }       \
      else if (mb_ == 8) { CALL(1, 8); }       \
      else { CALL(1, 16); }                    \
    }                                          \
  } while (0)

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int mink_paconv_gather(const float *x, const float *s, const int32_t *idx, int64_t n, int32_t k, int32_t M, int32_t C, float *A,
                       float *CX, int64_t ldz, float *S, void *stream) {
  if (int rc = paconv_args("paconv_gather", n, k, M, C, ldz)) return rc;
  MINK_REQUIRE(n == 0 || (x && s && idx && A), "paconv_gather: NULL pointer");
  if (n == 0) return MINK_OK;
  const bool vec = C % 4 == 0 && ldz % 4 == 0 && aligned16(x) && aligned16(A) && aligned16(CX);
  const bool vec_s = M % 4 == 0 && aligned16(s);
  const int VECr = vec ? 4 : 1, ncg = C / VECr, G = group_lanes(ncg);
  const dim3 grid((unsigned)cdiv(n, PT / G), (unsigned)cdiv(ncg, G));
#define CALL(V, MB) paconv_gather_kernel<V, MB><<<grid, PT, 0, (hipStream_t)stream>>>(x, s, idx, n, k, M, C, G, vec_s, A, CX, ldz, S)
  PACONV_DISPATCH(vec, M, CALL);
#undef CALL
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_paconv_score_bwd(const float *dA, const float *dCX, int64_t ldz, const float *x, const int32_t *idx, int64_t n, int32_t k,
                          int32_t M, int32_t C, float *ds, void *stream) {
  if (int rc = paconv_args("paconv_score_bwd", n, k, M, C, ldz)) return rc;
  MINK_REQUIRE(n == 0 || (dA && dCX && x && idx && ds), "paconv_score_bwd: NULL pointer");
  if (n == 0) return MINK_OK;
  const bool vec = C % 4 == 0 && ldz % 4 == 0 && aligned16(x) && aligned16(dA) && aligned16(dCX);
  const unsigned grid = (unsigned)cdiv(n * k, PT);
#define CALL(V, MB) paconv_score_bwd_kernel<V, MB><<<grid, PT, 0, (hipStream_t)stream>>>(dA, dCX, ldz, x, idx, n, k, M, C, ds)
  PACONV_DISPATCH(vec, M, CALL);
#undef CALL
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_paconv_scatter_bwd(const float *dA, const float *dCX, int64_t ldz, const float *s, const float *S, const int32_t *members,
                            const int32_t *seg, int64_t n, int32_t k, int32_t M, int32_t C, float *dx, void *stream) {
  if (int rc = paconv_args("paconv_scatter_bwd", n, k, M, C, ldz)) return rc;
  MINK_REQUIRE(n == 0 || (dA && dCX && s && S && members && seg && dx), "paconv_scatter_bwd: NULL pointer");
  if (n == 0) return MINK_OK;
  const bool vec = C % 4 == 0 && ldz % 4 == 0 && aligned16(dA) && aligned16(dCX) && aligned16(dx);
  const bool vec_s = M % 4 == 0 && aligned16(s) && aligned16(S);
  const int VECr = vec ? 4 : 1, ncg = C / VECr, G = group_lanes(ncg);
  const dim3 grid((unsigned)cdiv(n, PT / G), (unsigned)cdiv(ncg, G));
#define CALL(V, MB) \
  paconv_scatter_bwd_kernel<V, MB><<<grid, PT, 0, (hipStream_t)stream>>>(dA, dCX, ldz, s, S, members, seg, n, k, M, C, G, vec_s, dx)
  PACONV_DISPATCH(vec, M, CALL);
#undef CALL
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
