// Segmentation tail: weighted / ignore-label softmax cross entropy over per-point logits with the prediction, the
// confusion matrix and the label counts out of the same pass (mink_seg_ce_forward / _backward), and the row gather of
// SparseTensor.slice() (mink_rows_gather; its backward, mink_segment_sum, sits beside mink_segment_mean in field.hip).
//
// Streaming kernels: every logit is read once per direction.  A row of C = 20 / 21 floats (80 / 84 bytes) is not what a
// lane loads well, so a workgroup loads a contiguous tile of rows cooperatively (16-byte loads when the matrix is dense
// and 16-byte aligned, dword loads otherwise), stages it in LDS with an odd row stride (C | 1 dwords: thread r reading
// column j of row r hits bank (r * stride + j) % 32, all different over a 32-lane group) and then one thread owns one row.
//
// Determinism: tile t always goes to workgroup t % grid, each workgroup sums its rows' (num, den) in double in a fixed
// order and writes ONE partial to the workspace, and a second one-workgroup launch adds the partials in index order.
// No floating-point atomics; the histogram and the label counts are integers (LDS atomics, then one global atomic per
// non-zero cell and workgroup), whose sums do not depend on the order.
#include <algorithm>

#include "common.h"

namespace mink {

constexpr int SB = 256;           // threads per workgroup
constexpr int SEG_MAX_C = 128;    // classes
constexpr int SEG_MAX_GRID = 2048;
constexpr int SEG_HIST_LDS_C = 64;  // up to here the workgroup keeps a private C x C histogram in LDS

struct SegPartial {  // one per workgroup (40 bytes)
  double num, den;
  long long n_valid, n_ignored, n_bad;
};

// rows of a tile: the staged tile (rows x (C | 1) floats) stays below 48 KiB
static inline int seg_tile_rows(int C) { return C <= 40 ? 256 : (C <= 80 ? 128 : 64); }
static inline int64_t seg_grid(int64_t n, int C) {
  return std::max<int64_t>(1, std::min<int64_t>(cdiv(n, seg_tile_rows(C)), SEG_MAX_GRID));
}

__device__ __forceinline__ long long load_label(const void *labels, int is64, int64_t i) {
  return is64 ? ((const long long *)labels)[i] : (long long)((const int *)labels)[i];
}

// Stage rows [row0, row0 + rows) of z into `tile` (row stride LS).  VEC: the rows are one contiguous, 16-byte aligned run.
template <bool VEC>
__device__ __forceinline__ void stage_tile(const float *__restrict__ z, int64_t ldz, int C, int64_t row0, int rows, int LS,
                                           float *__restrict__ tile) {
  const int total = rows * C;
  if (VEC) {
    const float *src = z + row0 * C;
    for (int e = threadIdx.x * 4; e < total; e += SB * 4) {
      int r = e / C, c = e - r * C;
      if (e + 3 < total) {
        const float4 v = *reinterpret_cast<const float4 *>(src + e);
        const float q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          tile[r * LS + c] = q[k];
          if (++c == C) c = 0, ++r;
        }
      } else {
        for (int k = e; k < total; ++k) {
          tile[r * LS + c] = src[k];
          if (++c == C) c = 0, ++r;
        }
      }
    }
  } else {
    for (int e = threadIdx.x; e < total; e += SB) {
      const int r = e / C, c = e - r * C;
      tile[r * LS + c] = z[(row0 + r) * ldz + c];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(SB) void seg_ce_fwd_kernel(const float *__restrict__ z, int64_t ldz, const void *__restrict__ labels,
                                                        int is64, const float *__restrict__ w, long long ignore_label, int64_t n,
                                                        int C, int TR, float *__restrict__ lse_out, int *__restrict__ pred_out,
                                                        unsigned long long *__restrict__ hist, SegPartial *__restrict__ partial) {
  extern __shared__ __align__(16) float smem[];
  const int LS = C | 1;
  float *tile = smem;
  unsigned *lhist = reinterpret_cast<unsigned *>(smem + TR * LS);
  const bool lds_hist = hist != nullptr && C <= SEG_HIST_LDS_C;
  __shared__ double red[2][SB / 64];
  __shared__ unsigned cnt[3];
  if (lds_hist)
    for (int i = threadIdx.x; i < C * C; i += SB) lhist[i] = 0u;
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0u;

  double num = 0.0, den = 0.0;          // this thread's rows, in tile order
  unsigned nv = 0u, ni = 0u, nb = 0u;
  const int64_t ntiles = (n + TR - 1) / TR;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * TR;
    const int rows = (int)(n - row0 < TR ? n - row0 : TR);
    __syncthreads();  // the previous tile has been consumed (and the LDS histogram zeroed)
    stage_tile<VEC>(z, ldz, C, row0, rows, LS, tile);
    __syncthreads();
    if ((int)threadIdx.x < rows) {
      const float *row = tile + threadIdx.x * LS;
      float mx = row[0];
      int arg = 0;
      for (int j = 1; j < C; ++j) {
        const float v = row[j];
        if (v > mx) mx = v, arg = j;  // strict: the lowest index wins a tie
      }
      float se = 0.f;
      for (int j = 0; j < C; ++j) se += expf(row[j] - mx);
      const float lse = mx + logf(se);
      const int64_t i = row0 + threadIdx.x;
      lse_out[i] = lse;
      if (pred_out) pred_out[i] = arg;
      const long long y = load_label(labels, is64, i);
      if (y == ignore_label) {
        ++ni;
      } else if (y < 0 || y >= C) {
        ++nb;
      } else {
        ++nv;
        const float wy = w ? w[y] : 1.f;
        num += (double)wy * (double)(lse - row[y]);
        den += (double)wy;
        if (lds_hist) atomicAdd(&lhist[(int)y * C + arg], 1u);
        else if (hist) atomicAdd(&hist[(int64_t)y * C + arg], 1ull);
      }
    }
  }
  // workgroup sums: lanes of a wave by a fixed butterfly, then the four waves in order
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    num += __shfl_xor(num, o, 64);
    den += __shfl_xor(den, o, 64);
  }
  if (nv) atomicAdd(&cnt[0], nv);
  if (ni) atomicAdd(&cnt[1], ni);
  if (nb) atomicAdd(&cnt[2], nb);
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = num, red[1][threadIdx.x >> 6] = den;
  __syncthreads();
  if (threadIdx.x == 0) {
    SegPartial p;
    p.num = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    p.den = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    p.n_valid = cnt[0], p.n_ignored = cnt[1], p.n_bad = cnt[2];
    partial[blockIdx.x] = p;
  }
  if (lds_hist)
    for (int i = threadIdx.x; i < C * C; i += SB) {
      const unsigned v = lhist[i];
      if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

// stats = the partials summed in index order: thread t takes partials t, t + SB, ... in that order, then thread 0 adds the SB sums
__global__ __launch_bounds__(SB) void seg_ce_finish_kernel(const SegPartial *__restrict__ partial, int nparts, double *__restrict__ stats,
                                                           float *__restrict__ loss) {
  __shared__ double snum[SB], sden[SB];
  __shared__ long long scnt[3][SB];
  double num = 0.0, den = 0.0;
  long long c0 = 0, c1 = 0, c2 = 0;
  for (int i = threadIdx.x; i < nparts; i += SB) {
    const SegPartial p = partial[i];
    num += p.num, den += p.den, c0 += p.n_valid, c1 += p.n_ignored, c2 += p.n_bad;
  }
  snum[threadIdx.x] = num, sden[threadIdx.x] = den;
  scnt[0][threadIdx.x] = c0, scnt[1][threadIdx.x] = c1, scnt[2][threadIdx.x] = c2;
  __syncthreads();
  if (threadIdx.x == 0) {
    num = den = 0.0, c0 = c1 = c2 = 0;
    for (int i = 0; i < SB; ++i) num += snum[i], den += sden[i], c0 += scnt[0][i], c1 += scnt[1][i], c2 += scnt[2][i];
    stats[0] = num, stats[1] = den;
    long long *ic = reinterpret_cast<long long *>(stats);
    ic[2] = c0, ic[3] = c1, ic[4] = c2;
    *loss = (float)(num / den);  // 0 / 0 = NaN: nothing valid in the batch
  }
}

// dz = coef_i * (exp(z - lse_i) - [j == y_i]).  What a row needs (coef, lse, label) is staged in LDS once per tile; the logits
// themselves stream through registers in the same contiguous tile order they are written back in.
template <bool VEC>
__global__ __launch_bounds__(SB) void seg_ce_bwd_kernel(const float *__restrict__ z, int64_t ldz, const void *__restrict__ labels,
                                                        int is64, const float *__restrict__ w, long long ignore_label,
                                                        const float *__restrict__ lse, const double *__restrict__ stats,
                                                        const float *__restrict__ g, int64_t n, int C, float *__restrict__ dz) {
  __shared__ float s_coef[SB], s_lse[SB];
  __shared__ int s_y[SB];
  const double den = stats[1];
  const float scale = den != 0.0 ? (float)((double)*g / den) : 0.f;
  const int64_t ntiles = (n + SB - 1) / SB;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * SB;
    const int rows = (int)(n - row0 < SB ? n - row0 : SB);
    __syncthreads();
    if ((int)threadIdx.x < rows) {
      const int64_t i = row0 + threadIdx.x;
      const long long y = load_label(labels, is64, i);
      const bool valid = y != ignore_label && y >= 0 && y < C;
      s_y[threadIdx.x] = valid ? (int)y : -1;
      s_coef[threadIdx.x] = valid ? scale * (w ? w[y] : 1.f) : 0.f;
      s_lse[threadIdx.x] = lse[i];
    }
    __syncthreads();
    const int total = rows * C;
    if (VEC) {
      const float *src = z + row0 * C;
      float *dst = dz + row0 * C;
      for (int e = threadIdx.x * 4; e < total; e += SB * 4) {
        int r = e / C, c = e - r * C;
        if (e + 3 < total) {
          const float4 v = *reinterpret_cast<const float4 *>(src + e);
          const float q[4] = {v.x, v.y, v.z, v.w};
          float o[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float coef = s_coef[r];
            o[k] = coef != 0.f ? coef * (expf(q[k] - s_lse[r]) - (c == s_y[r] ? 1.f : 0.f)) : 0.f;
            if (++c == C) c = 0, ++r;
          }
          *reinterpret_cast<float4 *>(dst + e) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
          for (int k = e; k < total; ++k) {
            const float coef = s_coef[r];
            dst[k] = coef != 0.f ? coef * (expf(src[k] - s_lse[r]) - (c == s_y[r] ? 1.f : 0.f)) : 0.f;
            if (++c == C) c = 0, ++r;
          }
        }
      }
    } else {
      for (int e = threadIdx.x; e < total; e += SB) {
        const int r = e / C, c = e - r * C;
        const float coef = s_coef[r];
        dz[(row0 + r) * C + c] = coef != 0.f ? coef * (expf(z[(row0 + r) * ldz + c] - s_lse[r]) - (c == s_y[r] ? 1.f : 0.f)) : 0.f;
      }
    }
  }
}

// y[i][:] = x[idx[i]][:] (an index outside [0, n_src) yields a zero row, never a read out of bounds)
__global__ __launch_bounds__(SB) void rows_gather_kernel(const float *__restrict__ x, int64_t ldx, int64_t n_src, int C,
                                                         const int *__restrict__ idx, int64_t n, float *__restrict__ y) {
  const int64_t total = n * C;
  for (int64_t e = (int64_t)blockIdx.x * SB + threadIdx.x; e < total; e += (int64_t)gridDim.x * SB) {
    const int64_t i = e / C;
    const int c = (int)(e - i * C);
    const int64_t s = idx[i];
    y[e] = (s >= 0 && s < n_src) ? x[s * ldx + c] : 0.f;
  }
}

}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_seg_ce_workspace_bytes(int64_t n, int32_t C) {
  if (n < 0 || C < 2 || C > SEG_MAX_C) return -1;
  return (int64_t)sizeof(SegPartial) * seg_grid(n, C);
}

int mink_seg_ce_forward(const float *z, int64_t ldz, const void *labels, int32_t labels_int64, const float *w, int64_t ignore_label,
                        int64_t n, int32_t C, float *lse, int32_t *pred, int64_t *hist, void *stats, float *loss, void *workspace,
                        int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(n >= 0 && C >= 2 && C <= SEG_MAX_C && ldz >= C, "seg_ce_forward: bad shape (n=%lld, C=%d, ldz=%lld; 2 <= C <= %d)",
               (long long)n, C, (long long)ldz, SEG_MAX_C);
  MINK_REQUIRE(stats && loss && workspace, "seg_ce_forward: NULL pointer (stats, loss, workspace)");
  MINK_REQUIRE(n == 0 || (z && labels && lse), "seg_ce_forward: NULL pointer (logits, labels, lse)");
  MINK_REQUIRE((((uintptr_t)z | (uintptr_t)lse | (uintptr_t)pred | (uintptr_t)w | (uintptr_t)loss) & 3) == 0 &&
                   (((uintptr_t)stats | (uintptr_t)hist | (uintptr_t)workspace) & 7) == 0 &&
                   ((uintptr_t)labels & (labels_int64 ? 7 : 3)) == 0,
               "seg_ce_forward: misaligned pointer");
  const int64_t need = mink_seg_ce_workspace_bytes(n, C);
  MINK_REQUIRE(workspace_bytes >= need, "seg_ce_forward: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  if (hist) MINK_HIP(hipMemsetAsync(hist, 0, sizeof(int64_t) * (size_t)C * C, s));
  int nparts = 0;
  if (n > 0) {
    const int TR = seg_tile_rows(C);
    nparts = (int)seg_grid(n, C);
    const size_t shm = sizeof(float) * (size_t)TR * (C | 1) + (hist && C <= SEG_HIST_LDS_C ? sizeof(unsigned) * (size_t)C * C : 0);
    const bool vec = ldz == C && ((uintptr_t)z & 15) == 0;
    auto kern = vec ? seg_ce_fwd_kernel<true> : seg_ce_fwd_kernel<false>;
    kern<<<dim3((unsigned)nparts), SB, shm, s>>>(z, ldz, labels, labels_int64, w, (long long)ignore_label, n, C, TR, lse, pred,
                                                  (unsigned long long *)hist, (SegPartial *)workspace);
    MINK_CHECK_LAUNCH();
  }
  seg_ce_finish_kernel<<<dim3(1), SB, 0, s>>>((const SegPartial *)workspace, nparts, (double *)stats, loss);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_seg_ce_backward(const float *z, int64_t ldz, const void *labels, int32_t labels_int64, const float *w, int64_t ignore_label,
                         const float *lse, const void *stats, const float *grad_loss, int64_t n, int32_t C, float *dz, void *stream) {
  MINK_REQUIRE(n >= 0 && C >= 2 && C <= SEG_MAX_C && ldz >= C, "seg_ce_backward: bad shape (n=%lld, C=%d, ldz=%lld; 2 <= C <= %d)",
               (long long)n, C, (long long)ldz, SEG_MAX_C);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(z && labels && lse && stats && grad_loss && dz, "seg_ce_backward: NULL pointer");
  MINK_REQUIRE((((uintptr_t)z | (uintptr_t)lse | (uintptr_t)dz | (uintptr_t)w | (uintptr_t)grad_loss) & 3) == 0 &&
                   ((uintptr_t)stats & 7) == 0 && ((uintptr_t)labels & (labels_int64 ? 7 : 3)) == 0,
               "seg_ce_backward: misaligned pointer");
  const bool vec = ldz == C && (((uintptr_t)z | (uintptr_t)dz) & 15) == 0;
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n, SB), SEG_MAX_GRID);
  auto kern = vec ? seg_ce_bwd_kernel<true> : seg_ce_bwd_kernel<false>;
  kern<<<dim3(grid), SB, 0, (hipStream_t)stream>>>(z, ldz, labels, labels_int64, w, (long long)ignore_label, lse, (const double *)stats,
                                                   grad_loss, n, C, dz);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_rows_gather(const float *x, int64_t ldx, int64_t n_src, int32_t C, const int32_t *idx, int64_t n, float *y, void *stream) {
  MINK_REQUIRE(n >= 0 && n_src >= 0 && C >= 1 && ldx >= C, "rows_gather: bad shape");
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(x && idx && y, "rows_gather: NULL pointer");
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n * C, SB), 8192);
  rows_gather_kernel<<<dim3(grid), SB, 0, (hipStream_t)stream>>>(x, ldx, n_src, C, idx, n, y);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
