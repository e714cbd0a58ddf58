// Grouped convolution over a neighbour table on gfx950 (the 3x3 layers of the ResNeXt networks of the 2-D comparison), fp32 in,
// fp32 accumulate, fp32 out in every mink_conv_set_math mode.  Rows are [n][ld] fp32; group g owns the input columns
// g cg_in .. (g + 1) cg_in and the output columns g cg_out ..; the table is nbr[n_out][K] with -1 for "outside", as for
// mink_conv_gather_gemm; the weights are packed w[K][G][cg_in][cg_out].
//
//   forward / data gradient  y[r][g cg_out + o] = sum_k sum_c x[nbr[r][k]][g cg_in + c] w[k][g][c][o]
//   weight gradient          dw[k][g][c][o]     = sum_r x[nbr[r][k]][g cg_in + c] dy[r][g cg_out + o]
//
// The choice per group width, and why:
//   cg_in == cg_out in {16, 32, 64}: the fp32 matrix core v_mfma_f32_16x16x4_f32, one instruction per 4 input channels of a
//     16 x 16 tile.  Lane l = (c, q) = (l & 15, l >> 4) supplies A[i = c][k = q] and B[k = q][j = c] and receives
//     D[i = 4 q + r][j = c] in register r (the map attn.hip uses).
//       forward: i = output channel, j = row, so a lane ends with 4 contiguous channels of one row (one 16-byte store).  A sum
//         over k may visit k in any order when A and B agree: lane group q takes the input channels 16 s + 4 q .. + 3 of chunk s,
//         so its B operands of the four steps are ONE 16-byte gather of the neighbour's row, straight from memory (every x
//         element is used by exactly one lane of the tile: nothing to share through LDS), and its A operands are one 16-byte
//         LDS read of the weights, staged once per workgroup in that order ([k][s][lane][step]: conflict-free).  A workgroup owns
//         one group, 16 of its output channels and a run of rows; its four waves take 16 rows each.  K cg 64 bytes of LDS:
//         110,592 for K = 27 at width 64, asked for and refused cleanly where the device says no.
//       weight gradient: i = input channel, j = output channel, k = row.  A wave owns one 16 x 16 tile of one group for ALL K
//         offsets (K accumulators: dy is loaded once per row and used K times) over one row block, and writes its partial
//         tile; no LDS, no hand-off.
//     The 32x32x2 form was not built: a 16 x 16 tile already fills the instruction at width 16, 32 and 64 are whole multiples
//     of it, and the smaller tile keeps the K accumulators of the weight gradient in registers (K x 4 instead of K x 16).
//   cg_in == cg_out in {4, 8}: vector FMA with the weights of a 64-column slab in LDS as [k][c][column], so that the 16 threads
//     of a row read 64 contiguous floats (conflict-free) and the rows of a wave read the same address (broadcast).  A thread
//     owns 4 output columns of a row: 16-byte gathers of its group's input channels, 16-byte LDS reads of the weights, 4 FMAs per
//     read, one 16-byte store.  The multi-block MFMA forms (4x4x1, 16 blocks = 16 groups) leave 3/4 of every 4-wide result
//     tile's k-steps to a single channel and need a lane shuffle to store rows; they were not built.  The weight gradient of
//     these widths (K <= 9) gives a thread one 4 x 4 sub-block of a group for all K offsets: 16 K accumulators, per row one
//     16-byte load of dy and one 16-byte gather of x per offset for 16 FMAs each (the generic kernel, one element per thread and
//     one load per FMA, lost to the block-diagonal dense form at these widths: 0.38x .. 0.87x; this one is 2.2x .. 2.8x faster
//     than it once a row's table entries and gathers are all issued before the first FMA); row lanes are added through LDS.
//   anything else (depthwise, unequal widths, any G): a thread per output element, plain FMA.
// profiles/gconv_kernels.txt holds the measurements beside the block-diagonal dense form and torch.
//
// No atomics: every output element has one owner that sums in a fixed order; the weight gradient is split over row blocks
// [n_out rb / RB, n_out (rb + 1) / RB) whose partials are added in ascending rb.  Two runs give the same bits.  A table entry of
// -1 (or one outside [0, n_in)) is skipped by the FMA kernels; the matrix-core kernels feed it as a zero ROW (x and, in the
// weight gradient, dy too), which contributes nothing for finite operands on the other side and keeps a NaN of dy out of the
// offsets that row does not reach.  16-byte global accesses when x and y are 16-byte aligned and both pitches are multiples
// of 4, dwords otherwise; only logical columns of logical rows are touched.
#include "rowpass.h"

namespace mink {
namespace {

constexpr int GT = 256;                     // threads per workgroup
constexpr int GKM = MINK_GCONV_MAX_K;       // 27
constexpr int GSLAB = 64;                   // output columns of a slab of the FMA kernel

using f32x4 = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

struct GcArgs {
  const float *x;
  int64_t n_in;
  int ldx;
  const float *w;
  int wt, flip;
  const int32_t *nbr;
  int64_t n_out;
  int K, G, ci, co;
  float *y;
  int ldy;
};

// element (k, g, c, o) of the weights the launch reads: packed [K][G][ci][co], or [K][G][co][ci] when wt; offset K-1-k when flip
__device__ __forceinline__ int64_t w_index(const GcArgs &a, int k, int g, int c, int o) {
  const int kk = a.flip ? a.K - 1 - k : k;
  const int64_t base = ((int64_t)kk * a.G + g) * a.ci * a.co;
  return base + (a.wt ? (int64_t)o * a.ci + c : (int64_t)c * a.co + o);
}

__device__ __forceinline__ bool in_rows(int idx, int64_t n) { return idx >= 0 && (int64_t)idx < n; }

// ---- generic forward: a thread per output element
__global__ __launch_bounds__(GT) void gconv_fwd_generic_kernel(const GcArgs a) {
  const int64_t C = (int64_t)a.G * a.co, total = a.n_out * C;
  for (int64_t e = (int64_t)blockIdx.x * GT + threadIdx.x; e < total; e += (int64_t)gridDim.x * GT) {
    const int64_t r = e / C;
    const int col = (int)(e - r * C), g = col / a.co, o = col - g * a.co;
    float acc = 0.f;
    for (int k = 0; k < a.K; ++k) {
      const int idx = a.nbr[r * a.K + k];
      if (!in_rows(idx, a.n_in)) continue;
      const float *xr = a.x + (int64_t)idx * a.ldx + g * a.ci;
      for (int c = 0; c < a.ci; ++c) acc = fmaf(xr[c], a.w[w_index(a, k, g, c, o)], acc);
    }
    a.y[r * a.ldy + col] = acc;
  }
}

// ---- widths 4 and 8: vector FMA, the slab's weights in LDS as [k][c][64 columns]
template <int CI, bool VEC>
__global__ __launch_bounds__(GT) void gconv_fwd_fma_kernel(const GcArgs a, int rows_per_block, int slabs) {
  extern __shared__ __attribute__((aligned(16))) float Ws[];
  const int slab0 = (int)(blockIdx.x % slabs) * GSLAB, C = a.G * a.co;
  for (int e = threadIdx.x; e < a.K * CI * GSLAB; e += GT) {
    const int col = e % GSLAB, c = (e / GSLAB) % CI, k = e / (GSLAB * CI), oc = slab0 + col;
    float v = 0.f;
    if (oc < C) {
      const int g = oc / a.co;
      v = a.w[w_index(a, k, g, c, oc - g * a.co)];
    }
    Ws[e] = v;
  }
  __syncthreads();
  const int tl = threadIdx.x & 15, rl = threadIdx.x >> 4;  // 16 threads per row, 16 rows per pass
  const int col4 = slab0 + 4 * tl;
  if (col4 >= C) return;  // (no barrier below)
  const int g = col4 / a.co;
  const int64_t r_begin = (int64_t)(blockIdx.x / slabs) * rows_per_block;
  const int64_t r_end = r_begin + rows_per_block < a.n_out ? r_begin + rows_per_block : a.n_out;
  for (int64_t r = r_begin + rl; r < r_end; r += GT / 16) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < a.K; ++k) {
      const int idx = a.nbr[r * a.K + k];
      if (!in_rows(idx, a.n_in)) continue;
      const float *xr = a.x + (int64_t)idx * a.ldx + g * CI;
      float xv[CI];
#pragma unroll
      for (int c = 0; c < CI; c += 4) {
        float t[4];
        if constexpr (VEC) {
          ldv<4>(xr + c, t);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) t[j] = xr[c + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[c + j] = t[j];
      }
      const float *wk = Ws + k * CI * GSLAB + 4 * tl;
#pragma unroll
      for (int c = 0; c < CI; ++c) {
        const float4 wv = *reinterpret_cast<const float4 *>(wk + c * GSLAB);
        acc[0] = fmaf(xv[c], wv.x, acc[0]);
        acc[1] = fmaf(xv[c], wv.y, acc[1]);
        acc[2] = fmaf(xv[c], wv.z, acc[2]);
        acc[3] = fmaf(xv[c], wv.w, acc[3]);
      }
    }
    float *yr = a.y + r * a.ldy + col4;
    if constexpr (VEC) {
      stv<4>(yr, acc);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) yr[j] = acc[j];
    }
  }
}

// ---- widths 16, 32, 64: fp32 MFMA; workgroup = (row block, group, 16 output channels), wave = 16 rows
template <int CG, bool VEC>
__global__ __launch_bounds__(GT) void gconv_fwd_mfma_kernel(const GcArgs a, int rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) float Ws[];  // [k][s][lane][step]
  constexpr int S = CG / 16;
  const int g = blockIdx.x / S, os = blockIdx.x % S;
  for (int e = threadIdx.x; e < a.K * S * 256; e += GT) {
    const int t = e & 3, c = (e >> 2) & 15, q = (e >> 6) & 3, s = (e >> 8) % S, k = e / (256 * S);
    Ws[e] = a.w[w_index(a, k, g, 16 * s + 4 * q + t, 16 * os + c)];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int64_t r_begin = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r_end = r_begin + rows_per_block < a.n_out ? r_begin + rows_per_block : a.n_out;
  for (int64_t r0 = r_begin + 16 * wave; r0 < r_end; r0 += 16 * (GT / 64)) {  // (the bound is the same for a whole wave)
    const int64_t row = r0 + c;
    const bool ok = row < r_end;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < a.K; ++k) {
      const int idx = ok ? a.nbr[row * a.K + k] : -1;
      const bool valid = in_rows(idx, a.n_in);
      if (__ballot(valid) == 0ull) continue;  // none of the 16 rows reaches this offset: the whole wave skips it
      const float *xr = a.x + (int64_t)(valid ? idx : 0) * a.ldx + g * CG + 4 * q;
      const float *wk = Ws + ((int64_t)k * S * 64 + lane) * 4;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        float b[4] = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
          if constexpr (VEC) {
            ldv<4>(xr + 16 * s, b);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = xr[16 * s + j];
          }
        }
        const float4 av = *reinterpret_cast<const float4 *>(wk + s * 256);
        acc = mfma4(av.x, b[0], acc);
        acc = mfma4(av.y, b[1], acc);
        acc = mfma4(av.z, b[2], acc);
        acc = mfma4(av.w, b[3], acc);
      }
    }
    if (ok) {
      float *yr = a.y + row * a.ldy + g * CG + 16 * os + 4 * q;
      if constexpr (VEC) {
        const float v[4] = {acc[0], acc[1], acc[2], acc[3]};
        stv<4>(yr, v);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) yr[j] = acc[j];
      }
    }
  }
}

// ---- weight gradient
struct GwArgs {
  const float *x;
  int64_t n_in;
  int ldx;
  const float *dy;
  int ldy;
  const int32_t *nbr;
  int64_t n_out;
  int K, G, ci, co, RB;
  float *ws;  // [RB][K][G][ci][co]
};

// generic (and widths 4 and 8): a thread owns (g, c, o) for all K offsets over one row block
template <int KM>
__global__ __launch_bounds__(GT) void gconv_wgrad_generic_kernel(const GwArgs a) {
  const int64_t E = (int64_t)a.G * a.ci * a.co;
  const int64_t e = (int64_t)blockIdx.x * GT + threadIdx.x;
  if (e >= E) return;
  const int rb = blockIdx.y;
  const int g = (int)(e / (a.ci * a.co)), rem = (int)(e - (int64_t)g * a.ci * a.co), c = rem / a.co, o = rem - c * a.co;
  const int64_t r0 = a.n_out * rb / a.RB, r1 = a.n_out * (rb + 1) / a.RB;
  float acc[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) acc[k] = 0.f;
  const float *xc = a.x + g * a.ci + c, *dc = a.dy + g * a.co + o;
  for (int64_t r = r0; r < r1; ++r) {
    const float d = dc[r * a.ldy];
    const int32_t *nr = a.nbr + r * a.K;
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < a.K) {
        const int idx = nr[k];
        if (in_rows(idx, a.n_in)) acc[k] = fmaf(xc[(int64_t)idx * a.ldx], d, acc[k]);
      }
  }
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if (k < a.K) a.ws[((int64_t)rb * a.K + k) * E + e] = acc[k];
}

// widths 16, 32, 64: a wave owns the 16 x 16 tile (input channels 16 ta.., output channels 16 tb..) of group g, all offsets, one row block
template <int CG, int KM>
__global__ __launch_bounds__(GT) void gconv_wgrad_mfma_kernel(const GwArgs a) {
  constexpr int S = CG / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  const int rb = blockIdx.y * (GT / 64) + wave;
  if (rb >= a.RB) return;  // (a whole wave; no barrier in this kernel)
  const int g = blockIdx.x / (S * S), ta = (blockIdx.x / S) % S, tb = blockIdx.x % S;
  const int64_t r0 = a.n_out * rb / a.RB, r1 = a.n_out * (rb + 1) / a.RB;
  f32x4 acc[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float *xc = a.x + g * CG + 16 * ta + c, *dc = a.dy + g * CG + 16 * tb + c;
  for (int64_t base = r0; base < r1; base += 16) {  // step t of the product sums the rows base + 4 q + t
    float d[4];
    bool okr[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t row = base + 4 * q + t;
      okr[t] = row < r1;
      d[t] = okr[t] ? dc[row * a.ldy] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < a.K) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int idx = okr[t] ? a.nbr[(base + 4 * q + t) * a.K + k] : -1;
          const bool valid = in_rows(idx, a.n_in);
          const float xv = valid ? xc[(int64_t)idx * a.ldx] : 0.f;
          acc[k] = mfma4(xv, valid ? d[t] : 0.f, acc[k]);
        }
      }
  }
  const int64_t E = (int64_t)a.G * CG * CG;
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if (k < a.K) {
      float *p = a.ws + ((int64_t)rb * a.K + k) * E + ((int64_t)g * CG + 16 * ta + 4 * q) * CG + 16 * tb + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r * CG] = acc[k][r];
    }
}

// widths 4 and 8, K <= 9: a thread owns one 4 x 4 sub-block (input channels 4 c4.., output channels 4 o4..) of one group for
// all offsets -- 16 K accumulators; per row one 16-byte load of dy and, per offset that has a neighbour, one 16-byte gather of x
// for 16 FMAs.  The sub-blocks of a row sit side by side on the lanes (coalesced rows); a workgroup holds `row_lanes` row lanes
// that take the rows of its block in turn and are added through LDS in ascending lane order, offset by offset.
template <int CG, bool VEC>
__global__ __launch_bounds__(GT) void gconv_wgrad_sub4_kernel(const GwArgs a, int tasks_per_block, int row_lanes) {
  extern __shared__ __attribute__((aligned(16))) float red[];  // [row_lanes][tasks_per_block][16]
  constexpr int SB = CG / 4, KM = 9;
  const int tl = threadIdx.x % tasks_per_block, rl = threadIdx.x / tasks_per_block;
  const int tasks = a.G * SB * SB, ct = blockIdx.x * tasks_per_block + tl;
  const bool active = rl < row_lanes && ct < tasks;
  const int g = active ? ct / (SB * SB) : 0, c4 = (ct / SB) % SB, o4 = ct % SB;
  const int rb = blockIdx.y;
  const int64_t R0 = a.n_out * rb / a.RB, R1 = a.n_out * (rb + 1) / a.RB;
  float acc[KM][4][4];
#pragma unroll
  for (int k = 0; k < KM; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[k][i][j] = 0.f;
  if (active) {
    const float *xc = a.x + g * CG + 4 * c4, *dc = a.dy + g * CG + 4 * o4;
    for (int64_t r = R0 + rl; r < R1; r += row_lanes) {
      float d[4];
      if constexpr (VEC) {
        ldv<4>(dc + r * a.ldy, d);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = dc[r * a.ldy + j];
      }
      // every table entry of the row first, then every gather, then the FMAs: the loads of a row are in flight together
      // instead of one dependent pair (entry, gather) per offset
      const int32_t *nr = a.nbr + r * a.K;
      int idx[KM];
#pragma unroll
      for (int k = 0; k < KM; ++k) idx[k] = k < a.K ? nr[k] : -1;
      float xv[KM][4];
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        const bool valid = in_rows(idx[k], a.n_in);
        const float *xr = xc + (int64_t)(valid ? idx[k] : 0) * a.ldx;
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[k][i] = 0.f;
        if (valid) {
          if constexpr (VEC) {
            ldv<4>(xr, xv[k]);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[k][i] = xr[i];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (in_rows(idx[k], a.n_in)) {  // an entry of -1 is skipped, not multiplied by zero: a NaN of dy stays out of its offset
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[k][i][j] = fmaf(xv[k][i], d[j], acc[k][i][j]);
        }
    }
  }
  const int64_t E = (int64_t)a.G * CG * CG;
  const int here = min(tasks_per_block, tasks - (int)blockIdx.x * tasks_per_block);  // sub-blocks this workgroup holds
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    if (k >= a.K) continue;  // (the same for every thread: the barriers below are met by all or none)
    if (rl < row_lanes) {
      float *p = red + ((int64_t)rl * tasks_per_block + tl) * 16;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4 *>(p + 4 * i) = float4{acc[k][i][0], acc[k][i][1], acc[k][i][2], acc[k][i][3]};
    }
    __syncthreads();
    for (int i = threadIdx.x; i < here * 16; i += GT) {
      float sum = red[i];
      for (int l = 1; l < row_lanes; ++l) sum += red[(int64_t)l * tasks_per_block * 16 + i];
      const int t = blockIdx.x * tasks_per_block + i / 16, tg = t / (SB * SB), tc = (t / SB) % SB, to = t % SB;
      a.ws[((int64_t)rb * a.K + k) * E + ((int64_t)tg * CG + 4 * tc + ((i >> 2) & 3)) * CG + 4 * to + (i & 3)] = sum;
    }
    __syncthreads();
  }
}

// dw[i] = sum over the row blocks in ascending order
__global__ __launch_bounds__(GT) void gconv_wgrad_reduce_kernel(const float *__restrict__ ws, int RB, int64_t n, float *__restrict__ dw) {
  for (int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x; i < n; i += (int64_t)gridDim.x * GT) {
    float s = ws[i];
    for (int rb = 1; rb < RB; ++rb) s += ws[(int64_t)rb * n + i];
    dw[i] = s;
  }
}

bool mfma_width(int ci, int co) { return ci == co && (ci == 16 || ci == 32 || ci == 64); }
bool fma_width(int ci, int co) { return ci == co && (ci == 4 || ci == 8); }

// launch shape of the sub-block weight gradient: sub-blocks per workgroup, row lanes, workgroups along the sub-blocks
struct Sub4Shape {
  int tasks_per_block, row_lanes, gx;
  Sub4Shape(int G, int cg) {
    const int64_t tasks = (int64_t)G * (cg / 4) * (cg / 4);
    tasks_per_block = (int)std::min<int64_t>(tasks, GT), row_lanes = GT / tasks_per_block, gx = (int)cdiv(tasks, tasks_per_block);
  }
};
bool sub4_wgrad(int K, int ci, int co) { return fma_width(ci, co) && K <= 9; }

// row blocks of the weight gradient: about 4096 waves (matrix core) or workgroups (FMA), none below 128 / 256 rows; the
// sub-block kernel: about 1024 workgroups, no row lane below 32 rows
int wgrad_blocks(int64_t n_out, int K, int G, int ci, int co) {
  if (sub4_wgrad(K, ci, co)) {
    const Sub4Shape s(G, ci);
    return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(n_out, 32 * s.row_lanes), std::max(1, 1024 / s.gx)));
  }
  const bool mf = mfma_width(ci, co);
  const int64_t tasks = mf ? (int64_t)G * (ci / 16) * (ci / 16) : cdiv((int64_t)G * ci * co, GT);
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(512, 4096 / std::max<int64_t>(tasks, 1)));
  return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(n_out, mf ? 128 : 256), cap));
}

constexpr int kMfmaSmemMax = GKM * 64 * 64;  // K cg 64 bytes at K = 27, width 64

template <int CG>
int launch_fwd_mfma(const GcArgs &a, bool vec, hipStream_t st) {
  const int smem = a.K * CG * 64;
  if (smem > 64 * 1024) {
    static const bool attr_ok =
        hipFuncSetAttribute(reinterpret_cast<const void *>(&gconv_fwd_mfma_kernel<CG, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            kMfmaSmemMax) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&gconv_fwd_mfma_kernel<CG, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            kMfmaSmemMax) == hipSuccess;
    MINK_REQUIRE(attr_ok, "gconv_fwd: %d bytes of LDS per workgroup refused", smem);
  }
  const int64_t gy = (int64_t)a.G * (CG / 16);
  const int64_t want = std::max<int64_t>(1, 1024 / gy);
  const int rpb = (int)std::min<int64_t>(1 << 20, align_up(std::max<int64_t>(64, cdiv(a.n_out, want)), 64));
  const dim3 grid((unsigned)gy, (unsigned)cdiv(a.n_out, rpb));  // (at most 1025 row blocks)
  if (vec) gconv_fwd_mfma_kernel<CG, true><<<grid, GT, smem, st>>>(a, rpb);
  else gconv_fwd_mfma_kernel<CG, false><<<grid, GT, smem, st>>>(a, rpb);
  return MINK_OK;
}

template <int CI>
int launch_fwd_fma(const GcArgs &a, bool vec, hipStream_t st) {
  const int smem = a.K * CI * GSLAB * 4;  // <= 55,296 bytes
  const int rpb = 256;
  const int64_t slabs = cdiv((int64_t)a.G * a.co, GSLAB), blocks = cdiv(a.n_out, rpb) * slabs;
  MINK_REQUIRE(blocks < (1LL << 31), "gconv_fwd: %lld workgroups (below 2^31)", (long long)blocks);
  const dim3 grid((unsigned)blocks);
  if (vec) gconv_fwd_fma_kernel<CI, true><<<grid, GT, smem, st>>>(a, rpb, (int)slabs);
  else gconv_fwd_fma_kernel<CI, false><<<grid, GT, smem, st>>>(a, rpb, (int)slabs);
  return MINK_OK;
}

}  // namespace
}  // namespace mink

using namespace mink;

// what both entry points ask of a shape: G cg K < 2^31 keeps every weight index of a thread inside an int
#define MINK_GCONV_REQUIRE_SHAPE(name, n_in, n_out, K, G, ci, co)                                                                 \
  do {                                                                                                                            \
    MINK_REQUIRE((K) >= 1 && (K) <= MINK_GCONV_MAX_K, name ": K=%d offsets (1 <= K <= %d)", (int)(K), MINK_GCONV_MAX_K);          \
    MINK_REQUIRE((G) >= 1 && (ci) >= 1 && (co) >= 1, name ": G=%d groups of cg_in=%d -> cg_out=%d channels (all >= 1)", (int)(G), \
                 (int)(ci), (int)(co));                                                                                           \
    MINK_REQUIRE((int64_t)(G) * (ci) * (co) * (K) < (1LL << 31) && (int64_t)(G) * (ci) < (1LL << 31) && (int64_t)(G) * (co) < (1LL << 31), \
                 name ": K G cg_in cg_out = %lld weights (below 2^31)", (long long)(G) * (ci) * (co) * (K));                      \
    MINK_REQUIRE((n_in) >= 0 && (n_in) < (1LL << 31) && (n_out) >= 0 && (n_out) < (1LL << 31),                                    \
                 name ": n_in=%lld, n_out=%lld rows (0 <= n < 2^31)", (long long)(n_in), (long long)(n_out));                     \
  } while (0)

extern "C" {

int mink_gconv_fwd(const float *x, int64_t n_in, int32_t ldx, const float *w, int32_t w_transposed, int32_t flip_k, const int32_t *nbr,
                   int64_t n_out, int32_t K, int32_t G, int32_t cg_in, int32_t cg_out, float *y, int32_t ldy, void *stream) {
  MINK_GCONV_REQUIRE_SHAPE("gconv_fwd", n_in, n_out, K, G, cg_in, cg_out);
  MINK_REQUIRE((int64_t)ldx >= (int64_t)G * cg_in, "gconv_fwd: ldx=%d below the G cg_in = %lld columns of an x row", ldx,
               (long long)G * cg_in);
  MINK_REQUIRE((int64_t)ldy >= (int64_t)G * cg_out, "gconv_fwd: ldy=%d below the G cg_out = %lld columns of a y row", ldy,
               (long long)G * cg_out);
  if (n_out == 0) return MINK_OK;  // nothing to write: the pointers of empty matrices are not looked at
  MINK_REQUIRE(x && w && nbr && y, "gconv_fwd: NULL pointer (x, w, nbr, y)");
  MINK_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)nbr | (uintptr_t)y) & 3) == 0, "gconv_fwd: x, w, nbr and y must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  GcArgs a;
  a.x = x, a.n_in = n_in, a.ldx = ldx, a.w = w, a.wt = w_transposed != 0, a.flip = (flip_k & 1) != 0, a.nbr = nbr, a.n_out = n_out;
  a.K = K, a.G = G, a.ci = cg_in, a.co = cg_out, a.y = y, a.ldy = ldy;
  const bool vec = aligned16(x) && aligned16(y) && (ldx & 3) == 0 && (ldy & 3) == 0;
  int rc = MINK_OK;
  if (mfma_width(cg_in, cg_out)) {
    rc = cg_in == 16 ? launch_fwd_mfma<16>(a, vec, st) : cg_in == 32 ? launch_fwd_mfma<32>(a, vec, st) : launch_fwd_mfma<64>(a, vec, st);
  } else if (fma_width(cg_in, cg_out)) {
    rc = cg_in == 4 ? launch_fwd_fma<4>(a, vec, st) : launch_fwd_fma<8>(a, vec, st);
  } else {
    gconv_fwd_generic_kernel<<<dim3(flat_grid(n_out * G * cg_out, GT, 1 << 16)), GT, 0, st>>>(a);
  }
  if (rc) return rc;
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int64_t mink_gconv_wgrad_workspace_bytes(int64_t n_out, int32_t K, int32_t G, int32_t cg_in, int32_t cg_out) {
  if (n_out < 0 || K < 1 || K > MINK_GCONV_MAX_K || G < 1 || cg_in < 1 || cg_out < 1 || (int64_t)G * cg_in * cg_out * K >= (1LL << 31)) return 0;
  return align_up((int64_t)wgrad_blocks(n_out, K, G, cg_in, cg_out) * K * G * cg_in * cg_out * (int64_t)sizeof(float), 16);
}

int mink_gconv_wgrad(const float *x, int64_t n_in, int32_t ldx, const float *dy, int32_t ldy, const int32_t *nbr, int64_t n_out, int32_t K,
                     int32_t G, int32_t cg_in, int32_t cg_out, float *dw, void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_GCONV_REQUIRE_SHAPE("gconv_wgrad", n_in, n_out, K, G, cg_in, cg_out);
  MINK_REQUIRE((int64_t)ldx >= (int64_t)G * cg_in, "gconv_wgrad: ldx=%d below the G cg_in = %lld columns of an x row", ldx,
               (long long)G * cg_in);
  MINK_REQUIRE((int64_t)ldy >= (int64_t)G * cg_out, "gconv_wgrad: ldy=%d below the G cg_out = %lld columns of a dy row", ldy,
               (long long)G * cg_out);
  if (n_out == 0) {  // an empty sum: zeros, and the pointers of the empty matrices are not looked at
    MINK_REQUIRE(dw && ((uintptr_t)dw & 3) == 0, "gconv_wgrad: NULL or unaligned pointer (dw)");
    MINK_HIP(hipMemsetAsync(dw, 0, (size_t)K * G * cg_in * cg_out * sizeof(float), (hipStream_t)stream));
    return MINK_OK;
  }
  MINK_REQUIRE(x && dy && nbr && dw && workspace, "gconv_wgrad: NULL pointer (x, dy, nbr, dw, workspace)");
  MINK_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)nbr | (uintptr_t)dw) & 3) == 0, "gconv_wgrad: x, dy, nbr and dw must be 4-byte aligned");
  MINK_REQUIRE_WORKSPACE("gconv_wgrad", workspace_bytes, mink_gconv_wgrad_workspace_bytes(n_out, K, G, cg_in, cg_out), workspace);
  hipStream_t st = (hipStream_t)stream;
  GwArgs a;
  a.x = x, a.n_in = n_in, a.ldx = ldx, a.dy = dy, a.ldy = ldy, a.nbr = nbr, a.n_out = n_out, a.K = K, a.G = G, a.ci = cg_in, a.co = cg_out;
  a.RB = wgrad_blocks(n_out, K, G, cg_in, cg_out), a.ws = (float *)workspace;
  const int64_t E = (int64_t)G * cg_in * cg_out;
  if (mfma_width(cg_in, cg_out)) {  // (n_out == 0: one block of no rows writes the zeros)
    const int S = cg_in / 16;
    const dim3 grid((unsigned)(G * S * S), (unsigned)cdiv(a.RB, GT / 64));
#define MINK_GW(CG)                                                             \
  do {                                                                          \
    if (K <= 9) gconv_wgrad_mfma_kernel<CG, 9><<<grid, GT, 0, st>>>(a);          \
    else gconv_wgrad_mfma_kernel<CG, GKM><<<grid, GT, 0, st>>>(a);               \
  } while (0)
    if (cg_in == 16) MINK_GW(16);
    else if (cg_in == 32) MINK_GW(32);
    else MINK_GW(64);
#undef MINK_GW
  } else if (sub4_wgrad(K, cg_in, cg_out)) {
    const Sub4Shape s(G, cg_in);
    const dim3 grid((unsigned)s.gx, (unsigned)a.RB);
    const int smem = s.row_lanes * s.tasks_per_block * 16 * (int)sizeof(float);  // <= 16 KB
    const bool vec = aligned16(x) && aligned16(dy) && (ldx & 3) == 0 && (ldy & 3) == 0;
    if (cg_in == 4) {
      if (vec) gconv_wgrad_sub4_kernel<4, true><<<grid, GT, smem, st>>>(a, s.tasks_per_block, s.row_lanes);
      else gconv_wgrad_sub4_kernel<4, false><<<grid, GT, smem, st>>>(a, s.tasks_per_block, s.row_lanes);
    } else {
      if (vec) gconv_wgrad_sub4_kernel<8, true><<<grid, GT, smem, st>>>(a, s.tasks_per_block, s.row_lanes);
      else gconv_wgrad_sub4_kernel<8, false><<<grid, GT, smem, st>>>(a, s.tasks_per_block, s.row_lanes);
    }
  } else {
    const dim3 grid((unsigned)cdiv(E, GT), (unsigned)a.RB);
    if (K <= 9) gconv_wgrad_generic_kernel<9><<<grid, GT, 0, st>>>(a);
    else gconv_wgrad_generic_kernel<GKM><<<grid, GT, 0, st>>>(a);
  }
  gconv_wgrad_reduce_kernel<<<dim3(flat_grid(E * K, GT, 1 << 16)), GT, 0, st>>>(a.ws, a.RB, E * K, dw);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
