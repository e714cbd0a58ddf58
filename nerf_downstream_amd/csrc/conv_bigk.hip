// Sparse convolution with centred cubic kernels of 5^3 = 125 and 7^3 = 343 offsets (27 < K <= 343): the neighbour table of a
// cube, the forward / data-gradient gather-GEMM and the weight gradient.  conv.hip / conv_wgrad.hip stop at KMAX = 27 offsets
// (their LDS table staging is sized by it) and are not touched: these entries are reached only for K > 27.
//
// Arithmetic: exact fp32 on the matrix cores (v_mfma_f32_16x16x4_f32) in EVERY mink_conv_set_math mode, as gconv.hip is --
// the bf16 modes change nothing here.  No atomics in the convolution kernels, a fixed summation order (offsets ascending,
// channels ascending inside an offset, row splits of the weight gradient in ascending order): two runs give the same bits.
//
// Forward / data gradient (bigk_fwd_kernel): a workgroup owns MINK_BIGK_ROW_TILE output rows and up to 64 output columns and
// walks the table of its rows in chunks of 32 offsets staged through LDS.  The offsets of a chunk that no row of the tile has
// are dropped (a wave64 ballot over per-offset flags), and the reduction runs FLATTENED over (present offset, channel): 32
// reduction indices per step whatever cin is, so the 1 / 3 / 4-channel stems fill the MFMA's K dimension as the wide layers
// do.  An absent neighbour is a zero in the gathered operand: with finite weights it contributes an exact zero.
//
// Weight gradient (bigk_wgrad_kernel): grid = offset groups x row splits x (channel slab, column slab).  A workgroup keeps the
// dW tiles of its KG offsets in registers over its rows (wave w owns column tile w), stages the dy tile once per 32 rows and
// gathers the x rows of every present offset of its group in one round of loads; an offset no row of the 32 has is skipped.
// Here BOTH operands are data, so a zero-filled absent neighbour would turn a NaN of dy into a NaN of an offset the row does
// not have: the dy operand of offset k is masked by the presence of (row, k) when it is read from LDS.  Row splits go to the
// workspace and are summed in ascending order by a second kernel.
//
// Staging loads in both kernels are unconditional on clamped addresses (row 0 for an absent neighbour, the last row past the
// end) and discarded by a select, never multiplied: a thread's loads of a step are then in flight together instead of one
// round trip per branch (measured: forward 8.7 -> 6.6 ms, weight gradient 13.1 -> 7.5 ms at 825 k rows, 28 -> 64, K = 125).
// Measured and not kept: the forward kernel loading a step ahead into registers (24 more VGPRs, four waves per SIMD instead of
// five): 7.1 ms at that shape -- five workgroups per CU already overlap one another's staging.
//
// Table (mink_kernel_map_cube): a per-voxel hash map of the input rows built in the workspace (fill, insert, then one probe
// per (row, offset)) -- not the block index of the 27-offset tables, and independent of the level's own map, which the pyramid
// leaves empty for ascending rows.  Measured: 825 k rows x 125 offsets (a 413 MB table) in 1.09 ms, 116 k x 343 in 0.43 ms,
// beside 0.14 / 0.06 ms for the 3x3x3 tables of the same rows through the block index (profiles/bigk_kernels.txt).
#include <string.h>

#include "common.h"

namespace mink {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int TM = MINK_BIGK_ROW_TILE;  // output rows of a forward workgroup (4 waves x 16)
constexpr int KC = 32;                  // offsets of a table chunk
constexpr int RS = 32;                  // flattened reduction indices of a step
constexpr int AS = 36;                  // LDS pitch of the gathered tile (16 rows x 4 k land in distinct banks)
constexpr int BS = 81;                  // LDS pitch of the weight tile (odd: the transposed staging writes down a column)
constexpr int NCOL = 64;                // output columns of a workgroup
static_assert(TM == 64, "a forward workgroup is four waves of 16 rows");

// ------------------------------------------------------------------------------------------------ neighbour table of a cube
__global__ __launch_bounds__(kThreads) void cube_insert_kernel(const int *__restrict__ coords, int64_t n,
                                                               unsigned long long *tkeys, int *tvals, uint64_t mask) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int4 c = reinterpret_cast<const int4 *>(coords)[i];
  uint64_t key;
  if (!pack_key(c.x, c.y, c.z, c.w, key)) return;  // (rows of a map are in range: it was built from packed keys)
  uint64_t s = mix64(key) & mask;
  for (;;) {  // capacity >= 2 n: an empty slot is always found
    const unsigned long long prev = atomicCAS(&tkeys[s], (unsigned long long)kEmptyKey, (unsigned long long)key);
    if (prev == kEmptyKey || prev == key) {
      tvals[s] = (int)i;  // rows of a map are unique
      return;
    }
    s = (s + 1) & mask;
  }
}

__global__ __launch_bounds__(kThreads) void cube_map_kernel(const uint64_t *__restrict__ tkeys, const int *__restrict__ tvals,
                                                            uint64_t mask, const int *__restrict__ out_coords, int64_t n_out,
                                                            int ks, int step, int *__restrict__ nbr, int *nbr_t) {
  const int K = ks * ks * ks;
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= n_out * K) return;
  const int64_t o = idx / K;
  const int k = (int)(idx - o * K);
  const int r = (ks - 1) / 2;
  const int dx = (k % ks - r) * step, dy = (k / ks % ks - r) * step, dz = (k / (ks * ks) - r) * step;  // x fastest, z slowest
  const int4 c = reinterpret_cast<const int4 *>(out_coords)[o];
  uint64_t key;
  int v = -1;
  // a neighbour outside the packable range is absent: pack_key refuses it before the 16-bit fields could wrap onto another key
  if (pack_key(c.x, c.y + dx, c.z + dy, c.w + dz, key)) v = table_find(tkeys, tvals, mask, key);
  nbr[idx] = v;
  if (nbr_t && v >= 0) nbr_t[(int64_t)v * K + k] = (int)o;
}

// ------------------------------------------------------------------------------------------------ forward / data gradient
template <bool WT>
__global__ __launch_bounds__(kThreads) void bigk_fwd_kernel(const float *__restrict__ x, int ldx, int cin,
                                                            const float *__restrict__ w, int flip,
                                                            const int *__restrict__ nbr, int64_t n_out, int K,
                                                            float *__restrict__ y, int ldy, int cout,
                                                            const float *__restrict__ bias) {
  __shared__ int nb[TM][KC + 1];
  __shared__ int flags[KC];
  __shared__ int plist[KC];
  __shared__ int pcount;
  __shared__ float As[TM][AS];
  __shared__ float Bs[RS][BS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l = lane & 15, q = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * TM;
  const int n0 = blockIdx.y * NCOL;
  const int ncols = min(NCOL, cout - n0), ntiles = (ncols + 15) >> 4;
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += KC) {
    const int kc = min(KC, K - k0);
    if (tid < KC) flags[tid] = 0;
    __syncthreads();
    {  // (loads are unconditional on clamped addresses and discarded by a select: the eight of a thread are in flight together)
      const int kk = tid & 31, kkc = kk < kc ? kk : 0;
      int v[TM * KC / kThreads];
#pragma unroll
      for (int i = 0; i < TM * KC / kThreads; ++i) {
        const int64_t row = row0 + (tid >> 5) + i * (kThreads / KC);
        v[i] = nbr[(row < n_out ? row : n_out - 1) * K + k0 + kkc];
      }
#pragma unroll
      for (int i = 0; i < TM * KC / kThreads; ++i) {
        const int r = (tid >> 5) + i * (kThreads / KC);
        const int t = (row0 + r < n_out && kk < kc) ? v[i] : -1;
        nb[r][kk] = t;
        if (t >= 0) flags[kk] = 1;  // (every writer stores the same value)
      }
    }
    __syncthreads();
    if (wave == 0) {  // the present offsets of the chunk, ascending
      const bool f = lane < KC && flags[lane & (KC - 1)] != 0;
      const unsigned long long m = __ballot(f);
      if (f) plist[wave_rank(m)] = lane;
      if (lane == 0) pcount = __popcll(m);
    }
    __syncthreads();
    const int R = pcount * cin;  // flattened reduction length of the chunk
    for (int r0 = 0; r0 < R; r0 += RS) {
      {  // gathered tile: a thread keeps its reduction index (one division per step) and walks 8 rows
        const int rr = tid & 31, r = r0 + rr;
        const bool live = r < R;
        const int j = live ? r / cin : 0, c = live ? r - j * cin : 0, pj = plist[j];
        int idx[TM * RS / kThreads];
        float v[TM * RS / kThreads];
#pragma unroll
        for (int i = 0; i < TM * RS / kThreads; ++i) idx[i] = nb[(tid >> 5) + i * (kThreads / RS)][pj];
#pragma unroll
        for (int i = 0; i < TM * RS / kThreads; ++i) v[i] = x[(int64_t)(idx[i] < 0 ? 0 : idx[i]) * ldx + c];
#pragma unroll
        for (int i = 0; i < TM * RS / kThreads; ++i)
          As[(tid >> 5) + i * (kThreads / RS)][rr] = (live && idx[i] >= 0) ? v[i] : 0.f;  // an absent neighbour is an exact zero
      }
      float bv[RS * NCOL / kThreads];
      if (WT) {  // w[K][cout][cin]: consecutive lanes read consecutive channels of one output column
        const int rr = tid & 31, r = r0 + rr;
        const bool live = r < R;
        const int j = live ? r / cin : 0, c = live ? r - j * cin : 0;
        const int k = k0 + plist[j], kw = flip ? K - 1 - k : k;
#pragma unroll
        for (int i = 0; i < RS * NCOL / kThreads; ++i) {
          const int n = (tid >> 5) + i * (kThreads / RS);
          bv[i] = w[((int64_t)kw * cout + n0 + (n < ncols ? n : 0)) * cin + c];
        }
#pragma unroll
        for (int i = 0; i < RS * NCOL / kThreads; ++i) {
          const int n = (tid >> 5) + i * (kThreads / RS);
          Bs[rr][n] = (live && n < ncols) ? bv[i] : 0.f;
        }
      } else {   // w[K][cin][cout]: consecutive lanes read consecutive output columns; the index advances by 4 per pass
        const int n = tid & 63, nc = n < ncols ? n : 0;
        int j = (r0 + (tid >> 6)) / cin, c = (r0 + (tid >> 6)) - j * cin;
#pragma unroll
        for (int i = 0; i < RS * NCOL / kThreads; ++i) {
          const bool live = r0 + (tid >> 6) + i * (kThreads / NCOL) < R;
          const int k = k0 + plist[live ? j : 0], kw = flip ? K - 1 - k : k;
          bv[i] = w[((int64_t)kw * cin + (live ? c : 0)) * cout + n0 + nc];
          c += kThreads / NCOL;
          while (c >= cin) c -= cin, ++j;
        }
#pragma unroll
        for (int i = 0; i < RS * NCOL / kThreads; ++i) {
          const int rr = (tid >> 6) + i * (kThreads / NCOL);
          Bs[rr][n] = (r0 + rr < R && n < ncols) ? bv[i] : 0.f;
        }
      }
      __syncthreads();
      const int ksteps = (min(RS, R - r0) + 3) >> 2;  // (the tail of the last group of 4 is zero on both sides)
      for (int s = 0; s < ksteps; ++s) {
        const float a = As[wave * 16 + l][s * 4 + q];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          if (nt < ntiles) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[s * 4 + q][nt * 16 + l], acc[nt], 0, 0, 0);
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int n = nt * 16 + l;
    if (nt < ntiles && n < ncols) {
      const float b = bias ? bias[n0 + n] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t row = row0 + wave * 16 + q * 4 + j;
        if (row < n_out) y[row * ldy + n0 + n] = acc[nt][j] + b;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int RT = MINK_BIGK_WGRAD_ROWS;  // rows (the reduction dimension) of a weight-gradient step
constexpr int DS = 80;   // LDS pitch of the dy tile

template <int MT, int KG>  // MT channel tiles of 16 and KG offsets per workgroup: MT * KG = 16 accumulator tiles per wave
__global__ __launch_bounds__(kThreads) void bigk_wgrad_kernel(const float *__restrict__ x, int ldx, int cin,
                                                              const float *__restrict__ dy, int ldy, int cout,
                                                              const int *__restrict__ nbr, int64_t n_out, int K,
                                                              float *__restrict__ out, int64_t tiles, int tiles_per_split,
                                                              int cslabs) {
  constexpr int MW = 16 * MT;
  constexpr int XS = MT == 1 ? 16 : MT == 2 ? 48 : 80;
  __shared__ int nb[RT][KG + 1];
  __shared__ int flags[KG];
  __shared__ float Xs[KG][RT][XS];
  __shared__ float Ds[RT][DS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l = lane & 15, q = lane >> 4;
  const int k0 = blockIdx.x * KG, kg = min(KG, K - k0);
  const int c0 = (blockIdx.z % cslabs) * MW, n0 = (blockIdx.z / cslabs) * NCOL;
  const bool wave_live = n0 + wave * 16 < cout;
  f32x4 acc[KG][MT];
#pragma unroll
  for (int j = 0; j < KG; ++j)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[j][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t t0 = (int64_t)blockIdx.y * tiles_per_split, t1 = min(tiles, t0 + tiles_per_split);
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t row0 = t * RT;
    __syncthreads();  // the previous tile's readers of flags / nb / Ds / Xs are done
    if (tid < KG) flags[tid] = 0;
    __syncthreads();
    // (every load below is unconditional on a clamped address and discarded by a select, so that a thread's loads are in flight together)
    for (int e = tid; e < RT * KG; e += kThreads) {
      const int r = e / KG, j = e - r * KG;
      const int64_t row = row0 + r;
      const int t = nbr[(row < n_out ? row : n_out - 1) * K + k0 + (j < kg ? j : 0)];
      const int v = (row < n_out && j < kg) ? t : -1;
      nb[r][j] = v;
      if (v >= 0) flags[j] = 1;
    }
    {
      const int n = tid & 63, nc = n0 + n < cout ? n0 + n : 0;
      float v[RT * NCOL / kThreads];
#pragma unroll
      for (int i = 0; i < RT * NCOL / kThreads; ++i) {
        const int64_t row = row0 + (tid >> 6) + i * (kThreads / NCOL);
        v[i] = dy[(row < n_out ? row : n_out - 1) * ldy + nc];
      }
#pragma unroll
      for (int i = 0; i < RT * NCOL / kThreads; ++i) {
        const int r = (tid >> 6) + i * (kThreads / NCOL);
        Ds[r][n] = (row0 + r < n_out && n0 + n < cout) ? v[i] : 0.f;
      }
    }
    __syncthreads();
    // the gathered rows of every present offset of the group in one round of loads (an offset no row of the tile has is skipped)
#pragma unroll
    for (int j = 0; j < KG; ++j) {
      if (flags[j]) {  // (uniform over the workgroup)
        const int c = tid % MW, cc = c0 + c < cin ? c0 + c : 0;
        int idx[RT * MW / kThreads];
        float v[RT * MW / kThreads];
#pragma unroll
        for (int i = 0; i < RT * MW / kThreads; ++i) idx[i] = nb[tid / MW + i * (kThreads / MW)][j];
#pragma unroll
        for (int i = 0; i < RT * MW / kThreads; ++i) v[i] = x[(int64_t)(idx[i] < 0 ? 0 : idx[i]) * ldx + cc];
#pragma unroll
        for (int i = 0; i < RT * MW / kThreads; ++i)
          Xs[j][tid / MW + i * (kThreads / MW)][c] = (idx[i] >= 0 && c0 + c < cin) ? v[i] : 0.f;
      }
    }
    __syncthreads();
    if (wave_live) {
#pragma unroll
      for (int j = 0; j < KG; ++j) {
        if (flags[j]) {
#pragma unroll
          for (int s = 0; s < RT / 4; ++s) {
            const int row = s * 4 + q;
            // both operands are data: an absent (row, offset) pair must not meet a NaN of dy as 0 x NaN
            const float b = nb[row][j] >= 0 ? Ds[row][wave * 16 + l] : 0.f;
#pragma unroll
            for (int m = 0; m < MT; ++m)
              acc[j][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(Xs[j][row][m * 16 + l], b, acc[j][m], 0, 0, 0);
          }
        }
      }
    }
  }
  const int n = n0 + wave * 16 + l;
  float *dst = out + (int64_t)blockIdx.y * K * cin * cout;
  if (n < cout) {
#pragma unroll
    for (int j = 0; j < KG; ++j) {
      if (j < kg) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int c = c0 + m * 16 + q * 4 + i;
            if (c < cin) dst[((int64_t)(k0 + j) * cin + c) * cout + n] = acc[j][m][i];
          }
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void bigk_split_sum_kernel(const float *__restrict__ ws, int splits, int64_t count,
                                                                  float *__restrict__ dw) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  float s = ws[i];
  for (int p = 1; p < splits; ++p) s += ws[(int64_t)p * count + i];  // ascending row splits
  dw[i] = s;
}

struct WgradPlan {
  int mt, kg, groups, cslabs, nslabs, splits, tiles_per_split;
  int64_t tiles;
};

WgradPlan wgrad_plan(int64_t n_out, int K, int cin, int cout) {
  WgradPlan p;
  p.mt = cin <= 16 ? 1 : cin <= 32 ? 2 : 4;
  p.kg = 16 / p.mt;
  p.groups = (int)cdiv(K, p.kg);
  p.cslabs = (int)cdiv(cin, 16 * p.mt);
  p.nslabs = (int)cdiv(cout, NCOL);
  p.tiles = cdiv(n_out, RT);
  const int64_t wgs = (int64_t)p.groups * p.cslabs * p.nslabs;
  int64_t s = cdiv(2048, wgs);  // a few rounds of the two workgroups a CU holds
  if (s > 128) s = 128;
  if (s > p.tiles) s = p.tiles;
  if (s < 1) s = 1;
  p.tiles_per_split = (int)cdiv(p.tiles > 0 ? p.tiles : 1, s);
  p.splits = (int)cdiv(p.tiles > 0 ? p.tiles : 1, p.tiles_per_split);
  return p;
}

bool bigk_volume(int K) { return K > 27 && K <= MINK_BIGK_MAX_K; }

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_kernel_map_cube_workspace_bytes(int64_t n_in) { return 12 * mink_table_capacity(n_in > 0 ? n_in : 1); }

int mink_kernel_map_cube(const int32_t *in_coords, int64_t n_in, const int32_t *out_coords, int64_t n_out, int32_t ks,
                         int32_t step, int32_t *nbr, int32_t *nbr_t, void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(ks == 5 || ks == 7, "kernel_map_cube: kernel size %d unsupported (5 and 7; 1..3 go through mink_kernel_map)", ks);
  MINK_REQUIRE(step >= 1 && step <= 65535, "kernel_map_cube: step %d (dilation * tensor stride) out of range", step);
  const int64_t K = (int64_t)ks * ks * ks;
  MINK_REQUIRE(n_out >= 0 && n_in >= 0 && n_out * K < (1ll << 31) && (!nbr_t || n_in * K < (1ll << 31)),
               "kernel_map_cube: rows * K overflows int32 indexing");
  if (n_out == 0 && (n_in == 0 || !nbr_t)) return MINK_OK;
  MINK_REQUIRE(out_coords || n_out == 0, "kernel_map_cube: NULL pointer");
  MINK_REQUIRE((in_coords || n_in == 0) && (nbr || n_out == 0) && workspace, "kernel_map_cube: NULL pointer");
  MINK_REQUIRE((((uintptr_t)in_coords | (uintptr_t)out_coords | (uintptr_t)workspace) & 15) == 0,
               "kernel_map_cube: coordinates and workspace must be 16-byte aligned");
  const int64_t cap = mink_table_capacity(n_in > 0 ? n_in : 1);
  MINK_REQUIRE(workspace_bytes >= 12 * cap, "kernel_map_cube: workspace too small (%lld < %lld)", (long long)workspace_bytes,
               (long long)(12 * cap));
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *tkeys = (unsigned long long *)workspace;
  int *tvals = (int *)(tkeys + cap);
  MINK_HIP(hipMemsetAsync(tkeys, 0xFF, 8 * cap, st));
  if (nbr_t && n_in > 0) MINK_HIP(hipMemsetAsync(nbr_t, 0xFF, 4 * n_in * K, st));
  if (n_in > 0) {
    cube_insert_kernel<<<dim3((unsigned)cdiv(n_in, kThreads)), kThreads, 0, st>>>(in_coords, n_in, tkeys, tvals, (uint64_t)cap - 1);
    MINK_CHECK_LAUNCH();
  }
  if (n_out > 0) {
    cube_map_kernel<<<dim3((unsigned)cdiv(n_out * K, kThreads)), kThreads, 0, st>>>(
        (const uint64_t *)tkeys, tvals, (uint64_t)cap - 1, out_coords, n_out, ks, step, nbr, nbr_t);
    MINK_CHECK_LAUNCH();
  }
  return MINK_OK;
}

int mink_conv_bigk_gather_gemm(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *w, int32_t w_transposed,
                               int32_t flip_k, const int32_t *nbr, int64_t n_out, int32_t K, float *y, int32_t ldy, int32_t cout,
                               const float *bias, void *stream) {
  MINK_REQUIRE(bigk_volume(K), "conv_bigk: kernel volume %d unsupported (28..%d; up to 27 goes through mink_conv_gather_gemm)", K,
               MINK_BIGK_MAX_K);
  MINK_REQUIRE(cin >= 1 && cout >= 1 && ldx >= cin && ldy >= cout, "conv_bigk: bad channel counts / pitches");
  MINK_REQUIRE((flip_k & ~1) == 0, "conv_bigk: flip_k bit 0 only (no accumulate form)");
  MINK_REQUIRE(n_out >= 0 && n_in >= 0 && n_out * K < (1ll << 31), "conv_bigk: n_out*K overflows int32 indexing");
  if (n_out == 0) return MINK_OK;
  MINK_REQUIRE((x || n_in == 0) && w && nbr && y, "conv_bigk: NULL pointer");  // (an empty operand: every table entry is -1)
  if (n_in == 0) x = w;  // (every table entry is -1: the clamped loads of the kernel read elements 0 .. cin - 1 and discard them)
  const dim3 grid((unsigned)cdiv(n_out, TM), (unsigned)cdiv(cout, NCOL));
  hipStream_t st = (hipStream_t)stream;
  if (w_transposed)
    bigk_fwd_kernel<true><<<grid, kThreads, 0, st>>>(x, ldx, cin, w, flip_k & 1, nbr, n_out, K, y, ldy, cout, bias);
  else
    bigk_fwd_kernel<false><<<grid, kThreads, 0, st>>>(x, ldx, cin, w, flip_k & 1, nbr, n_out, K, y, ldy, cout, bias);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int64_t mink_conv_bigk_wgrad_workspace_bytes(int64_t n_out, int32_t K, int32_t cin, int32_t cout) {
  if (!bigk_volume(K) || cin < 1 || cout < 1 || n_out < 0) return 16;
  const WgradPlan p = wgrad_plan(n_out, K, cin, cout);
  return p.splits > 1 ? (int64_t)p.splits * K * cin * cout * 4 : 16;
}

int mink_conv_bigk_wgrad(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *dy, int32_t ldy, int32_t cout,
                         const int32_t *nbr, int64_t n_out, int32_t K, float *dw, void *workspace, int64_t workspace_bytes,
                         void *stream) {
  MINK_REQUIRE(bigk_volume(K), "conv_bigk_wgrad: kernel volume %d unsupported (28..%d; up to 27 goes through mink_conv_wgrad)", K,
               MINK_BIGK_MAX_K);
  MINK_REQUIRE(cin >= 1 && cout >= 1 && ldx >= cin && ldy >= cout, "conv_bigk_wgrad: bad channel counts / pitches");
  MINK_REQUIRE(n_out >= 0 && n_in >= 0 && n_out * K < (1ll << 31), "conv_bigk_wgrad: n_out*K overflows int32 indexing");
  MINK_REQUIRE(dw, "conv_bigk_wgrad: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t count = (int64_t)K * cin * cout;
  if (n_out == 0) {
    MINK_HIP(hipMemsetAsync(dw, 0, 4 * count, st));
    return MINK_OK;
  }
  MINK_REQUIRE((x || n_in == 0) && dy && nbr, "conv_bigk_wgrad: NULL pointer");
  if (n_in == 0) x = dw;  // (every table entry is -1: the clamped loads of the kernel read elements 0 .. cin - 1 and discard them)
  const WgradPlan p = wgrad_plan(n_out, K, cin, cout);
  const int64_t need = p.splits > 1 ? (int64_t)p.splits * count * 4 : 0;
  MINK_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "conv_bigk_wgrad: workspace too small (%lld < %lld)",
               (long long)workspace_bytes, (long long)need);
  float *out = p.splits > 1 ? (float *)workspace : dw;
  const dim3 grid((unsigned)p.groups, (unsigned)p.splits, (unsigned)(p.cslabs * p.nslabs));
  if (p.mt == 1)
    bigk_wgrad_kernel<1, 16><<<grid, kThreads, 0, st>>>(x, ldx, cin, dy, ldy, cout, nbr, n_out, K, out, p.tiles, p.tiles_per_split, p.cslabs);
  else if (p.mt == 2)
    bigk_wgrad_kernel<2, 8><<<grid, kThreads, 0, st>>>(x, ldx, cin, dy, ldy, cout, nbr, n_out, K, out, p.tiles, p.tiles_per_split, p.cslabs);
  else
    bigk_wgrad_kernel<4, 4><<<grid, kThreads, 0, st>>>(x, ldx, cin, dy, ldy, cout, nbr, n_out, K, out, p.tiles, p.tiles_per_split, p.cslabs);
  MINK_CHECK_LAUNCH();
  if (p.splits > 1) {
    bigk_split_sum_kernel<<<dim3((unsigned)cdiv(count, kThreads)), kThreads, 0, st>>>((const float *)workspace, p.splits, count, dw);
    MINK_CHECK_LAUNCH();
  }
  return MINK_OK;
}

}  // extern "C"
