// Multi-head self-attention on gfx950 (timm's Attention.forward between its `qkv` and `proj` linears), fp32, on the row layout:
// qkv[B N][ldq] holds q | k | v of token row b N + t at columns s H D + h D + d (what nn.Linear(dim, 3 dim) writes), out[B N][ldo]
// holds softmax_j(scale q_i . k_j) v_j of head h at columns h D + d (what `proj` reads), so neither side needs a permute copy.
// D = 64.  No N x N matrix reaches memory in either direction: the forward keeps lse[b][h][i] = max_j s_ij + log sum_j
// exp(s_ij - max) (s = scale q.k) and the backward recomputes P = exp(s - lse) from it.
//
// Every product runs on the fp32 MFMA v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain, one rounding per product).  Lane l of a
// wave is (c, g) = (l & 15, l >> 4); the instruction takes A[i = c][k = g], B[k = g][j = c] and returns D[i = 4 g + r][j = c] in
// register r.  A sum over k may visit k in any fixed order as long as A and B agree, which is used twice:
//   - a dot product over the 64 head channels gives lane group g the channels 16 g .. 16 g + 15 (step t uses 16 g + t), so a
//     lane's 16 operands are contiguous: four 16-byte reads from LDS, or four 16-byte loads for the operand kept in registers;
//   - a result tile D is the B operand of the next product with no lane movement when that product sums over D's ROW index:
//     register r of lane (c, g) is row 4 g + r, so step r of the next product sums rows r, 4 + r, 8 + r, 12 + r and the A
//     operand reads those rows of its LDS tile.
//
//   attn_fwd  : workgroup = 64 queries of one (b, h), wave = 16 of them; K and V pass through LDS 64 keys at a time.
//               S^T = K Q^T (key on the row, query on the lane), online softmax with the row statistics on the lane,
//               O^T += V^T P^T.  Keys past N are staged as zeros and get the weight 0, query rows past N are not stored.
//   attn_delta: delta[b][h][i] = sum_d dO O (16 lanes per row, fixed order) into the workspace.
//   attn_dkv  : workgroup = 64 keys, wave = 16 of them with their K and V rows in registers; Q and dO pass through LDS 64
//               queries at a time.  S = Q K^T, dP = dO V^T (query on the row), dV^T += dO^T P, dK^T += Q^T dS.
//   attn_dq   : the forward's structure: S^T = K Q^T, dP^T = V dO^T, dQ^T += K^T dS^T.
// Both backward kernels recompute S (seven products instead of five), so every element of dq, dk and dv has one owner that sums
// in a fixed order and stores once: no atomics, no hand-off between workgroups, two runs give the same bits.
//
// exp is the library's expf (about one ulp for every argument; the bounds of tests/attn_restate.py count on an error that
// does not grow faster than |x| 2^-24), the row maximum is subtracted before every exponential of the forward and lse before
// every one of the backward.  16-byte global accesses when every matrix pointer is 16-byte aligned and every pitch a multiple
// of 4, dwords otherwise.
#include <math.h>

#include "rowpass.h"

namespace mink {
namespace {

constexpr int AT = 256;   // threads per workgroup: 4 waves, 16 rows of the 64-row tile each
constexpr int TR = 64;    // rows of a tile (queries or keys)
constexpr int HD = MINK_ATTN_HEAD_DIM;
constexpr int LDT = 68;   // LDS row pitch in floats: 16-byte aligned rows, 4 banks further per row
static_assert(HD == 64, "the lane maps below are written for 64 channels per head");

using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// rows [r0, r0 + 64) x 64 columns at `base` (row 0 of the sample, first column of the head) -> t; rows from N on are zeros
template <int VEC>
__device__ __forceinline__ void stage_tile(float (*t)[LDT], const float *__restrict__ base, int64_t ld, int r0, int N) {
  constexpr int CG = HD / VEC;
  for (int e = threadIdx.x; e < TR * CG; e += AT) {
    const int r = e / CG, c = (e % CG) * VEC;
    float v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = 0.f;
    if (r0 + r < N) ldv<VEC>(base + (int64_t)(r0 + r) * ld + c, v);
    stv<VEC>(&t[r][c], v);
  }
}

// 16 contiguous floats of a global row into registers, zeros when the row does not exist
template <int VEC>
__device__ __forceinline__ void load16(const float *__restrict__ p, bool ok, float (&v)[16]) {
#pragma unroll
  for (int k = 0; k < 16; k += VEC) {
    float t[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) t[j] = 0.f;
    if (ok) ldv<VEC>(p + k, t);
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[k + j] = t[j];
  }
}

// 16 contiguous floats of an LDS row (always 16-byte aligned)
__device__ __forceinline__ void lds16(const float *p, float (&v)[16]) {
#pragma unroll
  for (int k = 0; k < 16; k += 4) {
    const float4 t = *reinterpret_cast<const float4 *>(p + k);
    v[k] = t.x, v[k + 1] = t.y, v[k + 2] = t.z, v[k + 3] = t.w;
  }
}

// D[4 g + r][c] = sum_d T[16 rt + .][d] * reg[d]: the tile's rows on the result's rows, the register operand's row on the lane
__device__ __forceinline__ f32x4 dot_tile(const float (*t)[LDT], int rt, int c, int g, const float (&reg)[16]) {
  float a[16];
  lds16(&t[16 * rt + c][16 * g], a);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 16; ++s) acc = mfma4(a[s], reg[s], acc);
  return acc;
}

// acc[db][r] (channel 16 db + 4 g + r, lane column c) += sum over the 16 rows of tile rt of T[row][channel] * x[row], where
// x = register r of lane (c, g) is row 4 g + r
__device__ __forceinline__ void accumulate_t(const float (*t)[LDT], int rt, int c, int g, const f32x4 x, f32x4 (&acc)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float *row = t[16 * rt + 4 * g + r];
#pragma unroll
    for (int db = 0; db < 4; ++db) acc[db] = mfma4(row[16 * db + c], x[r], acc[db]);
  }
}

// acc[db][r] * f -> 4 contiguous floats of row p at channels 16 db + 4 g
template <int VEC>
__device__ __forceinline__ void store_t(float *__restrict__ p, int g, const f32x4 (&acc)[4], float f, bool divide) {
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = divide ? acc[db][r] / f : acc[db][r] * f;
    float *d = p + 16 * db + 4 * g;
    if constexpr (VEC == 4) {
      stv<4>(d, v);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) d[r] = v[r];
    }
  }
}

__device__ __forceinline__ float group_max(float v) {  // over the four lanes (c, 0..3)
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

template <int VEC>
__global__ __launch_bounds__(AT) void attn_fwd_kernel(const float *__restrict__ qkv, int64_t ldq, int N, int H, int tiles, float scale,
                                                      float *__restrict__ out, int64_t ldo, float *__restrict__ lse) {
  __shared__ __attribute__((aligned(16))) float Ks[TR][LDT];
  __shared__ __attribute__((aligned(16))) float Vs[TR][LDT];
  const int bh = blockIdx.x / tiles, q0 = (blockIdx.x % tiles) * TR, b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const float *qb = qkv + (int64_t)b * N * ldq + h * HD, *kb = qb + H * HD, *vb = kb + H * HD;
  const int qrow = q0 + 16 * wave + c;
  float qr[16];
  load16<VEC>(qb + (int64_t)qrow * ldq + 16 * g, qrow < N, qr);
  f32x4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < N; k0 += TR) {
    __syncthreads();
    stage_tile<VEC>(Ks, kb, ldq, k0, N);
    stage_tile<VEC>(Vs, vb, ldq, k0, N);
    __syncthreads();
    f32x4 s[4];  // s[kt][r] = score of query c and key k0 + 16 kt + 4 g + r
    float tmax = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = dot_tile(Ks, kt, c, g, qr);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[kt][r] = k0 + 16 * kt + 4 * g + r < N ? s[kt][r] * scale : -INFINITY;
        tmax = fmaxf(tmax, s[kt][r]);
      }
    }
    const float mn = fmaxf(m, group_max(tmax));
    const float alpha = expf(m - mn);
    float psum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[kt][r] = expf(s[kt][r] - mn);
        psum += s[kt][r];
      }
    l = l * alpha + group_sum(psum);
    m = mn;
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] *= alpha;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) accumulate_t(Vs, kt, c, g, s[kt], o);
  }
  if (qrow < N) {
    store_t<VEC>(out + ((int64_t)b * N + qrow) * ldo + h * HD, g, o, l, true);
    if (g == 0) lse[(int64_t)bh * N + qrow] = m + logf(l);
  }
}

// delta[b][h][i] = sum_d dout * out over the head's 64 channels: 16 lanes per (row, head), 4 channels each
template <int VEC>
__global__ __launch_bounds__(AT) void attn_delta_kernel(const float *__restrict__ out, int64_t ldo, const float *__restrict__ dout,
                                                        int64_t lddo, int64_t rows, int N, int H, float *__restrict__ delta) {
  const int64_t total = rows * H;  // (b N + i) H + h
  const int sub = threadIdx.x & 15;
  // whole 16-lane groups stay together: the loop bound is the same for the 16 lanes of a group
  for (int64_t t = ((int64_t)blockIdx.x * AT + threadIdx.x) >> 4; t < total; t += ((int64_t)gridDim.x * AT) >> 4) {
    const int64_t row = t / H;
    const int h = (int)(t - row * H);
    float a[4], d[4];
    const float *pa = out + row * ldo + h * HD + 4 * sub, *pd = dout + row * lddo + h * HD + 4 * sub;
    if constexpr (VEC == 4) {
      ldv<4>(pa, a);
      ldv<4>(pd, d);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = pa[k], d[k] = pd[k];
    }
    float acc = a[0] * d[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) acc = fmaf(a[k], d[k], acc);
    acc += __shfl_xor(acc, 8);
    acc += __shfl_xor(acc, 4);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 1);
    if (sub == 0) {
      const int64_t b = row / N;
      delta[(b * H + h) * N + (row - b * N)] = acc;
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(AT) void attn_dq_kernel(const float *__restrict__ qkv, int64_t ldq, const float *__restrict__ lse,
                                                     const float *__restrict__ delta, const float *__restrict__ dout, int64_t lddo,
                                                     int N, int H, int tiles, float scale, float *__restrict__ dqkv, int64_t lddq) {
  __shared__ __attribute__((aligned(16))) float Ks[TR][LDT];
  __shared__ __attribute__((aligned(16))) float Vs[TR][LDT];
  const int bh = blockIdx.x / tiles, q0 = (blockIdx.x % tiles) * TR, b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const float *qb = qkv + (int64_t)b * N * ldq + h * HD, *kb = qb + H * HD, *vb = kb + H * HD;
  const int qrow = q0 + 16 * wave + c;
  const bool ok = qrow < N;
  float qr[16], dor[16];
  load16<VEC>(qb + (int64_t)qrow * ldq + 16 * g, ok, qr);
  load16<VEC>(dout + ((int64_t)b * N + qrow) * lddo + h * HD + 16 * g, ok, dor);
  const float lse_c = ok ? lse[(int64_t)bh * N + qrow] : 0.f, delta_c = ok ? delta[(int64_t)bh * N + qrow] : 0.f;
  f32x4 dq[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) dq[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < N; k0 += TR) {
    __syncthreads();
    stage_tile<VEC>(Ks, kb, ldq, k0, N);
    stage_tile<VEC>(Vs, vb, ldq, k0, N);
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const f32x4 s = dot_tile(Ks, kt, c, g, qr), dp = dot_tile(Vs, kt, c, g, dor);
      f32x4 ds;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ds[r] = k0 + 16 * kt + 4 * g + r < N ? expf(s[r] * scale - lse_c) * (dp[r] - delta_c) : 0.f;
      accumulate_t(Ks, kt, c, g, ds, dq);
    }
  }
  if (ok) store_t<VEC>(dqkv + ((int64_t)b * N + qrow) * lddq + h * HD, g, dq, scale, false);
}

template <int VEC>
__global__ __launch_bounds__(AT) void attn_dkv_kernel(const float *__restrict__ qkv, int64_t ldq, const float *__restrict__ lse,
                                                      const float *__restrict__ delta, const float *__restrict__ dout, int64_t lddo,
                                                      int N, int H, int tiles, float scale, float *__restrict__ dqkv, int64_t lddq) {
  __shared__ __attribute__((aligned(16))) float Qs[TR][LDT];
  __shared__ __attribute__((aligned(16))) float Gs[TR][LDT];  // dO
  __shared__ __attribute__((aligned(16))) float lse_s[TR];
  __shared__ __attribute__((aligned(16))) float delta_s[TR];
  const int bh = blockIdx.x / tiles, k0 = (blockIdx.x % tiles) * TR, b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const float *qb = qkv + (int64_t)b * N * ldq + h * HD, *kb = qb + H * HD, *vb = kb + H * HD;
  const float *gb = dout + (int64_t)b * N * lddo + h * HD;
  const int krow = k0 + 16 * wave + c;
  const bool ok = krow < N;
  float kr[16], vr[16];
  load16<VEC>(kb + (int64_t)krow * ldq + 16 * g, ok, kr);
  load16<VEC>(vb + (int64_t)krow * ldq + 16 * g, ok, vr);
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) dk[db] = dv[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < N; q0 += TR) {
    __syncthreads();
    stage_tile<VEC>(Qs, qb, ldq, q0, N);
    stage_tile<VEC>(Gs, gb, lddo, q0, N);
    if (threadIdx.x < TR) {
      const bool in = q0 + (int)threadIdx.x < N;
      lse_s[threadIdx.x] = in ? lse[(int64_t)bh * N + q0 + threadIdx.x] : 0.f;
      delta_s[threadIdx.x] = in ? delta[(int64_t)bh * N + q0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      // row 4 g + r of the results = query q0 + 16 qt + 4 g + r, the lane's column = key krow
      const f32x4 s = dot_tile(Qs, qt, c, g, kr), dp = dot_tile(Gs, qt, c, g, vr);
      f32x4 p, ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = 16 * qt + 4 * g + r;
        p[r] = q0 + qi < N ? expf(s[r] * scale - lse_s[qi]) : 0.f;
        ds[r] = p[r] * (dp[r] - delta_s[qi]);
      }
      accumulate_t(Gs, qt, c, g, p, dv);
      accumulate_t(Qs, qt, c, g, ds, dk);
    }
  }
  if (ok) {
    float *row = dqkv + ((int64_t)b * N + krow) * lddq + H * HD + h * HD;
    store_t<VEC>(row, g, dk, scale, false);
    store_t<VEC>(row + H * HD, g, dv, 1.f, false);
  }
}

}  // namespace
}  // namespace mink

using namespace mink;

// the shape checks every entry point shares; B H N < 2^31 keeps every row index and the grid inside an int
#define MINK_ATTN_REQUIRE_SHAPE(name, B, N, H, D)                                                                                  \
  do {                                                                                                                             \
    MINK_REQUIRE((D) == MINK_ATTN_HEAD_DIM, name ": D=%d channels per head (only D == %d is built)", (int)(D), MINK_ATTN_HEAD_DIM); \
    MINK_REQUIRE((N) >= 1 && (N) <= MINK_ATTN_MAX_TOKENS, name ": N=%lld tokens (1 <= N <= %d)", (long long)(N),                   \
                 MINK_ATTN_MAX_TOKENS);                                                                                            \
    MINK_REQUIRE((H) >= 1 && (H) <= MINK_ATTN_MAX_HEADS, name ": H=%d heads (1 <= H <= %d)", (int)(H), MINK_ATTN_MAX_HEADS);        \
    MINK_REQUIRE((B) >= 1 && (B) < (1LL << 31) && (int64_t)(B) * (H) * (N) < (1LL << 31) && (int64_t)(B) * (N) < (1LL << 31) / (3 * MINK_ATTN_HEAD_DIM), \
                 name ": B=%lld samples (B >= 1, B H N < 2^31, B N < 2^31 / 192)", (long long)(B));                                \
  } while (0)

extern "C" {

int64_t mink_attn_bwd_workspace_bytes(int64_t B, int64_t N, int32_t H, int32_t D) {
  (void)D;
  if (B < 1 || N < 1 || H < 1) return 0;
  return align_up(B * N * H * (int64_t)sizeof(float), 16);
}

int mink_attn_fwd(const float *qkv, int32_t ldq, int64_t B, int32_t N, int32_t H, int32_t D, float scale, float *out, int32_t ldo,
                  float *lse, void *stream) {
  MINK_ATTN_REQUIRE_SHAPE("attn_fwd", B, N, H, D);
  MINK_REQUIRE(ldq >= 3 * H * D, "attn_fwd: ldq=%d below the 3 H D = %d columns of a qkv row", ldq, 3 * H * D);
  MINK_REQUIRE(ldo >= H * D, "attn_fwd: ldo=%d below the H D = %d columns of an out row", ldo, H * D);
  MINK_REQUIRE(qkv && out && lse, "attn_fwd: NULL pointer (qkv, out, lse)");
  MINK_REQUIRE((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)lse) & 3) == 0, "attn_fwd: qkv, out and lse must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)cdiv(N, TR);
  const dim3 grid((unsigned)(B * H * tiles));
  const bool vec = aligned16(qkv) && aligned16(out) && (ldq & 3) == 0 && (ldo & 3) == 0;
  if (vec) attn_fwd_kernel<4><<<grid, AT, 0, st>>>(qkv, ldq, N, H, tiles, scale, out, ldo, lse);
  else attn_fwd_kernel<1><<<grid, AT, 0, st>>>(qkv, ldq, N, H, tiles, scale, out, ldo, lse);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_attn_bwd(const float *qkv, int32_t ldq, const float *out, int32_t ldo, const float *lse, const float *dout, int32_t lddo,
                  int64_t B, int32_t N, int32_t H, int32_t D, float scale, float *dqkv, int32_t lddq, void *workspace,
                  int64_t workspace_bytes, void *stream) {
  MINK_ATTN_REQUIRE_SHAPE("attn_bwd", B, N, H, D);
  MINK_REQUIRE(ldq >= 3 * H * D, "attn_bwd: ldq=%d below the 3 H D = %d columns of a qkv row", ldq, 3 * H * D);
  MINK_REQUIRE(lddq >= 3 * H * D, "attn_bwd: lddq=%d below the 3 H D = %d columns of a dqkv row", lddq, 3 * H * D);
  MINK_REQUIRE(ldo >= H * D, "attn_bwd: ldo=%d below the H D = %d columns of an out row", ldo, H * D);
  MINK_REQUIRE(lddo >= H * D, "attn_bwd: lddo=%d below the H D = %d columns of a dout row", lddo, H * D);
  MINK_REQUIRE(qkv && out && lse && dout && dqkv && workspace, "attn_bwd: NULL pointer (qkv, out, lse, dout, dqkv, workspace)");
  MINK_REQUIRE((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)lse | (uintptr_t)dout | (uintptr_t)dqkv) & 3) == 0,
               "attn_bwd: qkv, out, lse, dout and dqkv must be 4-byte aligned");
  MINK_REQUIRE_WORKSPACE("attn_bwd", workspace_bytes, mink_attn_bwd_workspace_bytes(B, N, H, D), workspace);
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)cdiv(N, TR);
  const dim3 grid((unsigned)(B * H * tiles));
  float *delta = (float *)workspace;  // [B][H][N]
  const int64_t rows = B * N;
  const dim3 dgrid(flat_grid(rows * H * 16, AT, 1 << 16));
  const bool vec = aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv) && (ldq & 3) == 0 && (ldo & 3) == 0 &&
                   (lddo & 3) == 0 && (lddq & 3) == 0;
  if (vec) {
    attn_delta_kernel<4><<<dgrid, AT, 0, st>>>(out, ldo, dout, lddo, rows, N, H, delta);
    attn_dkv_kernel<4><<<grid, AT, 0, st>>>(qkv, ldq, lse, delta, dout, lddo, N, H, tiles, scale, dqkv, lddq);
    attn_dq_kernel<4><<<grid, AT, 0, st>>>(qkv, ldq, lse, delta, dout, lddo, N, H, tiles, scale, dqkv, lddq);
  } else {
    attn_delta_kernel<1><<<dgrid, AT, 0, st>>>(out, ldo, dout, lddo, rows, N, H, delta);
    attn_dkv_kernel<1><<<grid, AT, 0, st>>>(qkv, ldq, lse, delta, dout, lddo, N, H, tiles, scale, dqkv, lddq);
    attn_dq_kernel<1><<<grid, AT, 0, st>>>(qkv, ldq, lse, delta, dout, lddo, N, H, tiles, scale, dqkv, lddq);
  }
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
