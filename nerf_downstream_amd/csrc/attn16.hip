// Multi-head self-attention on gfx950 with bf16 rows (the mixed-precision form of attn.hip): qkv, out, dout and dqkv are bf16 on
// the row layout of attn.hip (qkv[B N][ldq] holds q | k | v of token row b N + t at columns s H D + h D + d, out[B N][ldo] holds
// head h at columns h D + d, pitches in elements), lse and delta [B][H][N] are fp32.  D = 64.  No N x N matrix reaches memory.
//
// The arithmetic contract (include/mink_hip.h states it word for word): every product runs on v_mfma_f32_16x16x32_bf16 with fp32
// accumulation, everything else is fp32 except the roundings F1 (the weights as the operand of P V), F2 (the stored out), B1
// (P as the operand of dV), B2 (dS as the operand of dQ and dK) and B3 (the stored dqkv).
//
// Lane l of a wave is (c, g) = (l & 15, l >> 4).  The instruction takes A[i = c][k = 8 g + j] and B[k = 8 g + j][j' = c] in
// element j = 0..7 of a lane's fragment and returns D[i = 4 g + r][j' = c] in register r: the C/D map of the fp32 16x16x4 form,
// so the structure of attn.hip carries over:
//   - a dot product over the 64 head channels is two k-steps; lane group g takes channels 32 s + 8 g .. + 7 of step s, 16
//     contiguous bytes of a row-major LDS tile (A) or of a global row kept in registers (B);
//   - a result tile D is the B operand of the next product when that product sums over D's ROW index.  One k-step of 32 spans
//     two 16-row result tiles: the lane's four registers of the first tile and of the second, rounded to bf16, are elements
//     0..3 and 4..7, so element j of lane group g is row 16 (j >> 2) + 4 g + (j & 3) of the 32-row pair.  The A operand must
//     visit k in that same permuted order.  It is read from a TRANSPOSED LDS image T[channel][position] in which row
//     32 p + 16 a + 4 g + b of the tile sits at position 32 p + 8 g + 4 a + b (perm() below): the lane's eight operands are
//     again 16 contiguous bytes.  The image is written while the tile is staged, 2 bytes at a time.
//
//   attn16_fwd  : workgroup = 64 queries of one (b, h), wave = 16 of them; K (row-major) and V (transposed) pass through LDS 64
//                 keys at a time.  S^T = K Q^T, online softmax with the row statistics on the lane, O^T += V^T P^T.
//   attn16_delta: delta[b][h][i] = sum_d dO out, fp32 (16 lanes per row, fixed order) into the workspace.
//   attn16_dkv  : workgroup = 64 keys, wave = 16 of them with their K and V rows in registers; Q and dO pass through LDS 64
//                 queries at a time, row-major and transposed.  S = Q K^T, dP = dO V^T, dV^T += dO^T P, dK^T += Q^T dS.
//   attn16_dq   : the forward's structure: S^T = K Q^T, dP^T = V dO^T, dQ^T += K^T dS^T (K row-major and transposed).
// Every element of out, dq, dk and dv has one owner that sums in a fixed order and stores once: no atomics, two runs give the
// same bits.  Keys and queries past N are staged as zeros and masked by a select (never by a product with 0).
//
// 16-byte global loads and 8-byte stores when every matrix pointer is 16-byte aligned and every pitch a multiple of 8 elements,
// 2-byte accesses otherwise; the arithmetic is the same, so are the bits.
#include <math.h>

#include "rowpass.h"

namespace mink {
namespace {

constexpr int AT = 256;  // threads per workgroup: 4 waves, 16 rows of the 64-row tile each
constexpr int TR = 64;   // rows of a tile (queries or keys)
constexpr int HD = MINK_ATTN_HEAD_DIM;
constexpr int LDB = 72;  // LDS row pitch in bf16 elements: 144 bytes, 16-byte aligned rows
static_assert(HD == 64 && TR == 64 && AT == 256, "the lane maps below are written for 64 x 64 tiles and four waves");

using u16 = unsigned short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

__device__ __forceinline__ f32x4 mfma32(uint4 a, uint4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ u16 to_bf16(float a) { return __builtin_bit_cast(u16, (__bf16)a); }  // round to nearest even
__device__ __forceinline__ float from_bf16(u16 a) { return __builtin_bit_cast(float, (unsigned)a << 16); }
__device__ __forceinline__ unsigned pack2(float a, float b) { return (unsigned)to_bf16(a) | ((unsigned)to_bf16(b) << 16); }

// the fragment of one 32-row k-step from the two result tiles that span it
__device__ __forceinline__ uint4 pack_pair(const f32x4 lo, const f32x4 hi) {
  return make_uint4(pack2(lo[0], lo[1]), pack2(lo[2], lo[3]), pack2(hi[0], hi[1]), pack2(hi[2], hi[3]));
}

// 8 contiguous bf16 of a global row, zeros when the row does not exist
template <int VEC>
__device__ __forceinline__ uint4 load8(const u16 *__restrict__ p, bool ok) {
  uint4 u = make_uint4(0u, 0u, 0u, 0u);
  if (ok) {
    if constexpr (VEC == 8) {
      u = *reinterpret_cast<const uint4 *>(p);
    } else {
      u.x = (unsigned)p[0] | ((unsigned)p[1] << 16);
      u.y = (unsigned)p[2] | ((unsigned)p[3] << 16);
      u.z = (unsigned)p[4] | ((unsigned)p[5] << 16);
      u.w = (unsigned)p[6] | ((unsigned)p[7] << 16);
    }
  }
  return u;
}

// where row r of a 64-row tile sits in a row of the transposed image
__device__ __forceinline__ int perm(int r) { return (r & 32) | ((r & 12) << 1) | ((r & 16) >> 2) | (r & 3); }

// rows [r0, r0 + 64) x 64 columns at `base` (row 0 of the sample, first column of the head) -> R[row][column] and / or
// T[column][perm(row)] (either may be NULL); rows from N on are zeros.  A lane owns one row, a wave one group of 8 columns.
template <int VEC>
__device__ __forceinline__ void stage_tile(u16 (*R)[LDB], u16 (*T)[LDB], const u16 *__restrict__ base, int64_t ld, int r0, int N) {
  for (int e = threadIdx.x; e < TR * (HD / 8); e += AT) {
    const int r = e & (TR - 1), c = (e / TR) * 8;
    const uint4 u = load8<VEC>(base + (int64_t)(r0 + r) * ld + c, r0 + r < N);
    if (R) *reinterpret_cast<uint4 *>(&R[r][c]) = u;
    if (T) {
      const int pos = perm(r);
      T[c + 0][pos] = (u16)u.x, T[c + 1][pos] = (u16)(u.x >> 16);
      T[c + 2][pos] = (u16)u.y, T[c + 3][pos] = (u16)(u.y >> 16);
      T[c + 4][pos] = (u16)u.z, T[c + 5][pos] = (u16)(u.z >> 16);
      T[c + 6][pos] = (u16)u.w, T[c + 7][pos] = (u16)(u.w >> 16);
    }
  }
}

__device__ __forceinline__ uint4 lds8(const u16 *p) { return *reinterpret_cast<const uint4 *>(p); }  // (always 16-byte aligned)

// D[4 g + r][c] = sum_d R[16 rt + .][d] * reg[d]: the tile's rows on the result's rows, the register operand's row on the lane
__device__ __forceinline__ f32x4 dot_tile(const u16 (*R)[LDB], int rt, int c, int g, const uint4 (&reg)[2]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = mfma32(lds8(&R[16 * rt + c][32 * s + 8 * g]), reg[s], acc);
  return acc;
}

// acc[db][r] (channel 16 db + 4 g + r, lane column c) += sum over the 32 rows of pair p of the tile behind T of
// tile[row][channel] * x[row], x = pack_pair() of the two result tiles of that pair
__device__ __forceinline__ void accumulate_t(const u16 (*T)[LDB], int p, int c, int g, const uint4 x, f32x4 (&acc)[4]) {
#pragma unroll
  for (int db = 0; db < 4; ++db) acc[db] = mfma32(lds8(&T[16 * db + c][32 * p + 8 * g]), x, acc[db]);
}

// bf16(acc[db][r] * f) or bf16(acc[db][r] / f) -> 4 contiguous elements of row p at channels 16 db + 4 g
template <int VEC>
__device__ __forceinline__ void store_t(u16 *__restrict__ p, int g, const f32x4 (&acc)[4], float f, bool divide) {
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = divide ? acc[db][r] / f : acc[db][r] * f;
    u16 *d = p + 16 * db + 4 * g;
    if constexpr (VEC == 8) {
      *reinterpret_cast<uint2 *>(d) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) d[r] = to_bf16(v[r]);
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
__global__ __launch_bounds__(AT) void attn16_fwd_kernel(const u16 *__restrict__ qkv, int64_t ldq, int N, int H, int tiles, float scale,
                                                        u16 *__restrict__ out, int64_t ldo, float *__restrict__ lse) {
  __shared__ __attribute__((aligned(16))) u16 Ks[TR][LDB];
  __shared__ __attribute__((aligned(16))) u16 Vt[HD][LDB];
  const int bh = blockIdx.x / tiles, q0 = (blockIdx.x % tiles) * TR, b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const u16 *qb = qkv + (int64_t)b * N * ldq + h * HD, *kb = qb + H * HD, *vb = kb + H * HD;
  const int qrow = q0 + 16 * wave + c;
  uint4 qr[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) qr[s] = load8<VEC>(qb + (int64_t)qrow * ldq + 32 * s + 8 * g, qrow < N);
  f32x4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < N; k0 += TR) {
    __syncthreads();
    stage_tile<VEC>(Ks, nullptr, kb, ldq, k0, N);
    stage_tile<VEC>(nullptr, Vt, vb, ldq, k0, N);
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
        psum += s[kt][r];  // the unrounded weight: l and lse do not see F1
      }
    l = l * alpha + group_sum(psum);
    m = mn;
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] *= alpha;
#pragma unroll
    for (int p = 0; p < 2; ++p) accumulate_t(Vt, p, c, g, pack_pair(s[2 * p], s[2 * p + 1]), o);  // F1
  }
  if (qrow < N) {
    store_t<VEC>(out + ((int64_t)b * N + qrow) * ldo + h * HD, g, o, l, true);  // F2
    if (g == 0) lse[(int64_t)bh * N + qrow] = m + logf(l);
  }
}

// delta[b][h][i] = sum_d dout * out over the head's 64 channels, fp32: 16 lanes per (row, head), 4 channels each
template <int VEC>
__global__ __launch_bounds__(AT) void attn16_delta_kernel(const u16 *__restrict__ out, int64_t ldo, const u16 *__restrict__ dout,
                                                          int64_t lddo, int64_t rows, int N, int H, float *__restrict__ delta) {
  const int64_t total = rows * H;  // (b N + i) H + h
  const int sub = threadIdx.x & 15;
  // whole 16-lane groups stay together: the loop bound is the same for the 16 lanes of a group
  for (int64_t t = ((int64_t)blockIdx.x * AT + threadIdx.x) >> 4; t < total; t += ((int64_t)gridDim.x * AT) >> 4) {
    const int64_t row = t / H;
    const int h = (int)(t - row * H);
    float a[4], d[4];
    const u16 *pa = out + row * ldo + h * HD + 4 * sub, *pd = dout + row * lddo + h * HD + 4 * sub;
    if constexpr (VEC == 8) {
      const uint2 ua = *reinterpret_cast<const uint2 *>(pa), ud = *reinterpret_cast<const uint2 *>(pd);
      a[0] = from_bf16((u16)ua.x), a[1] = from_bf16((u16)(ua.x >> 16)), a[2] = from_bf16((u16)ua.y), a[3] = from_bf16((u16)(ua.y >> 16));
      d[0] = from_bf16((u16)ud.x), d[1] = from_bf16((u16)(ud.x >> 16)), d[2] = from_bf16((u16)ud.y), d[3] = from_bf16((u16)(ud.y >> 16));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = from_bf16(pa[k]), d[k] = from_bf16(pd[k]);
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
__global__ __launch_bounds__(AT) void attn16_dq_kernel(const u16 *__restrict__ qkv, int64_t ldq, const float *__restrict__ lse,
                                                       const float *__restrict__ delta, const u16 *__restrict__ dout, int64_t lddo,
                                                       int N, int H, int tiles, float scale, u16 *__restrict__ dqkv, int64_t lddq) {
  __shared__ __attribute__((aligned(16))) u16 Ks[TR][LDB];
  __shared__ __attribute__((aligned(16))) u16 Vs[TR][LDB];
  __shared__ __attribute__((aligned(16))) u16 Kt[HD][LDB];
  const int bh = blockIdx.x / tiles, q0 = (blockIdx.x % tiles) * TR, b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const u16 *qb = qkv + (int64_t)b * N * ldq + h * HD, *kb = qb + H * HD, *vb = kb + H * HD;
  const int qrow = q0 + 16 * wave + c;
  const bool ok = qrow < N;
  uint4 qr[2], dor[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    qr[s] = load8<VEC>(qb + (int64_t)qrow * ldq + 32 * s + 8 * g, ok);
    dor[s] = load8<VEC>(dout + ((int64_t)b * N + qrow) * lddo + h * HD + 32 * s + 8 * g, ok);
  }
  const float lse_c = ok ? lse[(int64_t)bh * N + qrow] : 0.f, delta_c = ok ? delta[(int64_t)bh * N + qrow] : 0.f;
  f32x4 dq[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) dq[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < N; k0 += TR) {
    __syncthreads();
    stage_tile<VEC>(Ks, Kt, kb, ldq, k0, N);
    stage_tile<VEC>(Vs, nullptr, vb, ldq, k0, N);
    __syncthreads();
    f32x4 ds[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const f32x4 s = dot_tile(Ks, kt, c, g, qr), dp = dot_tile(Vs, kt, c, g, dor);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ds[kt][r] = k0 + 16 * kt + 4 * g + r < N ? expf(s[r] * scale - lse_c) * (dp[r] - delta_c) : 0.f;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) accumulate_t(Kt, p, c, g, pack_pair(ds[2 * p], ds[2 * p + 1]), dq);  // B2
  }
  if (ok) store_t<VEC>(dqkv + ((int64_t)b * N + qrow) * lddq + h * HD, g, dq, scale, false);  // B3
}

template <int VEC>
__global__ __launch_bounds__(AT) void attn16_dkv_kernel(const u16 *__restrict__ qkv, int64_t ldq, const float *__restrict__ lse,
                                                        const float *__restrict__ delta, const u16 *__restrict__ dout, int64_t lddo,
                                                        int N, int H, int tiles, float scale, u16 *__restrict__ dqkv, int64_t lddq) {
  __shared__ __attribute__((aligned(16))) u16 Qs[TR][LDB];
  __shared__ __attribute__((aligned(16))) u16 Gs[TR][LDB];  // dO
  __shared__ __attribute__((aligned(16))) u16 Qt[HD][LDB];
  __shared__ __attribute__((aligned(16))) u16 Gt[HD][LDB];
  __shared__ __attribute__((aligned(16))) float lse_s[TR];
  __shared__ __attribute__((aligned(16))) float delta_s[TR];
  const int bh = blockIdx.x / tiles, k0 = (blockIdx.x % tiles) * TR, b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const u16 *qb = qkv + (int64_t)b * N * ldq + h * HD, *kb = qb + H * HD, *vb = kb + H * HD;
  const u16 *gb = dout + (int64_t)b * N * lddo + h * HD;
  const int krow = k0 + 16 * wave + c;
  const bool ok = krow < N;
  uint4 kr[2], vr[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    kr[s] = load8<VEC>(kb + (int64_t)krow * ldq + 32 * s + 8 * g, ok);
    vr[s] = load8<VEC>(vb + (int64_t)krow * ldq + 32 * s + 8 * g, ok);
  }
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) dk[db] = dv[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < N; q0 += TR) {
    __syncthreads();
    stage_tile<VEC>(Qs, Qt, qb, ldq, q0, N);
    stage_tile<VEC>(Gs, Gt, gb, lddo, q0, N);
    if (threadIdx.x < TR) {
      const bool in = q0 + (int)threadIdx.x < N;
      lse_s[threadIdx.x] = in ? lse[(int64_t)bh * N + q0 + threadIdx.x] : 0.f;
      delta_s[threadIdx.x] = in ? delta[(int64_t)bh * N + q0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    f32x4 p[4], ds[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      // row 4 g + r of the results = query q0 + 16 qt + 4 g + r, the lane's column = key krow
      const f32x4 s = dot_tile(Qs, qt, c, g, kr), dp = dot_tile(Gs, qt, c, g, vr);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = 16 * qt + 4 * g + r;
        const bool in = q0 + qi < N;
        p[qt][r] = in ? expf(s[r] * scale - lse_s[qi]) : 0.f;
        ds[qt][r] = in ? p[qt][r] * (dp[r] - delta_s[qi]) : 0.f;
      }
    }
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      accumulate_t(Gt, pp, c, g, pack_pair(p[2 * pp], p[2 * pp + 1]), dv);    // B1
      accumulate_t(Qt, pp, c, g, pack_pair(ds[2 * pp], ds[2 * pp + 1]), dk);  // B2
    }
  }
  if (ok) {
    u16 *row = dqkv + ((int64_t)b * N + krow) * lddq + H * HD + h * HD;
    store_t<VEC>(row, g, dk, scale, false);          // B3
    store_t<VEC>(row + H * HD, g, dv, 1.f, false);   // B3
  }
}

}  // namespace
}  // namespace mink

using namespace mink;

// the shape checks every entry point shares (those of attn.hip); B H N < 2^31 keeps every row index and the grid inside an int
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

int64_t mink_attn_bwd_b16_workspace_bytes(int64_t B, int64_t N, int32_t H, int32_t D) {
  (void)D;
  if (B < 1 || N < 1 || H < 1) return 0;
  return align_up(B * N * H * (int64_t)sizeof(float), 16);
}

int mink_attn_fwd_b16(const void *qkv, int32_t ldq, int64_t B, int32_t N, int32_t H, int32_t D, float scale, void *out, int32_t ldo,
                      float *lse, void *stream) {
  MINK_ATTN_REQUIRE_SHAPE("attn_fwd_b16", B, N, H, D);
  MINK_REQUIRE(ldq >= 3 * H * D, "attn_fwd_b16: ldq=%d below the 3 H D = %d columns of a qkv row", ldq, 3 * H * D);
  MINK_REQUIRE(ldo >= H * D, "attn_fwd_b16: ldo=%d below the H D = %d columns of an out row", ldo, H * D);
  MINK_REQUIRE(qkv && out && lse, "attn_fwd_b16: NULL pointer (qkv, out, lse)");
  MINK_REQUIRE((((uintptr_t)qkv | (uintptr_t)out) & 1) == 0, "attn_fwd_b16: qkv and out (bf16) must be 2-byte aligned");
  MINK_REQUIRE(((uintptr_t)lse & 3) == 0, "attn_fwd_b16: lse must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)cdiv(N, TR);
  const dim3 grid((unsigned)(B * H * tiles));
  const u16 *x = (const u16 *)qkv;
  u16 *y = (u16 *)out;
  const bool vec = aligned16(qkv) && aligned16(out) && (ldq & 7) == 0 && (ldo & 7) == 0;
  if (vec) attn16_fwd_kernel<8><<<grid, AT, 0, st>>>(x, ldq, N, H, tiles, scale, y, ldo, lse);
  else attn16_fwd_kernel<1><<<grid, AT, 0, st>>>(x, ldq, N, H, tiles, scale, y, ldo, lse);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_attn_bwd_b16(const void *qkv, int32_t ldq, const void *out, int32_t ldo, const float *lse, const void *dout, int32_t lddo,
                      int64_t B, int32_t N, int32_t H, int32_t D, float scale, void *dqkv, int32_t lddq, void *workspace,
                      int64_t workspace_bytes, void *stream) {
  MINK_ATTN_REQUIRE_SHAPE("attn_bwd_b16", B, N, H, D);
  MINK_REQUIRE(ldq >= 3 * H * D, "attn_bwd_b16: ldq=%d below the 3 H D = %d columns of a qkv row", ldq, 3 * H * D);
  MINK_REQUIRE(lddq >= 3 * H * D, "attn_bwd_b16: lddq=%d below the 3 H D = %d columns of a dqkv row", lddq, 3 * H * D);
  MINK_REQUIRE(ldo >= H * D, "attn_bwd_b16: ldo=%d below the H D = %d columns of an out row", ldo, H * D);
  MINK_REQUIRE(lddo >= H * D, "attn_bwd_b16: lddo=%d below the H D = %d columns of a dout row", lddo, H * D);
  MINK_REQUIRE(qkv && out && lse && dout && dqkv && workspace, "attn_bwd_b16: NULL pointer (qkv, out, lse, dout, dqkv, workspace)");
  MINK_REQUIRE((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dqkv) & 1) == 0,
               "attn_bwd_b16: qkv, out, dout and dqkv (bf16) must be 2-byte aligned");
  MINK_REQUIRE(((uintptr_t)lse & 3) == 0, "attn_bwd_b16: lse must be 4-byte aligned");
  MINK_REQUIRE_WORKSPACE("attn_bwd_b16", workspace_bytes, mink_attn_bwd_b16_workspace_bytes(B, N, H, D), workspace);
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)cdiv(N, TR);
  const dim3 grid((unsigned)(B * H * tiles));
  float *delta = (float *)workspace;  // [B][H][N]
  const int64_t rows = B * N;
  const dim3 dgrid(flat_grid(rows * H * 16, AT, 1 << 16));
  const u16 *x = (const u16 *)qkv, *o = (const u16 *)out, *g = (const u16 *)dout;
  u16 *dx = (u16 *)dqkv;
  const bool vec = aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv) && (ldq & 7) == 0 && (ldo & 7) == 0 &&
                   (lddo & 7) == 0 && (lddq & 7) == 0;
  if (vec) {
    attn16_delta_kernel<8><<<dgrid, AT, 0, st>>>(o, ldo, g, lddo, rows, N, H, delta);
    attn16_dkv_kernel<8><<<grid, AT, 0, st>>>(x, ldq, lse, delta, g, lddo, N, H, tiles, scale, dx, lddq);
    attn16_dq_kernel<8><<<grid, AT, 0, st>>>(x, ldq, lse, delta, g, lddo, N, H, tiles, scale, dx, lddq);
  } else {
    attn16_delta_kernel<1><<<dgrid, AT, 0, st>>>(o, ldo, g, lddo, rows, N, H, delta);
    attn16_dkv_kernel<1><<<grid, AT, 0, st>>>(x, ldq, lse, delta, g, lddo, N, H, tiles, scale, dx, lddq);
    attn16_dq_kernel<1><<<grid, AT, 0, st>>>(x, ldq, lse, delta, g, lddo, N, H, tiles, scale, dx, lddq);
  }
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
