// Weight-sparse convolution, forward only (reference co3d_3d/src/models/mink/modules/sparse_conv.py: one `spmm` per kernel offset
// over the CSR of W[k]^T, driven from Python).  Here one launch forms, per output row r,
//
//   y[r][co] = bias[co] + sum over valid offsets k (ascending) with i = nbr[r][k] >= 0,
//                         of sum over the nonzeros (ci, v) of row co of W[k]^T (ci ascending):  x[i][ci] * v
//
// as one fp32 fma chain per output element, on the vector ALUs: only products with a stored weight are formed, so a pruned
// input channel is never read into a result (a NaN there does not reach y; the dense kernel multiplies it by zero).
//
// Geometry.  Lanes are output rows: a workgroup of WS_THREADS threads owns a tile of TR = 64 * RPL consecutive rows (RPL rows per
// lane, 1 or 4) and MINK_WSCONV_COUT_TILE output channels, WS_CPW per wave.  Per valid offset and per chunk of MINK_WSCONV_CHUNK
// input channels the tile's neighbour rows are gathered into LDS channel-major ([ci][row]; rows without a neighbour as zeros), by
// loads with lanes as rows, so the transposing store is conflict free without padding.  A wave then walks its output channels
// (static accumulator indices) and, inside, the channel's nonzeros of that chunk (a wave-uniform dynamic loop: column index and
// value come through the scalar cache, the weight is a scalar operand of the fma); one ds_read of RPL consecutive rows feeds RPL fmas.
// An offset none of whose tile rows has a neighbour is skipped.  No atomics, fixed order: two runs give the same bits.
#include "rowpass.h"

namespace mink {
namespace {

constexpr int WS_THREADS = 256;
constexpr int WS_WAVES = WS_THREADS / 64;
constexpr int WS_CHUNK = MINK_WSCONV_CHUNK;          // input channels staged in LDS at a time
constexpr int WS_COT = MINK_WSCONV_COUT_TILE;        // output channels of a workgroup
constexpr int WS_CPW = WS_COT / WS_WAVES;            // output channels of a wave (accumulators: WS_CPW * RPL registers)
static_assert(WS_CHUNK % 4 == 0 && WS_CPW % 4 == 0 && WS_COT % WS_WAVES == 0, "tile geometry");

template <int RPL>
struct Rows {
  float v[RPL];
};

// RPL consecutive rows of one staged channel: one ds_read_b32 / ds_read_b128
template <int RPL>
__device__ __forceinline__ Rows<RPL> lds_rows(const float *p) {
  Rows<RPL> r;
  if constexpr (RPL == 4) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < RPL; ++i) r.v[i] = p[i];
  }
  return r;
}

template <int RPL>
__global__ __launch_bounds__(WS_THREADS) void wsconv_fwd_kernel(
    const float *__restrict__ x, int64_t n_in, int ldx, int cin, const int *__restrict__ nbr, int64_t n_out, int K,
    const int *__restrict__ koffs, int n_valid, const int *__restrict__ rowptr, const int *__restrict__ cptr,
    const int *__restrict__ colidx, const float *__restrict__ vals, int nnz, bool vec_x, float *__restrict__ y, int ldy, int cout,
    const float *__restrict__ bias, bool vec_y) {
  constexpr int TR = 64 * RPL;
  __shared__ __attribute__((aligned(16))) float tile[WS_CHUNK * TR];  // [ci][row]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int co0 = blockIdx.y * WS_COT + wave * WS_CPW;  // this wave's first output channel
  const int nchunks = (cin + WS_CHUNK - 1) / WS_CHUNK;

  float acc[WS_CPW][RPL];
#pragma unroll
  for (int j = 0; j < WS_CPW; ++j) {
    const float b = (bias != nullptr && co0 + j < cout) ? bias[co0 + j] : 0.f;
#pragma unroll
    for (int r = 0; r < RPL; ++r) acc[j][r] = b;
  }

  // gather roles: thread -> (tile row grow, first 4-channel group gq, groups advance by GSTEP)
  const int grow = tid % TR;
  constexpr int GSTEP = WS_THREADS / TR;
  const int gq = tid / TR;
  const int64_t gr = row0 + grow;

  for (int vi = 0; vi < n_valid; ++vi) {
    const int k = koffs[vi];
    if ((unsigned)k >= (unsigned)K) continue;  // (uniform; never follows an offset outside the table)
    int src = -1;
    if (gr < n_out) src = nbr[gr * K + k];
    if ((int64_t)(unsigned)src >= n_in) src = -1;  // negative or outside x: contributes nothing, never followed
    if (!__syncthreads_or(src >= 0)) continue;     // no row of the tile has a neighbour at this offset
    const float *__restrict__ xr = x + (int64_t)(src < 0 ? 0 : src) * ldx;
    for (int ch = 0; ch < nchunks; ++ch) {
      const int c0 = ch * WS_CHUNK;
      const int cw = min(WS_CHUNK, cin - c0);  // channels of this chunk
      if (ch > 0) __syncthreads();             // the previous chunk has been read by every wave
      for (int q = gq; q * 4 < cw; q += GSTEP) {
        const int c = q * 4;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (src >= 0) {
          if (vec_x && c + 4 <= cw) {
            t = *reinterpret_cast<const float4 *>(xr + c0 + c);
          } else {  // dwords: an unaligned pointer or pitch, or the ragged tail (columns >= cin are never read)
            t.x = xr[c0 + c];
            if (c + 1 < cw) t.y = xr[c0 + c + 1];
            if (c + 2 < cw) t.z = xr[c0 + c + 2];
            if (c + 3 < cw) t.w = xr[c0 + c + 3];
          }
        }
        tile[(c + 0) * TR + grow] = t.x;
        tile[(c + 1) * TR + grow] = t.y;
        tile[(c + 2) * TR + grow] = t.z;
        tile[(c + 3) * TR + grow] = t.w;
      }
      __syncthreads();
      // row pointers of (offset vi, channel co) for this chunk: the CSR's own when the row is one chunk
      const int *__restrict__ ptr = nchunks == 1 ? rowptr + (int64_t)vi * (cout + 1) + co0
                                                 : cptr + ((int64_t)vi * cout + co0) * (nchunks + 1) + ch;
      const int pstep = nchunks == 1 ? 1 : nchunks + 1;
      const float *lrow = tile + lane * RPL;
#pragma unroll
      for (int j = 0; j < WS_CPW; ++j) {
        if (co0 + j < cout) {
          int p0 = ptr[(int64_t)j * pstep], p1 = nchunks == 1 ? ptr[j + 1] : ptr[(int64_t)j * pstep + 1];
          p0 = __builtin_amdgcn_readfirstlane(max(p0, 0));
          p1 = __builtin_amdgcn_readfirstlane(min(p1, nnz));
          int p = p0;
          for (; p + 4 <= p1; p += 4) {
            int ci[4];
            float w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              ci[u] = min((unsigned)(colidx[p + u] - c0), (unsigned)(WS_CHUNK - 1));  // (never outside the tile, whatever colidx holds)
              w[u] = vals[p + u];
            }
            Rows<RPL> xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[u] = lds_rows<RPL>(lrow + ci[u] * TR);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int r = 0; r < RPL; ++r) acc[j][r] = fmaf(xv[u].v[r], w[u], acc[j][r]);
          }
          for (; p < p1; ++p) {
            const int ci = min((unsigned)(colidx[p] - c0), (unsigned)(WS_CHUNK - 1));
            const float w = vals[p];
            const Rows<RPL> xv = lds_rows<RPL>(lrow + ci * TR);
#pragma unroll
            for (int r = 0; r < RPL; ++r) acc[j][r] = fmaf(xv.v[r], w, acc[j][r]);
          }
        }
      }
    }
    // (the next offset's __syncthreads_or stands between these reads and the next gather)
  }

  // epilogue: lane -> rows row0 + lane * RPL + r, channels co0 .. co0 + WS_CPW
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    const int64_t row = row0 + lane * RPL + r;
    if (row >= n_out) continue;
    float *__restrict__ yr = y + row * ldy + co0;
#pragma unroll
    for (int j = 0; j < WS_CPW; j += 4) {
      if (vec_y && co0 + j + 4 <= cout) {
        *reinterpret_cast<float4 *>(yr + j) = make_float4(acc[j][r], acc[j + 1][r], acc[j + 2][r], acc[j + 3][r]);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (co0 + j + u < cout) yr[j + u] = acc[j + u][r];
      }
    }
  }
}

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int mink_wsconv_fwd(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const int32_t *nbr, int64_t n_out, int32_t K,
                    const int32_t *koffs, int32_t n_valid, const int32_t *rowptr, const int32_t *cptr, const int32_t *colidx,
                    const float *vals, int64_t nnz, float *y, int32_t ldy, int32_t cout, const float *bias, void *stream) {
  MINK_REQUIRE(n_in >= 0 && n_out >= 0 && K >= 1 && cin >= 1 && cout >= 1, "wsconv_fwd: n_in=%lld n_out=%lld K=%d cin=%d cout=%d",
               (long long)n_in, (long long)n_out, K, cin, cout);
  MINK_REQUIRE(ldx >= cin && ldy >= cout, "wsconv_fwd: leading dimension below the channel count (ldx=%d cin=%d ldy=%d cout=%d)", ldx,
               cin, ldy, cout);
  MINK_REQUIRE(n_valid >= 0 && n_valid <= K, "wsconv_fwd: n_valid=%d outside [0, K=%d]", n_valid, K);
  MINK_REQUIRE(nnz >= 0 && nnz <= (int64_t)n_valid * cin * cout && nnz < (1ll << 31), "wsconv_fwd: nnz=%lld for n_valid=%d, cin=%d, cout=%d",
               (long long)nnz, n_valid, cin, cout);
  if (n_out == 0) return MINK_OK;
  const bool live = n_valid > 0 && nnz > 0;  // otherwise every row is bias or zero and no table is read
  MINK_REQUIRE(y, "wsconv_fwd: NULL y");
  MINK_REQUIRE(!live || (nbr && koffs && rowptr && colidx && vals && (x || n_in == 0)), "wsconv_fwd: NULL pointer");
  MINK_REQUIRE(!live || cin <= WS_CHUNK || cptr, "wsconv_fwd: cin=%d > MINK_WSCONV_CHUNK needs the per-chunk row pointers", cin);
  const int RPL = n_out >= MINK_WSCONV_WIDE_ROWS ? 4 : 1;
  const int64_t tiles = cdiv(n_out, 64 * RPL);
  MINK_REQUIRE(tiles < (1ll << 31) && cdiv(cout, WS_COT) <= 65535, "wsconv_fwd: n_out=%lld, cout=%d exceed the launch grid", (long long)n_out, cout);
  const bool vec_x = ldx % 4 == 0 && aligned16(x), vec_y = ldy % 4 == 0 && aligned16(y);
  const dim3 grid((unsigned)tiles, (unsigned)cdiv(cout, WS_COT));
  const int nv = live ? n_valid : 0;
#define CALL(R)                                                                                                                     \
  wsconv_fwd_kernel<R><<<grid, WS_THREADS, 0, (hipStream_t)stream>>>(x, n_in, ldx, cin, nbr, n_out, K, koffs, nv, rowptr, cptr, colidx, \
                                                                     vals, (int)nnz, vec_x, y, ldy, cout, bias, vec_y)
  if (RPL == 4) CALL(4);
  else CALL(1);
#undef CALL
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
