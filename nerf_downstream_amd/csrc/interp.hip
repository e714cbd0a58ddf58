// Trilinear interpolation and its transpose, splat, for sparse tensors on gfx950 (ME.MinkowskiInterpolation,
// TensorField.splat).  [ME-recall of interpolation_map_weight / TensorField.splat; parity unpinned: ME is absent.]
//
// A query (b, x, y, z) in fp32 is read against a coordinate map of tensor stride ts.  Per axis lo = floor(x / ts) * ts with
// lo <= x < lo + ts enforced by exact comparisons (the fp32 quotient may land one cell off), r = x - lo, d = r / ts; corner c
// (bit 0 = x, bit 1 = y, bit 2 = z) sits at lo + ts with factor d where its bit is set and at lo with factor 1 - d where it
// is clear; its weight is (fx * fy) * fz.  r is exact in fp32 unless x is a tiny negative number next to a much larger cell
// origin (x = -1e-10, lo = -1), where it takes one rounding.  A corner absent from the map contributes nothing.
//
//   interp_map_weight : one thread per (query, corner) -- one hash probe each -- fills imap[n][8] (row of the corner, -1
//                       where absent) and w[n][8]
//   splat_coords      : one thread per (point, corner) writes the [8n][4] int32 corner rows of floor(coords) (and w)
//   interp_gather     : y[q] = sum_c w[q][c] * x[imap[q][c]], c ascending; row lanes as in pool.hip (16 bytes when C % 4 == 0)
//   interp_segsum     : dx[i] = sum over the pairs (q, c) with imap[q][c] = i of w[q][c] * dy[q], over a CSR of the pairs
//                       grouped by target row (seg[n_rows + 1], members[P] = q * 8 + c ascending inside a segment)
// The last two serve all four directions: interpolation forward / splat backward gather, interpolation backward / splat
// forward sum segments.  Both are HBM gathers of rows.  No floating-point atomics: a segment is owned by one team of threads,
// lane (rl, cl) takes the pairs rl, rl + rlanes, ... of column group cl in order and the row lanes are combined in order, so
// two runs are bitwise equal.  A segment may hold thousands of pairs (many points in one cell): segments of up to kLongSeg
// pairs go to one wave each, longer ones to a whole workgroup in a second launch (each launch skips the other's rows).
#include <algorithm>

#include "rowpass.h"

namespace mink {
namespace {

constexpr int IB = 256;          // threads per workgroup
constexpr int kLongSeg = 256;    // pairs (four waves' worth); longer segments take a workgroup instead of a wave
constexpr int kColLanes = 16;    // column groups a team reads side by side (the rest of the team are row lanes)

// one axis: cell origin (an integer, exact in fp32 for |x| < 65536) and the upper corner's factor
__device__ __forceinline__ void cell_axis(float x, float ts, int &lo_i, float &d) {
  float lo = floorf(x / ts) * ts;
  if (lo > x) lo -= ts;
  else if (x >= lo + ts) lo += ts;
  lo_i = (int)lo;
  d = (x - lo) / ts;
}

// query row -> batch index, corner coordinates and weight of corner c.  false: NaN / infinite / far outside the key space
__device__ __forceinline__ bool query_corner(const float4 q, int ts, int c, int &b, int &cx, int &cy, int &cz, float &w) {
  if (!query_in_range(q)) return false;
  const float fts = (float)ts;
  float dx, dy, dz;
  cell_axis(q.y, fts, cx, dx);
  cell_axis(q.z, fts, cy, dy);
  cell_axis(q.w, fts, cz, dz);
  b = (int)q.x;
  if (c & 1) cx += ts; else dx = 1.f - dx;
  if (c & 2) cy += ts; else dy = 1.f - dy;
  if (c & 4) cz += ts; else dz = 1.f - dz;
  w = (dx * dy) * dz;
  return true;
}

__global__ __launch_bounds__(IB) void interp_map_weight_kernel(const float4 *__restrict__ tfield, int64_t n, int ts,
                                                               const uint64_t *__restrict__ tkeys, const int32_t *__restrict__ tvals,
                                                               uint64_t mask, int64_t n_rows, int32_t *__restrict__ imap,
                                                               float *__restrict__ w, uint32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * IB + threadIdx.x;
  if (i >= 8 * n) return;
  int b, cx, cy, cz, row = -1;
  float wt = 0.f;
  uint64_t key;
  if (!query_corner(tfield[i >> 3], ts, (int)(i & 7), b, cx, cy, cz, wt)) {
    atomicOr(status, MINK_STATUS_RANGE);
    wt = 0.f;
  } else if (b >= 0 && b <= 65534) {  // (another batch index holds no voxel: a zero row)
    if (!pack_key(b, cx, cy, cz, key)) {
      atomicOr(status, MINK_STATUS_RANGE);
    } else {
      row = table_find(tkeys, tvals, mask, key);
      if (row < 0 || row >= n_rows) row = -1;
    }
  }
  imap[i] = row;
  w[i] = wt;
}

__global__ __launch_bounds__(IB) void splat_coords_kernel(const float4 *__restrict__ tfield, int64_t n, int4 *__restrict__ corners,
                                                          float *__restrict__ w, uint32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * IB + threadIdx.x;
  if (i >= 8 * n) return;
  int b = 0, cx = 0, cy = 0, cz = 0;
  float wt = 0.f;
  uint64_t key;
  if (!query_corner(tfield[i >> 3], 1, (int)(i & 7), b, cx, cy, cz, wt) || !pack_key(b, cx, cy, cz, key)) {
    atomicOr(status, MINK_STATUS_RANGE);
    b = cx = cy = cz = 0, wt = 0.f;  // keep the map build well-defined; the host raises on the status word
  }
  corners[i] = make_int4(b, cx, cy, cz);
  if (w) w[i] = wt;
}

template <int VEC>
__global__ __launch_bounds__(IB) void interp_gather_kernel(const float *__restrict__ x, int ldx, int64_t n_x, int C,
                                                           const int32_t *__restrict__ imap, const float *__restrict__ w,
                                                           int64_t n_q, float *__restrict__ y) {
  const int ncg = C / VEC;
  const int64_t total = n_q * ncg;
  for (int64_t idx = (int64_t)blockIdx.x * IB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * IB) {
    const int64_t q = idx / ncg;
    const int c = (int)(idx - q * ncg) * VEC;
    float s[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = imap[q * 8 + k];
      if (i >= 0 && i < n_x) {
        const float wt = w[q * 8 + k];
        float v[VEC];
        ldv<VEC>(x + (int64_t)i * ldx + c, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] = fmaf(wt, v[j], s[j]);
      }
    }
    stv<VEC>(y + q * C + c, s);
  }
}

// TEAM threads own one target row: TEAM == 64 takes the segments of up to kLongSeg pairs, TEAM == IB the longer ones.
// tprb = min(C / VEC, kColLanes) column lanes, TEAM / tprb row lanes; wider rows are walked in slabs of tprb column groups.
template <int VEC, int TEAM>
__global__ __launch_bounds__(IB) void interp_segsum_kernel(const float *__restrict__ dy, int ldy, int64_t n_q, int C,
                                                           const float *__restrict__ w, const int32_t *__restrict__ members,
                                                           const int32_t *__restrict__ seg, int64_t n_rows, int64_t P, int tprb,
                                                           float *__restrict__ dx) {
  __shared__ float s_red[IB * VEC];
  constexpr int TEAMS = IB / TEAM;
  const int team = threadIdx.x / TEAM, tl = threadIdx.x % TEAM;
  const int ncg = C / VEC, rlanes = TEAM / tprb, W = tprb * VEC;
  const int cl = tl % tprb, rl = tl / tprb;
  float *s_team = s_red + team * TEAM * VEC;
  for (int64_t base = (int64_t)blockIdx.x * TEAMS; base < n_rows; base += (int64_t)gridDim.x * TEAMS) {  // (uniform per workgroup)
    const int64_t row = base + team;
    int64_t j0 = 0, j1 = 0;
    if (row < n_rows) {
      j0 = seg[row], j1 = seg[row + 1];
      j0 = j0 < 0 ? 0 : (j0 > P ? P : j0);
      j1 = j1 < j0 ? j0 : (j1 > P ? P : j1);
    }
    const bool mine = row < n_rows && ((j1 - j0 > kLongSeg) == (TEAM == IB));
    if (TEAM == IB && !mine) continue;  // (one team per workgroup: uniform)
    for (int slab = 0; slab * tprb < ncg; ++slab) {
      const int cg = slab * tprb + cl;
      float s[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) s[k] = 0.f;
      if (mine && rl < rlanes && cg < ncg) {
        for (int64_t j = j0 + rl; j < j1; j += rlanes) {
          const int p = members[j];
          const int64_t q = p >> 3;
          if (p < 0 || q >= n_q) continue;
          const float wt = w[p];
          float g[VEC];
          ldv<VEC>(dy + q * ldy + cg * VEC, g);
#pragma unroll
          for (int k = 0; k < VEC; ++k) s[k] = fmaf(wt, g[k], s[k]);
        }
      }
      if (rl < rlanes) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) s_team[rl * W + cl * VEC + k] = s[k];
      }
      __syncthreads();
      if (mine) {
        for (int e = tl; e < W; e += TEAM) {
          const int c = slab * W + e;
          if (c >= C) continue;
          float t = 0.f;
          for (int r = 0; r < rlanes; ++r) t += s_team[r * W + e];
          dx[row * C + c] = t;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int mink_interp_map_weight(const float *tfield, int64_t n, int32_t ts, const uint64_t *table_keys, const int32_t *table_vals,
                           int64_t cap, int64_t n_rows, int32_t *imap, float *w, uint32_t *status, void *stream) {
  MINK_REQUIRE(n >= 0 && n <= 0x0fffffffLL && ts >= 1 && ts <= 32768 && n_rows >= 0,
               "interp_map_weight: bad arguments (n=%lld ts=%d rows=%lld)", (long long)n, ts, (long long)n_rows);
  MINK_REQUIRE(cap >= 64 && (cap & (cap - 1)) == 0, "interp_map_weight: table capacity %lld is not a power of two >= 64", (long long)cap);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(tfield && table_keys && table_vals && imap && w && status, "interp_map_weight: NULL pointer");
  MINK_REQUIRE(aligned16(tfield), "interp_map_weight: tfield must be 16-byte aligned rows of 4");
  interp_map_weight_kernel<<<dim3((unsigned)cdiv(8 * n, IB)), IB, 0, (hipStream_t)stream>>>(
      (const float4 *)tfield, n, ts, table_keys, table_vals, (uint64_t)cap - 1, n_rows, imap, w, status);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_splat_coords(const float *tfield, int64_t n, int32_t *corners, float *w, uint32_t *status, void *stream) {
  MINK_REQUIRE(n >= 0 && n <= 0x0fffffffLL, "splat_coords: bad row count %lld", (long long)n);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(tfield && corners && status, "splat_coords: NULL pointer");
  MINK_REQUIRE(aligned16(tfield) && aligned16(corners), "splat_coords: tfield and corners must be 16-byte aligned rows of 4");
  splat_coords_kernel<<<dim3((unsigned)cdiv(8 * n, IB)), IB, 0, (hipStream_t)stream>>>((const float4 *)tfield, n, (int4 *)corners, w,
                                                                                     status);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_interp_gather(const float *x, int32_t ldx, int64_t n_x, int32_t C, const int32_t *imap, const float *w, int64_t n_q,
                       float *y, void *stream) {
  MINK_REQUIRE_ROWS_C("interp_gather", n_q, 0x0fffffffLL, C);
  MINK_REQUIRE(ldx >= C && n_x >= 0, "interp_gather: bad arguments (ldx=%d, rows of x=%lld)", ldx, (long long)n_x);
  if (n_q == 0) return MINK_OK;
  MINK_REQUIRE(imap && w && y && (n_x == 0 || x), "interp_gather: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C & 3) == 0 && (ldx & 3) == 0 && aligned16(x) && aligned16(y);
  if (vec) interp_gather_kernel<4><<<dim3(flat_grid(n_q * (C / 4), IB, 1 << 16)), IB, 0, st>>>(x, ldx, n_x, C, imap, w, n_q, y);
  else interp_gather_kernel<1><<<dim3(flat_grid(n_q * C, IB, 1 << 16)), IB, 0, st>>>(x, ldx, n_x, C, imap, w, n_q, y);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_interp_segsum(const float *dy, int32_t ldy, int64_t n_q, int32_t C, const float *w, const int32_t *members,
                       const int32_t *seg, int64_t n_rows, int64_t n_pairs, float *dx, void *stream) {
  MINK_REQUIRE_ROWS_C("interp_segsum", n_rows, 0x0fffffffLL, C);
  MINK_REQUIRE(ldy >= C && n_q >= 0 && n_q <= 0x0fffffffLL && n_pairs >= 0 && n_pairs <= 8 * n_q,
               "interp_segsum: bad arguments (ldy=%d, queries=%lld, pairs=%lld)", ldy, (long long)n_q, (long long)n_pairs);
  if (n_rows == 0) return MINK_OK;
  MINK_REQUIRE(seg && dx && (n_pairs == 0 || (dy && w && members)), "interp_segsum: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C & 3) == 0 && (ldy & 3) == 0 && aligned16(dy) && aligned16(dx);
  const int tprb = std::min(vec ? C / 4 : C, kColLanes);
  const dim3 gw(flat_grid(n_rows, IB / 64, 1 << 16)), gl(flat_grid(n_rows, 8, 1 << 16));
  if (vec) {
    interp_segsum_kernel<4, 64><<<gw, IB, 0, st>>>(dy, ldy, n_q, C, w, members, seg, n_rows, n_pairs, tprb, dx);
    MINK_CHECK_LAUNCH();
    if (n_pairs > kLongSeg) interp_segsum_kernel<4, IB><<<gl, IB, 0, st>>>(dy, ldy, n_q, C, w, members, seg, n_rows, n_pairs, tprb, dx);
  } else {
    interp_segsum_kernel<1, 64><<<gw, IB, 0, st>>>(dy, ldy, n_q, C, w, members, seg, n_rows, n_pairs, tprb, dx);
    MINK_CHECK_LAUNCH();
    if (n_pairs > kLongSeg) interp_segsum_kernel<1, IB><<<gl, IB, 0, st>>>(dy, ldy, n_q, C, w, members, seg, n_rows, n_pairs, tprb, dx);
  }
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
