// The point stage of the point-based classifiers on gfx950: what happens on a TensorField before and after .sparse()
// (reference models/mink/fcnn.py:143-165, pointnet.py:100-109).  [ME-recall of the field's inverse mapping composed with the
// stride maps; parity unpinned: ME is absent.]  Conventions of pool.hip / interp.hip: fp32, row pitch arguments, 16-byte
// lanes where every pitch, width and pointer allows and dword lanes otherwise, no floating-point atomics, fixed summation
// order, -1 = absent, a device status word for range errors.
//
//   field_map        : one thread per field row (b, x, y, z): the row of the voxel of tensor stride ts that contains it,
//                      key = floor(floor(x) / ts) * ts per axis (integer floor, negative values included), one hash probe
//                      through pack_key / table_find of common.h -- the probe mink_interp_map_weight makes for its corners
//   field_gather_cat : y[i][off_s : off_s + C_s] = x_s[idx_s[i]][:] for up to 8 sources in one launch, one lane per column
//                      group of the CONCATENATED row, so ME.cat(y1.slice(x), ..., y4.slice(x)) writes every output row once
//                      and no [N, C_s] intermediate exists.  idx < 0 (or past the source) -> zeros in that source's columns.
//                      Its backward is mink_segment_sum per source over a column slice of dy (row pitch).
//   segment_mean     : mink_segment_mean (TensorField.sparse()) and mink_segment_sum (the backward of SparseTensor.slice()
//                      and of the gather above): one dword lane per output element, members added in input-row order.
//                      Outside the anonymous namespace, beside the other kernels of namespace mink proper.
//   segment_mean_bwd : dx[members[j]][:] = dy[u][:] / (seg[u + 1] - seg[u]) for j in segment u -- the backward of
//                      mink_segment_mean.  One lane per (member, column group): the segment of member j is found by a binary
//                      search in seg, so a voxel holding thousands of points costs no more than one holding one, and every
//                      input row is written exactly once.
#include <algorithm>

#include "ew_common.h"
#include "rowpass.h"

namespace mink {
namespace {

constexpr int FB = 256;       // threads per workgroup
constexpr int kMaxSrc = 8;    // sources of one gather-cat launch

struct CatSources {
  const float *x[kMaxSrc];
  const int32_t *idx[kMaxSrc];
  int64_t rows[kMaxSrc];
  int32_t ldx[kMaxSrc];
  int32_t off[kMaxSrc + 1];  // first column of every source in y; off[n_src] = the width of y
};

__global__ __launch_bounds__(FB) void field_map_kernel(const float4 *__restrict__ tfield, int64_t n, int ts,
                                                       const uint64_t *__restrict__ tkeys, const int32_t *__restrict__ tvals,
                                                       uint64_t mask, int64_t n_rows, int32_t *__restrict__ idx, uint32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (i >= n) return;
  const float4 q = tfield[i];
  int row = -1;
  if (!query_in_range(q)) {
    atomicOr(status, MINK_STATUS_RANGE);  // NaN / infinite / far outside the key space
  } else {
    const int b = (int)q.x;
    if (b >= 0 && b <= 65534) {  // (another batch index holds no voxel)
      uint64_t key;
      if (!pack_key(b, floor_to((int)floorf(q.y), ts), floor_to((int)floorf(q.z), ts), floor_to((int)floorf(q.w), ts), key)) {
        atomicOr(status, MINK_STATUS_RANGE);
      } else {
        row = table_find(tkeys, tvals, mask, key);
        if (row < 0 || row >= n_rows) row = -1;
      }
    }
  }
  idx[i] = row;
}

template <int VEC>
__global__ __launch_bounds__(FB) void field_gather_cat_kernel(const CatSources src, int n_src, int64_t n, float *__restrict__ y,
                                                              int ldy) {
  const int ncg = src.off[n_src] / VEC;
  const int64_t total = n * ncg;
  for (int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x; t < total; t += (int64_t)gridDim.x * FB) {
    const int64_t i = t / ncg;
    const int c = (int)(t - i * ncg) * VEC;
    // the source of column c: constant indices only, so the descriptor stays in scalar registers
    const float *x = src.x[0];
    const int32_t *ix = src.idx[0];
    int64_t rows = src.rows[0];
    int ldx = src.ldx[0], off = 0;
#pragma unroll
    for (int s = 1; s < kMaxSrc; ++s) {
      if (s < n_src && c >= src.off[s]) x = src.x[s], ix = src.idx[s], rows = src.rows[s], ldx = src.ldx[s], off = src.off[s];
    }
    const int r = ix[i];
    float v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = 0.f;
    if (r >= 0 && r < rows) ldv<VEC>(x + (int64_t)r * ldx + (c - off), v);
    stv<VEC>(y + i * ldy + c, v);
  }
}

template <int VEC>
__global__ __launch_bounds__(FB) void segment_mean_bwd_kernel(const float *__restrict__ dy, int ldy, int C,
                                                              const int32_t *__restrict__ members, const int32_t *__restrict__ seg,
                                                              int64_t n_out, int64_t n_members, int64_t n_in, float *__restrict__ dx,
                                                              int lddx) {
  const int ncg = C / VEC;
  const int64_t total = n_members * ncg;
  for (int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x; t < total; t += (int64_t)gridDim.x * FB) {
    const int64_t j = t / ncg;
    const int c = (int)(t - j * ncg) * VEC;
    const int r = members[j];
    if (r < 0 || r >= n_in) continue;
    int64_t lo = 0, hi = n_out;  // the last u with seg[u] <= j
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (seg[mid] <= j) lo = mid;
      else hi = mid;
    }
    const int cnt = seg[lo + 1] - seg[lo];
    if (j < seg[lo] || cnt <= 0 || j >= seg[lo + 1]) continue;  // (a member behind the last segment belongs to none)
    const float d = (float)cnt;
    float g[VEC];
    ldv<VEC>(dy + lo * ldy + c, g);
#pragma unroll
    for (int k = 0; k < VEC; ++k) g[k] = g[k] / d;
    stv<VEC>(dx + (int64_t)r * lddx + c, g);
  }
}

}  // namespace

// MEAN: TensorField.sparse(); !MEAN (the plain sum, same member order): the backward of SparseTensor.slice()
template <bool MEAN>
__global__ __launch_bounds__(EB) void segment_mean_kernel(const float *__restrict__ x, int ldx, int C,
                                                          const int *__restrict__ members,
                                                          const int *__restrict__ seg, int64_t n_out,
                                                          float *__restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (idx >= n_out * C) return;
  const int64_t u = idx / C;
  const int c = (int)(idx - u * C);
  const int beg = seg[u], end = seg[u + 1];
  float s = 0.f;
  for (int j = beg; j < end; ++j) s += x[(int64_t)members[j] * ldx + c];  // input-row order
  y[idx] = MEAN ? s / (float)(end - beg) : s;
}

}  // namespace mink

using namespace mink;

extern "C" {

int mink_field_map(const float *tfield, int64_t n, int32_t ts, const uint64_t *table_keys, const int32_t *table_vals, int64_t cap,
                   int64_t n_rows, int32_t *idx, uint32_t *status, void *stream) {
  MINK_REQUIRE(n >= 0 && n <= 0x0fffffffLL && ts >= 1 && ts <= 32768 && n_rows >= 0, "field_map: bad arguments (n=%lld ts=%d rows=%lld)",
               (long long)n, ts, (long long)n_rows);
  MINK_REQUIRE(cap >= 64 && (cap & (cap - 1)) == 0, "field_map: table capacity %lld is not a power of two >= 64", (long long)cap);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(tfield && table_keys && table_vals && idx && status, "field_map: NULL pointer");
  MINK_REQUIRE(aligned16(tfield), "field_map: tfield must be 16-byte aligned rows of 4");
  field_map_kernel<<<dim3((unsigned)cdiv(n, FB)), FB, 0, (hipStream_t)stream>>>((const float4 *)tfield, n, ts, table_keys, table_vals,
                                                                              (uint64_t)cap - 1, n_rows, idx, status);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_field_gather_cat(int32_t n_src, const float *const *x, const int32_t *ldx, const int64_t *rows, const int32_t *C,
                          const int32_t *const *idx, int64_t n, float *y, int32_t ldy, void *stream) {
  MINK_REQUIRE(n_src >= 1 && n_src <= kMaxSrc, "field_gather_cat: %d sources (1 <= sources <= %d)", n_src, kMaxSrc);
  MINK_REQUIRE(n >= 0 && n <= 0x0fffffffLL && x && ldx && rows && C && idx, "field_gather_cat: bad arguments (n=%lld)", (long long)n);
  CatSources src;
  int64_t width = 0;
  bool vec = aligned16(y) && (ldy & 3) == 0;
  for (int s = 0; s < kMaxSrc; ++s) {
    const int k = s < n_src ? s : 0;  // (unused slots repeat source 0: never selected, never NULL)
    MINK_REQUIRE(C[k] >= 1 && C[k] <= 4096 && ldx[k] >= C[k] && rows[k] >= 0 && rows[k] <= 0x0fffffffLL,
                 "field_gather_cat: source %d: bad shape (C=%d, ldx=%d, rows=%lld; 1 <= C <= 4096)", k, C[k], ldx[k], (long long)rows[k]);
    MINK_REQUIRE(n == 0 || (idx[k] && (rows[k] == 0 || x[k])), "field_gather_cat: source %d: NULL pointer", k);
    src.x[s] = x[k], src.idx[s] = idx[k], src.rows[s] = rows[k], src.ldx[s] = ldx[k];
    if (s < n_src) {
      src.off[s] = (int32_t)width;
      width += C[k];
      vec = vec && (C[k] & 3) == 0 && (ldx[k] & 3) == 0 && aligned16(x[k]);
    }
  }
  for (int s = n_src; s <= kMaxSrc; ++s) src.off[s] = (int32_t)width;
  MINK_REQUIRE(width <= 32768 && ldy >= width, "field_gather_cat: %lld columns in all, ldy=%d (at most 32768, ldy >= the sum)",
               (long long)width, ldy);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(y, "field_gather_cat: NULL output");
  hipStream_t st = (hipStream_t)stream;
  if (vec) field_gather_cat_kernel<4><<<dim3(flat_grid(n * (width / 4), FB, 1 << 16)), FB, 0, st>>>(src, n_src, n, y, ldy);
  else field_gather_cat_kernel<1><<<dim3(flat_grid(n * width, FB, 1 << 16)), FB, 0, st>>>(src, n_src, n, y, ldy);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_segment_mean_bwd(const float *dy, int32_t ldy, int32_t C, const int32_t *members, const int32_t *seg, int64_t n_out,
                          int64_t n_members, int64_t n_in, float *dx, int32_t lddx, void *stream) {
  MINK_REQUIRE(C >= 1 && C <= 4096 && ldy >= C && lddx >= C, "segment_mean_bwd: bad shape (C=%d, ldy=%d, lddx=%d; 1 <= C <= 4096)", C, ldy,
               lddx);
  MINK_REQUIRE(n_out >= 0 && n_out <= 0x0fffffffLL && n_members >= 0 && n_members <= 0x0fffffffLL && n_in >= 0 && n_in <= 0x0fffffffLL,
               "segment_mean_bwd: bad row counts (segments=%lld, members=%lld, rows=%lld)", (long long)n_out, (long long)n_members,
               (long long)n_in);
  if (n_out == 0 || n_members == 0 || n_in == 0) return MINK_OK;
  MINK_REQUIRE(dy && members && seg && dx, "segment_mean_bwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C & 3) == 0 && (ldy & 3) == 0 && (lddx & 3) == 0 && aligned16(dy) && aligned16(dx);
  const dim3 grid(flat_grid(n_members * (vec ? C / 4 : C), FB, 1 << 16));
  if (vec) segment_mean_bwd_kernel<4><<<grid, FB, 0, st>>>(dy, ldy, C, members, seg, n_out, n_members, n_in, dx, lddx);
  else segment_mean_bwd_kernel<1><<<grid, FB, 0, st>>>(dy, ldy, C, members, seg, n_out, n_members, n_in, dx, lddx);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_segment_mean(const float *x, int32_t ldx, int32_t C, const int32_t *members, const int32_t *seg,
                      int64_t n_out, float *y, void *stream) {
  MINK_REQUIRE(C >= 1 && ldx >= C && n_out >= 0, "segment_mean: bad shape");
  if (n_out == 0) return MINK_OK;
  MINK_REQUIRE(x && members && seg && y, "segment_mean: NULL pointer");
  segment_mean_kernel<true><<<dim3((unsigned)cdiv(n_out * C, EB)), EB, 0, (hipStream_t)stream>>>(x, ldx, C, members, seg,
                                                                                                n_out, y);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_segment_sum(const float *x, int32_t ldx, int32_t C, const int32_t *members, const int32_t *seg,
                     int64_t n_out, float *y, void *stream) {
  MINK_REQUIRE(C >= 1 && ldx >= C && n_out >= 0, "segment_sum: bad shape");
  if (n_out == 0) return MINK_OK;
  MINK_REQUIRE(x && members && seg && y, "segment_sum: NULL pointer");
  segment_mean_kernel<false><<<dim3((unsigned)cdiv(n_out * C, EB)), EB, 0, (hipStream_t)stream>>>(x, ldx, C, members, seg,
                                                                                                 n_out, y);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
