// Coordinate maps on gfx950: packed voxel keys, first-occurrence unique through a hash map, the coordinate pyramid (stride
// maps) and the batch offsets.  The neighbour tables built on these maps are in kmap.hip, their derived orders in rulebook.hip.
// HBM-bound integer work: one thread per row, coalesced 16-B row loads, hash probes served from L2 / Infinity Cache
// (table = 12 B per slot, 2-4x rows).  The exclusive scans every count -> scan -> fill scheme of these files goes through
// (launch_scan, launch_scan_batch) are defined here.
#include "coords_common.h"

namespace mink {

// ------------------------------------------------------------------------------ keys
// clear_keys / clear_vals (optional): the hash map these keys are about to be inserted into is emptied by the same launch
// (clear_cap slots, or the capacity for the device-resident row count) -- one launch per level less in the pyramid
template <int MODE>  // 0 = float field rows, 1 = int32 rows
__device__ __forceinline__ bool row_key(const void *__restrict__ coords, int64_t i, int out_ts, uint64_t &key) {
  int b, x, y, z;
  if (MODE == 0) {
    const float4 c = reinterpret_cast<const float4 *>(coords)[i];
    // the float-to-int conversion saturates and turns NaN into 0: NaN, +-inf and anything far outside the key space is
    // refused here, before it can come out of the conversion as a legal cell (the comparison is false for NaN)
    if (!(fabsf(c.x) < 65536.f && fabsf(c.y) < 65536.f && fabsf(c.z) < 65536.f && fabsf(c.w) < 65536.f)) {
      key = 0;
      return false;
    }
    b = (int)floorf(c.x), x = (int)floorf(c.y), y = (int)floorf(c.z), z = (int)floorf(c.w);
  } else {
    const int4 c = reinterpret_cast<const int4 *>(coords)[i];
    b = c.x, x = c.y, y = c.z, z = c.w;
  }
  if (out_ts > 1) x = floor_to(x, out_ts), y = floor_to(y, out_ts), z = floor_to(z, out_ts);
  return pack_key(b, x, y, z, key);
}

template <int MODE>
__device__ __forceinline__ void make_keys_body(const void *__restrict__ coords, int64_t n_host, const int *__restrict__ n_dev,
                                               int out_ts, uint64_t *__restrict__ keys, uint32_t *status,
                                               unsigned long long *__restrict__ clear_keys, int *__restrict__ clear_vals,
                                               uint64_t clear_cap, bool check_order = false) {
  const int64_t n = n_dev ? (int64_t)*n_dev : n_host;  // device-resident row count (level chains)
  if (clear_keys) {
    const uint64_t cap = n_dev ? table_capacity(n) : clear_cap;
    for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * kBlock) {
      clear_keys[s] = kEmptyKey;
      clear_vals[s] = 0x7F7F7F7F;
    }
  }
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint64_t key;
  if (!row_key<MODE>(coords, i, out_ts, key)) {
    atomicOr(status, MINK_STATUS_RANGE);
    key = 0;  // keep the pipeline well-defined; the host raises on the status word
  }
  keys[i] = key;
  if (check_order) {
    uint64_t before = 0;
    const bool bad = i > 0 && (!row_key<MODE>(coords, i - 1, out_ts, before) || before >= key);
    const unsigned long long m = __ballot(bad);
    if (bad && (threadIdx.x & 63) == __builtin_ctzll(m) &&
        !(__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & MINK_STATUS_NOT_ASCENDING))
      atomicOr(status, MINK_STATUS_NOT_ASCENDING);
  }
}
template <int MODE>
__global__ __launch_bounds__(kBlock) void make_keys_kernel(const void *__restrict__ coords, int64_t n_host,
                                                           const int *__restrict__ n_dev, int out_ts,
                                                           uint64_t *__restrict__ keys, uint32_t *status,
                                                           unsigned long long *__restrict__ clear_keys = nullptr,
                                                           int *__restrict__ clear_vals = nullptr, uint64_t clear_cap = 0,
                                                           bool check_order = false) {
  make_keys_body<MODE>(coords, n_host, n_dev, out_ts, keys, status, clear_keys, clear_vals, clear_cap, check_order);
}

// ---------------------------------------------------------------------------- unique
// Five passes: insert (insert_kernel, beside the block insert in kmap.hip: launch_insert), flag, scan, assign, inverse.
// flag first occurrences, count them per block
__global__ __launch_bounds__(kBlock) void flag_kernel(const int *__restrict__ tvals, const int *__restrict__ slot_of_row,
                                                      int64_t n_host, const int *__restrict__ n_dev,
                                                      uint8_t *__restrict__ flags, int *__restrict__ block_counts,
                                                      const uint32_t *__restrict__ asc_status) {
  __shared__ int s_cnt[kBlock / 64];
  const int64_t n = n_dev ? (int64_t)*n_dev : n_host;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool fast = asc_fast(asc_status);
  bool first = false;
  if (i < n) {
    first = fast || tvals[slot_of_row[i]] == (int)i;
    flags[i] = first;
  }
  const unsigned long long m = __ballot(first);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// single-workgroup exclusive scan of int32 (n up to a few 1e5); total -> *total_out.
// 256 threads x 16 consecutive items per trip: wave-level shuffles scan the per-thread sums.  (One wave per SIMD on
// purpose: a 1024-thread workgroup needs four free wave slots on EVERY SIMD of one CU at once, and beside a kernel that
// fills the register files -- the stem convolution runs while the next batch's maps are built -- it was seen waiting
// 590 us for that to happen.)
constexpr int kScanBlock = 256;
__device__ __forceinline__ void scan_body(const int *__restrict__ in, int *__restrict__ out, int64_t n, int *total_out) {
  constexpr int IT = 16;
  __shared__ int s_wave[kScanBlock / 64];
  __shared__ int s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t base = 0; base < n; base += kScanBlock * IT) {
    const int64_t i0 = base + (int64_t)threadIdx.x * IT;
    int v[IT], tsum = 0;
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      v[j] = (i0 + j < n) ? in[i0 + j] : 0;
      tsum += v[j];
    }
    int incl = tsum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kScanBlock / 64; ++w) {
      const int t = s_wave[w];
      if (w < wave) woff += t;
      total += t;
    }
    int run = s_carry + woff + incl - tsum;
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      if (i0 + j < n) out[i0 + j] = run;
      run += v[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) s_carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0 && total_out) *total_out = s_carry;
}
__global__ __launch_bounds__(kScanBlock) void scan_kernel(const int *__restrict__ in, int *__restrict__ out, int64_t n,
                                                          int *total_out) {
  scan_body(in, out, n, total_out);
}
__global__ __launch_bounds__(kScanBlock) void scan_batch_kernel(ScanBatch b) {  // one workgroup per array
  scan_body(b.in[blockIdx.x], b.out[blockIdx.x], b.n[blockIdx.x], b.total[blockIdx.x]);
}
int launch_scan(const int *in, int *out, int64_t n, int *total, hipStream_t st) {
  scan_kernel<<<1, kScanBlock, 0, st>>>(in, out, n, total);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}
int launch_scan_batch(const ScanBatch &b, int n, hipStream_t st) {
  scan_batch_kernel<<<dim3((unsigned)n), kScanBlock, 0, st>>>(b);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

__global__ __launch_bounds__(kBlock) void assign_kernel(const uint64_t *__restrict__ keys,
                                                        const uint8_t *__restrict__ flags,
                                                        const int *__restrict__ slot_of_row,
                                                        const int *__restrict__ block_offsets, int64_t n_host,
                                                        const int *__restrict__ n_dev, int *tvals,
                                                        int *__restrict__ out_coords, int *__restrict__ unique_index,
                                                        const uint32_t *__restrict__ asc_status) {
  __shared__ int s_cnt[kBlock / 64];
  const int64_t n = n_dev ? (int64_t)*n_dev : n_host;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool first = i < n && flags[i];
  const unsigned long long m = __ballot(first);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_cnt[wave] = __popcll(m);
  __syncthreads();
  if (first) {
    int uid = block_offsets[blockIdx.x] + wave_rank(m);
    for (int w = 0; w < wave; ++w) uid += s_cnt[w];
    if (unique_index) unique_index[uid] = (int)i;
    reinterpret_cast<int4 *>(out_coords)[uid] = unpack_key(keys[i]);
    if (!asc_fast(asc_status)) tvals[slot_of_row[i]] = uid;
  }
}

__global__ __launch_bounds__(kBlock) void inverse_kernel(const int *__restrict__ tvals,
                                                         const int *__restrict__ slot_of_row, int64_t n_host,
                                                         const int *__restrict__ n_dev, int *__restrict__ inverse,
                                                         const uint32_t *__restrict__ asc_status) {
  const int64_t n = n_dev ? (int64_t)*n_dev : n_host;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) inverse[i] = asc_fast(asc_status) ? (int)i : tvals[slot_of_row[i]];
}

// Level chains: the inverse map of level l and the keys of level l + 1 (made from level l's unique rows, with level l + 1's
// hash map emptied on the way) are independent row-parallel passes behind the same launch (assign of level l): one kernel.
// The last level's call carries the batch count instead (last_out).
__global__ __launch_bounds__(kBlock) void inverse_next_keys_kernel(const int *__restrict__ tvals, const int *__restrict__ slot_of_row,
                                                                   int64_t n_host, const int *__restrict__ n_dev,
                                                                   int *__restrict__ inverse, const void *__restrict__ next_coords,
                                                                   const int *__restrict__ next_n, int next_ts,
                                                                   uint64_t *__restrict__ keys, uint32_t *status,
                                                                   unsigned long long *__restrict__ next_tkeys,
                                                                   int *__restrict__ next_tvals, const int *__restrict__ coords0,
                                                                   const int *__restrict__ n0, int *last_out,
                                                                   const uint32_t *__restrict__ asc_status) {
  {
    const int64_t n = n_dev ? (int64_t)*n_dev : n_host;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) inverse[i] = asc_fast(asc_status) ? (int)i : tvals[slot_of_row[i]];
  }
  if (last_out && blockIdx.x == 0 && threadIdx.x == 0) {
    const int n = *n0;
    *last_out = n > 0 ? coords0[4 * (n - 1)] + 1 : 0;  // batch column is non-decreasing (checked by batch_offsets)
  }
  if (next_coords) make_keys_body<1>(next_coords, n_host, next_n, next_ts, keys, status, next_tkeys, next_tvals, 0);
}

__global__ void last_batch_kernel(const int *__restrict__ coords0, const int *__restrict__ n0, int *out) {
  const int n = *n0;
  *out = n > 0 ? coords0[4 * (n - 1)] + 1 : 0;  // batch column is non-decreasing (checked by batch_offsets)
}

// --------------------------------------------------------------------- batch offsets
__global__ __launch_bounds__(kBlock) void batch_offsets_kernel(const int *__restrict__ coords, int64_t n, int B,
                                                               int *__restrict__ batch_offsets, uint32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n && i > 0 && coords[4 * i] < coords[4 * (i - 1)]) atomicOr(status, MINK_STATUS_UNSORTED);
  if (i <= B) {  // lower_bound of batch index i
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (coords[4 * mid] < (int)i) lo = mid + 1;
      else hi = mid;
    }
    batch_offsets[i] = (int)lo;
  }
}

}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_table_capacity(int64_t n) { return (int64_t)table_capacity(n > 0 ? n : 0); }

static int64_t unique_nblocks(int64_t n) { return cdiv(n > 0 ? n : 1, kBlock); }

// enqueue the five kernels of insert_and_map; n_dev (optional) holds the row count on the device
static int unique_launch(const uint64_t *keys, int64_t n, const int *n_dev, uint64_t *table_keys, int32_t *table_vals,
                         int64_t cap, int32_t *out_coords, int32_t *unique_index, int32_t *inverse, int32_t *n_unique,
                         void *workspace, hipStream_t st, bool skip_inverse = false, const uint32_t *asc_status = nullptr) {
  const int64_t nb = unique_nblocks(n);
  char *ws = (char *)workspace;
  int *slot_of_row = (int *)ws;
  ws += align_up(4 * n, 256);
  uint8_t *flags = (uint8_t *)ws;
  ws += align_up(n, 256);
  int *block_counts = (int *)ws;
  ws += align_up(4 * nb, 256);
  int *block_offsets = (int *)ws;
  const dim3 grid((unsigned)nb);
  if (int rc = launch_insert(keys, n, n_dev, table_keys, table_vals, cap, slot_of_row, asc_status, st)) return rc;
  flag_kernel<<<grid, kBlock, 0, st>>>(table_vals, slot_of_row, n, n_dev, flags, block_counts, asc_status);
  MINK_CHECK_LAUNCH();
  if (int rc = launch_scan(block_counts, block_offsets, nb, n_unique, st)) return rc;
  assign_kernel<<<grid, kBlock, 0, st>>>(keys, flags, slot_of_row, block_offsets, n, n_dev, table_vals, out_coords,
                                         unique_index, asc_status);
  MINK_CHECK_LAUNCH();
  if (skip_inverse) return MINK_OK;  // (the caller fuses it with the next level's first pass)
  inverse_kernel<<<grid, kBlock, 0, st>>>(table_vals, slot_of_row, n, n_dev, inverse, asc_status);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int64_t mink_unique_workspace_bytes(int64_t n) {
  const int64_t nb = unique_nblocks(n);
  return align_up(4 * n, 256) + align_up(n, 256) + 2 * align_up(4 * nb, 256) + 256;
}

int mink_coords_make_keys(const void *coords, int mode, int64_t n, int32_t out_ts, uint64_t *keys, uint32_t *status,
                          void *stream) {
  MINK_REQUIRE(n >= 0 && out_ts >= 1 && (mode == 0 || mode == 1), "make_keys: bad arguments (n=%lld ts=%d mode=%d)",
               (long long)n, out_ts, mode);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(coords && keys && status, "make_keys: NULL pointer");
  MINK_REQUIRE(((uintptr_t)coords & 15) == 0, "make_keys: coords must be 16-byte aligned rows of 4");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(n, kBlock));
  if (mode == 0)
    make_keys_kernel<0><<<grid, kBlock, 0, st>>>(coords, n, nullptr, out_ts, keys, status);
  else
    make_keys_kernel<1><<<grid, kBlock, 0, st>>>(coords, n, nullptr, out_ts, keys, status);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_coords_unique(const uint64_t *keys, int64_t n, uint64_t *table_keys, int32_t *table_vals, int64_t cap,
                       int32_t *out_coords, int32_t *unique_index, int32_t *inverse, int32_t *n_unique,
                       void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(n >= 0 && n < (1ll << 31) - 1, "unique: n out of range");
  MINK_REQUIRE(cap >= mink_table_capacity(n) && (cap & (cap - 1)) == 0, "unique: table capacity %lld too small for n=%lld",
               (long long)cap, (long long)n);
  MINK_REQUIRE(table_keys && table_vals && n_unique, "unique: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  MINK_HIP(hipMemsetAsync(table_keys, 0xFF, cap * sizeof(uint64_t), st));
  MINK_HIP(hipMemsetAsync(table_vals, 0x7F, cap * sizeof(int32_t), st));
  if (n == 0) {
    MINK_HIP(hipMemsetAsync(n_unique, 0, sizeof(int32_t), st));
    return MINK_OK;
  }
  MINK_REQUIRE(keys && out_coords && unique_index && inverse && workspace, "unique: NULL pointer");
  MINK_REQUIRE(workspace_bytes >= mink_unique_workspace_bytes(n), "unique: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)(mink_unique_workspace_bytes(n)));
  MINK_REQUIRE(((uintptr_t)out_coords & 15) == 0 && ((uintptr_t)workspace & 255) == 0, "unique: misaligned buffer");
  int rc = unique_launch(keys, n, nullptr, table_keys, table_vals, cap, out_coords, unique_index, inverse, n_unique,
                         workspace, st);
  return rc;
}


/* ---- whole coordinate pyramid in one call ------------------------------------------------- */
int64_t mink_levels_workspace_bytes(int64_t n) { return align_up(8 * (n > 0 ? n : 1), 256) + mink_unique_workspace_bytes(n); }

int mink_coords_build_levels(const void *coords, int mode, int64_t n, int32_t nlev, const int32_t *out_ts_host,
                             uint64_t *const *table_keys, int32_t *const *table_vals, int64_t cap,
                             int32_t *const *out_coords, int32_t *const *index_a, int32_t *const *index_b,
                             int32_t *meta, void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(n >= 1 && n < (1ll << 31) - 1 && nlev >= 1 && nlev <= 16, "build_levels: bad sizes");
  MINK_REQUIRE(workspace_bytes >= mink_levels_workspace_bytes(n), "build_levels: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)(mink_levels_workspace_bytes(n)));
  MINK_REQUIRE(coords && out_ts_host && table_keys && table_vals && out_coords && index_a && index_b && meta && workspace,
               "build_levels: NULL pointer");
  MINK_REQUIRE(cap >= mink_table_capacity(n) && (cap & (cap - 1)) == 0, "build_levels: table capacity too small");
  MINK_REQUIRE(((uintptr_t)coords & 15) == 0 && ((uintptr_t)workspace & 255) == 0, "build_levels: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  uint64_t *keys = (uint64_t *)workspace;
  void *uws = (char *)workspace + align_up(8 * n, 256);
  uint32_t *status = (uint32_t *)(meta + nlev);
  MINK_HIP(hipMemsetAsync(meta, 0, sizeof(int32_t) * (nlev + 2), st));
  const dim3 grid((unsigned)cdiv(n, kBlock));
  const int *slot_of_row = (const int *)uws;  // (first region of the unique workspace: unique_launch)
  for (int l = 0; l < nlev; ++l) {
    MINK_REQUIRE(table_keys[l] && table_vals[l] && out_coords[l] && index_b[l] && (l > 0 || index_a[0]),
                 "build_levels: NULL level buffer");
    const void *src = l == 0 ? coords : (const void *)out_coords[l - 1];
    const int *n_dev = l == 0 ? nullptr : meta + (l - 1);
    if (l == 0) {
      // (the level's hash map is emptied by the same launch; levels > 0: by the fused pass at the end of the previous level)
      if (mode == 0)
        make_keys_kernel<0><<<grid, kBlock, 0, st>>>(src, n, n_dev, out_ts_host[l], keys, status, (unsigned long long *)table_keys[l],
                                                    table_vals[l], (uint64_t)cap, true);
      else
        make_keys_kernel<1><<<grid, kBlock, 0, st>>>(src, n, n_dev, out_ts_host[l], keys, status, (unsigned long long *)table_keys[l],
                                                    table_vals[l], (uint64_t)cap, true);
      MINK_CHECK_LAUNCH();
    }
    const uint32_t *asc = l == 0 ? status : nullptr;  // (strictly ascending input rows: level 0 without its hash insert)
    // index_a: first-occurrence rows (optional, kept for level 0), index_b: inverse / in2out
    int rc = unique_launch(keys, n, n_dev, table_keys[l], table_vals[l], cap, out_coords[l],
                           index_a[l], index_b[l], meta + l, uws, st, true, asc);
    if (rc) return rc;
    // inverse of this level + keys (and emptied hash map) of the next; the last level: + batch count
    // (meta[nlev] = status word, meta[nlev+1] = batch index of the last input row + 1)
    const bool last = l + 1 == nlev;
    inverse_next_keys_kernel<<<grid, kBlock, 0, st>>>(
        table_vals[l], slot_of_row, n, n_dev, index_b[l], last ? nullptr : (const void *)out_coords[l], last ? nullptr : meta + l,
        last ? 1 : out_ts_host[l + 1], keys, status, last ? nullptr : (unsigned long long *)table_keys[l + 1],
        last ? nullptr : table_vals[l + 1], (const int *)out_coords[0], meta, last ? meta + nlev + 1 : nullptr, asc);
    MINK_CHECK_LAUNCH();
  }
  return MINK_OK;
}

int mink_batch_offsets(const int32_t *coords, int64_t n, int32_t B, int32_t *batch_offsets, uint32_t *status,
                       void *stream) {
  MINK_REQUIRE(n >= 0 && B >= 0 && batch_offsets && status, "batch_offsets: bad arguments");
  MINK_REQUIRE(n == 0 || coords, "batch_offsets: NULL coords");
  const int64_t work = (n > B + 1) ? n : B + 1;
  batch_offsets_kernel<<<dim3((unsigned)cdiv(work, kBlock)), kBlock, 0, (hipStream_t)stream>>>(coords, n, B,
                                                                                              batch_offsets, status);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
