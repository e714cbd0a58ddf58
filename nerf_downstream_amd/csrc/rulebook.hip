// Derived orders of a neighbour table or a map on gfx950: the ME-format rulebook (wave64 ballot + prefix sums) and the
// parity-class permutation.  Both count per 256-row chunk, scan the counts (launch_scan: coords.hip) and fill.
#include <algorithm>

#include "coords_common.h"

namespace mink {

// Workspace of a count -> scan -> fill scheme over n rows and `columns` counters per 256-row chunk (K offsets for the
// rulebook, 8 classes for the partition): counts | offsets, each rounded up to 256 bytes, and the total in the trailing
// 256-byte pad, right behind the offsets.
struct ChunkWs {
  int *counts, *offsets, *total;
  int64_t nchunk;
};
static int64_t chunk_ws_bytes(int64_t n, int columns) {
  return 2 * align_up(4 * cdiv(n > 0 ? n : 1, kBlock) * columns, 256) + 256;
}
static ChunkWs chunk_ws(void *workspace, int64_t n, int columns) {
  const int64_t nchunk = cdiv(n, kBlock);
  int *offsets = (int *)((char *)workspace + align_up(4 * nchunk * columns, 256));
  return {(int *)workspace, offsets, offsets + nchunk * columns, nchunk};
}

// -------------------------------------------------------------------------- rulebook
// Pass 1: pairs per (offset, 256-row chunk); pass 2 (after the scan): fill, ordered by row.
template <bool FILL>
__global__ __launch_bounds__(kBlock) void rulebook_kernel(const int *__restrict__ nbr, int64_t n_out, int K,
                                                          int64_t nchunk, int *__restrict__ chunk_counts,
                                                          const int *__restrict__ chunk_offsets,
                                                          int *__restrict__ pairs_in, int *__restrict__ pairs_out) {
  __shared__ int s_cnt[kBlock / 64][27];
  const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = 0; k < K; ++k) {
    const int v = o < n_out ? nbr[o * K + k] : -1;
    const unsigned long long m = __ballot(v >= 0);
    if (lane == 0) s_cnt[wave][k] = __popcll(m);
    if (FILL) {
      __syncthreads();
      if (v >= 0) {
        int pos = chunk_offsets[(int64_t)k * nchunk + blockIdx.x] + wave_rank(m);
        for (int w = 0; w < wave; ++w) pos += s_cnt[w][k];
        pairs_in[pos] = v;
        pairs_out[pos] = (int)o;
      }
    }
  }
  if (!FILL) {
    __syncthreads();
    if (threadIdx.x < K)
      chunk_counts[(int64_t)threadIdx.x * nchunk + blockIdx.x] =
          s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
  }
}

__global__ void rulebook_counts_kernel(const int *__restrict__ chunk_offsets, int64_t nchunk, int K,
                                       const int *__restrict__ total, int *__restrict__ counts) {
  const int k = threadIdx.x;
  if (k < K) counts[k] = chunk_offsets[(int64_t)k * nchunk];
  if (k == K) counts[K] = *total;
}

// ------------------------------------------------------------------- parity classes
// Rows of a stride-ts map grouped by the parity of (c / ts) per axis (8 classes).  For the
// dgrad of a stride-2 convolution every row of one class can only be reached through the same
// 2^p kernel offsets, so class-pure 128-row tiles skip the other offsets entirely.
// Same count -> scan -> fill scheme as the rulebook; each class segment starts at a multiple of
// `pad` rows in the output permutation (pre-filled with -1).
__device__ __forceinline__ int parity_class(int4 c, int ts) {
  return ((c.y / ts) & 1) | (((c.z / ts) & 1) << 1) | (((c.w / ts) & 1) << 2);
}

template <bool FILL>
__device__ __forceinline__ void class_partition_body(const int *__restrict__ coords, int64_t n, int ts, int64_t nchunk, int pad,
                                                     int *__restrict__ chunk_counts, const int *__restrict__ chunk_offsets,
                                                     const int *__restrict__ total, int *__restrict__ perm) {
  __shared__ int s_cnt[kBlock / 64][8];
  __shared__ int s_shift[8];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cls = i < n ? parity_class(reinterpret_cast<const int4 *>(coords)[i], ts) : -1;
  if (FILL && threadIdx.x == 0) {  // padding inserted in front of each class segment
    int shift = 0;
    for (int c = 0; c < 8; ++c) {
      s_shift[c] = shift;
      const int beg = chunk_offsets[(int64_t)c * nchunk];
      const int end = c < 7 ? chunk_offsets[(int64_t)(c + 1) * nchunk] : *total;
      const int cnt = end - beg;
      shift += (cnt + pad - 1) / pad * pad - cnt;
    }
  }
  int my_rank = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const unsigned long long m = __ballot(cls == c);
    if (lane == 0) s_cnt[wave][c] = __popcll(m);
    if (cls == c) my_rank = wave_rank(m);
  }
  __syncthreads();
  if (FILL) {
    if (cls >= 0) {
      int pos = chunk_offsets[(int64_t)cls * nchunk + blockIdx.x] + s_shift[cls] + my_rank;
      for (int w = 0; w < wave; ++w) pos += s_cnt[w][cls];
      perm[pos] = (int)i;
    }
  } else if (threadIdx.x < 8) {
    chunk_counts[(int64_t)threadIdx.x * nchunk + blockIdx.x] =
        s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
  }
}

template <bool FILL>
__global__ __launch_bounds__(kBlock) void class_partition_kernel(const int *__restrict__ coords, int64_t n, int ts,
                                                                 int64_t nchunk, int pad,
                                                                 int *__restrict__ chunk_counts,
                                                                 const int *__restrict__ chunk_offsets,
                                                                 const int *__restrict__ total, int *__restrict__ perm) {
  class_partition_body<FILL>(coords, n, ts, nchunk, pad, chunk_counts, chunk_offsets, total, perm);
}
struct ClassPart {
  const int *coords;
  int64_t n, nchunk;
  int *chunk_counts, *chunk_offsets, *total, *perm;
  int ts, pad;
};
struct ClassPartBatch {
  ClassPart e[8];
};
template <bool FILL>
__global__ __launch_bounds__(kBlock) void class_partition_batch_kernel(ClassPartBatch b) {  // blockIdx.y = map
  const ClassPart &e = b.e[blockIdx.y];
  if ((int64_t)blockIdx.x >= e.nchunk) return;
  class_partition_body<FILL>(e.coords, e.n, e.ts, e.nchunk, e.pad, e.chunk_counts, e.chunk_offsets, e.total, e.perm);
}

}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_rulebook_workspace_bytes(int64_t n_out, int32_t K) { return chunk_ws_bytes(n_out, K); }

int mink_rulebook(const int32_t *nbr, int64_t n_out, int32_t K, int32_t *counts, int32_t *pairs_in,
                  int32_t *pairs_out, void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(K >= 1 && K <= 27 && n_out >= 0 && counts, "rulebook: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (n_out == 0) {
    MINK_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (K + 1), st));
    return MINK_OK;
  }
  MINK_REQUIRE(nbr && workspace && ((uintptr_t)workspace & 255) == 0, "rulebook: NULL/misaligned pointer");
  MINK_REQUIRE(workspace_bytes >= mink_rulebook_workspace_bytes(n_out, K), "rulebook: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)(mink_rulebook_workspace_bytes(n_out, K)));
  const ChunkWs w = chunk_ws(workspace, n_out, K);
  const dim3 grid((unsigned)w.nchunk);
  rulebook_kernel<false><<<grid, kBlock, 0, st>>>(nbr, n_out, K, w.nchunk, w.counts, nullptr, nullptr, nullptr);
  MINK_CHECK_LAUNCH();
  if (int rc = launch_scan(w.counts, w.offsets, w.nchunk * K, w.total, st)) return rc;
  rulebook_counts_kernel<<<1, 64, 0, st>>>(w.offsets, w.nchunk, K, w.total, counts);
  MINK_CHECK_LAUNCH();
  if (pairs_in && pairs_out) {
    rulebook_kernel<true><<<grid, kBlock, 0, st>>>(nbr, n_out, K, w.nchunk, nullptr, w.offsets, pairs_in, pairs_out);
    MINK_CHECK_LAUNCH();
  }
  return MINK_OK;
}

int64_t mink_class_partition_rows(int64_t n, int32_t pad) { return n + 8 * (int64_t)(pad - 1); }

int64_t mink_class_partition_workspace_bytes(int64_t n) { return chunk_ws_bytes(n, 8); }

int mink_class_partition(const int32_t *coords, int64_t n, int32_t ts, int32_t pad, int32_t *perm, void *workspace,
                         int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(n >= 0 && ts >= 1 && pad >= 1 && perm, "class_partition: bad arguments");
  MINK_REQUIRE(n == 0 || workspace_bytes >= mink_class_partition_workspace_bytes(n), "class_partition: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)mink_class_partition_workspace_bytes(n));
  hipStream_t st = (hipStream_t)stream;
  MINK_HIP(hipMemsetAsync(perm, 0xFF, sizeof(int32_t) * mink_class_partition_rows(n, pad), st));
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(coords && workspace && ((uintptr_t)coords & 15) == 0 && ((uintptr_t)workspace & 255) == 0,
               "class_partition: NULL/misaligned pointer");
  const ChunkWs w = chunk_ws(workspace, n, 8);
  const dim3 grid((unsigned)w.nchunk);
  class_partition_kernel<false><<<grid, kBlock, 0, st>>>(coords, n, ts, w.nchunk, pad, w.counts, nullptr, nullptr, nullptr);
  MINK_CHECK_LAUNCH();
  if (int rc = launch_scan(w.counts, w.offsets, w.nchunk * 8, w.total, st)) return rc;
  class_partition_kernel<true><<<grid, kBlock, 0, st>>>(coords, n, ts, w.nchunk, pad, nullptr, w.offsets, w.total, perm);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_class_partition_batch(int32_t n_maps, const MinkClassPartitionDesc *d, void *stream) {
  MINK_REQUIRE(n_maps >= 0 && n_maps <= 8 && (n_maps == 0 || d), "class_partition_batch: 0..8 maps per call");
  hipStream_t st = (hipStream_t)stream;
  FillQueue fills{st, false};
  ClassPartBatch cb;
  ScanBatch sb;
  int nb = 0;
  int64_t chunk_max = 0;
  for (int i = 0; i < n_maps; ++i) {
    const MinkClassPartitionDesc &e = d[i];
    MINK_REQUIRE(e.n >= 0 && e.ts >= 1 && e.pad >= 1 && e.perm, "class_partition_batch: bad arguments in descriptor %d", i);
    MINK_REQUIRE(e.n == 0 || e.workspace_bytes >= mink_class_partition_workspace_bytes(e.n),
                 "class_partition_batch: workspace of %lld bytes, %lld needed", (long long)e.workspace_bytes,
                 (long long)mink_class_partition_workspace_bytes(e.n));
    if (int rc = fills.add(e.perm, (int64_t)sizeof(int32_t) * mink_class_partition_rows(e.n, e.pad))) return rc;
    if (e.n == 0) continue;
    MINK_REQUIRE(e.coords && e.workspace && ((uintptr_t)e.coords & 15) == 0 && ((uintptr_t)e.workspace & 255) == 0,
                 "class_partition_batch: NULL/misaligned pointer in descriptor %d", i);
    const ChunkWs w = chunk_ws(e.workspace, e.n, 8);
    ClassPart &q = cb.e[nb];
    q.coords = e.coords, q.n = e.n, q.nchunk = w.nchunk, q.ts = e.ts, q.pad = e.pad, q.perm = e.perm;
    q.chunk_counts = w.counts, q.chunk_offsets = w.offsets, q.total = w.total;
    sb.in[nb] = w.counts, sb.out[nb] = w.offsets, sb.total[nb] = w.total, sb.n[nb] = w.nchunk * 8;
    chunk_max = std::max(chunk_max, w.nchunk);
    ++nb;
  }
  if (int rc = fills.flush()) return rc;  // (one launch: at most eight runs, before the kernels that write into them)
  if (nb == 0) return MINK_OK;
  const dim3 grid((unsigned)chunk_max, (unsigned)nb);
  class_partition_batch_kernel<false><<<grid, kBlock, 0, st>>>(cb);
  MINK_CHECK_LAUNCH();
  if (int rc = launch_scan_batch(sb, nb, st)) return rc;
  class_partition_batch_kernel<true><<<grid, kBlock, 0, st>>>(cb);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
