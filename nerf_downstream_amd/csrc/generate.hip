// Coordinate maps that a network makes and unmakes on gfx950: the children of a generative transposed convolution and the
// compaction behind MinkowskiPruning (ME's completion / reconstruction decoders: generative transpose -> classifier -> pruning).
// Conventions of pool.hip / field.hip: int32 coordinate rows (b, x, y, z) of 16 bytes, fp32 feature rows with a row pitch,
// 16-byte lanes where every pitch, width and pointer allows and dword lanes otherwise (rowpass.h), -1 = absent, no atomics.
//
//   generate_children : one thread per child.  Parent p at tensor stride ts spawns child k (0..7) at p + (k & 1, (k >> 1) & 1,
//                       (k >> 2) & 1) * ts / 2 -- kernel_offsets(2, ts / 2): x fastest, z slowest -- as row 8 p + k.  A parent is
//                       a multiple of ts inside the 16-bit key range, so its largest coordinate is at most 32767 - (ts - 1)
//                       and p + ts / 2 stays inside the range: children need no status word.
//   prune compaction  : the stable compaction of the rows a mask keeps, as THREE launches with nothing shared but memory
//                       that an earlier launch has finished writing -- (1) every workgroup counts the kept rows of its
//                       kPruneBlock rows, (2) ONE workgroup turns the counts into exclusive offsets and writes the total,
//                       (3) every workgroup ranks its rows again (ballot + the offset of its group) and scatters.  No
//                       workgroup ever waits for a word another workgroup of the same launch writes.
//                       Launch (3) also writes the batch offsets of the new map: the rank of a row is the number of kept rows
//                       before it, so the row at which the batch index steps from a to b knows new_off[a + 1 .. b] -- the
//                       kept count of a sample is the difference of two of them, and no further pass or counter is needed.
//   gather_rows       : dst[i][:] = src[idx[i]][:], zeros where idx[i] is absent.  Forward of the pruning (idx = the kept
//                       rows) and its backward (idx = old row -> new row, -1 for a pruned row: every row of dX is written
//                       exactly once, kept rows with their gradient row and pruned rows with zeros -- no memset + scatter).
//                       (mink_rows_gather of seghead.hip computes the same rows one dword per lane into an unpitched output;
//                       this one takes the 16-byte lanes of rowpass.h and a destination pitch.)
#include <algorithm>

#include "rowpass.h"

namespace mink {
namespace {

constexpr int GB = 256;                       // threads per workgroup of the flat passes
constexpr int kPruneBlock = MINK_PRUNE_BLOCK;  // rows one workgroup of the compaction owns (one per thread)
static_assert(kPruneBlock == 256 && kPruneBlock % 64 == 0, "the compaction ranks four wave64 ballots per workgroup");

__global__ __launch_bounds__(GB) void generate_children_kernel(const int4 *__restrict__ parents, int64_t n, int half,
                                                               int4 *__restrict__ children) {
  const int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x;
  if (i >= 8 * n) return;
  const int4 p = parents[i >> 3];
  const int k = (int)(i & 7);
  children[i] = make_int4(p.x, p.y + (k & 1) * half, p.z + ((k >> 1) & 1) * half, p.w + ((k >> 2) & 1) * half);
}

// kept rows of this workgroup's kPruneBlock rows before `row` of this thread (exclusive), and the workgroup's total
__device__ __forceinline__ int block_rank(bool keep, int &block_total) {
  __shared__ int wave_count[kPruneBlock / 64];
  const unsigned long long ballot = __ballot(keep);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(ballot);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kPruneBlock / 64; ++w) {
    const int c = wave_count[w];
    before += w < wave ? c : 0;
    total += c;
  }
  block_total = total;
  return before + wave_rank(ballot);
}

__global__ __launch_bounds__(kPruneBlock) void prune_count_kernel(const uint8_t *__restrict__ mask, int64_t n,
                                                                  int32_t *__restrict__ group_count) {
  const int64_t i = (int64_t)blockIdx.x * kPruneBlock + threadIdx.x;
  const bool keep = i < n && mask[i] != 0;
  int total;
  block_rank(keep, total);
  if (threadIdx.x == 0) group_count[blockIdx.x] = total;
}

// one workgroup: group_count[g] -> the kept rows before group g (in place), *total = all of them
__global__ __launch_bounds__(kPruneBlock) void prune_scan_kernel(int32_t *__restrict__ group_count, int64_t groups,
                                                                 int32_t *__restrict__ total) {
  __shared__ int part[kPruneBlock];
  int carry = 0;
  for (int64_t base = 0; base < groups; base += kPruneBlock) {
    const int64_t g = base + threadIdx.x;
    const int mine = g < groups ? group_count[g] : 0;
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < kPruneBlock; d <<= 1) {  // inclusive scan of the chunk
      const int add = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    if (g < groups) group_count[g] = carry + part[threadIdx.x] - mine;
    carry += part[kPruneBlock - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

__device__ __forceinline__ int clamp_batch(int b, int B) { return b < 0 ? 0 : (b > B - 1 ? B - 1 : b); }

__global__ __launch_bounds__(kPruneBlock) void prune_scatter_kernel(const uint8_t *__restrict__ mask, const int4 *__restrict__ coords,
                                                                    int64_t n, int B, const int32_t *__restrict__ group_offset,
                                                                    int32_t *__restrict__ kept, int32_t *__restrict__ old2new,
                                                                    int4 *__restrict__ out_coords, int32_t *__restrict__ new_off) {
  const int64_t i = (int64_t)blockIdx.x * kPruneBlock + threadIdx.x;
  const bool keep = i < n && mask[i] != 0;
  int total;
  const int rank = group_offset[blockIdx.x] + block_rank(keep, total);  // kept rows before row i
  if (i >= n) return;
  const int4 c = coords[i];
  old2new[i] = keep ? rank : -1;
  if (keep) {
    kept[rank] = (int32_t)i;
    out_coords[rank] = c;
  }
  // batch offsets of the kept rows: sample b begins at the rank of the first row whose batch index reaches b (indices
  // clamped into [0, B): whatever the batch column holds, the stores stay inside new_off[0 .. B])
  const int b = clamp_batch(c.x, B);
  const int first = i == 0 ? 0 : clamp_batch(coords[i - 1].x, B) + 1;
  for (int s = first; s <= b; ++s) new_off[s] = rank;
  if (i == n - 1)
    for (int s = b + 1; s <= B; ++s) new_off[s] = rank + (keep ? 1 : 0);
}

template <int VEC>
__global__ __launch_bounds__(GB) void gather_rows_kernel(const float *__restrict__ src, int ld_src, int64_t n_src, int C,
                                                         const int32_t *__restrict__ idx, int64_t n_dst, float *__restrict__ dst,
                                                         int ld_dst) {
  const int ncg = C / VEC;
  const int64_t total = n_dst * ncg;
  for (int64_t t = (int64_t)blockIdx.x * GB + threadIdx.x; t < total; t += (int64_t)gridDim.x * GB) {
    const int64_t i = t / ncg;
    const int c = (int)(t - i * ncg) * VEC;
    const int r = idx[i];
    float v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = 0.f;
    if (r >= 0 && r < n_src) ldv<VEC>(src + (int64_t)r * ld_src + c, v);
    stv<VEC>(dst + i * ld_dst + c, v);
  }
}

int gather_rows(const char *name, const float *src, int32_t ld_src, int64_t n_src, int32_t C, const int32_t *idx, int64_t n_dst,
                float *dst, int32_t ld_dst, void *stream) {
  MINK_REQUIRE(C >= 1 && C <= 4096 && ld_src >= C && ld_dst >= C, "%s: bad shape (C=%d, source pitch=%d, destination pitch=%d; 1 <= C <= 4096)",
               name, C, ld_src, ld_dst);
  MINK_REQUIRE(n_src >= 0 && n_src <= 0x0fffffffLL && n_dst >= 0 && n_dst <= 0x0fffffffLL, "%s: bad row counts (source=%lld, destination=%lld)",
               name, (long long)n_src, (long long)n_dst);
  if (n_dst == 0) return MINK_OK;
  MINK_REQUIRE(idx && dst && (src || n_src == 0), "%s: NULL pointer", name);
  const bool vec = (C & 3) == 0 && (ld_src & 3) == 0 && (ld_dst & 3) == 0 && aligned16(src) && aligned16(dst);
  const dim3 grid(flat_grid(n_dst * (vec ? C / 4 : C), GB, 1 << 16));
  hipStream_t st = (hipStream_t)stream;
  if (vec) gather_rows_kernel<4><<<grid, GB, 0, st>>>(src, ld_src, n_src, C, idx, n_dst, dst, ld_dst);
  else gather_rows_kernel<1><<<grid, GB, 0, st>>>(src, ld_src, n_src, C, idx, n_dst, dst, ld_dst);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int mink_generate_children(const int32_t *coords, int64_t n, int32_t ts, int32_t *children, void *stream) {
  MINK_REQUIRE(n >= 0 && 8 * n <= 0x0fffffffLL && ts >= 2 && ts <= 32768 && (ts & 1) == 0,
               "generate_children: bad arguments (n=%lld, ts=%d; an even tensor stride, at most 2^28 - 1 children)", (long long)n, ts);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(coords && children, "generate_children: NULL pointer");
  MINK_REQUIRE(aligned16(coords) && aligned16(children), "generate_children: coordinate rows must be 16-byte aligned");
  generate_children_kernel<<<dim3((unsigned)cdiv(8 * n, GB)), GB, 0, (hipStream_t)stream>>>((const int4 *)coords, n, ts / 2,
                                                                                          (int4 *)children);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int64_t mink_prune_workspace_bytes(int64_t n) { return align_up(4 * std::max<int64_t>(cdiv(n, kPruneBlock), 1), 256); }

int mink_prune_compact(const uint8_t *mask, const int32_t *coords, int64_t n, int32_t B, int32_t *kept, int32_t *old2new,
                       int32_t *out_coords, int32_t *batch_offsets, int32_t *total, void *workspace, int64_t workspace_bytes,
                       void *stream) {
  MINK_REQUIRE(n >= 1 && n <= 0x0fffffffLL && B >= 1 && B <= 65535, "prune_compact: bad arguments (n=%lld, B=%d; at least one row and one sample)",
               (long long)n, B);
  MINK_REQUIRE(mask && coords && kept && old2new && out_coords && batch_offsets && total, "prune_compact: NULL pointer");
  MINK_REQUIRE(aligned16(coords) && aligned16(out_coords), "prune_compact: coordinate rows must be 16-byte aligned");
  MINK_REQUIRE_WORKSPACE("prune_compact", workspace_bytes, mink_prune_workspace_bytes(n), workspace);
  MINK_REQUIRE(workspace, "prune_compact: NULL workspace");
  const int64_t groups = cdiv(n, kPruneBlock);
  int32_t *group_count = (int32_t *)workspace;
  hipStream_t st = (hipStream_t)stream;
  prune_count_kernel<<<dim3((unsigned)groups), kPruneBlock, 0, st>>>(mask, n, group_count);
  MINK_CHECK_LAUNCH();
  prune_scan_kernel<<<dim3(1), kPruneBlock, 0, st>>>(group_count, groups, total);
  MINK_CHECK_LAUNCH();
  prune_scatter_kernel<<<dim3((unsigned)groups), kPruneBlock, 0, st>>>(mask, (const int4 *)coords, n, B, group_count, kept, old2new,
                                                                     (int4 *)out_coords, batch_offsets);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_prune_gather(const float *x, int32_t ldx, int64_t n_in, int32_t C, const int32_t *kept, int64_t n_out, float *y, int32_t ldy,
                      void *stream) {
  return gather_rows("prune_gather", x, ldx, n_in, C, kept, n_out, y, ldy, stream);
}

int mink_prune_gather_bwd(const float *dy, int32_t ldy, int64_t n_out, int32_t C, const int32_t *old2new, int64_t n_in, float *dx,
                          int32_t lddx, void *stream) {
  return gather_rows("prune_gather_bwd", dy, ldy, n_out, C, old2new, n_in, dx, lddx, stream);
}

}  // extern "C"
