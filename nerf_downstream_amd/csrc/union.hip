// The union of sparse tensors that live on different coordinate maps (ME.MinkowskiUnion: the skip of a U-shaped completion
// net joins a decoder tensor with the encoder tensor of its tensor stride): the map of the union of k coordinate lists and
// the row pass that sums the inputs over it.  Conventions of generate.hip: int32 coordinate rows (b, x, y, z) of 16 bytes,
// fp32 feature rows with a row pitch, 16-byte lanes where every pitch, width and pointer allows and dword lanes otherwise
// (rowpass.h), -1 = absent, no float atomics.
//
// Row order of the union [ME-recall: ME's own order is unpinned, ME is absent; this is the definition here]: sample-major;
// inside sample b the rows of input 0 in their order, then the rows of input 1 that no earlier input holds, in their order,
// and so on.  Every input row (i, r) of sample b therefore has a POSITION
//     v = sum_j off_j[b]  +  sum_{j < i} (off_j[b + 1] - off_j[b])  +  (r - off_i[b])            (0 <= v < S = sum n_i)
// in the list of all rows in that order, the first occurrence of a key in (input, row) order is its occurrence of least v,
// and the union row of a first occurrence is the number of first occurrences before it.
//
//   insert   : one thread per input row: its position v, its key into the hash of all S rows (integer compare-and-swap, as
//              coords.hip / kmap.hip insert), an integer atomicMin of v on the slot -- the first occurrence wins, the rule
//              of mink_coords_unique.
//   mark     : one thread per input row: the row whose v the slot holds is the winner and writes its row at winner[v].
//   count / scan (launch_scan: coords.hip) / scatter : the compaction of generate.hip over the positions, kUnionBlock per
//              workgroup: the winner at v with u winners before it becomes union row u -- its coordinates, in2out, its column
//              of out2in (the row for its own input, -1 for every other), rank[v] = u.
//   resolve  : one thread per input row: a row that lost reads rank[] of the position its slot holds and fills in2out and its
//              entry of out2in.
//   offsets  : one thread per sample boundary s: the winners before the position at which sample s begins.
// Seven launches behind one 0xFF fill of the workspace; no kernel waits for memory that another workgroup of the same launch
// writes, and nothing here synchronises with the host.  A row the lists' contract excludes -- a batch index outside [0, B), a
// row outside its sample's offsets, a coordinate outside the key range -- takes part in nothing and gets in2out = -1; every
// index is checked against its array before it is used, whatever the lists hold.
//
//   union_sum : y[u][:] = the sum over the inputs that hold union row u, in ascending input index; the first one present is
//               COPIED (a row held by one input comes out bit for bit, -0.0 included), the later ones are added to it.
#include <algorithm>

#include "coords_common.h"
#include "rowpass.h"

namespace mink {
namespace {

constexpr int GB = 256;                        // threads per workgroup of the flat passes
constexpr int kUnionBlock = MINK_UNION_BLOCK;  // positions one workgroup of the compaction owns (one per thread)
constexpr int kMaxIn = MINK_UNION_MAX_INPUTS;
static_assert(kUnionBlock == 256 && kUnionBlock % 64 == 0, "the compaction ranks four wave64 ballots per workgroup");

struct UnionLists {
  const int4 *coords[kMaxIn];
  const int32_t *off[kMaxIn];  // [B + 1] each
  int32_t *in2out[kMaxIn];
  int64_t first[kMaxIn + 1];  // first[i] = n_0 + ... + n_{i-1}: input row (i, r) is row g = first[i] + r of all S = first[k]
  int k, B;
};

struct UnionWork {  // the workspace, every array 0xFF before the first launch
  unsigned long long *tkeys;  // [cap]
  unsigned *tvals;            // [cap]: the least position among the rows of the slot's key
  int32_t *pos;               // [S]: position v of row g, -1 = the row takes part in nothing
  int32_t *slot;              // [S]: slot of row g's key
  int32_t *winner;            // [S]: the row g that won position v, -1 = none
  int32_t *rank;              // [S]: union row of the winner at position v
  int32_t *group_count, *group_offset;  // [groups]
  uint64_t mask;
};

__device__ __forceinline__ int input_of(const UnionLists &L, int64_t g) {
  int i = 0;
  while (i + 1 < L.k && g >= L.first[i + 1]) ++i;
  return i;
}

__global__ __launch_bounds__(GB) void union_insert_kernel(UnionLists L, UnionWork W) {
  const int64_t g = (int64_t)blockIdx.x * GB + threadIdx.x, S = L.first[L.k];
  if (g >= S) return;
  const int i = input_of(L, g);
  const int64_t r = g - L.first[i];
  const int4 c = L.coords[i][r];
  uint64_t key;
  int64_t v = -1;
  if (pack_key(c.x, c.y, c.z, c.w, key) && c.x < L.B) {
    const int b = c.x;
    const int64_t lo = L.off[i][b], hi = L.off[i][b + 1];
    if (r >= lo && r < hi) {
      v = r - lo;
      for (int j = 0; j < L.k; ++j) {
        const int64_t a = L.off[j][b];
        v += a + (j < i ? (int64_t)L.off[j][b + 1] - a : 0);
      }
      if (v < 0 || v >= S) v = -1;
    }
  }
  W.pos[g] = (int32_t)v;
  if (v < 0) return;
  uint64_t s = mix64(key) & W.mask;
  for (;;) {
    const unsigned long long prev = atomicCAS(&W.tkeys[s], (unsigned long long)kEmptyKey, (unsigned long long)key);
    if (prev == kEmptyKey || prev == key) break;
    s = (s + 1) & W.mask;
  }
  atomicMin(&W.tvals[s], (unsigned)v);  // the first occurrence in (input, row) order wins
  W.slot[g] = (int32_t)s;
}

__global__ __launch_bounds__(GB) void union_mark_kernel(int64_t S, UnionWork W) {
  const int64_t g = (int64_t)blockIdx.x * GB + threadIdx.x;
  if (g >= S) return;
  const int32_t v = W.pos[g];
  if (v >= 0 && W.tvals[W.slot[g]] == (unsigned)v) W.winner[v] = (int32_t)g;
}

// winners among this workgroup's kUnionBlock positions before this thread's (exclusive), and the workgroup's total (the ranking
// of generate.hip's compaction)
__device__ __forceinline__ int block_rank(bool keep, int &block_total) {
  __shared__ int wave_count[kUnionBlock / 64];
  const unsigned long long ballot = __ballot(keep);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(ballot);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kUnionBlock / 64; ++w) {
    const int c = wave_count[w];
    before += w < wave ? c : 0;
    total += c;
  }
  block_total = total;
  return before + wave_rank(ballot);
}

__global__ __launch_bounds__(kUnionBlock) void union_count_kernel(int64_t S, UnionWork W) {
  const int64_t v = (int64_t)blockIdx.x * kUnionBlock + threadIdx.x;
  int total;
  block_rank(v < S && W.winner[v] >= 0, total);
  if (threadIdx.x == 0) W.group_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kUnionBlock) void union_scatter_kernel(UnionLists L, UnionWork W, int4 *__restrict__ out_coords,
                                                                    int32_t *__restrict__ out2in, int64_t pitch) {
  const int64_t v = (int64_t)blockIdx.x * kUnionBlock + threadIdx.x, S = L.first[L.k];
  const int64_t g = v < S ? W.winner[v] : -1;
  const bool keep = g >= 0 && g < S;
  int total;
  const int u = W.group_offset[blockIdx.x] + block_rank(keep, total);  // winners before position v
  if (!keep || u < 0 || u >= S) return;
  const int i = input_of(L, g);
  const int32_t r = (int32_t)(g - L.first[i]);
  out_coords[u] = L.coords[i][r];
  W.rank[v] = u;
  L.in2out[i][r] = u;
  for (int j = 0; j < L.k; ++j) out2in[j * pitch + u] = j == i ? r : -1;
}

__global__ __launch_bounds__(GB) void union_resolve_kernel(UnionLists L, UnionWork W, int32_t *__restrict__ out2in, int64_t pitch) {
  const int64_t g = (int64_t)blockIdx.x * GB + threadIdx.x, S = L.first[L.k];
  if (g >= S) return;
  const int i = input_of(L, g);
  const int64_t r = g - L.first[i];
  const int32_t v = W.pos[g];
  if (v < 0) {
    L.in2out[i][r] = -1;
    return;
  }
  const unsigned vw = W.tvals[W.slot[g]];  // the position that won this row's key
  if (vw == (unsigned)v || (int64_t)vw >= S) return;  // a winner: the scatter wrote its entries
  const int32_t u = W.rank[vw];
  const bool ok = u >= 0 && u < S;
  L.in2out[i][r] = ok ? u : -1;
  if (ok) out2in[i * pitch + u] = (int32_t)r;
}

// out_off[s] = the winners before the position at which sample s begins (s = B: all of them)
__global__ __launch_bounds__(GB) void union_offsets_kernel(UnionLists L, UnionWork W, const int32_t *__restrict__ total,
                                                           int32_t *__restrict__ out_off) {
  const int s = blockIdx.x * GB + threadIdx.x;
  if (s > L.B) return;
  const int64_t S = L.first[L.k];
  int64_t begin = 0;
  for (int j = 0; j < L.k; ++j) begin += L.off[j][s];
  begin = begin < 0 ? 0 : begin;
  if (begin >= S) {
    out_off[s] = *total;
    return;
  }
  const int64_t group = begin / kUnionBlock;
  int before = W.group_offset[group];
  for (int64_t v = group * kUnionBlock; v < begin; ++v) before += W.winner[v] >= 0;
  out_off[s] = before;
}

struct SumRows {
  const float *x[kMaxIn];
  int32_t ld[kMaxIn];
  int64_t n[kMaxIn];
  int k;
};

template <int VEC>
__global__ __launch_bounds__(GB) void union_sum_kernel(SumRows X, int C, const int32_t *__restrict__ out2in, int64_t pitch,
                                                       int64_t n_out, float *__restrict__ y, int ldy) {
  const int ncg = C / VEC;
  const int64_t total = n_out * ncg;
  for (int64_t t = (int64_t)blockIdx.x * GB + threadIdx.x; t < total; t += (int64_t)gridDim.x * GB) {
    const int64_t u = t / ncg;
    const int c = (int)(t - u * ncg) * VEC;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    bool first = true;
    for (int i = 0; i < X.k; ++i) {
      const int64_t r = out2in[i * pitch + u];
      if (r < 0 || r >= X.n[i]) continue;
      float v[VEC];
      ldv<VEC>(X.x[i] + r * X.ld[i] + c, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = first ? v[e] : acc[e] + v[e];
      first = false;
    }
    stv<VEC>(y + u * ldy + c, acc);
  }
}

int64_t sum_rows(int32_t k, const int64_t *n_host) {  // -1: a bad list of counts
  if (k < 2 || k > kMaxIn || !n_host) return -1;
  int64_t S = 0;
  for (int i = 0; i < k; ++i) {
    if (n_host[i] < 1 || n_host[i] > 0x7fffffffLL) return -1;
    S += n_host[i];
  }
  return S;
}

// byte offsets of the workspace arrays behind the hash keys, in the order of UnionWork
struct WorkLayout {
  int64_t cap, groups, tvals, pos, slot, winner, rank, group_count, group_offset, bytes;
  explicit WorkLayout(int64_t S) {
    cap = (int64_t)table_capacity(S), groups = cdiv(S, kUnionBlock);
    tvals = 8 * cap, pos = tvals + 4 * cap, slot = pos + 4 * S, winner = slot + 4 * S, rank = winner + 4 * S;
    group_count = rank + 4 * S, group_offset = group_count + 4 * groups;
    bytes = align_up(group_offset + 4 * groups, 256);
  }
};

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_union_workspace_bytes(int32_t k, const int64_t *n_host, int32_t B) {
  const int64_t S = sum_rows(k, n_host);
  if (S < 1 || S > 0x7fffffffLL || B < 1) {
    set_error("union_workspace_bytes: bad arguments (k=%d, B=%d; 2 <= k <= %d inputs of at least one row each, fewer than 2^31 rows in all)",
              k, B, kMaxIn);
    return -1;
  }
  return WorkLayout(S).bytes;
}

int mink_union_build(int32_t k, const int32_t *const *coords, const int32_t *const *batch_offsets, const int64_t *n_host, int32_t B,
                     int32_t *out_coords, int32_t *const *in2out, int32_t *out2in, int64_t out2in_pitch, int32_t *out_batch_offsets,
                     int32_t *total, void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(k >= 2 && k <= kMaxIn, "union_build: %d inputs (2 <= k <= %d)", k, kMaxIn);
  MINK_REQUIRE(B >= 1 && B <= 65535, "union_build: B=%d (at least one sample, at most 65535)", B);
  MINK_REQUIRE(coords && batch_offsets && n_host && in2out && out_coords && out2in && out_batch_offsets && total, "union_build: NULL pointer");
  int64_t S = 0;
  for (int i = 0; i < k; ++i) {
    MINK_REQUIRE(n_host[i] >= 1, "union_build: input %d has %lld rows (at least one row each)", i, (long long)n_host[i]);
    S += n_host[i];
    MINK_REQUIRE(S <= 0x7fffffffLL, "union_build: %lld rows up to input %d (fewer than 2^31 rows in all)", (long long)S, i);
  }
  for (int i = 0; i < k; ++i) {
    MINK_REQUIRE(coords[i] && batch_offsets[i] && in2out[i], "union_build: NULL pointer (input %d)", i);
    MINK_REQUIRE(aligned16(coords[i]), "union_build: coordinate rows must be 16-byte aligned (input %d)", i);
  }
  MINK_REQUIRE(aligned16(out_coords), "union_build: coordinate rows must be 16-byte aligned (out_coords)");
  MINK_REQUIRE(out2in_pitch >= S, "union_build: out2in pitch of %lld, %lld rows in all (pitch >= the sum of the row counts)",
               (long long)out2in_pitch, (long long)S);
  const WorkLayout lay(S);
  MINK_REQUIRE_WORKSPACE("union_build", workspace_bytes, lay.bytes, workspace);
  MINK_REQUIRE(workspace, "union_build: NULL workspace");

  UnionLists L;
  L.k = k, L.B = B, L.first[0] = 0;
  for (int i = 0; i < kMaxIn; ++i) {
    const bool live = i < k;
    L.coords[i] = live ? (const int4 *)coords[i] : nullptr, L.off[i] = live ? batch_offsets[i] : nullptr;
    L.in2out[i] = live ? in2out[i] : nullptr, L.first[i + 1] = L.first[i] + (live ? n_host[i] : 0);
  }
  char *ws = (char *)workspace;
  UnionWork W;
  W.tkeys = (unsigned long long *)ws, W.tvals = (unsigned *)(ws + lay.tvals), W.pos = (int32_t *)(ws + lay.pos);
  W.slot = (int32_t *)(ws + lay.slot), W.winner = (int32_t *)(ws + lay.winner), W.rank = (int32_t *)(ws + lay.rank);
  W.group_count = (int32_t *)(ws + lay.group_count), W.group_offset = (int32_t *)(ws + lay.group_offset);
  W.mask = (uint64_t)lay.cap - 1;

  hipStream_t st = (hipStream_t)stream;
  FillQueue fill{st, false};
  if (int rc = fill.add(workspace, lay.bytes)) return rc;
  if (int rc = fill.flush()) return rc;
  const dim3 rows((unsigned)cdiv(S, GB)), groups((unsigned)lay.groups);
  union_insert_kernel<<<rows, GB, 0, st>>>(L, W);
  MINK_CHECK_LAUNCH();
  union_mark_kernel<<<rows, GB, 0, st>>>(S, W);
  MINK_CHECK_LAUNCH();
  union_count_kernel<<<groups, kUnionBlock, 0, st>>>(S, W);
  MINK_CHECK_LAUNCH();
  if (int rc = launch_scan(W.group_count, W.group_offset, lay.groups, total, st)) return rc;
  union_scatter_kernel<<<groups, kUnionBlock, 0, st>>>(L, W, (int4 *)out_coords, out2in, out2in_pitch);
  MINK_CHECK_LAUNCH();
  union_resolve_kernel<<<rows, GB, 0, st>>>(L, W, out2in, out2in_pitch);
  MINK_CHECK_LAUNCH();
  union_offsets_kernel<<<dim3((unsigned)cdiv(B + 1, GB)), GB, 0, st>>>(L, W, total, out_batch_offsets);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_union_sum(int32_t k, const float *const *x, const int32_t *ldx_host, const int64_t *n_host, int32_t C, const int32_t *out2in,
                   int64_t out2in_pitch, int64_t n_out, float *y, int32_t ldy, void *stream) {
  MINK_REQUIRE(k >= 2 && k <= kMaxIn, "union_sum: %d inputs (2 <= k <= %d)", k, kMaxIn);
  MINK_REQUIRE(x && ldx_host && n_host, "union_sum: NULL pointer");
  MINK_REQUIRE_ROWS_C("union_sum", n_out, 0x7fffffffLL, C);
  MINK_REQUIRE(ldy >= C && out2in_pitch >= n_out, "union_sum: bad pitch (C=%d, pitch of y=%d, pitch of out2in=%lld for %lld rows)", C, ldy,
               (long long)out2in_pitch, (long long)n_out);
  SumRows X;
  X.k = k;
  bool vec = (C & 3) == 0 && (ldy & 3) == 0 && aligned16(y);
  for (int i = 0; i < kMaxIn; ++i) {
    const bool live = i < k;
    if (live) {
      MINK_REQUIRE(n_host[i] >= 1 && n_host[i] <= 0x7fffffffLL && ldx_host[i] >= C, "union_sum: bad shape (input %d: %lld rows, pitch=%d, C=%d)",
                   i, (long long)n_host[i], ldx_host[i], C);
      vec = vec && (ldx_host[i] & 3) == 0 && aligned16(x[i]);
    }
    X.x[i] = live ? x[i] : nullptr, X.ld[i] = live ? ldx_host[i] : 0, X.n[i] = live ? n_host[i] : 0;
  }
  if (n_out == 0) return MINK_OK;
  MINK_REQUIRE(out2in && y, "union_sum: NULL pointer");
  for (int i = 0; i < k; ++i) MINK_REQUIRE(x[i], "union_sum: NULL pointer (input %d)", i);
  const dim3 grid(flat_grid(n_out * (vec ? C / 4 : C), GB, 1 << 16));
  hipStream_t st = (hipStream_t)stream;
  if (vec) union_sum_kernel<4><<<grid, GB, 0, st>>>(X, C, out2in, out2in_pitch, n_out, y, ldy);
  else union_sum_kernel<1><<<grid, GB, 0, st>>>(X, C, out2in, out2in_pitch, n_out, y, ldy);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
