// Scene sub-sampling for the point networks (reference co3d_3d/src/data/transforms.py FarthestPointSample: a Python loop of
// num_points iterations over all voxels of one scene, on the CPU, in the DataLoader worker).
//
//   mink_fps_scenes : batched farthest-point sampling, ONE workgroup of MINK_FPS_THREADS threads per scene (no workgroup ever
//                     waits for another).  The m picks of a scene are serial; each is one pass over the scene's rows
//                         d = ((dx dx) + (dy dy)) + (dz dz), every product and sum rounded to fp32 on its own (no fma),
//                         dist[i] = d where d < dist[i],
//                     and an arg-max of dist with ties to the lowest row.  dist >= +0 and never NaN (it starts at 1e10 and is
//                     only replaced by something smaller), so its bits order like an unsigned integer and the arg-max is the
//                     maximum of the 64-bit key (bits(dist) << 32) | ~row: per thread over its rows, per wave by six butterfly
//                     exchanges, across the 16 waves through LDS.  Each thread carries the coordinates of its own best row and
//                     the winning lane of a wave stores them beside the key, so the next centre comes out of LDS with the
//                     reduction: one barrier per pick, no dependent global load.
//
// Thread t owns the scene-local rows t, t + T, t + 2T, ...  Three residencies, chosen by the scene's size alone (every one does
// the same arithmetic on the same rows, and the key order is total, so the picks do not depend on the choice), each a kernel
// of its own over the B scenes; scenes of different residencies in one batch therefore run one group after the other:
//   n <= MINK_FPS_XYZ_REG_ROWS  : coordinates and running distances in registers (2 or 8 rows per thread), memory is read once
//   n <= MINK_FPS_DIST_REG_ROWS : running distances in registers (56 per thread), coordinates re-read every pick (cache-resident)
//   larger                      : running distances in the caller's workspace, coordinates re-read every pick
#include <limits.h>

#include "common.h"

namespace mink {
namespace {

constexpr int FT = MINK_FPS_THREADS, FW = FT / 64;
constexpr float FPS_FAR = 1e10f;

struct FpsSlot {  // what one wave hands to the workgroup: the key of its best row and that row's coordinates
  unsigned long long key;
  float x, y, z, pad;
};

__device__ __forceinline__ float fps_d2(float x, float y, float z, float cx, float cy, float cz) {
  const float dx = __fsub_rn(x, cx), dy = __fsub_rn(y, cy), dz = __fsub_rn(z, cz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__device__ __forceinline__ unsigned long long fps_key(float d, int row) {
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(~row);
}

// one thread's running best: a later row replaces it only with a strictly larger distance (rows are visited in ascending order).
// `row` is whatever the caller numbers its rows by: the scene-local row, or the slot j of row j FT + tid (an inline constant of
// the unrolled loop, where the rows themselves would be PPT registers held across the picks).
struct FpsBest {
  float d, x, y, z;
  int row;
  __device__ __forceinline__ void init() { d = -1.f, x = y = z = 0.f, row = INT_MAX; }
  __device__ __forceinline__ void offer(float dd, int r, float px, float py, float pz) {
    const bool w = dd > d;
    d = w ? dd : d, row = w ? r : row, x = w ? px : x, y = w ? py : y, z = w ? pz : z;
  }
};

// thread bests -> the workgroup's pick (local row, centre).  `slots` holds two sets of FW entries used alternately, so that one
// barrier per pick suffices: a set is rewritten two picks later, behind the barrier every wave passed after reading it.
__device__ __forceinline__ int fps_reduce(const FpsBest &b, FpsSlot *slots, int it, float &cx, float &cy, float &cz) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mine = b.row == INT_MAX ? 0ull : fps_key(b.d, b.row);
  unsigned long long k = mine;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const unsigned long long o = __shfl_xor(k, s, 64);
    k = o > k ? o : k;
  }
  FpsSlot *set = slots + (it & 1) * FW;
  if (k == mine && (mine != 0ull || lane == 0)) {  // (keys of rows are distinct: exactly one lane, or lane 0 of a wave without rows)
    set[wave].key = k;
    set[wave].x = b.x, set[wave].y = b.y, set[wave].z = b.z;
  }
  __syncthreads();
  unsigned long long best = set[0].key;
  int w = 0;
#pragma unroll
  for (int j = 1; j < FW; ++j) {
    const unsigned long long o = set[j].key;
    w = o > best ? j : w, best = o > best ? o : best;
  }
  cx = set[w].x, cy = set[w].y, cz = set[w].z;
  return (int)~(unsigned)best;
}

// PPT rows per thread with the running distances in registers; XYZ: the coordinates too (else re-read every pick)
template <int PPT, bool XYZ>
__device__ __forceinline__ void fps_registers(const float *__restrict__ p, int64_t ld, int n, int off, int cur, int m,
                                              int *__restrict__ out, FpsSlot *slots) {
  const int tid = threadIdx.x;
  float dist[PPT], X[XYZ ? PPT : 1], Y[XYZ ? PPT : 1], Z[XYZ ? PPT : 1];
  // Row j FT + tid lies at p + min(tid ld + j FT ld, (n - 1) ld): 32-bit element offsets (ld <= MINK_FPS_MAX_LD), clamped to the
  // last row so that every load is unconditional and the loads of a group of rows can be in flight together.  A slot without a
  // row holds dist = -1 for good: no d is below it, and it never beats a row.
  unsigned tl = (unsigned)tid * (unsigned)ld;
  const int ldu = __builtin_amdgcn_readfirstlane((int)ld);
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    dist[j] = j * FT + tid < n ? FPS_FAR : -1.f;
    if (XYZ) {
      const float *q = p + min(tl + (unsigned)(j * FT) * (unsigned)ldu, (unsigned)(n - 1) * (unsigned)ldu);
      X[j] = q[0], Y[j] = q[1], Z[j] = q[2];
    }
  }
  float cx = p[(int64_t)cur * ld], cy = p[(int64_t)cur * ld + 1], cz = p[(int64_t)cur * ld + 2];
  constexpr int G = PPT < 8 ? PPT : 8;  // rows of a thread whose loads are issued together
#pragma unroll 1
  for (int it = 0; it < m; ++it) {
    if (tid == 0) out[it] = off + cur;
    if (it + 1 == m) break;
    FpsBest b;
    b.init();
    // (made opaque once per pick: the PPT addresses, row counts and row numbers are invariant over the picks and would
    //  otherwise be kept in registers beside the distances and spill them)
    unsigned step = (unsigned)(FT * ldu), last = (unsigned)(n - 1) * (unsigned)ldu;
    int left = n;  // rows from the current group on
    if (!XYZ) asm volatile("" : "+v"(tl), "+s"(step), "+s"(last), "+s"(left));
#pragma unroll
    for (int g = 0; g < PPT; g += G) {
      if (!XYZ) __builtin_amdgcn_sched_barrier(0);  // (one group's loads in flight, not all PPT rows')
      if (XYZ ? g * FT < n : left > 0) {  // (uniform over the workgroup)
        float x[G], y[G], z[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          if (XYZ) {
            x[u] = X[g + u], y[u] = Y[g + u], z[u] = Z[g + u];
          } else {
            const float *q = p + min(tl + (unsigned)(g + u) * step, last);
            x[u] = q[0], y[u] = q[1], z[u] = q[2];
          }
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
          const float d = fps_d2(x[u], y[u], z[u], cx, cy, cz);
          dist[g + u] = d < dist[g + u] ? d : dist[g + u];
          b.offer(dist[g + u], g + u, x[u], y[u], z[u]);  // (the slot: an inline constant; the row follows below)
        }
        left -= G * FT;
      }
    }
    if (b.row != INT_MAX) b.row = b.row * FT + tid;
    cur = fps_reduce(b, slots, it, cx, cy, cz);
  }
}

// any size: the running distances live in `dist` (n floats of the workspace; the first pick treats them as FPS_FAR unread)
__device__ __forceinline__ void fps_workspace(const float *__restrict__ p, int64_t ld, int n, int off, int cur, int m,
                                              int *__restrict__ out, FpsSlot *slots, float *__restrict__ dist) {
  const int tid = threadIdx.x;
  float cx = p[(int64_t)cur * ld], cy = p[(int64_t)cur * ld + 1], cz = p[(int64_t)cur * ld + 2];
#pragma unroll 1
  for (int it = 0; it < m; ++it) {
    if (tid == 0) out[it] = off + cur;
    if (it + 1 == m) break;
    FpsBest b;
    b.init();
    for (int i = tid; i < n; i += FT) {
      const float *r = p + (int64_t)i * ld;
      const float x = r[0], y = r[1], z = r[2];
      const float d = fps_d2(x, y, z, cx, cy, cz);
      const float old = it == 0 ? FPS_FAR : dist[i];
      const float now = d < old ? d : old;
      if (it == 0 || d < old) dist[i] = now;
      b.offer(now, i, x, y, z);
    }
    cur = fps_reduce(b, slots, it, cx, cy, cz);
  }
}

// One kernel per residency, so that each gets its own register allocation (together in one kernel they spill); a workgroup
// whose scene belongs to another residency leaves at once.  V = 0 also answers for the scenes that are not sampled at all.
template <int V>
__global__ __launch_bounds__(FT) void fps_kernel(const float *__restrict__ xyz, int64_t n_rows, int64_t ld,
                                                 const int *__restrict__ offsets, const int *__restrict__ start, int m, int64_t n_max,
                                                 int *__restrict__ idx, int *__restrict__ status, float *__restrict__ ws) {
  __shared__ FpsSlot slots[2 * FW];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t o0 = offsets[b], o1 = offsets[b + 1];
  const int64_t n64 = o1 - o0;
  const int cur = start[b];
  int *out = idx + (int64_t)b * m;
  int bad = 0;
  if (o0 < 0 || o1 > n_rows || n64 < 1) bad = MINK_FPS_EMPTY_SCENE;
  else if (n64 > n_max) bad = MINK_FPS_SCENE_TOO_LARGE;
  else if (cur < 0 || cur >= n64) bad = MINK_FPS_BAD_START;
  if (bad) {  // nothing of the scene is read; its picks are -1 and the status word says why
    if (V == 0) {
      for (int i = tid; i < m; i += FT) out[i] = -1;
      if (tid == 0) atomicOr(status, bad);
    }
    return;
  }
  const int n = (int)n64, off = (int)o0;
  const float *p = xyz + o0 * ld;
  const int v = n <= MINK_FPS_XYZ_REG_ROWS_SMALL ? 0 : n <= MINK_FPS_XYZ_REG_ROWS ? 1 : n <= MINK_FPS_DIST_REG_ROWS ? 2 : 3;
  if (v != V) return;
  if (V == 0) fps_registers<MINK_FPS_XYZ_REG_ROWS_SMALL / FT, true>(p, ld, n, off, cur, m, out, slots);
  if (V == 1) fps_registers<MINK_FPS_XYZ_REG_ROWS / FT, true>(p, ld, n, off, cur, m, out, slots);
  if (V == 2) fps_registers<MINK_FPS_DIST_REG_ROWS / FT, false>(p, ld, n, off, cur, m, out, slots);
  if (V == 3) fps_workspace(p, ld, n, off, cur, m, out, slots, ws + (int64_t)b * n_max);
}

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_fps_workspace_bytes(int64_t n_max, int32_t B) {
  if (n_max <= MINK_FPS_DIST_REG_ROWS || B < 1) return 0;
  return n_max * (int64_t)B * (int64_t)sizeof(float);
}

int mink_fps_scenes(const float *xyz, int64_t n, int64_t ld, const int32_t *offsets, const int32_t *start, int32_t B, int32_t m,
                    int64_t n_max, int32_t *idx, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(xyz && offsets && start && idx && status, "fps_scenes: NULL pointer");
  MINK_REQUIRE(ld >= 3 && ld <= MINK_FPS_MAX_LD, "fps_scenes: ld = %lld outside 3..%d", (long long)ld, MINK_FPS_MAX_LD);
  MINK_REQUIRE(m >= 1, "fps_scenes: m = %d below 1", m);
  MINK_REQUIRE(B >= 1, "fps_scenes: B = %d below 1", B);
  MINK_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && n_max >= 1 && n_max <= n && (int64_t)B * m < ((int64_t)1 << 31),
               "fps_scenes: bad shape (n %lld, n_max %lld, B m < 2^31)", (long long)n, (long long)n_max);
  const int64_t need = mink_fps_workspace_bytes(n_max, B);
  MINK_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "fps_scenes: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)need);
  MINK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream));
  const dim3 grid((unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  float *ws = (float *)workspace;
  // (a residency no scene of at most n_max rows can have is not launched)
  fps_kernel<0><<<grid, FT, 0, st>>>(xyz, n, ld, offsets, start, m, n_max, idx, status, ws);
  if (n_max > MINK_FPS_XYZ_REG_ROWS_SMALL) fps_kernel<1><<<grid, FT, 0, st>>>(xyz, n, ld, offsets, start, m, n_max, idx, status, ws);
  if (n_max > MINK_FPS_XYZ_REG_ROWS) fps_kernel<2><<<grid, FT, 0, st>>>(xyz, n, ld, offsets, start, m, n_max, idx, status, ws);
  if (n_max > MINK_FPS_DIST_REG_ROWS) fps_kernel<3><<<grid, FT, 0, st>>>(xyz, n, ld, offsets, start, m, n_max, idx, status, ws);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
