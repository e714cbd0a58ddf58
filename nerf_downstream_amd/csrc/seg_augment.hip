// GPU-side augmentation of the segmentation recipe (include/mink_hip.h MINK_SEGAUG_*): the reference's
// co3d_3d/configs/scannet_plenoxel.gin list -- RandomRotation, RandomCrop (transforms.py:194-244), RandomAffine,
// CoordinateDropout, RandomFeatureJitter, RandomHorizontalFlip, RandomTranslation, ElasticDistortion (:535-594) --
// applied to a whole batch.  Launches, in order:
//
//   crop_bounds : per-scene min / max of the pre-crop coordinates p (scenes that drew a crop)
//   crop_boxes  : per scene, the set of drawn crop boxes that contain at least one row (one bit per box)
//   count       : which rows survive (winning box, dropout coin), per-block counts, flip maxima over the live rows
//   scan        : exclusive scan of the block counts (one block), survivor count -> status[0]
//   apply       : coordinates and (jittered) features of the survivors, compacted in order, and their source rows
//   per elastic pass: min / max of the survivors -> grid dims (checked against the caller's bound) -> Philox noise ->
//   three separable blurs (each = the 3-tap box twice along one axis) -> trilinear displacement of every survivor.
//   A scene whose grid exceeds its bound gets no stored grid: the displacement kernel evaluates its blurred noise at the
//   8 corners of every point from the Philox noise of the 6^3 nodes around them (same values, more arithmetic).
//
// The host draws the per-scene randomness (matrices, crop boxes, gates); per-row and per-grid-node randomness is Philox.
// Coordinates are carried in double between the stages (p, q and r bit-reproducible by a float64 restatement; the elastic
// displacement then differs from float64 only by the float noise grid) and written as float once per stage that moves them.
#include "augment_common.h"

namespace mink {
namespace {

constexpr int kStatStride = 32;  // 64-bit words per scene in the statistics array (256 bytes: scenes do not share a line)
// words of one scene: min words hold ~ord (so every reduction is an atomicMax and 0 = no row)
constexpr int kPMin = 0, kPMax = 3, kBoxes = 6, kQMax = 7, kEMin = 10, kEMax = 13, kDims = 22;  // kEMin/kEMax + 6 * pass
constexpr int kGridMode = 25;  // of the current elastic pass: kModeGrid = noise grid in the workspace, kModeDirect = none
constexpr uint64_t kModeGrid = 1, kModeDirect = 2;
constexpr double kMaxDim = 65535.0;  // grid nodes per axis: the Philox counter packs two node indices per 32-bit word

__device__ __forceinline__ uint64_t d2ord(double d) {  // order-preserving double -> uint64
  const uint64_t u = (uint64_t)__double_as_longlong(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ord2d(uint64_t u) {
  return __longlong_as_double((long long)((u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u));
}

// out_j = ((v0*M[0][j] + v1*M[1][j]) + v2*M[2][j]) + t_j, every operation rounded
__device__ __forceinline__ void affine(const double v[3], const double *__restrict__ M, const double *__restrict__ t, double out[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double t0 = v[0] * M[j], t1 = v[1] * M[3 + j], t2 = v[2] * M[6 + j];
    out[j] = ((t0 + t1) + t2) + t[j];
  }
}

// max of v (0 = nothing) into word `w` of scene `scene`: one atomic per wave when the wave lies inside one scene.
// Every lane of the wave must call it.
__device__ __forceinline__ void scene_max(uint64_t *__restrict__ stats, int w, int scene, int b0, bool uniform, uint64_t v) {
  if (uniform) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint64_t)__shfl_xor((unsigned long long)v, d));
    uint64_t *a = stats + (int64_t)kStatStride * b0 + w;
    if ((threadIdx.x & 63) == 0 && v > __atomic_load_n(a, __ATOMIC_RELAXED)) atomicMax((unsigned long long *)a, (unsigned long long)v);
  } else if (v != 0u) {
    atomicMax((unsigned long long *)(stats + (int64_t)kStatStride * scene + w), (unsigned long long)v);
  }
}

__device__ __forceinline__ bool wave_uniform_scene(bool valid, int scene, int &b0) {
  b0 = __shfl(scene, 0);
  return __ballot(valid && scene != b0) == 0ull;
}

__device__ __forceinline__ void pre_crop(const double *__restrict__ P, float4 c4, double p[3]) {
  const double c[3] = {(double)c4.y, (double)c4.z, (double)c4.w};
  affine(c, P + MINK_SEGAUG_A0, P + MINK_SEGAUG_a0, p);
}

// the scene's crop frame: false = no crop (not drawn, empty scene, or the crop size covers the scene)
__device__ __forceinline__ bool crop_frame(const double *__restrict__ P, const uint64_t *__restrict__ st, double pmin[3],
                                           double range[3]) {
#pragma clang fp contract(off)
  if (P[MINK_SEGAUG_CROP] == 0.0 || st[kPMax] == 0u) return false;
  bool any = false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    pmin[j] = ord2d(~st[kPMin + j]);
    range[j] = fmax((ord2d(st[kPMax + j]) - pmin[j]) - P[MINK_SEGAUG_CROP_SIZE + j], 0.0);
    any = any || range[j] != 0.0;
  }
  return any;
}

__device__ __forceinline__ bool in_box(const double *__restrict__ P, const double p[3], const double pmin[3], const double range[3], int k) {
#pragma clang fp contract(off)
  bool in = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double n = p[j] - pmin[j], lo = P[MINK_SEGAUG_CROP_U + 3 * k + j] * range[j], hi = lo + P[MINK_SEGAUG_CROP_SIZE + j];
    in = in && lo < n && n < hi;
  }
  return in;
}

// crop membership of a row with pre-crop coordinates p (after crop_boxes has run)
__device__ __forceinline__ bool in_crop(const double *__restrict__ P, const uint64_t *__restrict__ st, const double p[3]) {
  double pmin[3], range[3];
  if (!crop_frame(P, st, pmin, range)) return true;
  const uint64_t boxes = st[kBoxes];
  if (boxes == 0u) return true;  // no box kept a row: the scene is not cropped (reference :240-244)
  return in_box(P, p, pmin, range, __ffsll((unsigned long long)boxes) - 1);
}

__global__ __launch_bounds__(kBlock) void seg_crop_bounds_kernel(const void *__restrict__ coords, bool as_int, int64_t n,
                                                                 const int *__restrict__ scene_offsets, int n_scenes,
                                                                 const double *__restrict__ params, uint64_t *__restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int scene = 0;
  uint64_t lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
  if (i < n) {
    scene = scene_of(scene_offsets, n_scenes, i);
    const double *P = params + (int64_t)scene * MINK_SEGAUG_PARAMS;
    if (P[MINK_SEGAUG_CROP] != 0.0) {
      double p[3];
      pre_crop(P, load_coord(coords, i, as_int), p);
#pragma unroll
      for (int j = 0; j < 3; ++j) lo[j] = ~d2ord(p[j]), hi[j] = d2ord(p[j]);
    }
  }
  int b0;
  const bool uniform = wave_uniform_scene(i < n, scene, b0);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    scene_max(stats, kPMin + j, scene, b0, uniform, lo[j]);
    scene_max(stats, kPMax + j, scene, b0, uniform, hi[j]);
  }
}

__global__ __launch_bounds__(kBlock) void seg_crop_boxes_kernel(const void *__restrict__ coords, bool as_int, int64_t n,
                                                                const int *__restrict__ scene_offsets, int n_scenes,
                                                                const double *__restrict__ params, uint64_t *__restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int scene = 0;
  uint64_t mask = 0u;
  if (i < n) {
    scene = scene_of(scene_offsets, n_scenes, i);
    const double *P = params + (int64_t)scene * MINK_SEGAUG_PARAMS;
    double pmin[3], range[3];
    if (crop_frame(P, stats + (int64_t)kStatStride * scene, pmin, range)) {
      double p[3];
      pre_crop(P, load_coord(coords, i, as_int), p);
      const int tries = (int)P[MINK_SEGAUG_CROP_TRIES];
      for (int k = 0; k < tries; ++k)
        if (in_box(P, p, pmin, range, k)) mask |= 1ull << k;
    }
  }
  int b0;
  const bool uniform = wave_uniform_scene(i < n, scene, b0);
  if (uniform) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mask |= (uint64_t)__shfl_xor((unsigned long long)mask, d);
    uint64_t *a = stats + (int64_t)kStatStride * b0 + kBoxes;
    if ((threadIdx.x & 63) == 0 && (mask & ~__atomic_load_n(a, __ATOMIC_RELAXED)) != 0u) atomicOr((unsigned long long *)a, (unsigned long long)mask);
  } else if (mask != 0u) {
    atomicOr((unsigned long long *)(stats + (int64_t)kStatStride * scene + kBoxes), (unsigned long long)mask);
  }
}

// a row up to the flip: (kept, alive at the flip, q)
__device__ __forceinline__ void front(const double *__restrict__ P, const uint64_t *__restrict__ st, float4 c4, float coin,
                                      bool &keep, bool &alive, double q[3]) {
  double p[3];
  pre_crop(P, c4, p);
  const bool in = in_crop(P, st, p);
  const bool lives = (double)coin >= P[MINK_SEGAUG_DROPOUT];
  keep = in && lives;
  alive = in && (lives || P[MINK_SEGAUG_FLIP_ALL] != 0.0);
  affine(p, P + MINK_SEGAUG_A1, P + MINK_SEGAUG_a1, q);
}

__global__ __launch_bounds__(kBlock) void seg_count_kernel(const void *__restrict__ coords, bool as_int, int64_t n,
                                                           const int *__restrict__ scene_offsets, int n_scenes,
                                                           const double *__restrict__ params, const uint32_t *__restrict__ streams,
                                                           uint32_t k0, uint32_t k1, int *__restrict__ block_counts,
                                                           uint64_t *__restrict__ stats) {
  __shared__ int s_count[kBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool keep = false;
  int scene = 0;
  uint64_t ord[3] = {0u, 0u, 0u};
  if (i < n) {
    const int b = scene = scene_of(scene_offsets, n_scenes, i);
    const double *P = params + (int64_t)b * MINK_SEGAUG_PARAMS;
    const Philox r = philox4x32_10((uint32_t)(i - scene_offsets[b]), 0u, streams[b], 0u, k0, k1);
    bool alive;
    double q[3];
    front(P, stats + (int64_t)kStatStride * b, load_coord(coords, i, as_int), u01(r.x), keep, alive, q);
    if (alive) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (P[MINK_SEGAUG_FLIP + j] != 0.0) ord[j] = d2ord(q[j]);
    }
  }
  int b0;
  const bool uniform = wave_uniform_scene(i < n, scene, b0);
#pragma unroll
  for (int j = 0; j < 3; ++j) scene_max(stats, kQMax + j, scene, b0, uniform, ord[j]);
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) t += s_count[w];
    block_counts[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(kBlock) void seg_apply_kernel(
    const void *__restrict__ coords, bool as_int, const float *__restrict__ feats, int64_t ldf, int C, int64_t n,
    const int *__restrict__ scene_offsets, int n_scenes, const double *__restrict__ params,
    const uint32_t *__restrict__ streams, uint32_t k0, uint32_t k1, const int *__restrict__ block_offsets,
    const uint64_t *__restrict__ stats, RawCols cols, float *__restrict__ out_coords, double *__restrict__ out_r,
    int32_t *__restrict__ out_rows, float *__restrict__ out_feats, int64_t ldo) {
#pragma clang fp contract(off)
  __shared__ int s_wave[kBlock / 64];
  __shared__ int s_dst[kBlock];  // output row of each row of this block, -1 = dropped
  __shared__ int s_scene[kBlock];
  __shared__ uint32_t s_vox[kBlock];
  __shared__ int s_lo[kBlock], s_hi[kBlock], s_start[kBlock];
  __shared__ float s_std[kBlock];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool keep = false;
  int b = 0;
  uint32_t vox = 0;
  const double *P = params;
  float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
  double q[3] = {0.0, 0.0, 0.0};
  if (i < n) {
    b = scene_of(scene_offsets, n_scenes, i);
    P = params + (int64_t)b * MINK_SEGAUG_PARAMS;
    vox = (uint32_t)(i - scene_offsets[b]);
    const Philox r = philox4x32_10(vox, 0u, streams[b], 0u, k0, k1);
    c4 = load_coord(coords, i, as_int);
    bool alive;
    front(P, stats + (int64_t)kStatStride * b, c4, u01(r.x), keep, alive, q);
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  int rank = block_offsets[blockIdx.x] + wave_rank(m);
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) rank += s_wave[w];
  s_dst[threadIdx.x] = keep ? rank : -1;
  s_scene[threadIdx.x] = b;
  s_vox[threadIdx.x] = vox;
  {  // raw columns [lo, hi) of this row take noise of scale s_std (an empty range without feature jitter)
    const bool fj = keep && P[MINK_SEGAUG_FEAT_STD] != 0.0;
    const int start = (int)P[MINK_SEGAUG_FEAT_START], lo = fj ? max(start, 0) : 0;
    s_lo[threadIdx.x] = lo;
    s_hi[threadIdx.x] = fj ? max(start + (int)P[MINK_SEGAUG_FEAT_DIM], lo) : 0;
    s_start[threadIdx.x] = fj ? start : 0;
    s_std[threadIdx.x] = fj ? (float)P[MINK_SEGAUG_FEAT_STD] : 0.f;
  }
  if (keep) {
    const uint64_t *st = stats + (int64_t)kStatStride * b;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (P[MINK_SEGAUG_FLIP + j] != 0.0) q[j] = ord2d(st[kQMax + j]) - q[j];
    double r[3];
    affine(q, P + MINK_SEGAUG_B, P + MINK_SEGAUG_b, r);
    *reinterpret_cast<float4 *>(out_coords + 4 * (int64_t)rank) = make_float4(c4.x, (float)r[0], (float)r[1], (float)r[2]);
    if (out_r) {
#pragma unroll
      for (int j = 0; j < 3; ++j) out_r[3 * (int64_t)rank + j] = r[j];
    }
    out_rows[rank] = (int32_t)i;
  }
  __syncthreads();
  // features: as augment_apply_kernel -- the block copies its [256, C] slab, then one thread per (row, Philox draw)
  // writes the four noise columns of that draw
  const int64_t row0 = (int64_t)blockIdx.x * kBlock;
  const int rows = (int)min((int64_t)kBlock, n - row0);
#pragma unroll 4
  for (int idx = threadIdx.x; idx < rows * C; idx += kBlock) {
    const int v = idx / C, col = idx - v * C;
    const int dst = s_dst[v], raw = cols.raw[col];
    if (dst < 0 || (raw >= s_lo[v] && raw < s_hi[v])) continue;
    out_feats[(int64_t)dst * ldo + col] = feats[(row0 + v) * ldf + col];
  }
  for (int idx = threadIdx.x; idx < rows * kDraws; idx += kBlock) {
    const int v = idx / kDraws, d = idx - v * kDraws;
    const int dst = s_dst[v];
    if (dst < 0) continue;
    const float std = s_std[v];
    const int start = s_start[v], dim = s_hi[v] - start;
    if (std == 0.f || 4 * d >= dim) continue;
    const Philox g = philox4x32_10(s_vox[v], 1u + (uint32_t)d, streams[s_scene[v]], 0u, k0, k1);
    float z[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t wa = h ? g.z : g.x, wb = h ? g.w : g.y;
      const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;  // (0,1]
      const float rad = sqrtf(-2.f * logf(u1)), ang = 6.283185307179586f * u01(wb);
      float sn, cs;
      sincosf(ang, &sn, &cs);
      z[2 * h] = rad * cs, z[2 * h + 1] = rad * sn;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * d + e, raw = start + j;
      if (j >= dim || raw < 0 || raw >= MINK_AUG_MAX_CHANNELS) continue;
      const int col = cols.inv[raw];
      if (col < 0) continue;
      out_feats[(int64_t)dst * ldo + col] = feats[(row0 + v) * ldf + col] + (z[e] - 0.5f) * std;  // "randn - 0.5" (:36)
    }
  }
}

// ------------------------------------------------------------------ elastic distortion
__device__ __forceinline__ double granularity(const double *__restrict__ P, int pass) { return P[MINK_SEGAUG_ELASTIC + 2 * pass]; }

// min / max of the survivors of the scenes that run this pass (survivors of one scene are contiguous)
__global__ __launch_bounds__(kBlock) void seg_elastic_bounds_kernel(const double *__restrict__ r, const int32_t *__restrict__ rows,
                                                                    const int32_t *__restrict__ status, int64_t n,
                                                                    const int *__restrict__ scene_offsets, int n_scenes,
                                                                    const double *__restrict__ params, int pass,
                                                                    uint64_t *__restrict__ stats) {
  const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool valid = o < n && o < (int64_t)status[0];
  int scene = 0;
  uint64_t lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
  if (valid) {
    scene = scene_of(scene_offsets, n_scenes, rows[o]);
    if (granularity(params + (int64_t)scene * MINK_SEGAUG_PARAMS, pass) > 0.0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) lo[j] = ~d2ord(r[3 * o + j]), hi[j] = d2ord(r[3 * o + j]);
    }
  }
  int b0;
  const bool uniform = wave_uniform_scene(valid, scene, b0);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    scene_max(stats, kEMin + 6 * pass + j, scene, b0, uniform, lo[j]);
    scene_max(stats, kEMax + 6 * pass + j, scene, b0, uniform, hi[j]);
  }
}

// one thread: the grid of every scene for this pass -- dims (0 = not run), node offsets and mode.  A grid within the
// caller's bound is stored in the workspace; one over it (e.g. a scene whose crop kept no box and so its full extent)
// is evaluated directly at every point instead (seg_interp_kernel) and counted in status[1]; a dim over kMaxDim (or
// NaN) cannot be keyed and is counted in status[2].
__global__ void seg_grid_plan_kernel(const double *__restrict__ params, int n_scenes, int pass, int64_t grid_nodes,
                                     uint64_t *__restrict__ stats, int64_t *__restrict__ goff, int32_t *__restrict__ status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t off = 0;
  for (int b = 0; b < n_scenes; ++b) {
    const double *P = params + (int64_t)b * MINK_SEGAUG_PARAMS;
    uint64_t *st = stats + (int64_t)kStatStride * b;
    int64_t bound[3], cap = 1;
    for (int j = 0; j < 3; ++j) {
      const double v = P[MINK_SEGAUG_GRID_BOUND + j];
      bound[j] = v >= 1.0 && v < 65536.0 ? (int64_t)v : 0;
      cap *= bound[j];
    }
    goff[b] = off;
    int64_t dims[3] = {0, 0, 0};
    uint64_t mode = 0;
    const double g = granularity(P, pass);
    if (g > 0.0 && st[kEMax + 6 * pass] != 0u) {
      bool keyable = true, fits = off + cap <= grid_nodes;
      for (int j = 0; j < 3; ++j) {
        const double lo = ord2d(~st[kEMin + 6 * pass + j]), hi = ord2d(st[kEMax + 6 * pass + j]);
        const double d = floor((hi - lo) / g) + 3.0;
        if (!(d <= kMaxDim)) keyable = false;  // (NaN included)
        else dims[j] = (int64_t)d;
        if (!(d <= (double)bound[j])) fits = false;
      }
      if (!keyable) {
        dims[0] = dims[1] = dims[2] = 0;
        status[2] += 1;
      } else if (fits) {
        mode = kModeGrid;
      } else {
        mode = kModeDirect;
        status[1] += 1;
      }
    }
    for (int j = 0; j < 3; ++j) st[kDims + j] = (uint64_t)dims[j];
    st[kGridMode] = mode;
    off += cap;
  }
  goff[n_scenes] = off;
}

// grid node t of the whole batch -> (scene, node within the scene's grid); false = beyond the scene's grid
__device__ __forceinline__ bool grid_node(int64_t t, const int64_t *__restrict__ goff, int n_scenes,
                                          const uint64_t *__restrict__ stats, int &b, int64_t &local, int64_t d[3]) {
  int lo = 0, hi = n_scenes;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (goff[mid] <= t) lo = mid;
    else hi = mid;
  }
  b = lo;
  local = t - goff[b];
  const uint64_t *st = stats + (int64_t)kStatStride * b;
  d[0] = (int64_t)st[kDims], d[1] = (int64_t)st[kDims + 1], d[2] = (int64_t)st[kDims + 2];
  return st[kGridMode] == kModeGrid && local < d[0] * d[1] * d[2];
}

// the N(0,1) noise of grid node (ix, iy, iz) of an elastic pass (Philox counter (ix | iy << 16, iz | pass << 16, stream, 1))
__device__ __forceinline__ void node_noise(uint32_t ix, uint32_t iy, uint32_t iz, int pass, uint32_t stream, uint32_t k0,
                                           uint32_t k1, float out[3]) {
  const Philox r = philox4x32_10(ix | (iy << 16), iz | ((uint32_t)pass << 16), stream, 1u, k0, k1);
  const double u1a = (double)((r.x >> 8) + 1u) * 0x1p-24, u1b = (double)((r.z >> 8) + 1u) * 0x1p-24;  // (0,1]
  const double ra = sqrt(-2.0 * log(u1a)), rb = sqrt(-2.0 * log(u1b));
  const double aa = 6.283185307179586 * (double)(r.y >> 8) * 0x1p-24, ab = 6.283185307179586 * (double)(r.w >> 8) * 0x1p-24;
  out[0] = (float)(ra * cos(aa)), out[1] = (float)(ra * sin(aa)), out[2] = (float)(rb * cos(ab));
}

// weight of node j in node i of one axis after the 3-tap box twice, zero outside [0, D): #{k in [0, D) : |k - i| <= 1,
// |k - j| <= 1} / 9 (i, j in [0, D))
__device__ __forceinline__ int64_t box2_count(int64_t i, int64_t j, int64_t D) {
  return max(min(min(i, j) + 1, D - 1) - max(max(i, j) - 1, (int64_t)0) + 1, (int64_t)0);
}

__global__ __launch_bounds__(kBlock) void seg_noise_kernel(int64_t grid_nodes, const int64_t *__restrict__ goff, int n_scenes,
                                                           const uint64_t *__restrict__ stats, const uint32_t *__restrict__ streams,
                                                           uint32_t k0, uint32_t k1, int pass, float *__restrict__ grid) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= grid_nodes) return;
  int b;
  int64_t local, d[3];
  if (!grid_node(t, goff, n_scenes, stats, b, local, d)) return;
  node_noise((uint32_t)(local / (d[1] * d[2])), (uint32_t)(local / d[2] % d[1]), (uint32_t)(local % d[2]), pass, streams[b], k0, k1,
             grid + 3 * t);
}

// dst = B_axis^2 src, B = 3-tap box (1/3) with zeros outside the grid: the weight of node j in node i is
// #{k in the grid : |k - i| <= 1, |k - j| <= 1} / 9
__global__ __launch_bounds__(kBlock) void seg_blur_kernel(int64_t grid_nodes, const int64_t *__restrict__ goff, int n_scenes,
                                                          const uint64_t *__restrict__ stats, int axis,
                                                          const float *__restrict__ src, float *__restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= grid_nodes) return;
  int b;
  int64_t local, d[3];
  if (!grid_node(t, goff, n_scenes, stats, b, local, d)) return;
  const int64_t stride = axis == 0 ? d[1] * d[2] : axis == 1 ? d[2] : 1;
  const int64_t D = d[axis], i = local / stride % D;
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int s = -2; s <= 2; ++s) {
    const int64_t j = i + s;
    if (j < 0 || j >= D) continue;
    const int64_t w = box2_count(i, j, D);
    if (w == 0) continue;
    const float *v = src + 3 * (t + s * stride);
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += (double)w * (double)v[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[3 * t + c] = (float)(acc[c] / 9.0);
}

__global__ __launch_bounds__(kBlock) void seg_interp_kernel(double *__restrict__ r, float *__restrict__ out_coords,
                                                            const int32_t *__restrict__ rows, const int32_t *__restrict__ status,
                                                            int64_t n, const int *__restrict__ scene_offsets, int n_scenes,
                                                            const double *__restrict__ params, int pass,
                                                            const uint64_t *__restrict__ stats, const int64_t *__restrict__ goff,
                                                            const float *__restrict__ grid, const uint32_t *__restrict__ streams,
                                                            uint32_t k0, uint32_t k1) {
  const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (o >= n || o >= (int64_t)status[0]) return;
  const int b = scene_of(scene_offsets, n_scenes, rows[o]);
  const double *P = params + (int64_t)b * MINK_SEGAUG_PARAMS;
  const uint64_t *st = stats + (int64_t)kStatStride * b;
  const int64_t d[3] = {(int64_t)st[kDims], (int64_t)st[kDims + 1], (int64_t)st[kDims + 2]};
  if (d[0] == 0) return;  // pass not drawn by this scene (or not keyable: reported in status[2])
  const double g = granularity(P, pass), mag = P[MINK_SEGAUG_ELASTIC + 2 * pass + 1];
  int64_t i0[3];
  double f[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double t = (r[3 * o + j] - ord2d(~st[kEMin + 6 * pass + j])) / g + 1.0;  // node i sits at lo - g + i g
    if (!(t >= 0.0 && t <= (double)(d[j] - 1))) return;  // outside the grid's box: no displacement (fill_value 0)
    const double fl = floor(t);
    i0[j] = (int64_t)fl, f[j] = t - fl;
  }
  double acc[3] = {0.0, 0.0, 0.0};
  if (st[kGridMode] == kModeDirect) {
    // no stored grid: the blurred noise of the 8 corner nodes, straight from the noise of the 6^3 nodes around them.
    // W[j][a] = weight of node i0 - 2 + a along axis j = sum over the two corners of (trilinear weight) * (blur weight)
    double W[3][6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const int64_t node = i0[j] - 2 + a;
        double w = 0.0;
        if (node >= 0 && node < d[j]) {
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int64_t corner = i0[j] + c;
            if (corner < d[j] && corner - node <= 2 && node - corner <= 2)
              w += (c ? f[j] : 1.0 - f[j]) * (double)box2_count(corner, node, d[j]) / 9.0;
          }
        }
        W[j][a] = w;
      }
    }
    const uint32_t stream = streams[b];
    for (int a = 0; a < 6; ++a) {
      if (W[0][a] == 0.0) continue;
      for (int bb = 0; bb < 6; ++bb) {
        const double wxy = W[0][a] * W[1][bb];
        if (wxy == 0.0) continue;
        for (int c = 0; c < 6; ++c) {
          if (W[2][c] == 0.0) continue;
          float v[3];
          node_noise((uint32_t)(i0[0] - 2 + a), (uint32_t)(i0[1] - 2 + bb), (uint32_t)(i0[2] - 2 + c), pass, stream, k0, k1, v);
#pragma unroll
          for (int e = 0; e < 3; ++e) acc[e] += wxy * W[2][c] * (double)v[e];
        }
      }
    }
  } else {
    const float *G = grid + 3 * goff[b];
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
      const int64_t x = i0[0] + (corner >> 2), y = i0[1] + ((corner >> 1) & 1), z = i0[2] + (corner & 1);
      if (x < 0 || x >= d[0] || y < 0 || y >= d[1] || z < 0 || z >= d[2]) continue;
      const double w = ((corner >> 2) ? f[0] : 1.0 - f[0]) * (((corner >> 1) & 1) ? f[1] : 1.0 - f[1]) * ((corner & 1) ? f[2] : 1.0 - f[2]);
      const float *v = G + 3 * ((x * d[1] + y) * d[2] + z);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += w * (double)v[c];
    }
  }
  double out[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = r[3 * o + j] + mag * acc[j], r[3 * o + j] = out[j];
  out_coords[4 * o + 1] = (float)out[0], out_coords[4 * o + 2] = (float)out[1], out_coords[4 * o + 3] = (float)out[2];
}

struct SegWorkspace {
  int *block_counts, *block_offsets;
  uint64_t *stats;
  int64_t *goff;
  double *r;
  float *grid0, *grid1;
};

SegWorkspace seg_workspace(void *ws, int64_t n, int32_t n_scenes, int64_t grid_nodes, int64_t *total) {
  const int64_t nb = cdiv(n > 0 ? n : 1, kBlock);
  char *p = (char *)ws;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char *q = p ? p + off : nullptr;
    off += align_up(bytes, 256);
    return q;
  };
  SegWorkspace w;
  w.block_counts = (int *)take(2 * nb * 4);
  w.block_offsets = w.block_counts ? w.block_counts + nb : nullptr;
  w.stats = (uint64_t *)take((int64_t)n_scenes * kStatStride * 8);
  w.goff = (int64_t *)take(((int64_t)n_scenes + 1) * 8);
  w.r = (double *)take(3 * n * 8);
  w.grid0 = (float *)take(3 * grid_nodes * 4);
  w.grid1 = (float *)take(3 * grid_nodes * 4);
  *total = off;
  return w;
}

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_augment_seg_workspace_bytes(int64_t n, int32_t n_scenes, int64_t grid_nodes) {
  int64_t total = 0;
  seg_workspace(nullptr, n, n_scenes, grid_nodes > 0 ? grid_nodes : 0, &total);
  return total;
}

int mink_augment_seg_scenes(const void *coords, int32_t coords_are_int32, const float *feats, int64_t ldf, int32_t C, int64_t n,
                            const int32_t *scene_offsets, int32_t n_scenes, const double *params, const uint32_t *streams,
                            uint64_t seed, const int32_t *raw_cols, int32_t n_elastic, int64_t grid_nodes, float *out_coords,
                            float *out_feats, int64_t ldo, int32_t *out_rows, int32_t *status, void *workspace,
                            int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(n >= 0 && n < (int64_t)1 << 31 && n_scenes >= 1 && C >= 1 && C <= MINK_AUG_MAX_CHANNELS && ldf >= C && ldo >= C,
               "augment_seg_scenes: bad shape (n %lld, scenes %d, C %d, ldf %lld, ldo %lld; at most %d channels)", (long long)n,
               n_scenes, C, (long long)ldf, (long long)ldo, MINK_AUG_MAX_CHANNELS);
  MINK_REQUIRE(n_elastic >= 0 && n_elastic <= MINK_SEGAUG_MAX_ELASTIC, "augment_seg_scenes: %d elastic passes (at most %d)",
               n_elastic, MINK_SEGAUG_MAX_ELASTIC);
  MINK_REQUIRE(grid_nodes >= 0 && grid_nodes < ((int64_t)1 << 31) / 3, "augment_seg_scenes: %lld grid nodes", (long long)grid_nodes);
  MINK_REQUIRE(workspace_bytes >= mink_augment_seg_workspace_bytes(n, n_scenes, grid_nodes) || n == 0,
               "augment_seg_scenes: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)mink_augment_seg_workspace_bytes(n, n_scenes, grid_nodes));
  MINK_REQUIRE(status && raw_cols, "augment_seg_scenes: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  MINK_HIP(hipMemsetAsync(status, 0, 3 * sizeof(int32_t), s));
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(coords && feats && scene_offsets && params && streams && out_coords && out_feats && out_rows && workspace,
               "augment_seg_scenes: NULL pointer");
  MINK_REQUIRE((((uintptr_t)coords | (uintptr_t)out_coords) & 15) == 0, "augment_seg_scenes: coordinates must be 16-byte aligned");
  MINK_REQUIRE(coords != (const void *)out_coords && feats != out_feats, "augment_seg_scenes: not an in-place operation");
  RawCols cols;
  for (int c = 0; c < MINK_AUG_MAX_CHANNELS; ++c) cols.raw[c] = c < C ? raw_cols[c] : -1, cols.inv[c] = -1;
  for (int c = 0; c < C; ++c) {
    MINK_REQUIRE(cols.raw[c] < MINK_AUG_MAX_CHANNELS, "augment_seg_scenes: raw column %d of feature column %d", cols.raw[c], c);
    if (cols.raw[c] >= 0) {
      MINK_REQUIRE(cols.inv[cols.raw[c]] < 0, "augment_seg_scenes: raw column %d is selected twice", cols.raw[c]);
      cols.inv[cols.raw[c]] = c;
    }
  }
  int64_t total = 0;
  const SegWorkspace w = seg_workspace(workspace, n, n_scenes, grid_nodes, &total);
  const int nb = (int)cdiv(n, kBlock);
  const bool as_int = coords_are_int32 != 0;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  MINK_HIP(hipMemsetAsync(w.stats, 0, (size_t)n_scenes * kStatStride * 8, s));
  seg_crop_bounds_kernel<<<nb, kBlock, 0, s>>>(coords, as_int, n, scene_offsets, n_scenes, params, w.stats);
  MINK_CHECK_LAUNCH();
  seg_crop_boxes_kernel<<<nb, kBlock, 0, s>>>(coords, as_int, n, scene_offsets, n_scenes, params, w.stats);
  MINK_CHECK_LAUNCH();
  seg_count_kernel<<<nb, kBlock, 0, s>>>(coords, as_int, n, scene_offsets, n_scenes, params, streams, k0, k1, w.block_counts, w.stats);
  MINK_CHECK_LAUNCH();
  augment_scan_kernel<<<1, kBlock, 0, s>>>(w.block_counts, nb, w.block_offsets, status);
  MINK_CHECK_LAUNCH();
  seg_apply_kernel<<<nb, kBlock, 0, s>>>(coords, as_int, feats, ldf, C, n, scene_offsets, n_scenes, params, streams, k0, k1,
                                         w.block_offsets, w.stats, cols, out_coords, n_elastic > 0 ? w.r : nullptr, out_rows,
                                         out_feats, ldo);
  MINK_CHECK_LAUNCH();
  const int gb = (int)cdiv(grid_nodes > 0 ? grid_nodes : 1, kBlock);
  for (int pass = 0; pass < n_elastic; ++pass) {
    seg_elastic_bounds_kernel<<<nb, kBlock, 0, s>>>(w.r, out_rows, status, n, scene_offsets, n_scenes, params, pass, w.stats);
    MINK_CHECK_LAUNCH();
    seg_grid_plan_kernel<<<1, 64, 0, s>>>(params, n_scenes, pass, grid_nodes, w.stats, w.goff, status);
    MINK_CHECK_LAUNCH();
    if (grid_nodes > 0) {
      seg_noise_kernel<<<gb, kBlock, 0, s>>>(grid_nodes, w.goff, n_scenes, w.stats, streams, k0, k1, pass, w.grid0);
      MINK_CHECK_LAUNCH();
      seg_blur_kernel<<<gb, kBlock, 0, s>>>(grid_nodes, w.goff, n_scenes, w.stats, 0, w.grid0, w.grid1);
      MINK_CHECK_LAUNCH();
      seg_blur_kernel<<<gb, kBlock, 0, s>>>(grid_nodes, w.goff, n_scenes, w.stats, 1, w.grid1, w.grid0);
      MINK_CHECK_LAUNCH();
      seg_blur_kernel<<<gb, kBlock, 0, s>>>(grid_nodes, w.goff, n_scenes, w.stats, 2, w.grid0, w.grid1);
      MINK_CHECK_LAUNCH();
    }
    seg_interp_kernel<<<nb, kBlock, 0, s>>>(w.r, out_coords, out_rows, status, n, scene_offsets, n_scenes, params, pass, w.stats,
                                            w.goff, w.grid1, streams, k0, k1);
    MINK_CHECK_LAUNCH();
  }
  return MINK_OK;
}

}  // extern "C"
