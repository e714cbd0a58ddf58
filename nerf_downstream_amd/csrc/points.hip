// Point-cloud input of the segmentation family (the reference's ScannetDataset, co3d_3d/src/data/scannet.py:149-275):
// voxel down-sampling with label voting (include/mink_hip.h MINK_VOXDS_*) and the colour program (MINK_COLORAUG_*), for a
// whole batch.  Down-sampling launches, in order:
//
//   keys    : per row, the packed key of its voxel (batch | floor(xyz / Q)), or of the row itself when Q == 0
//   unique  : mink_coords_unique -- first-occurrence numbering: representative u is the u-th voxel by its first row
//   vote    : per voxel, min / max of its raw labels (order-preserving int32 atomics: bitwise repeatable)
//   gather  : coordinates / VOXEL, features, voted label and input row of every representative; per-scene counts
//   offsets : one thread: exclusive scan of the per-scene counts -> the row range of every scene
//
// Nothing is read back: the representative count stays on the device (status[0]), and the rows past it form one more
// "scene" [out_offsets[S], out_offsets[S+1] = n) that a following program can be told to drop.
#include "augment_common.h"

namespace mink {
namespace {

__device__ __forceinline__ uint32_t label_ord(int32_t l) { return (uint32_t)l ^ 0x80000000u; }
__device__ __forceinline__ int32_t ord_label(uint32_t u) { return (int32_t)(u ^ 0x80000000u); }

__global__ __launch_bounds__(kBlock) void vds_keys_kernel(const float *__restrict__ coords, int64_t n,
                                                          const int *__restrict__ scene_offsets, int n_scenes,
                                                          const double *__restrict__ params, uint64_t *__restrict__ keys,
                                                          uint32_t *__restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int b = scene_of(scene_offsets, n_scenes, i);
  const float q = (float)params[(int64_t)b * MINK_VOXDS_PARAMS + MINK_VOXDS_Q];
  if (!(q > 0.f)) {  // no down-sampling: the row is its own voxel (the batch field keeps scenes apart)
    keys[i] = ((uint64_t)(unsigned)b << 48) | (uint64_t)(i - scene_offsets[b]);
    return;
  }
  const float4 c = *reinterpret_cast<const float4 *>(coords + 4 * i);
  const float f[3] = {floorf(c.y / q), floorf(c.z / q), floorf(c.w / q)};
  int k[3];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const bool in = f[j] >= -32768.f && f[j] <= 32767.f;  // (false for NaN)
    k[j] = in ? (int)f[j] : 0;
    ok = ok && in;
  }
  uint64_t key;
  ok = pack_key(b, k[0], k[1], k[2], key) && ok;
  if (!ok) atomicOr(status + 1, MINK_STATUS_RANGE);
  keys[i] = key;
}

__global__ __launch_bounds__(kBlock) void vds_vote_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ inverse,
                                                          int64_t n, uint32_t *__restrict__ lab_min, uint32_t *__restrict__ lab_max) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int u = inverse[i];
  const uint32_t l = label_ord(labels[i]);
  atomicMin(lab_min + u, l);
  atomicMax(lab_max + u, l);
}

__global__ __launch_bounds__(kBlock) void vds_gather_kernel(
    const float *__restrict__ coords, const float *__restrict__ feats, int64_t ldf, int C, int64_t n,
    const int *__restrict__ scene_offsets, int n_scenes, const double *__restrict__ params, const int32_t *__restrict__ unique_index,
    const int32_t *__restrict__ n_unique, const uint32_t *__restrict__ lab_min, const uint32_t *__restrict__ lab_max,
    float *__restrict__ out_coords, float *__restrict__ out_feats, int64_t ldo, int32_t *__restrict__ out_labels,
    int32_t *__restrict__ out_rows, int32_t *__restrict__ counts) {
  const int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (u >= n || u >= (int64_t)*n_unique) return;
  const int64_t rep = unique_index[u];
  const int b = scene_of(scene_offsets, n_scenes, rep);
  const double *P = params + (int64_t)b * MINK_VOXDS_PARAMS;
  const float vs = (float)P[MINK_VOXDS_VOXEL];
  const float4 c = *reinterpret_cast<const float4 *>(coords + 4 * rep);
  *reinterpret_cast<float4 *>(out_coords + 4 * u) = make_float4(c.x, c.y / vs, c.z / vs, c.w / vs);
  for (int j = 0; j < C; ++j) out_feats[u * ldo + j] = feats[rep * ldf + j];
  const uint32_t lo = lab_min[u], hi = lab_max[u];
  out_labels[u] = lo == hi ? ord_label(lo) : (int32_t)P[MINK_VOXDS_IGNORE];
  out_rows[u] = (int32_t)rep;
  atomicAdd(counts + b + 1, 1);
}

__global__ void vds_offsets_kernel(int32_t *__restrict__ offsets, int n_scenes, int64_t n) {
  if (threadIdx.x != 0) return;
  offsets[0] = 0;
  for (int b = 0; b < n_scenes; ++b) offsets[b + 1] += offsets[b];
  offsets[n_scenes + 1] = (int32_t)n;
}

struct VdsWorkspace {
  uint64_t *keys, *table_keys;
  int32_t *table_vals, *ucoords, *unique_index, *inverse;
  uint32_t *lab_min, *lab_max;
  void *unique_ws;
  int64_t cap;
};

VdsWorkspace vds_workspace(void *ws, int64_t n, int64_t *total) {
  char *p = (char *)ws;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char *q = p ? p + off : nullptr;
    off += align_up(bytes, 256);
    return q;
  };
  VdsWorkspace w;
  w.cap = mink_table_capacity(n);
  w.keys = (uint64_t *)take(8 * n);
  w.table_keys = (uint64_t *)take(8 * w.cap);
  w.table_vals = (int32_t *)take(4 * w.cap);
  w.ucoords = (int32_t *)take(16 * n);
  w.unique_index = (int32_t *)take(4 * n);
  w.inverse = (int32_t *)take(4 * n);
  w.lab_min = (uint32_t *)take(4 * n);
  w.lab_max = (uint32_t *)take(4 * n);
  w.unique_ws = take(mink_unique_workspace_bytes(n));
  *total = off;
  return w;
}

// the three N(0,1) normals of op k of a row (Philox counter (row, k, stream, 2)), Box-Muller as the elastic grid noise
__device__ __forceinline__ void color_normals(uint32_t row, int k, uint32_t stream, uint32_t k0, uint32_t k1, double out[3]) {
  const Philox r = philox4x32_10(row, (uint32_t)k, stream, 2u, k0, k1);
  const double u1a = (double)((r.x >> 8) + 1u) * 0x1p-24, u1b = (double)((r.z >> 8) + 1u) * 0x1p-24;  // (0,1]
  const double ra = sqrt(-2.0 * log(u1a)), rb = sqrt(-2.0 * log(u1b));
  const double aa = 6.283185307179586 * (double)(r.y >> 8) * 0x1p-24, ab = 6.283185307179586 * (double)(r.w >> 8) * 0x1p-24;
  out[0] = ra * cos(aa), out[1] = ra * sin(aa), out[2] = rb * cos(ab);
}

__global__ __launch_bounds__(kBlock) void color_kernel(float *__restrict__ feats, int64_t ldf, int c0, int c1, int c2, int64_t n,
                                                       const int *__restrict__ scene_offsets, int n_scenes,
                                                       const double *__restrict__ params, const uint32_t *__restrict__ streams,
                                                       uint32_t k0, uint32_t k1, const int32_t *__restrict__ key_rows,
                                                       const int32_t *__restrict__ key_offsets) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || i >= (int64_t)scene_offsets[n_scenes]) return;
  const int b = scene_of(scene_offsets, n_scenes, i);
  const double *P = params + (int64_t)b * MINK_COLORAUG_PARAMS;
  const int count = (int)P[MINK_COLORAUG_COUNT];
  float *row = feats + i * ldf;
  const int col[3] = {c0, c1, c2};
  float c[3] = {row[c0], row[c1], row[c2]};
  for (int k = 0; k < count && k < MINK_COLORAUG_MAX_OPS; ++k) {
    const double *op = P + MINK_COLORAUG_OPS + k * MINK_COLORAUG_OP_STRIDE;
    const int kind = (int)op[0];
    if (kind == MINK_COLORAUG_TRANSLATE) {
#pragma unroll
      for (int j = 0; j < 3; ++j) c[j] = (float)fmin(fmax((double)c[j] + op[1 + j], 0.0), 255.0);
    } else if (kind == MINK_COLORAUG_JITTER) {
      double z[3];
      color_normals((uint32_t)(key_rows[i] - key_offsets[b]), k, streams[b], k0, k1, z);
#pragma unroll
      for (int j = 0; j < 3; ++j) c[j] = (float)fmin(fmax(z[j] * op[1] + (double)c[j], 0.0), 255.0);
    } else if (kind == MINK_COLORAUG_NORMALIZE) {
#pragma unroll
      for (int j = 0; j < 3; ++j) c[j] = (c[j] - (float)op[1 + j]) / (float)op[4 + j];
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) row[col[j]] = c[j];
}

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_voxel_downsample_workspace_bytes(int64_t n) {
  int64_t total = 0;
  vds_workspace(nullptr, n > 0 ? n : 1, &total);
  return total;
}

int mink_voxel_downsample_scenes(const float *coords, const float *feats, int64_t ldf, int32_t C, const int32_t *labels, int64_t n,
                                 const int32_t *scene_offsets, int32_t n_scenes, const double *params, float *out_coords,
                                 float *out_feats, int64_t ldo, int32_t *out_labels, int32_t *out_rows, int32_t *out_offsets,
                                 int32_t *status, void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) - 1 && n_scenes >= 1 && n_scenes <= 65535 && C >= 0 && ldf >= C && ldo >= C,
               "voxel_downsample_scenes: bad shape (n %lld, scenes %d, C %d, ldf %lld, ldo %lld)", (long long)n, n_scenes, C,
               (long long)ldf, (long long)ldo);
  MINK_REQUIRE(status && out_offsets, "voxel_downsample_scenes: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  MINK_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), s));
  MINK_HIP(hipMemsetAsync(out_offsets, 0, ((size_t)n_scenes + 2) * sizeof(int32_t), s));
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(coords && (feats || C == 0) && labels && scene_offsets && params && out_coords && (out_feats || C == 0) &&
                   out_labels && out_rows && workspace,
               "voxel_downsample_scenes: NULL pointer");
  MINK_REQUIRE(workspace_bytes >= mink_voxel_downsample_workspace_bytes(n), "voxel_downsample_scenes: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)mink_voxel_downsample_workspace_bytes(n));
  MINK_REQUIRE((((uintptr_t)coords | (uintptr_t)out_coords) & 15) == 0 && ((uintptr_t)workspace & 255) == 0,
               "voxel_downsample_scenes: misaligned buffer");
  MINK_REQUIRE((const void *)coords != (void *)out_coords && (C == 0 || feats != out_feats),
               "voxel_downsample_scenes: not an in-place operation");
  int64_t total = 0;
  const VdsWorkspace w = vds_workspace(workspace, n, &total);
  const int nb = (int)cdiv(n, kBlock);
  vds_keys_kernel<<<nb, kBlock, 0, s>>>(coords, n, scene_offsets, n_scenes, params, w.keys, (uint32_t *)status);
  MINK_CHECK_LAUNCH();
  int rc = mink_coords_unique(w.keys, n, w.table_keys, w.table_vals, w.cap, w.ucoords, w.unique_index, w.inverse, status,
                              w.unique_ws, mink_unique_workspace_bytes(n), stream);
  if (rc != MINK_OK) return rc;
  MINK_HIP(hipMemsetAsync(w.lab_min, 0xFF, (size_t)n * 4, s));
  MINK_HIP(hipMemsetAsync(w.lab_max, 0, (size_t)n * 4, s));
  vds_vote_kernel<<<nb, kBlock, 0, s>>>(labels, w.inverse, n, w.lab_min, w.lab_max);
  MINK_CHECK_LAUNCH();
  vds_gather_kernel<<<nb, kBlock, 0, s>>>(coords, feats, ldf, C, n, scene_offsets, n_scenes, params, w.unique_index, status, w.lab_min,
                                          w.lab_max, out_coords, out_feats, ldo, out_labels, out_rows, out_offsets);
  MINK_CHECK_LAUNCH();
  vds_offsets_kernel<<<1, 64, 0, s>>>(out_offsets, n_scenes, n);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_color_augment_scenes(float *feats, int64_t ldf, const int32_t *cols_host, int64_t n, const int32_t *scene_offsets,
                              int32_t n_scenes, const double *params, const uint32_t *streams, uint64_t seed,
                              const int32_t *key_rows, const int32_t *key_offsets, void *stream) {
  MINK_REQUIRE(n >= 0 && n < (int64_t)1 << 31 && n_scenes >= 1 && cols_host, "color_augment_scenes: bad arguments (n %lld, scenes %d)",
               (long long)n, n_scenes);
  for (int j = 0; j < 3; ++j)
    MINK_REQUIRE(cols_host[j] >= 0 && cols_host[j] < ldf, "color_augment_scenes: colour column %d outside a row of %lld", cols_host[j],
                 (long long)ldf);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(feats && scene_offsets && params && streams && key_rows && key_offsets, "color_augment_scenes: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  color_kernel<<<(int)cdiv(n, kBlock), kBlock, 0, s>>>(feats, ldf, cols_host[0], cols_host[1], cols_host[2], n, scene_offsets, n_scenes,
                                                        params, streams, k0, k1, key_rows, key_offsets);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
