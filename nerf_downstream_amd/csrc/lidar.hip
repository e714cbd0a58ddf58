// LiDAR scans of the segmentation family (the reference's SemanticKITTIDataset, co3d_3d/src/data/semantic_kitti.py:165-222):
// what its loader does to a raw scan before and after the recipe, for a whole batch (include/mink_hip.h, "LiDAR scans").
//
//   decode : per row, the .bin record (x, y, z, intensity) -> coordinates (scene, x, y, z) and features (x, y, z, intensity),
//            the .label word -> lut[word & 0xFFFF] (the class BEFORE the voxel vote; the instance id in the upper half goes)
//   finish : per row below the survivor count the program left on the device, the transformed metric coordinates go into
//            three feature columns and the coordinates are divided by the voxel size
//
// Conventions of rowpass.h: a thread owns one row, rows move as one 16-byte access (VEC = 4) when every pointer and pitch
// involved is a multiple of 16 bytes and as dwords (VEC = 1) otherwise; every output element is written once, by one thread,
// from that row's inputs alone, so results are bitwise identical run to run.  The only atomic is the count of semantic ids
// the table does not hold (an integer sum, taken on that error path alone).
#include "rowpass.h"

namespace mink {
namespace {

constexpr int LB = 256;  // threads per workgroup

template <int VEC>
__global__ __launch_bounds__(LB) void lidar_decode_kernel(const float *__restrict__ scan, const uint32_t *__restrict__ raw_labels,
                                                          int64_t n, const int *__restrict__ scene_offsets, int n_scenes,
                                                          const int32_t *__restrict__ lut, int lut_size, int32_t ignore_label,
                                                          float *__restrict__ coords, float *__restrict__ feats, int64_t ldo,
                                                          int32_t *__restrict__ labels, int32_t *__restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * LB + threadIdx.x;
  if (i >= n) return;
  float p[4];
  if constexpr (VEC == 4) {
    ldv<4>(scan + 4 * i, p);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = scan[4 * i + j];
  }
  const float c[4] = {(float)sample_of(scene_offsets, n_scenes, i), p[0], p[1], p[2]};
  if constexpr (VEC == 4) {
    stv<4>(coords + 4 * i, c);
    stv<4>(feats + i * ldo, p);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) coords[4 * i + j] = c[j], feats[i * ldo + j] = p[j];
  }
  const uint32_t id = raw_labels ? (raw_labels[i] & 0xFFFFu) : 0u;  // (no .label file: every word is 0)
  if (id < (uint32_t)lut_size) {
    labels[i] = lut[id];
  } else {
    labels[i] = ignore_label;
    atomicAdd(status, 1);
  }
}

template <int VEC>
__global__ __launch_bounds__(LB) void lidar_finish_kernel(float *__restrict__ coords, int64_t n, const int32_t *__restrict__ n_rows,
                                                          float voxel_size, float *__restrict__ feats, int64_t ldf, int c0) {
  const int64_t i = (int64_t)blockIdx.x * LB + threadIdx.x;
  if (i >= n || i >= (int64_t)*n_rows) return;
  float c[4];
  if constexpr (VEC == 4) {
    float f[4];
    ldv<4>(coords + 4 * i, c);
    ldv<4>(feats + i * ldf + c0, f);  // (c0 % 4 == 0 and ldf % 4 == 0: the group lies inside the row; its 4th column goes back as read)
    f[0] = c[1], f[1] = c[2], f[2] = c[3];
    stv<4>(feats + i * ldf + c0, f);
    const float v[4] = {c[0], c[1] / voxel_size, c[2] / voxel_size, c[3] / voxel_size};
    stv<4>(coords + 4 * i, v);
  } else {
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      c[j] = coords[4 * i + j];
      feats[i * ldf + c0 + j - 1] = c[j];
      coords[4 * i + j] = c[j] / voxel_size;
    }
  }
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  (an absent, NULL operand shares none)
static inline bool ranges_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && na > 0 && nb > 0 && pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int mink_lidar_decode_scans(const float *scan, const uint32_t *raw_labels, int64_t n, const int32_t *scene_offsets, int32_t n_scenes,
                            const int32_t *lut, int32_t lut_size, int32_t ignore_label, float *coords, float *feats, int64_t ldo,
                            int32_t *labels, int32_t *status, void *stream) {
  MINK_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) - 1 && n_scenes >= 1 && n_scenes <= 65535 && lut_size >= 0 && lut_size <= 65536 &&
                   ldo >= 4,
               "lidar_decode_scans: bad shape (n %lld, scenes %d, table of %d, ldo %lld; ldo >= 4)", (long long)n, n_scenes, lut_size,
               (long long)ldo);
  MINK_REQUIRE(status, "lidar_decode_scans: NULL status word");
  hipStream_t s = (hipStream_t)stream;
  MINK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(scan && scene_offsets && (lut || lut_size == 0) && coords && feats && labels, "lidar_decode_scans: NULL pointer");
  {  // the kernel's pointers are __restrict__: no output range may share a byte with an input's or another output's
    const void *in[2] = {scan, raw_labels}, *out[3] = {coords, feats, labels};
    const int64_t in_bytes[2] = {16 * n, 4 * n}, out_bytes[3] = {16 * n, 4 * n * ldo, 4 * n};
    for (int o = 0; o < 3; ++o) {
      for (int i = 0; i < 2; ++i)
        MINK_REQUIRE(!ranges_overlap(in[i], in_bytes[i], out[o], out_bytes[o]), "lidar_decode_scans: an output overlaps an input");
      for (int p = 0; p < o; ++p)
        MINK_REQUIRE(!ranges_overlap(out[p], out_bytes[p], out[o], out_bytes[o]), "lidar_decode_scans: two outputs overlap");
    }
  }
  const bool vec = aligned16(scan) && aligned16(coords) && aligned16(feats) && (ldo & 3) == 0;
  const unsigned nb = (unsigned)cdiv(n, LB);
  if (vec)
    lidar_decode_kernel<4><<<nb, LB, 0, s>>>(scan, raw_labels, n, scene_offsets, n_scenes, lut, lut_size, ignore_label, coords, feats,
                                             ldo, labels, status);
  else
    lidar_decode_kernel<1><<<nb, LB, 0, s>>>(scan, raw_labels, n, scene_offsets, n_scenes, lut, lut_size, ignore_label, coords, feats,
                                             ldo, labels, status);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_lidar_finish_rows(float *coords, int64_t n, const int32_t *n_rows, float voxel_size, float *feats, int64_t ldf, int32_t c0,
                           void *stream) {
  MINK_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) - 1 && c0 >= 0 && ldf >= (int64_t)c0 + 3,
               "lidar_finish_rows: bad shape (n %lld, columns [%d, %d) of a row of %lld)", (long long)n, c0, c0 + 3, (long long)ldf);
  MINK_REQUIRE(voxel_size > 0.f && voxel_size <= 3.0e38f, "lidar_finish_rows: voxel size %g (positive and finite)", (double)voxel_size);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(coords && n_rows && feats, "lidar_finish_rows: NULL pointer");
  MINK_REQUIRE(!ranges_overlap(coords, 16 * n, feats, 4 * n * ldf) && !ranges_overlap(n_rows, 4, coords, 16 * n) &&
                   !ranges_overlap(n_rows, 4, feats, 4 * n * ldf),
               "lidar_finish_rows: coordinates, features and the row count overlap");
  const bool vec = aligned16(coords) && aligned16(feats) && (ldf & 3) == 0 && (c0 & 3) == 0;
  const unsigned nb = (unsigned)cdiv(n, LB);
  hipStream_t s = (hipStream_t)stream;
  if (vec) lidar_finish_kernel<4><<<nb, LB, 0, s>>>(coords, n, n_rows, voxel_size, feats, ldf, c0);
  else lidar_finish_kernel<1><<<nb, LB, 0, s>>>(coords, n, n_rows, voxel_size, feats, ldf, c0);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
