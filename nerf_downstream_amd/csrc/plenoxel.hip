// PeRFception `data.npz` front-end on gfx950: a batch of Plenoxel voxel grids (links, density, quantised spherical
// harmonics) decoded into coordinate rows and feature columns on the device.
#include "coords_common.h"

using namespace mink;

// One thread per (voxel, group of four feature columns).  links -> (batch, x, y, z); features =
// the selected columns of [density | sh_q * sh_scale + sh_min (27) | ones] in the caller's order.
// "xyzs" feature of the reference loader (co3d.py:209-214): every point minus the mean of ITS OWN three coordinates (the
// reference reduces over dim=1, not over the points -- kept as it is), divided by the largest norm of the scene.  Every
// product, sum and the division are rounded separately, in the order ((x + y) + z) / 3 and sqrt((dx^2 + dy^2) + dz^2).
__device__ __forceinline__ float xyz_centred(int x, int y, int z, float (&d)[3]) {
  const float fx = (float)x, fy = (float)y, fz = (float)z;
  float s = fx + fy;
  asm volatile("" : "+v"(s));
  s = s + fz;
  asm volatile("" : "+v"(s));
  const float m = __fdiv_rn(s, 3.f);
  d[0] = fx - m, d[1] = fy - m, d[2] = fz - m;
  return m;
}

// per-scene max of the centred norm, as float bits (non-negative floats order like unsigned integers: atomicMax is exact
// and order-independent)
__global__ __launch_bounds__(kBlock) void decode_xyz_maxnorm_kernel(const int *__restrict__ links,
                                                                    const int *__restrict__ scene_offsets, int n_scenes,
                                                                    int64_t n, int ry, int rz,
                                                                    unsigned *__restrict__ scene_maxnorm) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = n_scenes;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)scene_offsets[mid] <= i) lo = mid;
    else hi = mid;
  }
  const int l = links[i];
  const int yz = ry * rz;
  const int x = l / yz, rem = l - x * yz;
  const int y = rem / rz, z = rem - y * rz;
  float d[3];
  xyz_centred(x, y, z, d);
  float a = d[0] * d[0], b2 = d[1] * d[1], c2 = d[2] * d[2];
  asm volatile("" : "+v"(a), "+v"(b2), "+v"(c2));
  float s = a + b2;
  asm volatile("" : "+v"(s));
  s = s + c2;
  asm volatile("" : "+v"(s));
  atomicMax(scene_maxnorm + lo, __float_as_uint(__fsqrt_rn(s)));
}

// The de-quantisation is a separate multiply and add (no fma): bit-identical to numpy's
// `sh.astype(float32) * sh_scale + sh_min` of the reference loader (co3d.py:160-166).
__global__ __launch_bounds__(kBlock) void decode_plenoxel_kernel(
    const int *__restrict__ links, const float *__restrict__ density, const unsigned char *__restrict__ sh_q,
    const int *__restrict__ scene_offsets, int n_scenes, const float *__restrict__ sh_scale,
    const float *__restrict__ sh_min, int64_t n, int ry, int rz, int col_density, int col_sh, int col_ones, int col_xyzs,
    const float *__restrict__ scene_maxnorm, int C, int *__restrict__ coords, float *__restrict__ feats, int ldf, bool vec) {
  const int groups = (C + 3) >> 2;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n * groups) return;
  const int64_t i = t / groups;
  const int gq = (int)(t - i * groups);
  int lo = 0, hi = n_scenes;  // scene b with scene_offsets[b] <= i < scene_offsets[b+1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)scene_offsets[mid] <= i) lo = mid;
    else hi = mid;
  }
  const int b = lo;
  const int l = links[i];
  const int yz = ry * rz;
  const int x = l / yz, rem = l - x * yz;
  const int y = rem / rz, z = rem - y * rz;
  if (gq == 0) *reinterpret_cast<int4 *>(coords + 4 * i) = make_int4(b, x, y, z);
  float ctr[3] = {0.f, 0.f, 0.f};
  if (col_xyzs >= 0) {
    const float m = xyz_centred(x, y, z, ctr);
    (void)m;
  }
  float out[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = 4 * gq + e;
    if (c >= C) break;
    float v;
    if (col_sh >= 0 && c >= col_sh && c < col_sh + 27) {
      const int j = c - col_sh;
      float prod = (float)sh_q[i * 27 + j] * sh_scale[b * 27 + j];
      asm volatile("" : "+v"(prod));  // keep the product rounded: hipcc contracts a*b+c (and __fmul_rn is a plain multiply)
      v = prod + sh_min[b * 27 + j];
    } else if (c == col_density) {
      v = density[i];
    } else if (col_xyzs >= 0 && c >= col_xyzs && c < col_xyzs + 3) {
      v = __fdiv_rn(ctr[c - col_xyzs], scene_maxnorm[b]);
    } else {  // c == col_ones
      v = 1.f;
    }
    out[e] = v;
  }
  float *dst = feats + i * ldf + 4 * gq;
  if (vec && 4 * gq + 4 <= C) {
    *reinterpret_cast<float4 *>(dst) = make_float4(out[0], out[1], out[2], out[3]);  // one 16-byte store per thread
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * gq + e < C) dst[e] = out[e];
  }
}

extern "C" {

int mink_decode_plenoxel(const int32_t *links, const float *density, const uint8_t *sh_q, const int32_t *scene_offsets,
                         int32_t n_scenes, const float *sh_scale, const float *sh_min, int64_t n, int32_t reso_y,
                         int32_t reso_z, int32_t col_density, int32_t col_sh, int32_t col_ones, int32_t col_xyzs,
                         float *scene_scratch, int32_t C, int32_t *coords, float *feats, int32_t ldf, void *stream) {
  MINK_REQUIRE(n >= 0 && n_scenes >= 1 && reso_y >= 1 && reso_z >= 1 && C >= 1 && ldf >= C, "decode_plenoxel: bad shape");
  const int want = (col_density >= 0) + 27 * (col_sh >= 0) + (col_ones >= 0) + 3 * (col_xyzs >= 0);
  MINK_REQUIRE(want == C && col_density < C && col_ones < C && (col_sh < 0 || col_sh + 27 <= C) && (col_xyzs < 0 || col_xyzs + 3 <= C),
               "decode_plenoxel: the feature columns (density %d, sh %d, ones %d, xyzs %d) do not tile %d channels", col_density,
               col_sh, col_ones, col_xyzs, C);
  MINK_REQUIRE(col_xyzs < 0 || scene_scratch, "decode_plenoxel: the xyzs feature needs scene_scratch[n_scenes]");
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(links && scene_offsets && coords && feats && (col_density < 0 || density) &&
                   (col_sh < 0 || (sh_q && sh_scale && sh_min)),
               "decode_plenoxel: NULL pointer");
  MINK_REQUIRE(((uintptr_t)coords & 15) == 0, "decode_plenoxel: coords must be 16-byte aligned");
  const int64_t threads = n * ((C + 3) / 4);
  if (col_xyzs >= 0) {  // per-scene largest centred norm first (one extra pass over the links)
    MINK_HIP(hipMemsetAsync(scene_scratch, 0, sizeof(float) * n_scenes, (hipStream_t)stream));
    decode_xyz_maxnorm_kernel<<<dim3((unsigned)cdiv(n, kBlock)), kBlock, 0, (hipStream_t)stream>>>(
        links, scene_offsets, n_scenes, n, reso_y, reso_z, (unsigned *)scene_scratch);
    MINK_CHECK_LAUNCH();
  }
  decode_plenoxel_kernel<<<dim3((unsigned)cdiv(threads, kBlock)), kBlock, 0, (hipStream_t)stream>>>(
      links, density, sh_q, scene_offsets, n_scenes, sh_scale, sh_min, n, reso_y, reso_z, col_density, col_sh, col_ones, col_xyzs,
      scene_scratch, C, coords, feats, ldf, ((uintptr_t)feats & 15) == 0 && (ldf & 3) == 0);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
