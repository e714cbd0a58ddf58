// What the 16-byte-lane feature-matrix units share: batchnorm.hip, elementwise.hip, pool.hip (the stem's sum pool, the dense
// max pool, the global average) and field.hip (segment mean / sum).  The rule of conv_common.h: only what at least two of
// them reference lives here; a helper with one user stays with that user.
#pragma once
#include "common.h"

namespace mink {

constexpr int EB = 256;

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }

static inline unsigned ew_grid(int64_t work) {
  int64_t g = cdiv(work, EB);
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}

}  // namespace mink

#define REQ_C4(C, name) MINK_REQUIRE((C) >= 4 && ((C)&3) == 0, name ": channel count %d must be a multiple of 4", (C))
#define REQ_A16(ptr, name) MINK_REQUIRE(((uintptr_t)(ptr)&15) == 0, name ": pointer must be 16-byte aligned")
