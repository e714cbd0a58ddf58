// What the two halves of the sparse convolution share: conv.hip (forward / data gradient, the switch setters, the
// timing registry) and conv_wgrad.hip (weight gradient).  Only what BOTH reference lives here; a helper that one
// half uses stays in that half.
#pragma once
#include "common.h"

namespace mink {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int BM = 128;    // output rows per workgroup (4 waves x 32 rows)
constexpr int BN = 64;     // output columns per workgroup (2 MFMA tiles per wave)
constexpr int BK = 32;     // reduction chunk (input channels) per stage
constexpr int KMAX = 27;

__device__ __forceinline__ float4 ld4_guard(const float *p, int valid, bool vec) {
  // valid = number of in-bounds floats at p (may be <= 0 or >= 4)
  if (valid >= 4 && vec) return *reinterpret_cast<const float4 *>(p);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid > 0) v.x = p[0];
  if (valid > 1) v.y = p[1];
  if (valid > 2) v.z = p[2];
  if (valid > 3) v.w = p[3];
  return v;
}

// Branch-free 16-byte load: `ok == false` reads element 0 of `base` (always mapped) and returns
// zeros.  Keeps every load of a staging pass independent so they are all in flight together
// (the guarded form above compiles to serialized load/wait branches).
__device__ __forceinline__ float4 ld4_sel(const float *base, int64_t off, bool ok) {
  const float4 v = *reinterpret_cast<const float4 *>(base + (ok ? off : 0));
  return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

using f32x4 = __attribute__((ext_vector_type(4))) float;
using i32x4 = __attribute__((ext_vector_type(4))) int;
// raw buffer loads with a per-lane byte offset (VGPR) and a per-item byte offset (SGPR): no address arithmetic per load
__device__ f32x4 raw_load_v4(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
__device__ int raw_load_i32(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.i32");
// descriptor of a raw buffer of `bytes` bytes: a load at byte offset >= bytes touches no memory and returns 0
__device__ __forceinline__ i32x4 raw_rsrc(const void *ptr, unsigned bytes) {
  const unsigned long long a = (unsigned long long)ptr;
  i32x4 r;
  r.x = (int)(unsigned)a, r.y = (int)((a >> 32) & 0xFFFFu), r.z = (int)bytes, r.w = 0x00020000;
  return r;
}

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
  return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)a) |
         ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)b) << 16);
}

__device__ __forceinline__ bf16x8 pack_bf16x8(const float (&v)[8]) {
  const uint4 u = make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7]));
  return __builtin_bit_cast(bf16x8, u);
}

// ---- the switches of both dispatchers and planners: one object per library, defined in conv.hip.  mink_conv_set_stagger
// is the only decoder of its bit mask; mink_conv_set_math, mink_conv_set_pipeline and mink_conv_trace write the rest.
struct ConvKnobs {
  int stagger = 0;         // set_stagger bits 0-7: handed to the kernels as GemmParams::stagger / WgradParams::ablate
  int flat = 1;            // set_stagger bit 9 = off: no flattened-K stem path
  int math = 0;  // 0 fp32, 1 bf16 MFMA, 3 split-bf16
  int wgrad_stream = 1;    // set_stagger bit 10 = off: tiled (LDS) wgrad kernel for the stem
  int wgrad_force = 0;  // bits 0-3: G code, bits 4..: row splits (scripts/kbench.py wsweep)
  int wgrad_bf16_off = 0;  // bf16 math: stem weight gradient on the bf16 MFMA too (set_stagger bit 28 switches it off: A/B tests)
  int b16t_off = 0;      // set_stagger bit 11: the bf16-storage stem weight gradient without the LDS transposition (A/B tests)
  int compact = 1;  // fp32 mid layers on compact_gemm_kernel (set_stagger bit 30: the dense kernel, for the tests that compare the two)
  int compact_perm16 = 1;  // --math bf16: the class-permuted data gradients on compact_gemm_kernel<.., MATH = 1> (set_stagger bit 27 = off: the dense bf16 kernel, A/B)
  int compact_cin32 = 0;  // set_stagger bit 8 (measurement only, scripts/kbench.py stemc): the class-permuted form also takes cin = 32
  int compact_perm = 1;  // ... and the class-permuted strided data gradients (bit 31)
  unsigned long long *trace_buf = nullptr;  // mink_conv_trace
  int64_t trace_cap = 0;
  int compact_p3 = 0;    // mink_conv_set_pipeline: the three-stage form of compact_gemm_kernel (1: stride-1 layers, 2: class-permuted too, 3: both)
  int wgrad_xcd = 1;  // streaming wgrad: groups of a row split share an XCD (stream_slot; bit 29: plain order)
};
extern ConvKnobs g_conv;

// a planner's answer in the words of mink_conv_*_launch_info (workgroups are 256 threads in both halves)
inline MinkConvLaunchInfo launch_info(int kernel, const int *targ, int ntarg, dim3 grid, int lds, int slabs, int epilogue) {
  MinkConvLaunchInfo info = {};
  info.kernel = kernel;
  for (int i = 0; i < ntarg; ++i) info.targ[i] = targ[i];
  info.grid[0] = (int32_t)grid.x, info.grid[1] = (int32_t)grid.y, info.grid[2] = (int32_t)grid.z;
  info.block = 256, info.lds_bytes = lds, info.slabs = slabs, info.epilogue = epilogue;
  return info;
}

// ---- kernel timing registry (measurement only; see mink_conv_timing in the header): state and bodies in conv.hip
struct TimedLaunch {
  MinkTimingEntry e;
  hipEvent_t a, b;
};

struct ScopedTimer {  // records an event pair around the launches of one convolution call, on the launch stream
  bool on = false;
  TimedLaunch t;
  hipStream_t st;
  ScopedTimer(int kind, int64_t n_in, int64_t n_out, int K, int cin, int cout, const int32_t *nbr, hipStream_t stream);
  ~ScopedTimer();
};

}  // namespace mink
