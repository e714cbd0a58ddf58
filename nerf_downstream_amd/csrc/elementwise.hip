// Elementwise passes over a feature matrix on gfx950: the SGD step over flat buffers, ReLU / masked copy / add
// (mink_eltwise) and the pointwise activations beyond ReLU.  Bandwidth-bound: 16-byte accesses per lane where the
// layout allows.  Batch norm is in batchnorm.hip, every pool in pool.hip, the segment mean / sum in field.hip.
#include <algorithm>

#include "ew_common.h"

namespace mink {

// ------------------------------------------------------------------ SGD with momentum over flat buffers
// torch.optim.SGD's update (the reference's optimizer: co3d_3d/src/modules/optim.py:12-14, configs/co3d_cls.gin) for parameters,
// gradients and momentum buffers that each live in ONE flat fp32 buffer of the same layout (parallel.BucketedGradAllReduce):
//   g' = g + wd w;  m = mu m + g'  (a zero buffer makes the first step m = g', as torch's clone does);  w = w - lr m
// one pass instead of torch's multi-tensor chunks (ResNet34: 5 launches, 314 us for 85 MB of parameters), and the gradient
// buffer is cleared on the way out (the memset of the next step's zero_grad).
__global__ __launch_bounds__(EB) void sgd_flat_kernel(float *__restrict__ w, float *__restrict__ g, float *__restrict__ m, int64_t n4,
                                                      float lr, float mu, float wd, int zero_grad) {
#pragma clang fp contract(off)  // (the products and sums of torch's own kernel, one rounding each)
  for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n4; i += (int64_t)gridDim.x * EB) {
    float4 wv = ld4(w + 4 * i), gv = ld4(g + 4 * i), mv = ld4(m + 4 * i);
    gv.x += wd * wv.x, gv.y += wd * wv.y, gv.z += wd * wv.z, gv.w += wd * wv.w;
    mv.x = mu * mv.x + gv.x, mv.y = mu * mv.y + gv.y, mv.z = mu * mv.z + gv.z, mv.w = mu * mv.w + gv.w;
    wv.x -= lr * mv.x, wv.y -= lr * mv.y, wv.z -= lr * mv.z, wv.w -= lr * mv.w;
    st4(w + 4 * i, wv), st4(m + 4 * i, mv);
    if (zero_grad) st4(g + 4 * i, make_float4(0.f, 0.f, 0.f, 0.f));
  }
}

// mode 0: y = relu(a) (a NaN stays); mode 1: y = b>0 ? a : 0; mode 2: y = a + b
__global__ __launch_bounds__(EB) void eltwise_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                     int64_t count, int mode, float *__restrict__ y) {
  const int64_t n4 = count >> 2;
  for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n4; i += (int64_t)gridDim.x * EB) {
    const float4 va = ld4(a + 4 * i);
    float4 o;
    if (mode == 0) {
      o = relu_keep_nan(va);
    } else {
      const float4 vb = ld4(b + 4 * i);
      if (mode == 1)
        o = make_float4(vb.x > 0.f ? va.x : 0.f, vb.y > 0.f ? va.y : 0.f, vb.z > 0.f ? va.z : 0.f,
                        vb.w > 0.f ? va.w : 0.f);
      else
        o = make_float4(va.x + vb.x, va.y + vb.y, va.z + vb.z, va.w + vb.w);
    }
    st4(y + 4 * i, o);
  }
  if (blockIdx.x == 0 && threadIdx.x < (count & 3)) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    y[i] = mode == 0 ? relu_keep_nan(a[i]) : (mode == 1 ? (b[i] > 0.f ? a[i] : 0.f) : a[i] + b[i]);
  }
}

// Pointwise activations of the ME module surface beyond ReLU (reference modules/common.py:36-43 lists them at import):
// forward (gy == nullptr): out = f(x); backward: out = gy * f'(x).  `slope`: per-channel PReLU weights (C entries,
// or one shared entry when C == 1); channels are the fastest axis of the [rows, C] feature matrix.
enum { ACT_LEAKY = 1, ACT_ELU = 2, ACT_CELU = 3, ACT_SELU = 4, ACT_GELU = 5, ACT_PRELU = 6 };

template <bool BWD>
__device__ __forceinline__ float act_eval(int kind, float x, float alpha) {
  constexpr float kSeluAlpha = 1.6732632423543772f, kSeluScale = 1.0507009873554805f;
  switch (kind) {
    case ACT_LEAKY:
    case ACT_PRELU:
      return BWD ? (x > 0.f ? 1.f : alpha) : (x > 0.f ? x : alpha * x);
    case ACT_ELU:
      return BWD ? (x > 0.f ? 1.f : alpha * expf(x)) : (x > 0.f ? x : alpha * (expf(x) - 1.f));
    case ACT_CELU:
      return BWD ? (x > 0.f ? 1.f : expf(x / alpha)) : (x > 0.f ? x : alpha * (expf(x / alpha) - 1.f));
    case ACT_SELU:
      return BWD ? kSeluScale * (x > 0.f ? 1.f : kSeluAlpha * expf(x))
                 : kSeluScale * (x > 0.f ? x : kSeluAlpha * (expf(x) - 1.f));
    default: {  // ACT_GELU, exact (erf) form
      const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
      return BWD ? cdf + x * 0.3989422804014327f * expf(-0.5f * x * x) : x * cdf;
    }
  }
}

template <bool BWD>
__global__ __launch_bounds__(EB) void activation_kernel(const float *__restrict__ x, const float *__restrict__ gy,
                                                        const float *__restrict__ slope, int C, int64_t count, int kind,
                                                        float alpha, float *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < count; i += (int64_t)gridDim.x * EB) {
    const float a = slope ? slope[C > 1 ? (int)(i % C) : 0] : alpha;
    const float v = act_eval<BWD>(kind, x[i], a);
    out[i] = BWD ? gy[i] * v : v;
  }
}

}  // namespace mink

using namespace mink;

extern "C" {

int mink_sgd_step(float *w, float *g, float *m, int64_t n, float lr, float momentum, float weight_decay, int32_t zero_grad, void *stream) {
  MINK_REQUIRE(w && g && m && n >= 0 && (n & 3) == 0, "sgd_step: bad arguments (n = %lld must be a multiple of 4)", (long long)n);
  REQ_A16(w, "sgd_step");
  REQ_A16(g, "sgd_step");
  REQ_A16(m, "sgd_step");
  if (n == 0) return MINK_OK;
  const int64_t n4 = n >> 2;
  sgd_flat_kernel<<<dim3((unsigned)std::min<int64_t>(cdiv(n4, EB), 8192)), EB, 0, (hipStream_t)stream>>>(w, g, m, n4, lr, momentum, weight_decay,
                                                                                                   zero_grad);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_eltwise(const float *a, const float *b, int64_t count, int32_t mode, float *y, void *stream) {
  MINK_REQUIRE(count >= 0 && mode >= 0 && mode <= 2, "eltwise: bad arguments");
  if (count == 0) return MINK_OK;
  MINK_REQUIRE(a && y && (mode == 0 || b), "eltwise: NULL pointer");
  REQ_A16(a, "eltwise");
  REQ_A16(y, "eltwise");
  eltwise_kernel<<<dim3(ew_grid(count >> 2)), EB, 0, (hipStream_t)stream>>>(a, b, count, mode, y);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_activation(const float *x, const float *gy, const float *slope, int32_t C, int64_t count, int32_t kind, float alpha,
                    float *out, void *stream) {
  MINK_REQUIRE(count >= 0 && kind >= ACT_LEAKY && kind <= ACT_PRELU && C >= 1, "activation: bad arguments (kind %d)", kind);
  MINK_REQUIRE(kind != ACT_PRELU || slope, "activation: PReLU needs its slope vector");
  MINK_REQUIRE(kind != ACT_CELU || alpha != 0.f, "activation: CELU alpha must be non-zero");
  if (count == 0) return MINK_OK;
  MINK_REQUIRE(x && out, "activation: NULL pointer");
  const float *sl = kind == ACT_PRELU ? slope : nullptr;
  const dim3 grid(ew_grid(count));
  if (gy) activation_kernel<true><<<grid, EB, 0, (hipStream_t)stream>>>(x, gy, sl, C, count, kind, alpha, out);
  else activation_kernel<false><<<grid, EB, 0, (hipStream_t)stream>>>(x, nullptr, sl, C, count, kind, alpha, out);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
