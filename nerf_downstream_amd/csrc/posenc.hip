// MinkowskiPositionalEncoding on gfx950 (reference co3d_3d/src/models/mink/modules/encoding.py:74-209): every input channel
// of x[n][C] becomes 2L sinusoids, y[i][q] = sin(freq[q] * x[i][q / (2L)] + phase[q]) for q < Q = 2LC, and the columns
// [lo, hi) of x follow them unchanged.  Conventions of rowpass.h: fp32, row pitch arguments, VEC = 4 (16-byte) lanes where the
// width 2L, the pitch and the pointers allow and dword lanes otherwise, no atomics, a fixed summation order.
//
//   posenc_fwd : one lane per column group of the Q encoded columns (VEC | 2L, so a group lies inside one channel and reads one
//                x), then one dword lane per pass-through column; every output element is written exactly once and
//                consecutive lanes write consecutive addresses.
//   posenc_bwd : one lane per (row, channel): it walks the channel's 2L contiguous columns of dy in ascending order, adds the
//                pass-through column last and writes dx[i][c] once.
//
// The argument is one fmaf (a single rounding of freq * x + phase), the sine is the library's sinf / cosf: its error is a few
// ulps of a result of at most 1 for every finite argument, which the bound |y - sin(a)| <= (|a| + 4) 2^-23 needs; deriving the
// upper octaves by angle doubling would double the error per octave and was not taken.
#include "rowpass.h"

namespace mink {
namespace {

constexpr int PB = 256;  // threads per workgroup

template <int VEC>
__global__ __launch_bounds__(PB) void posenc_fwd_kernel(const float *__restrict__ x, int64_t n, int C, int ldx,
                                                        const float *__restrict__ freq, const float *__restrict__ phase, int L2,
                                                        int lo, int hi, float *__restrict__ y, int ldy) {
  const int Q = L2 * C, ncg = Q / VEC, W = ncg + (hi - lo);  // lanes of one row: the column groups, then the pass-through columns
  const int64_t total = n * W;
  for (int64_t t = (int64_t)blockIdx.x * PB + threadIdx.x; t < total; t += (int64_t)gridDim.x * PB) {
    const int64_t i = t / W;
    const int g = (int)(t - i * W);
    if (g < ncg) {
      const int q = g * VEC;
      const float xv = x[i * ldx + q / L2];
      float f[VEC], p[VEC], v[VEC];
      ldv<VEC>(freq + q, f);
      ldv<VEC>(phase + q, p);
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = sinf(fmaf(f[k], xv, p[k]));
      stv<VEC>(y + i * ldy + q, v);
    } else {
      const int c = lo + (g - ncg);
      y[i * ldy + Q + (g - ncg)] = x[i * ldx + c];
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(PB) void posenc_bwd_kernel(const float *__restrict__ dy, int ldy, const float *__restrict__ x,
                                                        int64_t n, int C, int ldx, const float *__restrict__ freq,
                                                        const float *__restrict__ phase, int L2, int lo, int hi,
                                                        float *__restrict__ dx, int lddx) {
  const int Q = L2 * C;
  const int64_t total = n * C;
  for (int64_t t = (int64_t)blockIdx.x * PB + threadIdx.x; t < total; t += (int64_t)gridDim.x * PB) {
    const int64_t i = t / C;
    const int c = (int)(t - i * C);
    const float xv = x[i * ldx + c];
    const float *g = dy + i * ldy;
    float acc = 0.f;
    for (int q = c * L2; q < (c + 1) * L2; q += VEC) {
      float f[VEC], p[VEC], d[VEC];
      ldv<VEC>(freq + q, f);
      ldv<VEC>(phase + q, p);
      ldv<VEC>(g + q, d);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc = fmaf(f[k] * cosf(fmaf(f[k], xv, p[k])), d[k], acc);
    }
    if (c >= lo && c < hi) acc += g[Q + (c - lo)];
    dx[i * lddx + c] = acc;
  }
}

// the checks both entry points share; Q + hi - lo <= 2 * 32 * 4096 + 4096 fits an int
#define MINK_POSENC_REQUIRE(name, n, C, ldx, L, lo, hi, ldy)                                                                      \
  do {                                                                                                                            \
    MINK_REQUIRE_ROWS_C(name, n, 0x0fffffffLL, C);                                                                                \
    MINK_REQUIRE((L) >= 1 && (L) <= 32, name ": %d encoding functions (1 <= L <= 32)", (int)(L));                                 \
    MINK_REQUIRE((lo) >= 0 && (lo) <= (hi) && (hi) <= (C), name ": pass-through range [%d, %d) of %d channels (0 <= lo <= hi <= C)", \
                 (int)(lo), (int)(hi), (int)(C));                                                                                  \
    MINK_REQUIRE((ldx) >= (C), name ": ldx=%d below C=%d", (int)(ldx), (int)(C));                                                 \
    MINK_REQUIRE((ldy) >= 2 * (L) * (C) + (hi) - (lo), name ": ldy=%d below the %d columns of a row", (int)(ldy),                 \
                 (int)(2 * (L) * (C) + (hi) - (lo)));                                                                              \
  } while (0)

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int mink_posenc_fwd(const float *x, int64_t n, int32_t C, int32_t ldx, const float *freq, const float *phase, int32_t L, int32_t lo,
                    int32_t hi, float *y, int32_t ldy, void *stream) {
  MINK_POSENC_REQUIRE("posenc_fwd", n, C, ldx, L, lo, hi, ldy);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(x && freq && phase && y, "posenc_fwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const int L2 = 2 * L, Q = L2 * C;
  const bool vec = (L2 & 3) == 0 && (ldy & 3) == 0 && aligned16(y) && aligned16(freq) && aligned16(phase);
  const dim3 grid(flat_grid(n * ((vec ? Q / 4 : Q) + (hi - lo)), PB, 1 << 16));
  if (vec) posenc_fwd_kernel<4><<<grid, PB, 0, st>>>(x, n, C, ldx, freq, phase, L2, lo, hi, y, ldy);
  else posenc_fwd_kernel<1><<<grid, PB, 0, st>>>(x, n, C, ldx, freq, phase, L2, lo, hi, y, ldy);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_posenc_bwd(const float *dy, int32_t ldy, const float *x, int64_t n, int32_t C, int32_t ldx, const float *freq,
                    const float *phase, int32_t L, int32_t lo, int32_t hi, float *dx, int32_t lddx, void *stream) {
  MINK_POSENC_REQUIRE("posenc_bwd", n, C, ldx, L, lo, hi, ldy);
  MINK_REQUIRE(lddx >= C, "posenc_bwd: lddx=%d below C=%d", lddx, C);
  if (n == 0) return MINK_OK;
  MINK_REQUIRE(dy && x && freq && phase && dx, "posenc_bwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const int L2 = 2 * L;
  const bool vec = (L2 & 3) == 0 && (ldy & 3) == 0 && aligned16(dy) && aligned16(freq) && aligned16(phase);
  const dim3 grid(flat_grid(n * C, PB, 1 << 16));
  if (vec) posenc_bwd_kernel<4><<<grid, PB, 0, st>>>(dy, ldy, x, n, C, ldx, freq, phase, L2, lo, hi, dx, lddx);
  else posenc_bwd_kernel<1><<<grid, PB, 0, st>>>(dy, ldy, x, n, C, ldx, freq, phase, L2, lo, hi, dx, lddx);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
