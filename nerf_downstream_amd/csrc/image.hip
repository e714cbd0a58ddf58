// Images of the 2-D comparison (the reference's co3d_2d/src/data: loader.py:100-107, augmix.py:184-215, transforms.py): what its
// workers do to a decoded frame through Pillow and torchvision, for a whole batch (include/mink_hip.h, "images").
//
//   chain_round : round r of every AugMix chain -- (1) 256-bin histograms per (sample, chain, channel) for autocontrast / equalize,
//                 (2) the 3 x 256 tables of the four point ops, (3) one apply pass: table look-up or BILINEAR affine warp
//   finish      : per output tile and branch, crop + separable resize (horizontal pass of the needed source rows into LDS, 8 bits),
//                 vertical pass, ColorJitter steps, flip, / 255, PCA lighting, Normalize, weighted sum over the branches in registers
//
// Every 8-bit value is the integer Pillow computes; the arithmetic is restated in tests/image_restate.py.  Integer sums (histogram
// atomics, resize taps) do not depend on their order and every float is computed by one thread in a fixed order, so results are
// bitwise identical run to run.
//
// Floating-point contraction is OFF for this whole file: Pillow's C and torch's float32 kernels round every product before the
// addition that follows.  Fused, `d + f * (p - d)` (brightness / saturation), `a + (b - a) * dx` (the warp), the HSV products
// `v * (1 - s * f)`, the resize weights and `(1 - m) * p + m * mix` round once instead of twice, which moves 8-bit results that sit
// on a truncation boundary by one level and float results by an ulp.
#include "common.h"

#pragma clang fp contract(off)

namespace mink {
namespace {

constexpr int TB = 256;            // threads per workgroup
constexpr int64_t SPAN = 32768;    // bytes of the packed batch one workgroup of the chain kernels walks
constexpr int FP = 4;              // output pixels per thread of the finish kernel
constexpr int FCOLS = 256;         // widest output tile
constexpr int FROWS = 48;          // source rows per LDS pass
constexpr int PREC = 22;           // fractional bits of a resize coefficient (Pillow: 32 - 8 - 2)

struct Layout {
  int64_t hist, lut, bufA, bufB, stride, total;
};

static Layout layout_of(int64_t total_pixels, int B, int width) {
  Layout L;
  const int64_t n = (int64_t)B * width * 768;
  L.hist = 0;
  L.lut = align_up(n * 4, 256);
  L.bufA = L.lut + align_up(n, 256);
  L.stride = align_up(3 * total_pixels, 256);
  L.bufB = L.bufA + width * L.stride;
  L.total = L.bufB + width * L.stride;
  return L;
}

struct Batch {
  const uint8_t *packed;
  const int64_t *offsets;
  const int32_t *sizes;
  const double *programs;
  int64_t total;  // bytes of `packed`
  int B, width;
};

// largest b < B with offsets[b] <= pos (offsets ascending; any garbage still gives 0 <= b < B)
__device__ __forceinline__ int sample_at(const int64_t *__restrict__ offsets, int B, int64_t pos) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ bool sample_ok(const Batch &t, int b, int &w, int &h, int64_t &off) {
  w = t.sizes[2 * b], h = t.sizes[2 * b + 1];
  off = t.offsets[b];
  if (w < 1 || h < 1 || off < 0) return false;
  const int64_t bytes = 3 * (int64_t)w * h;
  return bytes <= 3 * (int64_t)0x7FFFFFFF && t.offsets[b + 1] - off == bytes && off + bytes <= t.total;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the op of chain i (1-based) of sample b in round r, or 0
__device__ __forceinline__ int chain_op(const Batch &t, int b, int i, int r, const double *&op) {
  const double *P = t.programs + (int64_t)b * MINK_IMG_PARAMS;
  const double wd = P[MINK_IMG_WIDTH];
  if (!(wd >= i && wd <= t.width)) return 0;
  const double *br = P + MINK_IMG_BRANCH + i * MINK_IMG_BRANCH_STRIDE;
  const double d = br[MINK_IMG_B_DEPTH];
  if (!(d > r && d <= MINK_IMG_MAX_DEPTH)) return 0;
  op = br + MINK_IMG_B_OPS + r * MINK_IMG_OP_STRIDE;
  const double k = op[0];
  return (k >= 1 && k <= 9) ? (int)k : 0;
}

__device__ __forceinline__ bool is_hist_op(int k) { return k == MINK_IMG_OP_AUTOCONTRAST || k == MINK_IMG_OP_EQUALIZE; }
__device__ __forceinline__ bool is_point_op(int k) { return is_hist_op(k) || k == MINK_IMG_OP_POSTERIZE || k == MINK_IMG_OP_SOLARIZE; }

// where chain i's batch lives after d ops
__device__ __forceinline__ const uint8_t *chain_image(const Batch &t, const uint8_t *ws, const Layout &L, int i, int d) {
  if (i < 1 || d < 1) return t.packed;
  return ws + ((d == 2) ? L.bufB : L.bufA) + (int64_t)(i - 1) * L.stride;
}

// h[bin] += 1 for every lane with `valid`; lanes of a wave that hold the same bin are merged into one atomic for the first three
// distinct bins met (a constant image: 16-byte chunks put the three channels on lanes l % 3, so three bins cover the wave).
// Must be called by whole waves.
__device__ __forceinline__ void hist_add(int32_t *h, bool valid, int bin) {
  const int lane = threadIdx.x & 63;
  bool rem = valid;
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const unsigned long long act = __ballot(rem);
    if (!act) return;
    const int lb = __shfl(bin, __ffsll((long long)act) - 1);
    const bool same = rem && bin == lb;
    const unsigned long long m = __ballot(same);
    if (same && __ffsll((long long)m) - 1 == lane) atomicAdd(&h[lb], (int32_t)__popcll(m));
    rem = rem && !same;
  }
  if (rem) atomicAdd(&h[bin], 1);
}

// One 16-byte chunk [lo, lo + 16) of address space clipped to [a, e): the bytes of `src` (address-aligned to the chunk grid by the
// caller or not: memcpy makes no alignment promise).  mask bit j = byte j is inside.
__device__ __forceinline__ unsigned load_chunk(const uint8_t *src, int64_t lo, int64_t a, int64_t e, uint8_t v[16]) {
  if (lo >= a && lo + 16 <= e) {
    uint4 q;
    __builtin_memcpy(&q, src + lo, 16);
    __builtin_memcpy(v, &q, 16);
    return 0xFFFFu;
  }
  unsigned mask = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int64_t p = lo + j;
    const bool in = p >= a && p < e;
    v[j] = in ? src[p] : (uint8_t)0;
    mask |= in ? (1u << j) : 0u;
  }
  return mask;
}

// the chunk grid of a destination: positions lo = g0 + 16 q with (dst + lo) 16-byte aligned, covering [a, e)
__device__ __forceinline__ int64_t chunk_origin(const uint8_t *dst, int64_t a) {
  return a - (int64_t)(((uintptr_t)dst + (uintptr_t)a) & 15);
}

__global__ __launch_bounds__(TB) void img_hist_kernel(Batch t, const uint8_t *__restrict__ ws, Layout L, int round,
                                                      int32_t *__restrict__ hist) {
  __shared__ int32_t h[768];
  const int i = blockIdx.y + 1;
  const int64_t start = (int64_t)blockIdx.x * SPAN, end = min(start + SPAN, t.total);
  const uint8_t *src = chain_image(t, ws, L, i, round);
  for (int b = sample_at(t.offsets, t.B, start); b < t.B; ++b) {
    int w, hgt;
    int64_t off;
    const bool ok = sample_ok(t, b, w, hgt, off);
    if (t.offsets[b] >= end) break;
    const double *op;
    if (!ok || !is_hist_op(chain_op(t, b, i, round, op))) continue;
    const int64_t a = max(off, start), e = min(off + 3 * (int64_t)w * hgt, end);
    if (a >= e) continue;
    for (int j = threadIdx.x; j < 768; j += TB) h[j] = 0;
    __syncthreads();
    const int64_t g0 = chunk_origin(src, a);
    const int64_t nchunks = (e - g0 + 15) >> 4;
    for (int64_t q0 = 0; q0 < nchunks; q0 += TB) {  // (whole waves stay in the loop: hist_add votes)
      const int64_t q = q0 + threadIdx.x;
      const int64_t lo = g0 + 16 * q;
      uint8_t v[16];
      const unsigned mask = q < nchunks ? load_chunk(src, lo, a, e, v) : 0u;
      int c = (int)(((lo - off) % 3 + 3) % 3);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        hist_add(h, (mask >> j) & 1u, c * 256 + v[j]);
        c = c == 2 ? 0 : c + 1;
      }
    }
    __syncthreads();
    int32_t *g = hist + ((int64_t)b * t.width + (i - 1)) * 768;
    for (int j = threadIdx.x; j < 768; j += TB)
      if (h[j]) atomicAdd(&g[j], h[j]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(TB) void img_lut_kernel(Batch t, int round, const int32_t *__restrict__ hist, uint8_t *__restrict__ luts) {
  const int b = blockIdx.x, i = blockIdx.y + 1;
  int w, hgt;
  int64_t off;
  const double *op;
  if (!sample_ok(t, b, w, hgt, off)) return;
  const int kind = chain_op(t, b, i, round, op);
  if (!is_point_op(kind)) return;
  uint8_t *lut = luts + ((int64_t)b * t.width + (i - 1)) * 768;
  if (kind == MINK_IMG_OP_POSTERIZE || kind == MINK_IMG_OP_SOLARIZE) {
    const int p = clampi((int)fmin(fmax(op[1], -1.0), 1024.0), 0, 256);
    const int keep = 0xFF & ~((1 << (8 - min(p, 8))) - 1);
    for (int j = threadIdx.x; j < 768; j += TB) {
      const int v = j & 255;
      lut[j] = (uint8_t)(kind == MINK_IMG_OP_POSTERIZE ? (v & keep) : (v < p ? v : 255 - v));
    }
    return;
  }
  if (threadIdx.x >= 3) return;
  const int32_t *h = hist + ((int64_t)b * t.width + (i - 1)) * 768 + threadIdx.x * 256;
  lut += threadIdx.x * 256;
  int lo = 256, hi = -1, bins = 0;
  int64_t sum = 0;
  for (int j = 0; j < 256; ++j)
    if (h[j]) {
      if (lo == 256) lo = j;
      hi = j, ++bins, sum += h[j];
    }
  if (kind == MINK_IMG_OP_AUTOCONTRAST) {
    if (hi <= lo) {
      for (int j = 0; j < 256; ++j) lut[j] = (uint8_t)j;
    } else {
      const double scale = 255.0 / (double)(hi - lo), offs = (double)(-lo) * scale;
      for (int j = 0; j < 256; ++j) lut[j] = (uint8_t)clampi((int)((double)j * scale + offs), 0, 255);
    }
  } else {
    const int64_t step = bins > 1 ? (sum - h[hi]) / 255 : 0;
    if (step == 0) {
      for (int j = 0; j < 256; ++j) lut[j] = (uint8_t)j;
    } else {
      int64_t n = step / 2;
      for (int j = 0; j < 256; ++j) {
        const int64_t v = n / step;
        lut[j] = (uint8_t)(v > 255 ? 255 : v);
        n += h[j];
      }
    }
  }
}

// Image.transform(AFFINE, BILINEAR) of one pixel, all three channels: double arithmetic, unfused, truncated.
__device__ __forceinline__ void warp_pixel(const uint8_t *__restrict__ img, int w, int h, const double m[6], int x, int y, uint8_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  const double xs = (double)x + 0.5, ys = (double)y + 0.5;
  double xin = m[0] * xs + m[1] * ys + m[2];
  double yin = m[3] * xs + m[4] * ys + m[5];
  if (!(xin >= 0.0 && xin < (double)w && yin >= 0.0 && yin < (double)h)) return;
  xin -= 0.5, yin -= 0.5;
  const int x0 = xin < 0.0 ? (int)floor(xin) : (int)xin, y0 = yin < 0.0 ? (int)floor(yin) : (int)yin;
  const double dx = xin - (double)x0, dy = yin - (double)y0;
  const int xa = clampi(x0, 0, w - 1), xb = clampi(x0 + 1, 0, w - 1);
  const uint8_t *r0 = img + (int64_t)clampi(y0, 0, h - 1) * w * 3;
  const bool below = y0 + 1 >= 0 && y0 + 1 < h;
  const uint8_t *r1 = img + (int64_t)clampi(y0 + 1, 0, h - 1) * w * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double a = (double)r0[3 * xa + c], b = (double)r0[3 * xb + c];
    const double v1 = a + (b - a) * dx;
    double v2 = v1;
    if (below) {
      const double a2 = (double)r1[3 * xa + c], b2 = (double)r1[3 * xb + c];
      v2 = a2 + (b2 - a2) * dx;
    }
    out[c] = (uint8_t)(int)(v1 + (v2 - v1) * dy);
  }
}

__global__ __launch_bounds__(TB) void img_apply_kernel(Batch t, uint8_t *__restrict__ ws, Layout L, int round,
                                                       const uint8_t *__restrict__ luts) {
  __shared__ uint8_t lut[768];
  const int i = blockIdx.y + 1;
  const int64_t start = (int64_t)blockIdx.x * SPAN, end = min(start + SPAN, t.total);
  const uint8_t *src = chain_image(t, ws, L, i, round);
  uint8_t *dst = ws + ((round == 1) ? L.bufB : L.bufA) + (int64_t)(i - 1) * L.stride;
  for (int b = sample_at(t.offsets, t.B, start); b < t.B; ++b) {
    int w, hgt;
    int64_t off;
    const bool ok = sample_ok(t, b, w, hgt, off);
    if (t.offsets[b] >= end) break;
    const double *op;
    const int kind = ok ? chain_op(t, b, i, round, op) : 0;
    if (!kind) continue;
    const int64_t a = max(off, start), e = min(off + 3 * (int64_t)w * hgt, end);
    if (a >= e) continue;
    const bool point = is_point_op(kind);
    if (point) {
      __syncthreads();  // (the previous segment's look-ups are done)
      for (int j = threadIdx.x; j < 768; j += TB) lut[j] = luts[((int64_t)b * t.width + (i - 1)) * 768 + j];
      __syncthreads();
    }
    double m[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) m[j] = op[1 + j];
    const int64_t g0 = chunk_origin(dst, a);
    const int64_t nchunks = (e - g0 + 15) >> 4;
    for (int64_t q = threadIdx.x; q < nchunks; q += TB) {
      const int64_t lo = g0 + 16 * q;
      uint8_t v[16];
      unsigned mask;
      const int64_t rel = lo - off;  // (>= -15)
      int64_t pix = (rel + 18) / 3 - 6;
      int c = (int)(rel - 3 * pix);
      if (point) {
        mask = load_chunk(src, lo, a, e, v);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          v[j] = lut[c * 256 + v[j]];
          c = c == 2 ? 0 : c + 1;
        }
      } else {
        mask = 0;
        uint8_t px[3] = {0, 0, 0};
        int x = 0, y = 0;  // the pixel of the byte at hand: one division per chunk, then counted on
        bool located = false, fresh = false;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int64_t p = lo + j;
          const bool in = p >= a && p < e;
          if (in && !located) {
            y = (int)((uint32_t)pix / (uint32_t)w), x = (int)pix - y * w;  // (a sample has fewer than 2^31 pixels: sample_ok)
            located = fresh = true;
          }
          if (in && fresh) {
            warp_pixel(src + off, w, hgt, m, x, y, px);
            fresh = false;
          }
          v[j] = in ? (c == 0 ? px[0] : (c == 1 ? px[1] : px[2])) : (uint8_t)0;
          mask |= in ? (1u << j) : 0u;
          if (c == 2) {
            c = 0, ++pix;
            if (located) {
              fresh = true;
              if (++x == w) x = 0, ++y;
            }
          } else {
            ++c;
          }
        }
      }
      if (mask == 0xFFFFu) {
        uint4 o;
        __builtin_memcpy(&o, v, 16);
        *reinterpret_cast<uint4 *>(dst + lo) = o;  // (dst + lo is 16-byte aligned: chunk_origin)
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if ((mask >> j) & 1u) dst[lo + j] = v[j];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the fused tail
// BILINEAR resize of `len` samples to `out`: taps [xmin, xmax) and the normalising sum of output index i (Pillow's precompute_coeffs)
struct Taps {
  double center, ss, ww;
  int xmin, xmax;
};

__device__ __forceinline__ double tap_weight(const Taps &k, int x) {  // x absolute, xmin <= x < xmax
  double a = ((double)x - k.center + 0.5) * k.ss;
  if (a < 0.0) a = -a;
  return a < 1.0 ? 1.0 - a : 0.0;
}

__device__ __forceinline__ Taps taps_of(int len, int out, int i) {
  Taps k;
  const double scale = (double)len / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  k.ss = 1.0 / fs;
  k.center = ((double)i + 0.5) * scale;
  k.xmin = (int)(k.center - fs + 0.5);
  if (k.xmin < 0) k.xmin = 0;
  k.xmax = (int)(k.center + fs + 0.5);
  if (k.xmax > len) k.xmax = len;
  k.ww = 0.0;
  for (int x = k.xmin; x < k.xmax; ++x) k.ww += tap_weight(k, x);
  return k;
}

__device__ __forceinline__ int tap_coeff(const Taps &k, int x) {
  double v = tap_weight(k, x);
  if (k.ww != 0.0) v = v / k.ww;
  return (int)(0.5 + v * (double)(1 << PREC));
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow's Image.blend(degenerate d, image p, f) of one channel: float32, truncated; clipped when f is outside [0, 1]
__device__ __forceinline__ int blend8(int p, int d, float f) {
  const float t = (float)d + f * (float)(p - d);
  if (f >= 0.f && f <= 1.0f) return (int)(uint8_t)(int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ void rgb_to_hsv(const int p[3], int hsv[3]) {
  const int r = p[0], g = p[1], b = p[2];
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  hsv[2] = mx;
  if (mx == mn) {
    hsv[0] = hsv[1] = 0;
    return;
  }
  const float cr = (float)(mx - mn);
  const float s = cr / (float)mx;
  const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
  float h;
  if (r == mx) h = bc - gc;                                        // a float expression in Pillow's C
  else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);    // double ones: the literal is a double
  else h = (float)(4.0 + (double)gc - (double)rc);
  h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
  hsv[0] = clip8((int)((double)h * 255.0));
  hsv[1] = clip8((int)((double)s * 255.0));
}

__device__ __forceinline__ void hsv_to_rgb(const int hsv[3], int p[3]) {
  const int v = hsv[2];
  if (hsv[1] == 0) {
    p[0] = p[1] = p[2] = v;
    return;
  }
  const float h6 = (float)hsv[0] * 6.0f / 255.0f;
  const float fi = floorf(h6);
  const float f = h6 - fi;
  const float fs = (float)hsv[1] / 255.0f;
  const float fv = (float)v;
  const int pp = clip8((int)floorf(fv * (1.0f - fs) + 0.5f));
  const int q = clip8((int)floorf(fv * (1.0f - fs * f) + 0.5f));
  const int tt = clip8((int)floorf(fv * (1.0f - fs * (1.0f - f)) + 0.5f));
  switch ((int)fi % 6) {
    case 0: p[0] = v, p[1] = tt, p[2] = pp; break;
    case 1: p[0] = q, p[1] = v, p[2] = pp; break;
    case 2: p[0] = pp, p[1] = v, p[2] = tt; break;
    case 3: p[0] = pp, p[1] = q, p[2] = v; break;
    case 4: p[0] = tt, p[1] = pp, p[2] = v; break;
    default: p[0] = v, p[1] = pp, p[2] = q; break;
  }
}

__device__ __forceinline__ void jitter_step(int kind, const double *factors, int p[3]) {
  if (kind == MINK_IMG_JIT_BRIGHTNESS) {
    const float f = (float)factors[0];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = blend8(p[c], 0, f);
  } else if (kind == MINK_IMG_JIT_SATURATION) {
    const float f = (float)factors[1];
    const int l = (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 0x8000) >> 16;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = blend8(p[c], l, f);
  } else if (kind == MINK_IMG_JIT_HUE) {
    const double sh = fmin(fmax(factors[2], -1.0e6), 1.0e6) * 255.0;
    int hsv[3];
    rgb_to_hsv(p, hsv);
    hsv[0] = (hsv[0] + (int)sh) & 255;
    hsv_to_rgb(hsv, p);
  }
}

struct Geometry {
  int bx, by, bw, bh, ow, oh, wx, wy;
};

__device__ __forceinline__ bool read_int(double v, int lo, int hi, int &out) {
  if (!(v >= (double)lo && v <= (double)hi)) return false;
  out = (int)v;
  return true;
}

__device__ __forceinline__ bool geometry_of(const double *br, int w, int h, int S, Geometry &g) {
  const int big = 1 << 30;
  const double *bx = br + MINK_IMG_B_BOX, *tg = br + MINK_IMG_B_TARGET, *wn = br + MINK_IMG_B_WINDOW;
  const int ok = (int)read_int(bx[0], 0, w - 1, g.bx) & (int)read_int(bx[1], 0, h - 1, g.by) & (int)read_int(bx[2], 1, w, g.bw) &
                 (int)read_int(bx[3], 1, h, g.bh) & (int)read_int(tg[0], S, big, g.ow) & (int)read_int(tg[1], S, big, g.oh) &
                 (int)read_int(wn[0], 0, big, g.wx) & (int)read_int(wn[1], 0, big, g.wy);
  if (!ok) return false;
  return g.bx + g.bw <= w && g.by + g.bh <= h && (int64_t)g.wx + S <= g.ow && (int64_t)g.wy + S <= g.oh;
}

__global__ __launch_bounds__(TB) void img_finish_kernel(Batch t, const uint8_t *__restrict__ ws, Layout L, int S, int TC, int TR,
                                                        int ntx, float *__restrict__ out, uint8_t *__restrict__ stages) {
  __shared__ uint8_t rows[FROWS * FCOLS * 3];
  const int b = blockIdx.y;
  const int cx0 = (blockIdx.x % ntx) * TC, oy0 = (blockIdx.x / ntx) * TR;
  const int ncols = min(TC, S - cx0), nrows = min(TR, S - oy0);
  const double *P = t.programs + (int64_t)b * MINK_IMG_PARAMS;
  int w, h, width = 0;
  int64_t off;
  bool good = sample_ok(t, b, w, h, off) && read_int(P[MINK_IMG_WIDTH], 0, min(t.width, (int)MINK_IMG_MAX_WIDTH), width);
  for (int k = 0; good && k <= width; ++k) {
    Geometry g;
    good = geometry_of(P + MINK_IMG_BRANCH + k * MINK_IMG_BRANCH_STRIDE, w, h, S, g);
  }
  const float nanv = __int_as_float(0x7FC00000);
  const float mean[3] = {(float)(123.68 / 255), (float)(116.779 / 255), (float)(103.939 / 255)};
  const float stdv[3] = {(float)(58.393 / 255), (float)(57.12 / 255), (float)(57.375 / 255)};
  const float m = (float)P[MINK_IMG_M];

  int ox[FP], oy[FP];
  bool mine[FP];
  float pre0[FP][3], mix[FP][3];
#pragma unroll
  for (int j = 0; j < FP; ++j) {
    const int p = j * TB + threadIdx.x;
    const int ly = p / ncols;
    mine[j] = ly < nrows;
    oy[j] = oy0 + ly, ox[j] = cx0 + (p - ly * ncols);
#pragma unroll
    for (int c = 0; c < 3; ++c) pre0[j][c] = 0.f, mix[j][c] = 0.f;
  }

  for (int k = 0; good && k <= width; ++k) {
    const double *br = P + MINK_IMG_BRANCH + k * MINK_IMG_BRANCH_STRIDE;
    Geometry g;
    geometry_of(br, w, h, S, g);
    int depth = 0;
    if (k > 0) read_int(br[MINK_IMG_B_DEPTH], 0, MINK_IMG_MAX_DEPTH, depth);
    const uint8_t *img = chain_image(t, ws, L, k, depth) + off;
    const bool flip = br[MINK_IMG_B_FLIP] != 0.0;
    const int rc0 = flip ? S - (cx0 + ncols) : cx0;  // first resized column of the window this tile reads
    // source rows of the crop the tile's vertical taps read
    const Taps first = taps_of(g.bh, g.oh, g.wy + oy0), last = taps_of(g.bh, g.oh, g.wy + oy0 + nrows - 1);
    const int R0 = first.xmin, R1 = last.xmax;
    int acc[FP][3];
    Taps kv[FP];
#pragma unroll
    for (int j = 0; j < FP; ++j) {
      acc[j][0] = acc[j][1] = acc[j][2] = 0;
      if (mine[j]) kv[j] = taps_of(g.bh, g.oh, g.wy + oy[j]);
    }
    for (int r0 = R0; r0 < R1; r0 += FROWS) {
      const int nr = min(FROWS, R1 - r0);
      __syncthreads();  // (the previous pass's rows have been read)
      // horizontal pass: a thread owns one resized column of the tile and every ngrp-th source row of the pass
      const int grp = threadIdx.x / ncols, ngrp = TB / ncols, cc = threadIdx.x - grp * ncols;
      if (grp < ngrp) {
        const Taps kh = taps_of(g.bw, g.ow, g.wx + rc0 + cc);
        for (int rr = grp; rr < nr; rr += ngrp) {
          const uint8_t *srow = img + ((int64_t)(g.by + r0 + rr) * w + g.bx) * 3;
          int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
          for (int x = kh.xmin; x < kh.xmax; ++x) {
            const int kc = tap_coeff(kh, x);
            s0 += kc * srow[3 * x], s1 += kc * srow[3 * x + 1], s2 += kc * srow[3 * x + 2];
          }
          uint8_t *d = rows + (rr * FCOLS + cc) * 3;
          d[0] = (uint8_t)clip8(s0 >> PREC), d[1] = (uint8_t)clip8(s1 >> PREC), d[2] = (uint8_t)clip8(s2 >> PREC);
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < FP; ++j) {
        if (!mine[j]) continue;
        const int rx = (flip ? S - 1 - ox[j] : ox[j]) - rc0;
        const int ya = max(kv[j].xmin, r0), yb = min(kv[j].xmax, r0 + nr);
        for (int y = ya; y < yb; ++y) {
          const int kc = tap_coeff(kv[j], y);
          const uint8_t *s = rows + ((y - r0) * FCOLS + rx) * 3;
          acc[j][0] += kc * s[0], acc[j][1] += kc * s[1], acc[j][2] += kc * s[2];
        }
      }
    }
    int order[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) order[s] = (int)fmin(fmax(br[MINK_IMG_B_ORDER + s], 0.0), 4.0);
    const float wk = k > 0 ? (float)P[MINK_IMG_WS + k - 1] : 0.f;
#pragma unroll
    for (int j = 0; j < FP; ++j) {
      if (!mine[j]) continue;
      int p[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) p[c] = clip8(((1 << (PREC - 1)) + acc[j][c]) >> PREC);
#pragma unroll
      for (int s = 0; s < 3; ++s) jitter_step(order[s], br + MINK_IMG_B_FACTORS, p);
      if (stages) {
        uint8_t *d = stages + ((((int64_t)b * (t.width + 1) + k) * S + oy[j]) * S + ox[j]) * 3;
        d[0] = (uint8_t)p[0], d[1] = (uint8_t)p[1], d[2] = (uint8_t)p[2];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float x = (float)p[c] / 255.0f;
        x = x + (float)br[MINK_IMG_B_RGB + c];
        x = (x - mean[c]) / stdv[c];
        if (k == 0) pre0[j][c] = x;
        else mix[j][c] = mix[j][c] + wk * x;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < FP; ++j) {
    if (!mine[j]) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      out[(((int64_t)b * 3 + c) * S + oy[j]) * S + ox[j]] = good ? (1.0f - m) * pre0[j][c] + m * mix[j][c] : nanv;
  }
}

static int check_batch(const char *who, const void *packed, const void *offsets, const void *sizes, const void *programs,
                       int64_t total_pixels, int B, int width) {
  MINK_REQUIRE(B >= 0 && B <= 65535 && width >= 0 && width <= MINK_IMG_MAX_WIDTH && total_pixels >= 0 &&
                   total_pixels < ((int64_t)1 << 40),
               "%s: bad shape (B %d, width %d of at most %d, %lld pixels)", who, B, width, (int)MINK_IMG_MAX_WIDTH,
               (long long)total_pixels);
  if (B == 0) return MINK_OK;
  MINK_REQUIRE(packed && offsets && sizes && programs, "%s: NULL pointer (packed, offsets, sizes or programs)", who);
  MINK_REQUIRE(total_pixels >= B, "%s: %lld pixels for %d images", who, (long long)total_pixels, B);
  return MINK_OK;
}

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int64_t mink_img_workspace_bytes(int64_t total_pixels, int32_t B, int32_t width, int32_t S) {
  (void)S;
  if (total_pixels < 0 || B < 0 || width < 0 || width > MINK_IMG_MAX_WIDTH) return -1;
  return layout_of(total_pixels, B, width).total;
}

int64_t mink_img_chain_buffer_offset(int64_t total_pixels, int32_t B, int32_t width, int32_t chain, int32_t depth) {
  if (total_pixels < 0 || B < 0 || width < 1 || width > MINK_IMG_MAX_WIDTH || chain < 1 || chain > width || depth < 1 ||
      depth > MINK_IMG_MAX_DEPTH)
    return -1;
  const Layout L = layout_of(total_pixels, B, width);
  return (depth == 2 ? L.bufB : L.bufA) + (int64_t)(chain - 1) * L.stride;
}

int mink_img_chain_round(const uint8_t *packed, const int64_t *offsets, const int32_t *sizes, const double *programs,
                         int64_t total_pixels, int32_t B, int32_t width, int32_t round, void *workspace, int64_t workspace_bytes,
                         void *stream) {
  if (int rc = check_batch("img_chain_round", packed, offsets, sizes, programs, total_pixels, B, width)) return rc;
  MINK_REQUIRE(round >= 0 && round < MINK_IMG_MAX_DEPTH, "img_chain_round: round %d (0 .. %d)", round, MINK_IMG_MAX_DEPTH - 1);
  if (B == 0 || width == 0) return MINK_OK;
  const Layout L = layout_of(total_pixels, B, width);
  MINK_REQUIRE(workspace, "img_chain_round: NULL workspace");
  MINK_REQUIRE(workspace_bytes >= L.total, "img_chain_round: workspace of %lld bytes, %lld needed (mink_img_workspace_bytes)",
               (long long)workspace_bytes, (long long)L.total);
  hipStream_t s = (hipStream_t)stream;
  uint8_t *ws = (uint8_t *)workspace;
  const Batch t = {packed, offsets, sizes, programs, 3 * total_pixels, B, width};
  int32_t *hist = (int32_t *)(ws + L.hist);
  MINK_HIP(hipMemsetAsync(hist, 0, (size_t)B * width * 768 * 4, s));
  const dim3 spans((unsigned)cdiv(t.total, SPAN), (unsigned)width);
  img_hist_kernel<<<spans, TB, 0, s>>>(t, ws, L, round, hist);
  MINK_CHECK_LAUNCH();
  img_lut_kernel<<<dim3((unsigned)B, (unsigned)width), TB, 0, s>>>(t, round, hist, ws + L.lut);
  MINK_CHECK_LAUNCH();
  img_apply_kernel<<<spans, TB, 0, s>>>(t, ws, L, round, ws + L.lut);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_img_finish(const uint8_t *packed, const int64_t *offsets, const int32_t *sizes, const double *programs,
                    int64_t total_pixels, int32_t B, int32_t width, int32_t S, const void *workspace, int64_t workspace_bytes,
                    float *out, uint8_t *stages, void *stream) {
  if (int rc = check_batch("img_finish", packed, offsets, sizes, programs, total_pixels, B, width)) return rc;
  MINK_REQUIRE(S >= 1 && S <= 16384, "img_finish: output size %d (1 .. 16384)", S);
  if (B == 0) return MINK_OK;
  MINK_REQUIRE(out, "img_finish: NULL output");
  const Layout L = layout_of(total_pixels, B, width);
  MINK_REQUIRE(width == 0 || workspace, "img_finish: NULL workspace");
  MINK_REQUIRE(width == 0 || workspace_bytes >= L.total, "img_finish: workspace of %lld bytes, %lld needed (mink_img_workspace_bytes)",
               (long long)workspace_bytes, (long long)L.total);
  const Batch t = {packed, offsets, sizes, programs, 3 * total_pixels, B, width};
  const int TC = S < FCOLS ? S : FCOLS;
  int TR = (TB * FP) / TC;
  if (TR > S) TR = S;
  const int ntx = (int)cdiv(S, TC), nty = (int)cdiv(S, TR);
  img_finish_kernel<<<dim3((unsigned)(ntx * nty), (unsigned)B), TB, 0, (hipStream_t)stream>>>(t, (const uint8_t *)workspace, L, S, TC, TR,
                                                                                             ntx, out, stages);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
