// Background augmentation of the PeRFception renders (the reference's co3d_2d/src/data/transforms.py:113-159): a rendered frame and
// its mask are resized by Pillow's default filter and pasted, through the mask, over the centre of another scene's background --
// for a whole batch, in place in the packed frames (include/mink_hip.h, "images: background paste").
//
//   paste : per tile of a paste rectangle -- BICUBIC resize of the frame (three planes), then of the mask (one plane, its own
//           source size): horizontal pass of the source rows the tile's vertical taps need into LDS, 8 bits; vertical pass from
//           LDS, 8 bits; then out = fg * m + (1 - m) * bg in double, truncated, stored over the bg pixel.  Coefficients are
//           computed in double as Pillow's precompute_coeffs does, a column's once per thread that owns it, a row's once per
//           tile row into LDS; more source rows than the LDS holds are taken FROWS at a time (the vertical sums are integers)
//           and a tap loop runs over any count, so no ratio is too large
//
// Every 8-bit value is the integer Pillow computes and the composite is numpy's float64 expression; the arithmetic is restated in
// tests/paste_restate.py.  A thread reads and writes only its own pixels of `packed`, every integer sum is exact and every double
// is computed by one thread in a fixed order: no atomics, two calls agree bit for bit.
//
// Floating-point contraction is OFF for this whole file: Pillow's C rounds every product of the filter polynomial before the
// addition that follows, and `255 * m + (1 - m) * 255` falls just below 255 for many m only when both products are rounded.
#include "common.h"

#pragma clang fp contract(off)

namespace mink {
namespace {

constexpr int TB = 256;      // threads per workgroup
constexpr int FP = 4;        // output pixels per thread
constexpr int TC = 64;       // columns of an output tile
constexpr int TR = 16;       // rows of an output tile (TC * TR = TB * FP)
constexpr int FROWS = 48;    // source rows per LDS pass
constexpr int HROWS = FROWS / (TB / TC);  // source rows of an LDS pass one thread resizes, at most
constexpr int PREC = 22;     // fractional bits of a resize coefficient (Pillow: 32 - 8 - 2)

struct Paste {
  uint8_t *packed;
  const int64_t *offsets;
  const int32_t *sizes;
  const uint8_t *fg, *mask;
  const int64_t *table;
  int64_t total, fg_bytes, mask_bytes;  // bytes of the three buffers
  int B, max_w, max_h;
};

// what one table row describes, checked: nothing of a sample is read or written unless all of it fits
struct Job {
  const uint8_t *fg, *mask;
  uint8_t *bg;
  int fw, fh, mw, mh, rw, rh;  // source sizes of frame and mask, the resized size
  int bw;                      // row pitch of the slot in pixels
  int x0, y0, ew, eh;          // the paste rectangle in the slot
  int sx, sy;                  // its first column and row in the resized frame
};

__device__ __forceinline__ bool side_of(int64_t v, int &out) {
  if (v < 1 || v > MINK_PASTE_MAX_SIDE) return false;
  out = (int)v;
  return true;
}

__device__ __forceinline__ bool job_of(const Paste &t, int b, Job &j) {
  const int64_t *P = t.table + (int64_t)b * MINK_PASTE_PARAMS;
  if (P[MINK_PASTE_RW] == 0) return false;  // this sample does not paste
  const int w = t.sizes[2 * b], h = t.sizes[2 * b + 1];
  const int64_t off = t.offsets[b];
  if (w < 1 || h < 1 || off < 0) return false;
  const int64_t bytes = 3 * (int64_t)w * h;
  if (bytes > 3 * (int64_t)0x7FFFFFFF || t.offsets[b + 1] - off != bytes || off + bytes > t.total) return false;
  if (!(side_of(P[MINK_PASTE_FG_W], j.fw) && side_of(P[MINK_PASTE_FG_H], j.fh) && side_of(P[MINK_PASTE_MASK_W], j.mw) &&
        side_of(P[MINK_PASTE_MASK_H], j.mh) && side_of(P[MINK_PASTE_RW], j.rw) && side_of(P[MINK_PASTE_RH], j.rh)))
    return false;
  const int64_t fo = P[MINK_PASTE_FG_OFFSET], mo = P[MINK_PASTE_MASK_OFFSET];
  if (fo < 0 || fo > t.fg_bytes || 3 * (int64_t)j.fw * j.fh > t.fg_bytes - fo) return false;
  if (mo < 0 || mo > t.mask_bytes || (int64_t)j.mw * j.mh > t.mask_bytes - mo) return false;
  // the rectangle: centred in the slot, clipped to it; the window of the resized frame is centred the same way
  j.y0 = max(0, (h - j.rh) / 2), j.x0 = max(0, (w - j.rw) / 2);
  j.eh = min(h, (h + j.rh) / 2) - j.y0, j.ew = min(w, (w + j.rw) / 2) - j.x0;
  j.sy = j.rh / 2 - j.eh / 2, j.sx = j.rw / 2 - j.ew / 2;
  if (j.ew < 1 || j.eh < 1 || j.ew > t.max_w || j.eh > t.max_h) return false;
  if (j.x0 + j.ew > w || j.y0 + j.eh > h || j.sx < 0 || j.sy < 0 || j.sx + j.ew > j.rw || j.sy + j.eh > j.rh) return false;
  j.fg = t.fg + fo, j.mask = t.mask + mo, j.bg = t.packed + off, j.bw = w;
  return true;
}

// Pillow's bicubic_filter (a = -0.5, support 2)
__device__ __forceinline__ double bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// BICUBIC resize of `len` samples to `out`: taps [xmin, xmax) and the normalising sum of output index i (Pillow's
// precompute_coeffs).  len == out: Image.resize skips the pass, which is the one tap i with coefficient 1.
struct Taps {
  double center, ss, ww;
  int xmin, xmax;
  bool copy;
};

__device__ __forceinline__ double tap_weight(const Taps &k, int x) {  // x absolute, xmin <= x < xmax
  return bicubic(((double)x - k.center + 0.5) * k.ss);
}

__device__ __forceinline__ Taps taps_of(int len, int out, int i) {
  Taps k;
  k.copy = len == out;
  if (k.copy) {
    k.center = k.ss = k.ww = 0.0, k.xmin = i, k.xmax = i + 1;
    return k;
  }
  const double scale = (double)len / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs;
  k.ss = 1.0 / fs;
  k.center = ((double)i + 0.5) * scale;
  k.xmin = (int)(k.center - support + 0.5);
  if (k.xmin < 0) k.xmin = 0;
  k.xmax = (int)(k.center + support + 0.5);
  if (k.xmax > len) k.xmax = len;
  k.ww = 0.0;
  for (int x = k.xmin; x < k.xmax; ++x) k.ww += tap_weight(k, x);
  return k;
}

__device__ __forceinline__ int tap_coeff(const Taps &k, int x) {
  if (k.copy) return 1 << PREC;
  double v = tap_weight(k, x);
  if (k.ww != 0.0) v = v / k.ww;
  return v < 0.0 ? (int)(-0.5 + v * (double)(1 << PREC)) : (int)(0.5 + v * (double)(1 << PREC));
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the LDS of a workgroup
struct Tile {
  uint8_t rows[FROWS * TC * 3];  // the source rows of a pass after the horizontal pass
  int vk[TR * FROWS];            // per row of the tile, its vertical coefficients on the source rows of the pass (0: no tap)
  Taps vt[TR];                   // per row of the tile, its vertical taps
};

// The tile's pixels of src (sw x sh pixels of NC bytes) resized to rw x rh: columns c0 .. c0 + ncols - 1 and rows y0 .. y0 + nrows - 1
// of the resized image, a thread's pixel j at (lx[j], ly[j]) of the tile.  Called by the whole workgroup.
template <int NC>
__device__ __forceinline__ void resize_tile(const uint8_t *__restrict__ src, int sw, int sh, int rw, int rh, int c0, int y0, int ncols,
                                            int nrows, const int lx[FP], const int ly[FP], const bool mine[FP], Tile &lds,
                                            int out[FP][NC]) {
  uint8_t *rows = lds.rows;
  __syncthreads();  // (the previous image's taps have been read)
  if ((int)threadIdx.x < nrows) lds.vt[threadIdx.x] = taps_of(sh, rh, y0 + (int)threadIdx.x);
  __syncthreads();
  const int R0 = lds.vt[0].xmin, R1 = lds.vt[nrows - 1].xmax;  // source rows the tile's vertical taps read
  int acc[FP][NC];
#pragma unroll
  for (int j = 0; j < FP; ++j)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[j][c] = 0;
  // horizontal pass: a thread owns one resized column of the tile and every ngrp-th source row of the pass
  const int grp = threadIdx.x / ncols, ngrp = TB / ncols, cc = threadIdx.x - grp * ncols;
  Taps kh;
  if (grp < ngrp) kh = taps_of(sw, rw, c0 + cc);
  for (int r0 = R0; r0 < R1; r0 += FROWS) {
    const int nr = min(FROWS, R1 - r0);
    __syncthreads();  // (the previous pass's rows and coefficients have been read)
    // the vertical coefficients of this pass, each computed once for the whole row of the tile
    for (int e = threadIdx.x; e < nrows * FROWS; e += TB) {
      const int row = e / FROWS, y = r0 + (e - row * FROWS);
      const Taps &k = lds.vt[row];
      lds.vk[e] = (y >= k.xmin && y < k.xmax && y < r0 + nr) ? tap_coeff(k, y) : 0;
    }
    if (grp < ngrp) {
      // (a coefficient is computed once per tap and used for all of the thread's rows: at most HROWS, as ngrp >= TB / TC)
      int s[HROWS][NC];
#pragma unroll
      for (int q = 0; q < HROWS; ++q)
#pragma unroll
        for (int c = 0; c < NC; ++c) s[q][c] = 1 << (PREC - 1);
      const uint8_t *scol = src + (int64_t)(r0 + grp) * sw * NC;
      const int64_t pitch = (int64_t)ngrp * sw * NC;
      for (int x = kh.xmin; x < kh.xmax; ++x) {
        const int kc = tap_coeff(kh, x);
#pragma unroll
        for (int q = 0; q < HROWS; ++q) {
          if (grp + q * ngrp < nr) {
#pragma unroll
            for (int c = 0; c < NC; ++c) s[q][c] += kc * scol[q * pitch + (int64_t)NC * x + c];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < HROWS; ++q) {
        if (grp + q * ngrp < nr) {
          uint8_t *d = rows + ((grp + q * ngrp) * TC + cc) * NC;
#pragma unroll
          for (int c = 0; c < NC; ++c) d[c] = (uint8_t)clip8(s[q][c] >> PREC);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FP; ++j) {
      if (!mine[j]) continue;
      const int ya = max(lds.vt[ly[j]].xmin, r0), yb = min(lds.vt[ly[j]].xmax, r0 + nr);
      for (int y = ya; y < yb; ++y) {
        const int kc = lds.vk[ly[j] * FROWS + (y - r0)];
        const uint8_t *s = rows + ((y - r0) * TC + lx[j]) * NC;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[j][c] += kc * s[c];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < FP; ++j)
#pragma unroll
    for (int c = 0; c < NC; ++c) out[j][c] = clip8(((1 << (PREC - 1)) + acc[j][c]) >> PREC);
}

__global__ __launch_bounds__(TB) void img_paste_kernel(Paste t) {
  __shared__ Tile lds;
  const int b = blockIdx.y;
  Job g;
  if (!job_of(t, b, g)) return;  // (the whole workgroup: one table row)
  const int ntx = (t.max_w + TC - 1) / TC;
  const int cx0 = (blockIdx.x % ntx) * TC, cy0 = (blockIdx.x / ntx) * TR;
  if (cx0 >= g.ew || cy0 >= g.eh) return;
  const int ncols = min(TC, g.ew - cx0), nrows = min(TR, g.eh - cy0);
  int lx[FP], ly[FP];
  bool mine[FP];
#pragma unroll
  for (int j = 0; j < FP; ++j) {
    const int p = j * TB + threadIdx.x;
    ly[j] = p / ncols;
    mine[j] = ly[j] < nrows;
    lx[j] = p - ly[j] * ncols;
  }
  int rgb[FP][3], m8[FP][1];
  resize_tile<3>(g.fg, g.fw, g.fh, g.rw, g.rh, g.sx + cx0, g.sy + cy0, ncols, nrows, lx, ly, mine, lds, rgb);
  resize_tile<1>(g.mask, g.mw, g.mh, g.rw, g.rh, g.sx + cx0, g.sy + cy0, ncols, nrows, lx, ly, mine, lds, m8);
#pragma unroll
  for (int j = 0; j < FP; ++j) {
    if (!mine[j]) continue;
    uint8_t *px = g.bg + ((int64_t)(g.y0 + cy0 + ly[j]) * g.bw + (g.x0 + cx0 + lx[j])) * 3;
    const double m = (double)m8[j][0] / 255.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (uint8_t)(int)((double)rgb[j][c] * m + (1.0 - m) * (double)px[c]);
  }
}

static bool overlap(const void *a, int64_t na, const void *b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return na > 0 && nb > 0 && pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

}  // namespace
}  // namespace mink

using namespace mink;

extern "C" {

int mink_img_paste(uint8_t *packed, const int64_t *offsets, const int32_t *sizes, int64_t total_pixels, int32_t B, const uint8_t *fg,
                   int64_t fg_bytes, const uint8_t *mask, int64_t mask_bytes, const int64_t *table, int32_t max_w, int32_t max_h,
                   void *stream) {
  MINK_REQUIRE(B >= 0 && B <= 65535 && total_pixels >= 0 && total_pixels < ((int64_t)1 << 40) && fg_bytes >= 0 && mask_bytes >= 0,
               "img_paste: bad shape (B %d, %lld pixels, %lld frame bytes, %lld mask bytes)", B, (long long)total_pixels,
               (long long)fg_bytes, (long long)mask_bytes);
  MINK_REQUIRE(max_w >= 0 && max_w <= MINK_PASTE_MAX_SIDE && max_h >= 0 && max_h <= MINK_PASTE_MAX_SIDE,
               "img_paste: largest rectangle %d x %d (0 .. %d a side)", max_w, max_h, (int)MINK_PASTE_MAX_SIDE);
  if (B == 0 || max_w == 0 || max_h == 0) return MINK_OK;  // (no sample pastes: no launch)
  MINK_REQUIRE(packed && offsets && sizes && fg && mask && table, "img_paste: NULL pointer (packed, offsets, sizes, fg, mask or table)");
  MINK_REQUIRE(total_pixels >= B, "img_paste: %lld pixels for %d images", (long long)total_pixels, B);
  MINK_REQUIRE(!overlap(packed, 3 * total_pixels, fg, fg_bytes) && !overlap(packed, 3 * total_pixels, mask, mask_bytes),
               "img_paste: the frames or the masks overlap the packed batch, which is written");
  const int64_t tiles = cdiv(max_w, TC) * cdiv(max_h, TR);
  MINK_REQUIRE(tiles <= 0x7FFFFFFF, "img_paste: %lld tiles per sample", (long long)tiles);
  const Paste t = {packed, offsets, sizes, fg, mask, table, 3 * total_pixels, fg_bytes, mask_bytes, B, max_w, max_h};
  img_paste_kernel<<<dim3((unsigned)tiles, (unsigned)B), TB, 0, (hipStream_t)stream>>>(t);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

}  // extern "C"
