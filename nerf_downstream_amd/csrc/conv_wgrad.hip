// Sparse convolution on gfx950, the weight-gradient half:  dW[k] = x[nbr[.][k]]^T @ dy  (mink_conv_wgrad*).
// The forward / data-gradient half, the switch setters (mink_conv_set_stagger, mink_conv_set_math) and the timing
// registry are conv.hip; what both halves share is conv_common.h.
#include "conv_common.h"

namespace mink {

typedef unsigned u32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 pack_bits_bf16x8(const float (&v)[8]) {  // registers that already hold bf16 bits in their low halves
  auto lo = [&](int i) { return __float_as_uint(v[i]); };
  const uint4 u = make_uint4(lo(0) | (lo(1) << 16), lo(2) | (lo(3) << 16), lo(4) | (lo(5) << 16), lo(6) | (lo(7) << 16));
  return __builtin_bit_cast(bf16x8, u);
}

// ------------------------------------------------------------------------------ wgrad
// dW[k][ci][co] = sum over pairs (i,o) of offset k:  x[i][ci] * dy[o][co].
//
// Workgroup = (group of G offsets) x (64x64 ci/co super-tile) x (row range).  Per 128-row tile
// of the range the dy tile is staged ONCE in LDS and shared by the G offsets; for each offset
// the rows that really have a neighbour are compacted with a wave64 ballot + prefix rank (the
// rulebook of that tile, built on the fly), only those x rows are gathered, and the MFMA
// contraction runs over the compacted pairs -- no work is spent on missing neighbours.
// Partial sums stay in registers over the whole row range; row splits are reduced
// deterministically through a slab workspace (no atomics).
constexpr int WT = 64;      // ci / co super-tile
constexpr int WROWS = 128;  // rows per tile
constexpr int WLD = WT + 4; // LDS row stride (floats)

struct WgradParams {
  const float *x;
  const float *dy;
  const int *nbr;
  float *out;  // dw (nsplit == 1) or workspace [nsplit][K][cin][cout]
  int64_t n_out, rows_per_split;
  int ldx, cin, ldy, cout, K, ct_tiles, ngroups, ablate;
  unsigned x_bytes, dy_bytes, nbr_bytes;  // buffer descriptors (streaming kernels; tiled kernel when buf_ok)
  int buf_ok;                             // every byte size < 2^31 and n_in < 2^24: 32-bit offset arithmetic is safe
  // streaming kernel, FUSE: `dy` is the batch-norm INPUT y and the B operand is recomputed on the fly as the
  // input gradient of  pool(relu(bn(y)))  from the pooled gradient -- that gradient is never materialised
  const float *dyp;   // [n_pool][cout] gradient of the pooled output
  const int *in2out;  // [n_out] fine row -> pooled row
  const float *mean, *invstd, *gamma, *beta, *dgamma, *dbeta;
  float inv_n;
  unsigned dyp_bytes, i2o_bytes;
};

// G: offsets per workgroup.  NARROW: cin <= 32 -- the x tile is 32 floats wide and the two
// wave rows split the pair list instead of the (empty) second ci tile.
// Software pipeline per tile: all G pair lists are built up front from one nbr load per row;
// then for each offset the x gather of offset g+1 is in flight (registers) while the MFMAs
// of offset g run from LDS.
// BUF (VEC operands whose byte sizes fit 31 bits, fewer than 2^24 input rows): table, dy and gathered x rows come through
// raw buffer loads -- a missing neighbour / a row past the end / a column past the width is an out-of-range offset that
// returns zeros, so a load costs one 24-bit multiply-add instead of a 64-bit address, a select and (as the guarded form
// compiled) a branch around every load.
// (Round 5, measured and removed: 64-row tiles -- 36 KB of LDS, four workgroups per CU instead of two: l1.conv2 102.5 us against 96.7,
//  l3 93 / 82, only l4 63 / 66.5; the step 3.61-3.62 ms against 3.57-3.58.  Half the rows per tile pad an offset's pairs to 16 twice as
//  often and pay the tile's three barriers twice per 128 rows; occupancy was not what held this kernel back.  The bf16 form, whose
//  matrix work is a sixteenth, does gain from four workgroups per CU: wgrad16_kernel.)
template <int G, bool NARROW, bool VEC, bool BUF = false>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(WgradParams p) {
  static_assert(!BUF || VEC, "buffer loads are 16 bytes wide");
  constexpr int XW = NARROW ? 32 : 64;      // x tile width (floats)
  constexpr int XLD = XW + 4;               // LDS row stride
  constexpr int XC4 = XW / 4;               // float4 columns per x row
  constexpr int XRP = 256 / XC4;            // x rows per staging pass
  constexpr int XNI = WROWS / XRP;          // staging passes (float4 registers per thread)
  constexpr int LL = WROWS;                 // list length (pair count is padded to 16, <= 128)
  __shared__ __attribute__((aligned(16))) float sD[WROWS * WLD];
  __shared__ __attribute__((aligned(16))) float sX[WROWS * XLD];
  __shared__ __attribute__((aligned(16))) int s_row[G * LL];
  __shared__ int s_src[G * LL];
  __shared__ int s_cnt[G * 2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Workgroup -> (offset group / weight tile bx, row split by).  All workgroups of one row split read the same rows of x and
  // dy; in plain launch order (x fastest) they are dealt round-robin to the eight XCDs and every L2 fetches those rows for
  // itself (layer 1: 175 MB of traffic beyond L2 for 24 MB of operands, PMC r04).  When the split count is a multiple of
  // eight the workgroups of a split are given to consecutive slots of ONE XCD (as stream_slot does for the stem).
  unsigned wbx = blockIdx.x, wby = blockIdx.y;
  if (!(p.ablate & 4096) && (gridDim.y & 7u) == 0u) {  // uniform
    const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y, xcd = lin & 7u, slot = lin >> 3;
    wbx = slot % gridDim.x, wby = (slot / gridDim.x) * 8u + xcd;
  }
  const int grp = wbx % p.ngroups;
  const int tile_id = wbx / p.ngroups;
  const int ci0 = (tile_id / p.ct_tiles) * WT, co0 = (tile_id % p.ct_tiles) * WT;
  const int k0 = grp * G;
  const int ng = min(G, p.K - k0);  // offsets handled by this workgroup (uniform)
  const int64_t rbeg = (int64_t)wby * p.rows_per_split;
  const int64_t rend = min(p.n_out, rbeg + p.rows_per_split);

  const int d_c4 = tid & 15, d_rr = tid >> 4;       // dy staging: float4 column, rows d_rr + 16 i
  const int x_c4 = tid % XC4, x_rr = tid / XC4;     // x staging: float4 column, rows x_rr + XRP i

  const int wa = wave >> 1, wn = wave & 1, h = lane >> 5, col = lane & 31;
  const int wm = NARROW ? 0 : wa;

  f32x16 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = (f32x16){0};

  float4 rx[XNI] = {};
  const i32x4 bx = raw_rsrc(p.x, BUF ? p.x_bytes : 0u), bd = raw_rsrc(p.dy, BUF ? p.dy_bytes : 0u), bn = raw_rsrc(p.nbr, BUF ? p.nbr_bytes : 0u);
  const unsigned ldx4 = 4u * (unsigned)p.ldx, ldy4 = 4u * (unsigned)p.ldy, K4 = 4u * (unsigned)p.K;
  const unsigned x_coff = ci0 + 4 * x_c4 < p.cin ? 4u * (unsigned)(ci0 + 4 * x_c4) : 0x80000000u;
  const unsigned d_coff = co0 + 4 * d_c4 < p.cout ? 4u * (unsigned)(co0 + 4 * d_c4) : 0x80000000u;
  auto gather = [&](int g) {  // x rows of the compacted pairs of offset g -> registers
    if (p.ablate & 64) return;
    if constexpr (BUF) {
      // (list entries behind the padded pair count are stale rows of an earlier offset: loaded, stored, never multiplied;
      //  the tail pairs carry -1 = row 0xFFFFFF, beyond x)
#pragma unroll
      for (int i = 0; i < XNI; ++i)
        rx[i] = __builtin_bit_cast(float4, raw_load_v4(bx, (int)(__umul24((unsigned)s_src[g * LL + x_rr + XRP * i], ldx4) + x_coff), 0, 0));
      return;
    }
    const int m = s_cnt[2 * g] + s_cnt[2 * g + 1];
    const int mpad = (m + 15) & ~15;
#pragma unroll
    for (int i = 0; i < XNI; ++i) {
      const int pr = x_rr + XRP * i;
      int src = -1;
      if (pr < mpad) src = s_src[g * LL + pr];
      const int ci = ci0 + 4 * x_c4;
      if (VEC)
        rx[i] = ld4_sel(p.x, (int64_t)src * p.ldx + ci, src >= 0 && ci < p.cin);
      else
        rx[i] = src >= 0 ? ld4_guard(p.x + (int64_t)src * p.ldx + ci, p.cin - ci, false) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < XNI; ++i) *reinterpret_cast<float4 *>(&sX[(x_rr + XRP * i) * XLD + 4 * x_c4]) = rx[i];
  };

  // BUF (round 5): the table entries and the dy tile of the NEXT tile are requested before the MFMAs of this tile's last
  // offset and wait in registers: the tile prologue no longer starts with a memory round trip (one of its two).
  constexpr bool PF = BUF && G <= 3;  // (nine accumulators leave no registers for it)
  int nb_n[G];
  float4 dy_n[8];
  auto request_tile = [&](int64_t r0) __attribute__((always_inline)) {
    const int64_t row = r0 + tid;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bool ok = tid < WROWS && row < rend && g < ng;
      const int v = raw_load_i32(bn, (int)(ok ? (unsigned)row * K4 + 4u * (unsigned)(k0 + g) : 0x80000000u), 0, 0);
      nb_n[g] = ok ? v : -1;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t rw_ = r0 + d_rr + 16 * i;
      dy_n[i] = __builtin_bit_cast(float4, raw_load_v4(bd, (int)((rw_ < rend ? (unsigned)rw_ * ldy4 : 0x80000000u) + d_coff), 0, 0));
    }
  };
  if constexpr (PF) {
    if (rbeg < rend) request_tile(rbeg);
  }
  for (int64_t r0 = rbeg; r0 < rend; r0 += WROWS) {
    __syncthreads();  // previous tile fully consumed
    // ---- this tile's neighbour entries (one row per thread of waves 0/1) and dy tile
    int nb[G], rank[G];
    if constexpr (PF) {
#pragma unroll
      for (int g = 0; g < G; ++g) nb[g] = nb_n[g];
    } else if (tid < WROWS) {
      const int64_t row = r0 + tid;
      if constexpr (BUF) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const bool ok = row < rend && g < ng;
          const int v = raw_load_i32(bn, (int)(ok ? (unsigned)row * K4 + 4u * (unsigned)(k0 + g) : 0x80000000u), 0, 0);
          nb[g] = ok ? v : -1;
        }
      } else {
#pragma unroll
        for (int g = 0; g < G; ++g) nb[g] = (row < rend && g < ng) ? p.nbr[row * p.K + k0 + g] : -1;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = d_rr + 16 * i;
      const int64_t row = r0 + r;
      const int co = co0 + 4 * d_c4;
      float4 v;
      if constexpr (PF)
        v = dy_n[i];
      else if constexpr (BUF)
        v = __builtin_bit_cast(float4, raw_load_v4(bd, (int)((row < rend ? (unsigned)row * ldy4 : 0x80000000u) + d_coff), 0, 0));
      else if (VEC)
        v = ld4_sel(p.dy, row * p.ldy + co, row < rend && co < p.cout);
      else
        v = row < rend ? ld4_guard(p.dy + row * p.ldy + co, p.cout - co, false) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4 *>(&sD[r * WLD + 4 * d_c4]) = v;
    }
    // ---- rulebook of the tile: wave64 ballot + prefix rank per offset
    if (tid < WROWS) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const unsigned long long mm = __ballot(nb[g] >= 0);
        rank[g] = wave_rank(mm);
        if (lane == 0) s_cnt[2 * g + wave] = __popcll(mm);
      }
    }
    __syncthreads();
    if (tid < WROWS) {
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (nb[g] >= 0) {
          const int pos = (wave == 1 ? s_cnt[2 * g] : 0) + rank[g];
          s_row[g * LL + pos] = tid * WLD;  // LDS offset of the dy row
          s_src[g * LL + pos] = nb[g];
        }
    } else {
#pragma unroll
      for (int g = 0; g < G; ++g) {  // tail pairs: dy row 0 times a zero x row
        const int m = s_cnt[2 * g] + s_cnt[2 * g + 1];
        const int t = tid - WROWS;
        if (t < ((m + 15) & ~15) - m) {
          s_row[g * LL + m + t] = 0;
          s_src[g * LL + m + t] = -1;
        }
      }
    }
    __syncthreads();
    gather(0);
    stash();
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (g < ng) {  // uniform
      if (g + 1 < ng) gather(g + 1);  // in flight during the MFMAs below
      else if constexpr (PF) {
        if (r0 + WROWS < rend) request_tile(r0 + WROWS);  // (uniform) the next tile's table entries and dy rows, likewise
      }
      const int m = s_cnt[2 * g] + s_cnt[2 * g + 1];
      const int nsteps = ((m + 15) & ~15) >> 1;  // multiple of 8; lane half h takes pairs [h*nsteps, (h+1)*nsteps)
      const int *lrow = s_row + g * LL + h * nsteps;
      const float *xa = sX + (h * nsteps) * XLD + 32 * wm + col;
      const float *db = sD + 32 * wn + col;
      const int sbeg = NARROW ? wa * (nsteps >> 1) : 0;
      const int send = NARROW ? sbeg + (nsteps >> 1) : nsteps;
      // 4 MFMAs per trip.  Software pipeline over the trips (round 5): the dy-row offsets of trip t + 2 and the eight operands
      // of trip t + 1 are requested before the MFMAs of trip t -- as one trip at a time (round 4) every trip stood behind two
      // dependent LDS round trips (row offsets -> dy values) plus a third for its second operand pair: ~300 exposed cycles
      // per 256 of matrix work at two waves per SIMD (pipe busy 0.33-0.38).  Lists are padded to whole trips; the reads one
      // and two trips past the end are clamped to the last trip and never used.
#ifndef MINK_WPIPE
#define MINK_WPIPE 1
#endif
      if (!MINK_WPIPE) {  // (A/B builds: the round-4 loop)
        if (!(p.ablate & 128))
          for (int s = sbeg; s < send; s += 4) {
            const int4 ro = *reinterpret_cast<const int4 *>(lrow + s);
            const float a0 = xa[(s + 0) * XLD], a1 = xa[(s + 1) * XLD], a2 = xa[(s + 2) * XLD], a3 = xa[(s + 3) * XLD];
            const float b0 = db[ro.x], b1 = db[ro.y], b2 = db[ro.z], b3 = db[ro.w];
            acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[g], 0, 0, 0);
            acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[g], 0, 0, 0);
            acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b2, acc[g], 0, 0, 0);
            acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b3, acc[g], 0, 0, 0);
          }
      } else if (!(p.ablate & 128) && sbeg < send) {  // uniform
        const int last = send - 4;
        auto rows_of = [&](int s_) __attribute__((always_inline)) { return *reinterpret_cast<const int4 *>(lrow + min(s_, last)); };
        struct Ops { float a0, a1, a2, a3, b0, b1, b2, b3; };
        auto ops_of = [&](int s_, const int4 &ro) __attribute__((always_inline)) {
          const int t = min(s_, last);
          return Ops{xa[(t + 0) * XLD], xa[(t + 1) * XLD], xa[(t + 2) * XLD], xa[(t + 3) * XLD], db[ro.x], db[ro.y], db[ro.z], db[ro.w]};
        };
        auto mfma4 = [&](const Ops &o) __attribute__((always_inline)) {
          __builtin_amdgcn_sched_barrier(0);  // (left alone, the scheduler sinks every read to its use: the round-4 loop again)
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a0, o.b0, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a1, o.b1, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a2, o.b2, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a3, o.b3, acc[g], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        };
        // two trips per pass, two operand sets in turn: no register rotation beside the MFMAs
        int4 r1 = rows_of(sbeg);
        Ops A = ops_of(sbeg, r1);
        r1 = rows_of(sbeg + 4);
        for (int s = sbeg; s < send; s += 8) {
          const int4 r2 = rows_of(s + 8);
          const Ops B = ops_of(s + 4, r1);
          mfma4(A);
          if (s + 4 < send) {  // uniform
            r1 = rows_of(s + 12);
            A = ops_of(s + 8, r2);
            mfma4(B);
          }
        }
      }
      if (g + 1 < ng) {
        __syncthreads();  // everyone done reading sX
        stash();
        __syncthreads();
      }
      }
    }
  }

  // ---- epilogue: (narrow: add the two pair halves through LDS) then store the partial slab
  float *dst = p.out + (int64_t)wby * p.K * p.cin * p.cout;
  const int co = co0 + 32 * wn + col;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g < ng) {  // uniform
      const int k = k0 + g;
      if (NARROW) {
        __syncthreads();
        if (wa == 1) {
#pragma unroll
          for (int r = 0; r < 16; ++r) sD[(wn * 16 + r) * 64 + lane] = acc[g][r];
        }
        __syncthreads();
        if (wa == 0) {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[g][r] += sD[(wn * 16 + r) * 64 + lane];
        }
      }
      if (!NARROW || wa == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ci = ci0 + 32 * wm + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (ci < p.cin && co < p.cout) dst[((int64_t)k * p.cin + ci) * p.cout + co] = acc[g][r];
        }
      }
    }
  }
}

// ----------------------------------------------------------------- streaming wgrad (cin <= 32)
// The stem's weight gradient (28 -> 64 over ~8e5 rows, the largest kernel of a training step)
// as a plain streamed GEMM  dW[k] (32 x 32 per wave) += X[nbr[.][k]]^T (32 x 2) * dY (2 x 32):
// the MFMA operands are loaded straight from global memory in the 32x32x2 register layout
// (a half-wave reads one 128-byte row segment), so there is no LDS tile, no pair list and no
// barrier in the loop.  Missing neighbours and rows past the end become out-of-range buffer
// offsets, which a buffer load returns as 0:  offset = (nb & 0xFFFFFF) * 4 ldx + column is
// >= the size of x for nb = -1 as long as n_in < 2^24 and ldx < 64 (checked by the launcher).
// D row pairs of operands and D pairs of neighbour rows are in flight per wave.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *ptr, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(ptr), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float buf_load(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 0));
}
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));

// Workgroup -> (offset group, cout tile, row split) of the streaming kernels.  Workgroups are dealt to the eight XCDs
// round-robin in launch order, and the three offset groups of one row split read the same conv output, pooled gradient
// and table rows: with the plain (x = group, y = split) order they land on three different XCDs and every L2 fetches
// those rows for itself (r01: 2.0 GB of HBM reads against 0.43 GB algorithmic).  When the split count is a multiple of
// eight the groups of a split are given to consecutive slots of ONE XCD instead.
struct StreamSlot {
  int grp, cot, split;
};
__device__ __forceinline__ StreamSlot stream_slot(const WgradParams &p) {
  StreamSlot s;
  if ((int)gridDim.x == p.ngroups && (gridDim.y & 7) == 0 && !(p.ablate & 4096)) {
    const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y, xcd = lin & 7, slot = lin >> 3;
    s.grp = (int)(slot % (unsigned)p.ngroups), s.cot = 0, s.split = (int)((slot / (unsigned)p.ngroups) * 8 + xcd);
  } else {
    s.grp = blockIdx.x % p.ngroups, s.cot = blockIdx.x / p.ngroups, s.split = blockIdx.y;
  }
  return s;
}

// FLAT: the (offset, channel) axis of dW is tiled as ONE flattened axis f = k * cin + ci in runs of 32 (the forward
// kernel's FLAT=28 idea): 27 x 28 = 756 rows are 24 tiles instead of 27 offset tiles padded from 28 to 32 channels --
// a ninth fewer MFMAs, gathers and address instructions.  A lane's row of a tile then belongs to one of two offsets,
// so every lane picks ITS neighbour entry from the staged table row (a per-lane LDS read at an address that is a
// constant of (lane, tile)) instead of the half-wave sharing a broadcast; a lane past the end of the axis adds an
// out-of-range column offset.  A group is eight tiles = 256 flat rows = at most 16 offsets from kb = 256 grp / cin.
template <int D, bool FUSE = false, bool FLAT = false>
__global__ __launch_bounds__(256, 2) void wgrad_stream_kernel(WgradParams p) {
  static_assert(D % 2 == 0, "the neighbour staging ring has two slots");
  constexpr int G = FLAT ? 8 : 9;        // K == 27: three groups of nine offsets / of eight 32-row tiles of the flat axis
  constexpr int NK = FLAT ? 16 : 9;      // table entries of a row staged per group
  constexpr unsigned OOB = 0x80000000u;  // beyond any descriptor this kernel is launched with
  __shared__ float sR[2 * 16 * 64];
  // wave-private staging of the neighbour entries of one row pair: one lane per entry loads
  // them, every lane of the half reads them back (LDS broadcast) -- a same-address vector load
  // would cost as much L1 return bandwidth as the x rows themselves
  __shared__ __attribute__((aligned(16))) unsigned sN[4][2][2][32];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave & 1, wa = wave >> 1, h = lane >> 5, col = lane & 31;
  const StreamSlot ss = stream_slot(p);
  const int grp = ss.grp;
  const int co0 = ss.cot * WT;
  const int k0 = grp * G;
  constexpr int ng = G;
  const int64_t rbeg = (int64_t)ss.split * p.rows_per_split;
  const int64_t rend = min(p.n_out, rbeg + p.rows_per_split);
  const unsigned ldx4 = 4u * p.ldx, ldy4 = 4u * p.ldy, K4 = 4u * p.K;
  // The descriptors of everything indexed by the OUTPUT row end at this split's last row: a row past the end reads zeros
  // (table entry 0, dy 0, parent 0) without a test per load -- its dy operand is zero (FUSE: forced below), so whatever x
  // row its entries name contributes nothing.
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes), rd = make_rsrc(p.dy, (unsigned)rend * ldy4),
                               rn = make_rsrc(p.nbr, (unsigned)rend * K4);
  // lanes beyond cin / cout only feed rows / columns of the product that are never stored
  const unsigned xcol = 4u * min(col, p.cin - 1);
  const unsigned dcol = 4u * min(co0 + 32 * wn + col, p.cout - 1);
  const int kb = FLAT ? (256 * grp) / p.cin : k0;  // first offset this group touches
  const unsigned ncol = col < NK && kb + col < p.K ? 4u * (kb + col) : OOB;
  unsigned kidx[G], xoff[G];  // FLAT: this lane's table entry (relative to kb) and column byte offset in tile g
  if (FLAT) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int f = 32 * (grp * G + g) + col, k = f / p.cin;
      const bool in = k < p.K;
      kidx[g] = in ? (unsigned)(k - kb) : 0u;
      xoff[g] = in ? 4u * (unsigned)(f - k * p.cin) : OOB;
    }
  }
  // FUSE: per-lane constants of this lane's output channel
  const int cco = min(co0 + 32 * wn + col, p.cout - 1);
  const __amdgpu_buffer_rsrc_t rp = make_rsrc(FUSE ? (const void *)p.dyp : (const void *)p.dy, FUSE ? p.dyp_bytes : 0u),
                               ri = make_rsrc(FUSE ? (const void *)p.in2out : (const void *)p.nbr, FUSE ? (unsigned)rend * 4u : 0u);
  const float c_mu = FUSE ? p.mean[cco] : 0.f, c_is = FUSE ? p.invstd[cco] : 0.f, c_ga = FUSE ? p.gamma[cco] : 0.f,
              c_be = FUSE ? p.beta[cco] : 0.f, c_dgn = FUSE ? p.dgamma[cco] * p.inv_n : 0.f,
              c_dbn = FUSE ? p.dbeta[cco] * p.inv_n : 0.f;
  const float c_nmu = -c_mu * c_is, c_a = c_ga * c_is;
  float dp[D];        // FUSE: pooled gradient of the row's parent
  unsigned i2or[D];   // FUSE: parent row of a pair whose operands are still to be requested

  f32x16 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = (f32x16){0};
  float xa[D][G], db[D];
  unsigned nraw[D];  // lane (h, col < 9): nbr[R0 + h][k0 + col] of a pair still to be staged

  // this wave's q-th pair covers rows R0, R0 + 1 (lane half h takes R0 + h); the two wave
  // rows interleave their pairs
  const int64_t npairs = (rend - rbeg + 1) >> 1;
  const int nq = (int)((npairs + 1 - wa) >> 1);
  // 32-bit row arithmetic relative to the split (every VALU instruction issued here is a slot the matrix pipe
  // does not get: PMC shows MFMA busy + 4 x VALU instructions ~ 87 % of the SIMD cycles, no co-execution)
  const int nrel = (int)(rend - rbeg);
  const unsigned nbase = (unsigned)rbeg * K4 + ncol;     // >= 2^31 for the padding lanes (ncol == OOB): stays out of range
  const unsigned ibase = (unsigned)rbeg * 4u;
  const unsigned dbase = (unsigned)rbeg * ldy4 + dcol;
  auto rel_of = [&](int q) { return 2 * (2 * q + wa) + h; };
  auto load_raw = [&](int s, int q) {  // rows past the end read as entry 0; their x offset is forced out of range below
    const int r = rel_of(q);
    nraw[s] = __builtin_amdgcn_raw_buffer_load_b32(rn, (int)(__umul24(r, K4) + nbase), 0, 0);
  };
  auto stash = [&](int s, int slot, int q) {
    sN[wave][slot][h][col] = nraw[s];  // lanes col >= NK store padding: no exec-mask branch in the loop
  };
  auto load_i2o = [&](int s, int q) {  // (a row past the end reads parent 0: its x operand is zero anyway)
    if (FUSE) {
      const int r = rel_of(q);
      i2or[s] = __builtin_amdgcn_raw_buffer_load_b32(ri, (int)(4u * r + ibase), 0, 0);
    }
  };
  auto load_dy = [&](int s, int q) {
    const int r = rel_of(q);
    db[s] = buf_load(rd, __umul24(r, ldy4) + dbase);
    if (FUSE) dp[s] = buf_load(rp, __umul24(i2or[s], ldy4) + dcol);  // the pooled gradient has the same row pitch
  };
  auto b_operand = [&](int s, int q) {
    if (!FUSE) return db[s];
    const float xh = fmaf(db[s], c_is, c_nmu);
    const float m = fmaf(xh, c_ga, c_be) > 0.f ? 1.f : 0.f;  // (a select of the loaded value itself became an exec branch
                                                              //  and, with it, a copy of all 144 accumulators per trip)
    const float v = fmaf(-c_dgn, xh, fmaf(dp[s], m, -c_dbn));
    return (rel_of(q) < nrel ? c_a : 0.f) * v;  // a row past the end: zero
  };
  // FLAT: the lane's table entries of the pair whose x values are requested NEXT, read from the staging slot one stage
  // ahead (right behind the stash that fills it) -- read where they are used, every gather stood behind an LDS round trip
  unsigned nbn[G];
  auto read_entries = [&](int slot) {
    if constexpr (FLAT) {
#pragma unroll
      for (int g = 0; g < G; ++g) nbn[g] = sN[wave][slot][h][kidx[g]];
    }
  };
  auto load_xs = [&](int s, int slot, int q, auto &&between) {  // the nine x values of pair q
    if constexpr (FLAT) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        between(g);
        xa[s][g] = buf_load(rx, __umul24(nbn[g], ldx4) + xoff[g]);
      }
      return;
    }
    const uint4 n0 = *reinterpret_cast<const uint4 *>(&sN[wave][slot][h][0]);
    const uint4 n1 = *reinterpret_cast<const uint4 *>(&sN[wave][slot][h][4]);
    const unsigned n2 = sN[wave][slot][h][8];
    const unsigned nbv[9] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2};
#pragma unroll
    for (int g = 0; g < G; ++g) {
      between(g);
      xa[s][g] = buf_load(rx, __umul24(nbv[g], ldx4) + xcol);
    }
  };

  if (rbeg < rend) {
#pragma unroll
    for (int s = 0; s < D; ++s) {
      load_raw(s, s);
      load_i2o(s, s);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < D; ++s) {  // same load order as the loop body: the vmcnt waits there are FIFO distances
      stash(s, s & 1, s);
      read_entries(s & 1);
      load_xs(s, s & 1, s, [](int) {});
      load_dy(s, s);
      load_raw(s, s + D);
      load_i2o(s, s + D);
      __builtin_amdgcn_sched_barrier(0);
    }
    stash(0, 0, D);  // pair D
    read_entries(0);
    for (int q0 = 0; q0 < nq; q0 += D) {
#pragma unroll
      for (int s = 0; s < D; ++s) {  // pair q0 + s from slot s; pairs past nq were loaded as zeros
        const float b = b_operand(s, q0 + s);
        float a[G];
#pragma unroll
        for (int g = 0; g < G; ++g) a[g] = xa[s][g];
        load_xs(s, s & 1, q0 + s + D, [&](int g) {
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g], b, acc[g], 0, 0, 0);
        });
        load_dy(s, q0 + s + D);
        stash((s + 1) % D, (s + 1) & 1, q0 + s + D + 1);  // pair q0 + s + D + 1, loaded D - 1 pairs ago
        read_entries((s + 1) & 1);
        load_raw(s, q0 + s + 2 * D);
        load_i2o(s, q0 + s + 2 * D);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
          __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);  // VALU (offset)
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the slots (and with them the load FIFO) in program order
      }
    }
  }

  // ---- epilogue: add the two wave rows through LDS, store the partial slab
  float *dst = p.out + (int64_t)ss.split * p.K * p.cin * p.cout;
  const int co = co0 + 32 * wn + col;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g < ng) {
      const int k = k0 + g;
      __syncthreads();
      if (wa == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sR[(wn * 16 + r) * 64 + lane] = acc[g][r];
      }
      __syncthreads();
      if (wa == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ci = (r & 3) + 8 * (r >> 2) + 4 * h;
          const float v = acc[g][r] + sR[(wn * 16 + r) * 64 + lane];
          if (FLAT) {
            const int f = 32 * (grp * G + g) + ci;  // flat row of the [K * cin][cout] matrix
            if (f < p.K * p.cin && co < p.cout) dst[(int64_t)f * p.cout + co] = v;
          } else if (ci < p.cin && co < p.cout) dst[((int64_t)k * p.cin + ci) * p.cout + co] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------- streaming wgrad on the bf16 matrix cores (cin <= 32)
// BASELINE config "bf16 mixed precision": the stem's weight gradient with bf16 MFMA operands and fp32 accumulation
// (v_mfma_f32_32x32x16_bf16: sixteen rows per instruction, 16x the fp32 matrix rate).  Same ownership as the fp32
// streaming kernel -- a wave holds the nine 32 x 32 accumulators of one offset group and one 32-column half, two wave
// rows interleave the 16-row blocks -- and the same "operands straight from global memory in register layout" idea:
// lane (h, m) of the A operand holds x[nbr[R + 8h + j][k0 + g]][m], j = 0..7 (eight gathered rows of channel m), lane
// (h, n) of the B operand dY[R + 8h + j][n]; values are loaded as fp32 and packed to bf16 in registers (HBM tensors
// stay fp32).  With the matrix work down 16x the kernel is bound by its gathers, which are the fp32 kernel's.
// Pipeline per wave: table entries of block b+1 are fetched during block b and broadcast through a wave-private LDS
// slot; the x gathers run one three-offset sub-batch ahead of the MFMAs; FUSE recomputes dY from the conv output and
// the pooled gradient as the fp32 kernel does (parents one block ahead).

// B16 (bf16 STORAGE of the full-resolution stage, stem16.hip): x is the bf16 copy of the input ([n][32], 64-byte rows) and
// `dy` -- FUSE: the convolution output -- is bf16 too; the operands are then 2-byte loads that need no conversion.
template <bool FUSE, bool B16 = false>
__global__ __launch_bounds__(256, 2) void wgrad_stream_bf16_kernel(WgradParams p) {
  constexpr int G = 9, SB = 1;           // offsets per group, offsets per sub-batch (gathers run one sub-batch ahead)
  __shared__ float sR[2 * 16 * 64];
  __shared__ __attribute__((aligned(16))) unsigned sN[4][2][12][16];  // [wave][slot][offset (9 used)][row of the block]: a lane's eight rows of one offset are two 16-byte reads
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave & 1, wa = wave >> 1, h = lane >> 5, col = lane & 31;
  const StreamSlot ss = stream_slot(p);
  const int grp = ss.grp;
  const int co0 = ss.cot * WT;
  const int k0 = grp * G;
  const int64_t rbeg = (int64_t)ss.split * p.rows_per_split;
  const int64_t rend = min(p.n_out, rbeg + p.rows_per_split);
  const int nrel = (int)(rend - rbeg);
  const int nblocks = (nrel + 15) >> 4;
  const int nq = (nblocks + 1 - wa) >> 1;  // this wave's blocks: b = 2 q + wa
  const unsigned ldx4 = (B16 ? 2u : 4u) * p.ldx, ldy4 = (B16 ? 2u : 4u) * p.ldy, ldp4 = 4u * p.ldy, K4 = 4u * p.K;
  // (as in the fp32 kernel: what is indexed by the output row ends at this split's last row -- rows past it read zeros)
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes), rd = make_rsrc(p.dy, (unsigned)rend * ldy4), rn = make_rsrc(p.nbr, p.nbr_bytes);
  const __amdgpu_buffer_rsrc_t rp = make_rsrc(FUSE ? (const void *)p.dyp : (const void *)p.dy, FUSE ? p.dyp_bytes : 0u),
                               ri = make_rsrc(FUSE ? (const void *)p.in2out : (const void *)p.nbr, FUSE ? (unsigned)rend * 4u : 0u);
  const unsigned xcol = (B16 ? 2u : 4u) * min(col, p.cin - 1);
  const unsigned dcol = (B16 ? 2u : 4u) * min(co0 + 32 * wn + col, p.cout - 1), pcol = 4u * min(co0 + 32 * wn + col, p.cout - 1);
  const int cco = min(co0 + 32 * wn + col, p.cout - 1);
  const float c_mu = FUSE ? p.mean[cco] : 0.f, c_is = FUSE ? p.invstd[cco] : 0.f, c_ga = FUSE ? p.gamma[cco] : 0.f,
              c_be = FUSE ? p.beta[cco] : 0.f, c_dgn = FUSE ? p.dgamma[cco] * p.inv_n : 0.f,
              c_dbn = FUSE ? p.dbeta[cco] * p.inv_n : 0.f;
  const float c_nmu = -c_mu * c_is, c_a = c_ga * c_is;
  const unsigned nbase = (unsigned)rbeg * K4, ibase = (unsigned)rbeg * 4u, dbase = (unsigned)rbeg * ldy4 + dcol;

  f32x16 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = (f32x16){0};
  if (nq <= 0) goto epilogue;
  {
    // table loader lanes: row kk = lane >> 2 of the block, entries 3 (lane & 3) .. + 2 (lanes with (lane & 3) == 3 idle)
    const int t_row = lane >> 2, t_part = lane & 3;
    unsigned traw[3];
    auto load_table = [&](int q) __attribute__((always_inline)) {  // block 2 q + wa (rows past the end read as "no neighbour")
      const int r = 16 * (2 * q + wa) + t_row;
      const bool ok = q < nq && r < nrel && t_part < 3;
#pragma unroll
      for (int e = 0; e < 3; ++e)
        traw[e] = ok ? (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rn, (int)(__umul24(r, K4) + nbase + 4u * (k0 + 3 * t_part + e)), 0, 0)
                     : 0xFFFFFFFFu;
    };
    auto stash_table = [&](int slot) __attribute__((always_inline)) {
      if (t_part < 3) {
#pragma unroll
        for (int e = 0; e < 3; ++e) sN[wave][slot][3 * t_part + e][t_row] = traw[e];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private slot: in-order LDS, visible to the reads below
    };
    unsigned par[8];  // FUSE: pooled parent of this lane's eight rows, one block ahead
    auto load_par = [&](int q) __attribute__((always_inline)) {
      if (FUSE) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = 16 * (2 * q + wa) + 8 * h + j;
          par[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(ri, (int)(4u * r + ibase), 0, 0);  // (past the end: parent 0)
        }
      }
    };
    float braw[8], bpool[8];
    auto load_b = [&](int q) __attribute__((always_inline)) {  // dY rows (FUSE: conv output rows + pooled gradient of their parents)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = 16 * (2 * q + wa) + 8 * h + j;
        if constexpr (B16)
          braw[j] = __uint_as_float((unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rd, (int)(__umul24(r, ldy4) + dbase), 0, 0) << 16);
        else
          braw[j] = buf_load(rd, __umul24(r, ldy4) + dbase);
        if (FUSE) bpool[j] = buf_load(rp, __umul24(par[j], ldp4) + pcol);
      }
    };
    auto b_fragment = [&](int q) __attribute__((always_inline)) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!FUSE) {
          v[j] = braw[j];
        } else {
          const int r = 16 * (2 * q + wa) + 8 * h + j;
          const float xh = fmaf(braw[j], c_is, c_nmu);
          const float m = fmaf(xh, c_ga, c_be) > 0.f ? 1.f : 0.f;
          v[j] = (r < nrel ? c_a : 0.f) * fmaf(-c_dgn, xh, fmaf(bpool[j], m, -c_dbn));  // a row past the end must not contribute
        }
      }
      return pack_bf16x8(v);
    };
    float xraw[3][SB][8];
    auto load_x = [&](int buf, int slot, int sb) __attribute__((always_inline)) {  // the x gathers of one sub-batch (three offsets x eight rows)
#pragma unroll
      for (int g = 0; g < SB; ++g) {
        const uint4 n0 = *reinterpret_cast<const uint4 *>(&sN[wave][slot][SB * sb + g][8 * h]);
        const uint4 n1 = *reinterpret_cast<const uint4 *>(&sN[wave][slot][SB * sb + g][8 * h + 4]);
        const unsigned nbv[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if constexpr (B16)  // (the bf16 bits, kept in the low half of the register)
            xraw[buf][g][j] = __uint_as_float((unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rx, (int)(__umul24(nbv[j], ldx4) + xcol), 0, 0));
          else
            xraw[buf][g][j] = buf_load(rx, __umul24(nbv[j], ldx4) + xcol);  // (-1 is row 0xFFFFFF: beyond x, reads as zero)
      }
    };
    // ---- prologue: table of block 0 staged, of block 1 in flight; B operands and first x sub-batch of block 0 in flight
    load_table(0);
    load_par(0);
    stash_table(0);
    load_b(0);
    load_table(1);
    load_par(1);
    load_x(0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    // one block = nine one-offset sub-batches; the gathers run one sub-batch ahead through a ring of three buffers
    // (nine is a multiple of three: every register index is a compile-time constant without unrolling over blocks)
    for (int q = 0; q < nq; ++q) {
      const int slot = q & 1;
      const bf16x8 bfrag = b_fragment(q);
#pragma unroll
      for (int sb = 0; sb < G; ++sb) {
        const int cur = sb % 3, nxt = (sb + 1) % 3;
        if (sb == 0) load_b(q + 1);  // (parents of block q + 1 arrived one block ago)
        if (sb == 1) load_par(q + 2);
        if (sb < G - 1) {
          load_x(nxt, slot, sb + 1);
        } else {
          stash_table(slot ^ 1);  // entries of block q + 1, in flight since the previous block
          load_x(nxt, slot ^ 1, 0);
          load_table(q + 2);
        }
        acc[sb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(B16 ? pack_bits_bf16x8(xraw[cur][0]) : pack_bf16x8(xraw[cur][0]), bfrag, acc[sb], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);  // keep the sub-batches (and the load FIFO) in program order
      }
    }
  }
epilogue:
  // ---- add the two wave rows through LDS, store the partial slab
  float *dst = p.out + (int64_t)ss.split * p.K * p.cin * p.cout;
  const int co = co0 + 32 * wn + col;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int k = k0 + g;
    __syncthreads();
    if (wa == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sR[(wn * 16 + r) * 64 + lane] = acc[g][r];
    }
    __syncthreads();
    if (wa == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float v = acc[g][r] + sR[(wn * 16 + r) * 64 + lane];
        if (ci < p.cin && co < p.cout) dst[((int64_t)k * p.cin + ci) * p.cout + co] = v;
      }
    }
  }
}

// ---------------------------------------------------- streaming wgrad over bf16 STORAGE, operands transposed through LDS
// With x ([n][32] bf16, 64-byte rows) and the convolution output in bf16 (stem16.hip) the kernel above still issues eight
// 2-byte gathers per MFMA operand: a lane of the A operand holds ONE channel of EIGHT different rows.  Here the sixteen
// gathered rows of an operand are fetched the way they lie in memory -- four lanes x 16 bytes per row, ONE load per lane --
// written to a wave-private 1 KB LDS image [16 rows][32 channels] and read back with ds_read_b64_tr_b16, gfx950's
// transposing LDS read (a lane receives its channel of four rows), two reads per operand.  The B operand (dY recomputed
// from the convolution output, the pooled gradient and the batch-norm constants, FUSE of the kernels above) takes the same
// route: a lane computes eight consecutive columns of one row (constants per column from LDS), packs them and the wave
// reads the block back transposed -- 3 loads per block instead of 16.  ~16 load instructions per 16-row block instead of
// ~100.  Ownership, row splits, slabs and epilogue are those of wgrad_stream_bf16_kernel; LDS traffic is wave-private and
// in issue order (no barrier in the loop).  cout == 64, K == 27, x pitch 32.
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 lds_tr16(const unsigned short *p) {  // ds_read_b64_tr_b16 (EXEC must be all ones)
  return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)p));
}
template <int A>
__device__ __forceinline__ unsigned quad_bcast(unsigned v) {  // lane A of every quad
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, A | (A << 2) | (A << 4) | (A << 6), 0xF, 0xF, false);
}

// (A variant whose two column-half waves shared ONE set of gathered operands through a double-buffered image and a
// barrier per block measured 246 us against 244: the gathers are not what bounds this kernel -- PMC: 184 vector-ALU
// instructions per 16-row block and wave, the recomputation of dY, beside nine MFMAs.)
__global__ __launch_bounds__(256, 2) void wgrad_stream_b16t_kernel(WgradParams p) {
  constexpr int G = 9;
  constexpr unsigned OOB = 0x80000000u;
  constexpr int NSL = 4 * 3;  // 1 KB operand images: [wave][ring]
  __shared__ float sR[2 * 16 * 64];
  __shared__ __attribute__((aligned(16))) unsigned short sA[NSL][16 * 32];  // [row][channel]
  __shared__ __attribute__((aligned(16))) unsigned short sB[4][16 * 32];    // [wave][row][column of the wave's half]
  __shared__ __attribute__((aligned(16))) float sC[7][64];                  // per column: invstd, -mean*invstd, gamma, beta, gamma*invstd, dgamma/n, dbeta/n
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave & 1, wa = wave >> 1, h = lane >> 5, col = lane & 31;
  const StreamSlot ss = stream_slot(p);
  const int grp = ss.grp;
  const int k0 = grp * G;
  const int64_t rbeg = (int64_t)ss.split * p.rows_per_split;
  const int64_t rend = min(p.n_out, rbeg + p.rows_per_split);
  const int nrel = (int)(rend - rbeg);
  const int nblocks = (nrel + 15) >> 4;
  const int nq = (nblocks + 1 - wa) >> 1;  // this wave's blocks: b = 2 q + wa
  if (tid < 64) {
    const float is = p.invstd[tid], mu = p.mean[tid], ga = p.gamma[tid];
    sC[0][tid] = is, sC[1][tid] = -mu * is, sC[2][tid] = ga, sC[3][tid] = p.beta[tid], sC[4][tid] = ga * is;
    sC[5][tid] = p.dgamma[tid] * p.inv_n, sC[6][tid] = p.dbeta[tid] * p.inv_n;
  }
  __syncthreads();
  f32x16 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = (f32x16){0};
  if (nq > 0) {  // (wave-uniform)
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes), ry = make_rsrc(p.dy, (unsigned)rend * 128u),
                                 rn = make_rsrc(p.nbr, (unsigned)rend * 4u * 27u), rp = make_rsrc(p.dyp, p.dyp_bytes),
                                 ri = make_rsrc(p.in2out, (unsigned)rend * 4u);
    const int g_row = lane >> 2, g_ch = lane & 3;  // gather / compute role: row of the block, 16-byte chunk
    const unsigned nbase = (unsigned)rbeg * 108u + 4u * (unsigned)(k0 + 3 * g_ch), ibase = (unsigned)rbeg * 4u;
    const unsigned ybase = (unsigned)rbeg * 128u + 64u * wn + 16u * g_ch, pcol = 128u * wn + 32u * g_ch;
    unsigned short *sBw = &sB[wave][0];
    const int st_off = g_row * 32 + 8 * g_ch;                                        // halfword offset of this lane's 16 bytes
    const int tr_off = (8 * h + ((lane & 15) >> 2)) * 32 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);  // transposed read, rows 8h..8h+3 (+128: rows 8h+4..)
    unsigned traw[3], par, ent[G];
    u32x4v ga[G], yraw, dp0, dp1;
    auto rel_row = [&](int q) { return 16 * (2 * q + wa) + g_row; };
    auto load_table = [&](int q) __attribute__((always_inline)) {  // entries 3 g_ch .. + 2 of the lane's row (g_ch == 3: idle)
      const int r = rel_row(q);
      const bool ok = q < nq && r < nrel && g_ch < 3;
#pragma unroll
      for (int e = 0; e < 3; ++e)
        traw[e] = ok ? (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rn, (int)(__umul24(r, 108u) + nbase + 4u * e), 0, 0) : 0xFFFFFFFFu;
    };
    auto load_par = [&](int q) __attribute__((always_inline)) {
      const int r = rel_row(q);
      par = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(ri, (int)(q < nq && r < nrel ? 4u * r + ibase : OOB), 0, 0);  // (past the end: parent 0)
    };
    auto spread = [&]() __attribute__((always_inline)) {  // every lane of a row's quad gets the row's nine entries
      ent[0] = quad_bcast<0>(traw[0]), ent[1] = quad_bcast<0>(traw[1]), ent[2] = quad_bcast<0>(traw[2]);
      ent[3] = quad_bcast<1>(traw[0]), ent[4] = quad_bcast<1>(traw[1]), ent[5] = quad_bcast<1>(traw[2]);
      ent[6] = quad_bcast<2>(traw[0]), ent[7] = quad_bcast<2>(traw[1]), ent[8] = quad_bcast<2>(traw[2]);
    };
    auto gather = [&](int g) __attribute__((always_inline)) {  // (-1 is row 0xFFFFFF: beyond x, reads as zeros)
      ga[g] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(__umul24(ent[g], 64u) + 16u * g_ch), 0, 0);
    };
    auto load_b = [&](int q) __attribute__((always_inline)) {  // conv output row chunk + pooled gradient of its parent
      const int r = rel_row(q);
      yraw = __builtin_amdgcn_raw_buffer_load_b128(ry, (int)(q < nq && r < nrel ? __umul24(r, 128u) + ybase : OOB), 0, 0);
      const unsigned po = __umul24(par, 256u) + pcol;
      dp0 = __builtin_amdgcn_raw_buffer_load_b128(rp, (int)po, 0, 0);
      dp1 = __builtin_amdgcn_raw_buffer_load_b128(rp, (int)(po + 16u), 0, 0);
    };
    auto b_operand = [&](int q) __attribute__((always_inline)) {  // dY of block q: computed row-major, read back transposed
      const int cb = 32 * wn + 8 * g_ch;
      const unsigned yw[4] = {yraw[0], yraw[1], yraw[2], yraw[3]};
      const float dpv[8] = {__uint_as_float(dp0[0]), __uint_as_float(dp0[1]), __uint_as_float(dp0[2]), __uint_as_float(dp0[3]),
                            __uint_as_float(dp1[0]), __uint_as_float(dp1[1]), __uint_as_float(dp1[2]), __uint_as_float(dp1[3])};
      const bool live = rel_row(q) < nrel;
      float v[8];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {  // four columns at a time: 28 constants live, not 56
        float4 cs[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) cs[c] = *reinterpret_cast<const float4 *>(&sC[c][cb + 4 * hf]);
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const int e = 4 * hf + e4;
          auto at = [&](int c) { return e4 == 0 ? cs[c].x : e4 == 1 ? cs[c].y : e4 == 2 ? cs[c].z : cs[c].w; };
          const float y = __uint_as_float((e & 1) ? (yw[e >> 1] & 0xFFFF0000u) : (yw[e >> 1] << 16));
          const float xh = fmaf(y, at(0), at(1));
          const float m = fmaf(xh, at(2), at(3)) > 0.f ? 1.f : 0.f;
          v[e] = (live ? at(4) : 0.f) * fmaf(-at(5), xh, fmaf(dpv[e], m, -at(6)));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      *reinterpret_cast<uint4 *>(sBw + st_off) = make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7]));
      const uint2 b_lo = lds_tr16(sBw + tr_off), b_hi = lds_tr16(sBw + tr_off + 128);
      return __builtin_bit_cast(bf16x8, make_uint4(b_lo.x, b_lo.y, b_hi.x, b_hi.y));
    };
    // ---- prologue
    load_table(0);
    load_par(0);
    spread();
#pragma unroll
    for (int g = 0; g < G; ++g) gather(g);
    load_b(0);
    load_table(1);
    load_par(1);
    __builtin_amdgcn_sched_barrier(0);
    for (int q = 0; q < nq; ++q) {
      spread();  // entries of block q + 1
      {
        unsigned short *sAw = &sA[wave * 3][0];
        const bf16x8 bfrag = b_operand(q);
        load_b(q + 1);  // (its parents arrived one block ago)
        load_par(q + 2);
        load_table(q + 2);
        __builtin_amdgcn_sched_barrier(0);
        // ---- nine offsets: gathered rows of block q -> LDS -> transposed fragment; the registers take block q + 1's rows
        *reinterpret_cast<u32x4v *>(sAw + st_off) = ga[0];
        gather(0);
        uint2 a_lo = lds_tr16(sAw + tr_off), a_hi = lds_tr16(sAw + tr_off + 128);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const bf16x8 afrag = __builtin_bit_cast(bf16x8, make_uint4(a_lo.x, a_lo.y, a_hi.x, a_hi.y));
          if (g + 1 < G) {
            unsigned short *slot = sAw + ((g + 1) % 3) * 512;
            *reinterpret_cast<u32x4v *>(slot + st_off) = ga[g + 1];
            gather(g + 1);
            a_lo = lds_tr16(slot + tr_off), a_hi = lds_tr16(slot + tr_off + 128);
          }
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag, bfrag, acc[g], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  // ---- epilogue: add the two wave rows through LDS, store the partial slab
  float *dst = p.out + (int64_t)ss.split * p.K * p.cin * p.cout;
  const int co = 32 * wn + col;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int k = k0 + g;
    __syncthreads();
    if (wa == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sR[(wn * 16 + r) * 64 + lane] = acc[g][r];
    }
    __syncthreads();
    if (wa == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float v = acc[g][r] + sR[(wn * 16 + r) * 64 + lane];
        if (ci < p.cin) dst[((int64_t)k * p.cin + ci) * p.cout + co] = v;
      }
    }
  }
}

// out[i] = sum_z ws[z][i]: 64 outputs x 4 slab lanes per workgroup (fixed order -> deterministic)
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float *__restrict__ ws, int64_t count, int nslab,
                                                          float *__restrict__ out) {
  __shared__ float s_part[4][64];
  const int lane = threadIdx.x >> 6, o = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 64 + o;
  // four independent chains per thread (slabs z, z + 4, z + 8, z + 12 of its lane): sixteen loads in flight instead of the
  // one-after-the-other adds of a single chain -- the stem's 168-slab reduce is the LAST kernel of a training step
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < count) {
    const float *q = ws + i;
    int z = lane;
    for (; z + 12 < nslab; z += 16) {
      const float a = q[(int64_t)z * count], b = q[(int64_t)(z + 4) * count], c = q[(int64_t)(z + 8) * count], d = q[(int64_t)(z + 12) * count];
      s0 += a, s1 += b, s2 += c, s3 += d;
    }
    for (; z < nslab; z += 4) s0 += q[(int64_t)z * count];
  }
  const float s = (s0 + s1) + (s2 + s3);
  s_part[lane][o] = s;
  __syncthreads();
  if (lane == 0 && i < count) out[i] = (s_part[0][o] + s_part[1][o]) + (s_part[2][o] + s_part[3][o]);
}

// ---- decide, then do: what a weight-gradient call looks like, and the launch wgrad_plan makes of it.  wgrad_impl launches the
// plan; mink_conv_wgrad_workspace_bytes, mink_conv_wgrad_bn_relu_pool_supported and mink_conv_wgrad_launch_info read it.
struct WgradCall {
  int64_t n_in, n_out, n_pool;
  int ldx, cin, ldy, cout, K;
  int fuse;      // 0 plain, 1 dy recomputed from pool(relu(bn(y))), 2 the same with x and y stored as bf16
  bool aligned;  // x | dy on 16 bytes
};

struct WgradPlan {
  int G, ngroups, nsplit;
  int64_t rows_per_split;
  int family;   // MINK_KERNEL_WGRAD {G, NARROW, VEC, BUF} / _WGRAD16 {G} / _WGRAD_STREAM {D, FUSE, FLAT} / _WGRAD_STREAM_BF16 {FUSE, B16} / _WGRAD_STREAM_B16T
  int targ[4];  // ... the template arguments of the instantiation
  dim3 grid;
  int ct_tiles;
  unsigned x_bytes, dy_bytes, nbr_bytes;
  bool buf_ok;       // every byte size < 2^31 and n_in < 2^24: 32-bit offset arithmetic is safe
  bool flat;         // flattened (offset, channel) tiling of the streaming fp32 kernel
  bool streaming;    // the stem shape on the streaming kernels (what a fused call needs)
  bool bf16_stream;  // ... on the bf16 matrix cores (what a fused call with bf16 storage needs)
};

static WgradPlan wgrad_plan(const WgradCall &c, const ConvKnobs &kn) {
  WgradPlan pl = {};
  const int64_t n_out = c.n_out;
  const int K = c.K, cin = c.cin, cout = c.cout;
  const int64_t tiles = cdiv(cin, WT) * cdiv(cout, WT);
  const int64_t row_tiles = cdiv(n_out, WROWS);
  // offsets per workgroup: share the dy tile between as many offsets as parallelism allows
  pl.G = 1;
  if (K >= 9 && tiles * cdiv(K, 9) * row_tiles >= 1024) pl.G = 9;
  else if (K >= 3 && tiles * cdiv(K, 3) * row_tiles >= 1024) pl.G = 3;
  const bool tiny = row_tiles <= 4 && tiles * K >= 512;  // few rows, many weight tiles: one workgroup per (tile, offset), no slabs
  if (tiny) pl.G = 1;
  // (layer1, one 64 x 64 weight tile and many rows: alone, one offset per workgroup and three times the workgroups win --
  //  kbench wsweep: l1.conv2 G1 z64 89 us against G3 z48 101 -- but inside a step, beside the data-gradient chain, the 1296
  //  workgroups take 208 us where the 432 take 125: the plan stays)
  if (kn.wgrad_force & 0xF) pl.G = (kn.wgrad_force & 0xF) == 1 ? 1 : (kn.wgrad_force & 0xF) == 2 ? 3 : 9;  // tuning hook
  pl.ngroups = (int)cdiv(K, pl.G);
  const int64_t xy = tiles * pl.ngroups;
  int64_t z = cdiv(512, xy);  // ~2 resident workgroups per CU: fewer partial slabs to write and reduce
  if (tiny) z = 1;
  if (kn.wgrad_force >> 4) z = kn.wgrad_force >> 4;
  if (z > row_tiles) z = row_tiles;
  if (z < 1) z = 1;
  const bool streamed = pl.G == 9 && K == 27 && cin <= 32 && tiles == 1 && z >= 16;  // see stream_slot: splits in eights
  if (streamed) z = z / 8 * 8;  // rounded DOWN: 3 x 176 workgroups no longer fit the 512 resident slots (measured 1.21 ms against 0.86)
  pl.rows_per_split = align_up(cdiv(n_out, z), WROWS);
  pl.nsplit = (int)cdiv(n_out, pl.rows_per_split);
  if (pl.nsplit < 1) pl.nsplit = 1;
  if (streamed) pl.nsplit = (int)align_up(pl.nsplit, 8);  // trailing splits may be empty: they store zero slabs

  // ---- the kernel and its launch configuration
  pl.ct_tiles = (int)cdiv(cout, WT);
  pl.grid = dim3((unsigned)(pl.ngroups * cdiv(cin, WT) * pl.ct_tiles), (unsigned)pl.nsplit);
  const int esz = c.fuse == 2 ? 2 : 4;
  const int64_t xb = esz * c.n_in * c.ldx, db = esz * n_out * c.ldy, nb = 4 * n_out * K;
  pl.x_bytes = (unsigned)xb, pl.dy_bytes = (unsigned)db, pl.nbr_bytes = (unsigned)nb;
  pl.buf_ok = xb < (1ll << 31) && db < (1ll << 31) && nb < (1ll << 31) && c.n_in < (1 << 24) && xb <= 0xFFFFFFll * 4 * c.ldx;
  // "No neighbour" is row 0xFFFFFF, and the kernels form its byte offset as the low 32 bits of 0xFFFFFF * 4 ldx (__umul24):
  // with ldx > 64 the product passes 2^32 and the offset the load sees is the wrapped one -- 2^26 (ldx mod 64) - 4 ldx, e.g.
  // 2^28 - 272 at ldx = 68 -- which lies INSIDE an x of more bytes than that: a tile's padding pairs then multiply real rows
  // of x instead of zeros.  The 64-bit comparison above does not see the wrap; on top of it, the offset as the kernel computes
  // it must lie at or beyond the end of x for every column of a row (+ 4 cin without passing 2^32), and so must that offset
  // with the "column past the width" bit 31 added.
  const uint32_t none32 = (uint32_t)(0xFFFFFFull * 4ull * (uint64_t)c.ldx);
  pl.buf_ok = pl.buf_ok && (int64_t)none32 >= xb && (int64_t)none32 + 4ll * cin <= (1ll << 32) && (int64_t)(uint32_t)(none32 + 0x80000000u) >= xb;
  const bool stream_ok = K == 27 && cin <= 32 && c.ldx < 64 && c.n_in < (1 << 24) && 4 * c.n_in * c.ldx < (1ll << 31) &&
                         4 * n_out * c.ldy < (1ll << 31) && 4 * n_out * K < (1ll << 31);  // what the buffer-offset arithmetic assumes
  pl.streaming = pl.G == 9 && stream_ok && kn.wgrad_stream;
  const bool bf16_math = kn.math == 1 && !kn.wgrad_bf16_off;
  pl.bf16_stream = bf16_math && pl.streaming;
  // flattened (offset, channel) tiling: 24 instead of 27 tiles when the axis fits three groups of 256 rows and the
  // padded channels are worth saving; ldx <= 32 keeps "no neighbour" + "past the axis" inside 32-bit offset arithmetic
  pl.flat = K * cin <= 768 && K * cin > 512 && c.ldx <= 32 && cin >= 16;
  const bool strides4 = ((c.ldx | c.ldy) & 3) == 0;
  if (c.fuse == 2 && cout == 64 && c.ldx == 32 && !kn.b16t_off) {  // (set_stagger bit 11: the 2-byte-gather kernel, A/B tests)
    pl.family = MINK_KERNEL_WGRAD_STREAM_B16T;
  } else if (c.fuse == 2 || pl.bf16_stream) {  // (four row pairs in flight: 2 / 6 / 8 measured, DESIGN appendix)
    pl.family = MINK_KERNEL_WGRAD_STREAM_BF16;
    pl.targ[0] = c.fuse != 0, pl.targ[1] = c.fuse == 2;
  } else if (c.fuse || pl.streaming) {  // (a fused call the streaming kernels do not take is refused: wgrad_plan_check)
    pl.family = MINK_KERNEL_WGRAD_STREAM;
    pl.targ[0] = 4, pl.targ[1] = c.fuse != 0, pl.targ[2] = pl.flat;
  } else if (bf16_math && pl.G != 9 && cin % WT == 0 && cout % WT == 0 && pl.buf_ok && c.aligned && strides4) {
    // --math bf16: the mid-layer weight gradients on the bf16 matrix cores too (wgrad16_kernel)
    pl.family = MINK_KERNEL_WGRAD16;
    pl.targ[0] = pl.G == 3 ? 3 : 1;
  } else {
    const bool vec = c.aligned && strides4 && ((cin | cout) & 3) == 0;
    pl.family = MINK_KERNEL_WGRAD;
    pl.targ[0] = pl.G, pl.targ[1] = cin <= 32, pl.targ[2] = vec, pl.targ[3] = vec && pl.buf_ok;
  }
  return pl;
}

// The refusals of a fused call, which need the plan; before any launch.
static int wgrad_plan_check(const WgradCall &c, const WgradPlan &pl) {
  if (!c.fuse) return MINK_OK;
  MINK_REQUIRE(pl.streaming && 4 * c.n_pool * c.ldy < (1ll << 31),
               "wgrad_bn_relu_pool: shape not supported by the streaming kernel (ask mink_conv_wgrad_bn_relu_pool_supported)");
  MINK_REQUIRE(c.fuse != 2 || pl.bf16_stream, "wgrad_bn_relu_pool_b16: needs bf16 math (mink_conv_set_math(1))");
  return MINK_OK;
}

// ------------------------------------------------ tiled weight gradient on the bf16 matrix cores (mid layers, --math bf16)
// BASELINE config #4 ("MFMA bf16 on the rulebook GEMM") for the twelve mid-layer weight gradients, which until round 4 stayed on
// wgrad_kernel's exact-fp32 MFMAs (0.8 ms of that step's weight-gradient stream).  Same ownership as wgrad_kernel -- workgroup =
// (G offsets) x (64 x 64 ci / co tile) x (row range); per 128-row tile the dy tile is staged once, per offset the rows that have
// a neighbour are compacted (wave64 ballot + prefix rank) and only their x rows gathered -- but both tiles live in LDS as
// bf16, ROW-major as they arrive (an 8-byte store per gathered float4), and the MFMA fragments come out of them through
// gfx950's transposing LDS read (ds_read_b64_tr_b16: sixteen lanes hand in four rows x sixteen channels and each receives its
// channel of the four rows): v_mfma_f32_32x32x16_bf16 contracts SIXTEEN pairs per instruction where the fp32 kernel's
// 32x32x2 contracts two.  The dy rows of an offset's pairs are reached through the pair list (a lane's row address is its
// own: no compacted copy of the tile).  LDS: 2 x 128 rows x 128 bytes + lists = 37 KB -> four workgroups per CU where the
// fp32 kernel's 74 KB allow two.  fp32 accumulation, fp32 slabs, deterministic (no atomics).  cin, cout multiples of 64,
// 16-byte aligned operands, 32-bit buffer offsets (the launcher checks).
// Bank conflicts of the transposing read: a half-wave reads four rows x 64 bytes; with 128-byte rows, rows r and r + 2 would
// share banks, so the two 64-byte halves of a row are swapped on rows with bit 1 set (a row's pieces then cover all 256 bytes
// over any four consecutive rows).
template <int G>
__global__ __launch_bounds__(256, 4) void wgrad16_kernel(WgradParams p) {
  constexpr int LL = WROWS;  // list length (pair count padded to 16, <= 128)
  constexpr int PITCH = 64;  // halfwords per row of both images
  __shared__ __attribute__((aligned(16))) unsigned short sD[WROWS * PITCH];  // dy tile, bf16 [row][co]
  __shared__ __attribute__((aligned(16))) unsigned short sX[WROWS * PITCH];  // gathered x rows of one offset, bf16 [pair][ci]
  __shared__ int s_row[G * LL];  // tile row of the p-th pair (padding: row 0)
  __shared__ int s_src[G * LL];  // its x row (padding: -1 = a row beyond x: zeros)
  __shared__ int s_cnt[G * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned wbx = blockIdx.x, wby = blockIdx.y;
  if (!(p.ablate & 4096) && (gridDim.y & 7u) == 0u) {  // uniform: the workgroups of a row split share an XCD (see wgrad_kernel)
    const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y, xcd = lin & 7u, slot = lin >> 3;
    wbx = slot % gridDim.x, wby = (slot / gridDim.x) * 8u + xcd;
  }
  const int grp = wbx % p.ngroups, tile_id = wbx / p.ngroups;
  const int ci0 = (tile_id / p.ct_tiles) * WT, co0 = (tile_id % p.ct_tiles) * WT;
  const int k0 = grp * G;
  const int ng = min(G, p.K - k0);
  const int64_t rbeg = (int64_t)wby * p.rows_per_split;
  const int64_t rend = min(p.n_out, rbeg + p.rows_per_split);
  const int c4 = tid & 15, rr = tid >> 4;  // staging: float4 column, rows rr + 16 i (both tiles)
  const int wm = wave >> 1, wn = wave & 1, h = lane >> 5, col = lane & 31;
  // image address of (row, halfword column c): the 64-byte halves of a row are swapped where bit 1 of the row is set
  auto img = [](int row, int c) { return row * PITCH + (c ^ ((row & 2) << 4)); };
  // transposing read: this lane hands in four channels (4 (lane & 3) .. of the sixteen at 16 ((lane >> 4) & 1)) of row (lane & 15) >> 2
  const int tr_row = 8 * h + ((lane & 15) >> 2), tr_c = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  f32x16 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = (f32x16){0};
  const i32x4 bx = raw_rsrc(p.x, p.x_bytes), bd = raw_rsrc(p.dy, p.dy_bytes), bn = raw_rsrc(p.nbr, p.nbr_bytes);
  const unsigned ldx4 = 4u * (unsigned)p.ldx, ldy4 = 4u * (unsigned)p.ldy, K4 = 4u * (unsigned)p.K;
  const unsigned x_coff = 4u * (unsigned)(ci0 + 4 * c4), d_coff = 4u * (unsigned)(co0 + 4 * c4);
  float4 rx[8];
  auto gather = [&](int g) __attribute__((always_inline)) {  // x rows of the compacted pairs of offset g -> registers (-1: zeros)
#pragma unroll
    for (int i = 0; i < 8; ++i)
      rx[i] = __builtin_bit_cast(float4, raw_load_v4(bx, (int)(__umul24((unsigned)s_src[g * LL + rr + 16 * i], ldx4) + x_coff), 0, 0));
  };
  auto put = [&](unsigned short *im, int row, const float4 &v) __attribute__((always_inline)) {
    *reinterpret_cast<uint2 *>(im + img(row, 4 * c4)) = make_uint2(pack_bf16(v.x, v.y), pack_bf16(v.z, v.w));
  };
  auto stash = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 8; ++i) put(sX, rr + 16 * i, rx[i]);
  };
  for (int64_t r0 = rbeg; r0 < rend; r0 += WROWS) {
    __syncthreads();  // previous tile fully consumed
    int nb[G], rank[G];
    if (tid < WROWS) {
      const int64_t row = r0 + tid;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const bool ok = row < rend && g < ng;
        const int v = raw_load_i32(bn, (int)(ok ? (unsigned)row * K4 + 4u * (unsigned)(k0 + g) : 0x80000000u), 0, 0);
        nb[g] = ok ? v : -1;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t row = r0 + rr + 16 * i;
      const float4 v = __builtin_bit_cast(float4, raw_load_v4(bd, (int)((row < rend ? (unsigned)row * ldy4 : 0x80000000u) + d_coff), 0, 0));
      put(sD, rr + 16 * i, v);
    }
    if (tid < WROWS) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const unsigned long long mm = __ballot(nb[g] >= 0);
        rank[g] = wave_rank(mm);
        if (lane == 0) s_cnt[2 * g + wave] = __popcll(mm);
      }
    }
    __syncthreads();
    if (tid < WROWS) {
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (nb[g] >= 0) {
          const int pos = (wave == 1 ? s_cnt[2 * g] : 0) + rank[g];
          s_row[g * LL + pos] = tid, s_src[g * LL + pos] = nb[g];
        }
    } else {
#pragma unroll
      for (int g = 0; g < G; ++g) {  // tail pairs: dy row 0 times a zero x row
        const int m = s_cnt[2 * g] + s_cnt[2 * g + 1];
        const int t = tid - WROWS;
        if (t < ((m + 15) & ~15) - m) s_row[g * LL + m + t] = 0, s_src[g * LL + m + t] = -1;
      }
    }
    __syncthreads();
    gather(0);
    stash();
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (g < ng) {  // uniform
        if (g + 1 < ng) gather(g + 1);  // in flight during the MFMAs below
        const int m = s_cnt[2 * g] + s_cnt[2 * g + 1];
        const int nk16 = (m + 15) >> 4;  // sixteen pairs per MFMA
        for (int kk = 0; kk < nk16; ++kk) {
          const int pa = 16 * kk + tr_row;  // this lane's pair of the low half (high half: + 4)
          const int r_lo = s_row[g * LL + pa], r_hi = s_row[g * LL + pa + 4];
          const uint2 a_lo = lds_tr16(sX + img(pa, 32 * wm + tr_c)), a_hi = lds_tr16(sX + img(pa + 4, 32 * wm + tr_c));
          const uint2 b_lo = lds_tr16(sD + img(r_lo, 32 * wn + tr_c)), b_hi = lds_tr16(sD + img(r_hi, 32 * wn + tr_c));
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, make_uint4(a_lo.x, a_lo.y, a_hi.x, a_hi.y)),
                                                           __builtin_bit_cast(bf16x8, make_uint4(b_lo.x, b_lo.y, b_hi.x, b_hi.y)), acc[g], 0, 0, 0);
        }
        if (g + 1 < ng) {
          __syncthreads();  // everyone done reading sX
          stash();
          __syncthreads();
        }
      }
    }
  }
  // ---- epilogue: the partial slab (C/D layout of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 h)
  float *dst = p.out + (int64_t)wby * p.K * p.cin * p.cout;
  const int co = co0 + 32 * wn + col;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g < ng) {  // uniform
      const int k = k0 + g;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = ci0 + 32 * wm + (r & 3) + 8 * (r >> 2) + 4 * h;
        dst[((int64_t)k * p.cin + ci) * p.cout + co] = acc[g][r];
      }
    }
  }
}

template <int G>
static void launch_wgrad(const WgradParams &p, const WgradPlan &pl, hipStream_t st) {  // wgrad_kernel<G, NARROW, VEC, BUF> of the plan
  const bool narrow = pl.targ[1], vec = pl.targ[2], buf = pl.targ[3];
  if (narrow) {
    if (buf) wgrad_kernel<G, true, true, true><<<pl.grid, 256, 0, st>>>(p);
    else if (vec) wgrad_kernel<G, true, true><<<pl.grid, 256, 0, st>>>(p);
    else wgrad_kernel<G, true, false><<<pl.grid, 256, 0, st>>>(p);
  } else {
    if (buf) wgrad_kernel<G, false, true, true><<<pl.grid, 256, 0, st>>>(p);
    else if (vec) wgrad_kernel<G, false, true><<<pl.grid, 256, 0, st>>>(p);
    else wgrad_kernel<G, false, false><<<pl.grid, 256, 0, st>>>(p);
  }
}

}  // namespace mink

using namespace mink;

extern "C" {

static WgradCall wgrad_call(int64_t n_in, int32_t ldx, int32_t cin, int32_t ldy, int32_t cout, int64_t n_out, int32_t K) {
  WgradCall c = {};
  c.n_in = n_in, c.n_out = n_out, c.ldx = ldx, c.cin = cin, c.ldy = ldy, c.cout = cout, c.K = K;
  return c;
}

int64_t mink_conv_wgrad_workspace_bytes(int64_t n_out, int32_t K, int32_t cin, int32_t cout) {
  const WgradPlan pl = wgrad_plan(wgrad_call(0, cin, cin, cout, cout, n_out, K), g_conv);  // (the split needs only these four)
  return pl.nsplit > 1 ? (int64_t)pl.nsplit * K * cin * cout * 4 : 0;
}

struct WgradFuse {  // dy = input gradient of pool(relu(bn(y))): see mink_conv_wgrad_bn_relu_pool
  const float *dyp;
  const int32_t *in2out;
  int64_t n_pool;
  const float *mean, *invstd, *gamma, *beta, *dgamma, *dbeta;
  int b16;  // x and y are bf16 (x: [n_in][ldx] with ldx = 32; y: [n_out][cout]) -- bf16 storage of the full-resolution stage
};

static int wgrad_shape_check(const WgradCall &c) {
  MINK_REQUIRE(c.K >= 1 && c.K <= KMAX && c.cin >= 1 && c.cout >= 1 && c.ldx >= c.cin && c.ldy >= c.cout && c.n_out >= 0 && c.n_in >= 0,
               "wgrad: bad shape");
  return MINK_OK;
}

// Validate, plan (wgrad_plan), launch, reduce the row splits.
static int wgrad_impl(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *dy, int32_t ldy, int32_t cout,
                      const int32_t *nbr, int64_t n_out, int32_t K, float *dw, void *workspace, int64_t workspace_bytes,
                      const WgradFuse *fuse, void *stream) {
  WgradCall c = wgrad_call(n_in, ldx, cin, ldy, cout, n_out, K);
  c.fuse = !fuse ? 0 : fuse->b16 ? 2 : 1, c.n_pool = fuse ? fuse->n_pool : 0;
  c.aligned = (((uintptr_t)x | (uintptr_t)dy) & 15) == 0;
  if (const int rc = wgrad_shape_check(c)) return rc;
  MINK_REQUIRE(dw, "wgrad: NULL dw");
  hipStream_t st = (hipStream_t)stream;
  if (n_out == 0) {
    MINK_HIP(hipMemsetAsync(dw, 0, sizeof(float) * K * cin * cout, st));
    return MINK_OK;
  }
  MINK_REQUIRE(x && dy && nbr, "wgrad: NULL pointer");
  const WgradPlan pl = wgrad_plan(c, g_conv);
  MINK_REQUIRE(pl.nsplit == 1 || workspace, "wgrad: needs a workspace");
  // (the slab count comes from the plan, which tuning knobs can change between the caller's size query and this launch)
  MINK_REQUIRE(pl.nsplit == 1 || workspace_bytes >= (int64_t)pl.nsplit * K * cin * cout * 4,
               "wgrad: workspace of %lld bytes, %lld needed for the %d row splits of this plan", (long long)workspace_bytes,
               (long long)((int64_t)pl.nsplit * K * cin * cout * 4), pl.nsplit);
  if (const int rc = wgrad_plan_check(c, pl)) return rc;
  ScopedTimer timer(2, n_in, n_out, K, cin, cout, nbr, st);
  WgradParams p;
  p.x = x, p.dy = dy, p.nbr = nbr, p.out = pl.nsplit > 1 ? (float *)workspace : dw;
  p.n_out = n_out, p.rows_per_split = pl.rows_per_split, p.ldx = ldx, p.cin = cin, p.ldy = ldy, p.cout = cout, p.K = K;
  p.ct_tiles = pl.ct_tiles;
  p.ngroups = pl.ngroups;
  p.ablate = g_conv.stagger | (g_conv.wgrad_xcd ? 0 : 4096);
  p.x_bytes = pl.x_bytes, p.dy_bytes = pl.dy_bytes, p.nbr_bytes = pl.nbr_bytes;
  p.buf_ok = pl.buf_ok;
  if (fuse) {
    p.dyp = fuse->dyp, p.in2out = fuse->in2out, p.mean = fuse->mean, p.invstd = fuse->invstd, p.gamma = fuse->gamma;
    p.beta = fuse->beta, p.dgamma = fuse->dgamma, p.dbeta = fuse->dbeta, p.inv_n = 1.f / (float)n_out;
    p.dyp_bytes = (unsigned)(4 * fuse->n_pool * ldy), p.i2o_bytes = (unsigned)(4 * n_out);
  }
  const bool t0 = pl.targ[0], t1 = pl.targ[1], t2 = pl.targ[2];
  switch (pl.family) {
    case MINK_KERNEL_WGRAD_STREAM_B16T: wgrad_stream_b16t_kernel<<<pl.grid, 256, 0, st>>>(p); break;
    case MINK_KERNEL_WGRAD_STREAM_BF16:  // <FUSE, B16>
      if (t1) wgrad_stream_bf16_kernel<true, true><<<pl.grid, 256, 0, st>>>(p);
      else if (t0) wgrad_stream_bf16_kernel<true><<<pl.grid, 256, 0, st>>>(p);
      else wgrad_stream_bf16_kernel<false><<<pl.grid, 256, 0, st>>>(p);
      break;
    case MINK_KERNEL_WGRAD_STREAM:  // <4, FUSE, FLAT>
      if (t1 && t2) wgrad_stream_kernel<4, true, true><<<pl.grid, 256, 0, st>>>(p);
      else if (t1) wgrad_stream_kernel<4, true><<<pl.grid, 256, 0, st>>>(p);
      else if (t2) wgrad_stream_kernel<4, false, true><<<pl.grid, 256, 0, st>>>(p);
      else wgrad_stream_kernel<4><<<pl.grid, 256, 0, st>>>(p);
      break;
    case MINK_KERNEL_WGRAD16:
      if (pl.targ[0] == 3) wgrad16_kernel<3><<<pl.grid, 256, 0, st>>>(p);
      else wgrad16_kernel<1><<<pl.grid, 256, 0, st>>>(p);
      break;
    default:
      if (pl.G == 9) launch_wgrad<9>(p, pl, st);
      else if (pl.G == 3) launch_wgrad<3>(p, pl, st);
      else launch_wgrad<1>(p, pl, st);
  }
  MINK_CHECK_LAUNCH();
  if (pl.nsplit > 1) {
    const int64_t count = (int64_t)K * cin * cout;
    slab_reduce_kernel<<<dim3((unsigned)cdiv(count, 64)), 256, 0, st>>>((const float *)workspace, count, pl.nsplit, dw);
    MINK_CHECK_LAUNCH();
  }
  return MINK_OK;
}

int mink_conv_wgrad(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *dy, int32_t ldy, int32_t cout,
                    const int32_t *nbr, int64_t n_out, int32_t K, float *dw, void *workspace, int64_t workspace_bytes,
                    void *stream) {
  return wgrad_impl(x, n_in, ldx, cin, dy, ldy, cout, nbr, n_out, K, dw, workspace, workspace_bytes, nullptr, stream);
}

int mink_conv_wgrad_bn_relu_pool_supported(int64_t n_in, int32_t ldx, int32_t cin, int64_t n_out, int32_t K, int32_t cout) {
  if (n_out <= 0) return 0;
  return wgrad_plan(wgrad_call(n_in, ldx, cin, cout, cout, n_out, K), g_conv).streaming;
}

int mink_conv_wgrad_launch_info(int64_t n_in, int32_t ldx, int32_t cin, int32_t ldy, int32_t cout, int64_t n_out, int32_t K,
                                int32_t fuse, int64_t n_pool, int32_t aligned, MinkConvLaunchInfo *info) {
  MINK_REQUIRE(info, "wgrad_launch_info: NULL info");
  *info = MinkConvLaunchInfo{};
  MINK_REQUIRE(fuse >= 0 && fuse <= 2, "wgrad_launch_info: fuse %d", fuse);
  WgradCall c = wgrad_call(n_in, ldx, cin, ldy, cout, n_out, K);
  c.fuse = fuse, c.n_pool = n_pool, c.aligned = aligned != 0;
  if (const int rc = wgrad_shape_check(c)) return rc;
  if (n_out == 0) return MINK_OK;  // (a memset, no kernel: the info stays zero)
  const WgradPlan pl = wgrad_plan(c, g_conv);
  if (const int rc = wgrad_plan_check(c, pl)) return rc;
  *info = launch_info(pl.family, pl.targ, 4, pl.grid, 0, pl.nsplit, pl.nsplit > 1 ? MINK_EPILOGUE_SLAB_REDUCE : MINK_EPILOGUE_NONE);
  return MINK_OK;
}

int mink_conv_wgrad_bn_relu_pool(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *y, int32_t cout,
                                 const float *dy_pool, int64_t n_pool, const int32_t *in2out, const float *mean,
                                 const float *invstd, const float *gamma, const float *beta, const float *dgamma,
                                 const float *dbeta, const int32_t *nbr, int64_t n_out, int32_t K, float *dw,
                                 void *workspace, int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(y && dy_pool && in2out && mean && invstd && gamma && beta && dgamma && dbeta && n_pool >= 1,
               "wgrad_bn_relu_pool: NULL pointer");
  const WgradFuse f = {dy_pool, in2out, n_pool, mean, invstd, gamma, beta, dgamma, dbeta, 0};
  return wgrad_impl(x, n_in, ldx, cin, y, cout, cout, nbr, n_out, K, dw, workspace, workspace_bytes, &f, stream);
}

int mink_conv_wgrad_bn_relu_pool_b16(const void *xb, int64_t n_in, int32_t cin, const void *yb, int32_t cout, const float *dy_pool,
                                     int64_t n_pool, const int32_t *in2out, const float *mean, const float *invstd,
                                     const float *gamma, const float *beta, const float *dgamma, const float *dbeta,
                                     const int32_t *nbr, int64_t n_out, int32_t K, float *dw, void *workspace,
                                     int64_t workspace_bytes, void *stream) {
  MINK_REQUIRE(xb && yb && dy_pool && in2out && mean && invstd && gamma && beta && dgamma && dbeta && n_pool >= 1 && cin >= 1 && cin <= 32,
               "wgrad_bn_relu_pool_b16: bad arguments");
  const WgradFuse f = {dy_pool, in2out, n_pool, mean, invstd, gamma, beta, dgamma, dbeta, 1};
  return wgrad_impl((const float *)xb, n_in, 32, cin, (const float *)yb, cout, cout, nbr, n_out, K, dw, workspace, workspace_bytes, &f,
                    stream);
}

}  // extern "C"
