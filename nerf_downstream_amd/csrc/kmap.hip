// Neighbour tables (kernel maps) on gfx950: the per-voxel hash look-up, the 4x4x4 block index over a map's rows and the
// tables read through it, and the batched 0xFF fills they start from.  The two hash inserts sit side by side here: the
// per-voxel one (first pass of unique in coords.hip, reached through launch_insert) and the block one.  The rest of a map's
// build is in coords.hip; the rulebook and the parity classes derived from a table are in rulebook.hip.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "coords_common.h"

namespace mink {

// Timing diagnostic (MINK_DIAG_DUP, bit mask): launch an idempotent map kernel a second time -- what the step pays for one
// more of it is what it pays for the first.  1 = 3x3x3 tables, 2 = block insert, 4 = leader pass 2, 8 = level insert,
// 16 = leader pass 1, 32 = block fill, 64 = 0xFF fills.
static int diag_dup() {
  static const int v = [] {
    const char *e = getenv("MINK_DIAG_DUP");
    return e ? atoi(e) : 0;
  }();
  return v;
}

// ---------------------------------------------------------------------- hash inserts
// Runs of equal keys in ADJACENT lanes insert once.  Device-scope atomics are what a map build costs the convolutions it runs
// beside (a second launch of a hash insert adds 0.13-0.22 ms to a step, a second launch of the 3x3x3 tables nothing:
// DESIGN.md Appendix A), and rows arrive in scan order: the cells of a 4^3 block, and the children of a coarser cell, sit
// next to each other.  `head_mask` = ballot of the lanes that start a run; a lane's run starts at the highest head at or below it.
__device__ __forceinline__ uint64_t shfl_up1_u64(uint64_t v) {
  const unsigned lo = __shfl_up((unsigned)v, 1), hi = __shfl_up((unsigned)(v >> 32), 1);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ int run_head_lane(unsigned long long head_mask, int lane) {
  return 63 - __builtin_clzll(head_mask & ((2ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBlock) void insert_kernel(const uint64_t *__restrict__ keys, int64_t n_host,
                                                        const int *__restrict__ n_dev, unsigned long long *tkeys,
                                                        int *tvals, uint64_t mask, int *__restrict__ slot_of_row,
                                                        const uint32_t *__restrict__ asc_status) {
  if (asc_fast(asc_status)) return;  // (ascending level 0: nothing to look up, the map stays empty)
  const int64_t n = n_dev ? (int64_t)*n_dev : n_host;
  if (n_dev) mask = table_capacity(n) - 1;  // chained level: the map is sized for the rows that arrive
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if ((int64_t)blockIdx.x * kBlock >= n) return;  // (whole workgroups: every lane of a live wave reaches the shuffles)
  const bool live = i < n;
  const int lane = threadIdx.x & 63;
  const uint64_t key = live ? keys[i] : kEmptyKey;  // (no packed key is all ones: an idle lane never joins a run)
  const uint64_t before = shfl_up1_u64(key);
  const bool head = live && (lane == 0 || before != key);
  const unsigned long long head_mask = __ballot(head);
  int s32 = 0;
  if (head) {
    uint64_t s = mix64(key) & mask;
    for (;;) {
      const unsigned long long prev = atomicCAS(&tkeys[s], (unsigned long long)kEmptyKey, (unsigned long long)key);
      if (prev == kEmptyKey || prev == key) break;
      s = (s + 1) & mask;
    }
    atomicMin(&tvals[s], (int)i);  // first occurrence wins (the head is the lowest row of its run)
    s32 = (int)s;
  }
  s32 = __shfl(s32, live ? run_head_lane(head_mask, lane) : lane);
  if (live) slot_of_row[i] = s32;
}
int launch_insert(const uint64_t *keys, int64_t n, const int *n_dev, uint64_t *table_keys, int32_t *table_vals, int64_t cap,
                  int *slot_of_row, const uint32_t *asc_status, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(n > 0 ? n : 1, kBlock));
  for (int rep = 0; rep < 1 + ((diag_dup() & 8) != 0); ++rep)
    insert_kernel<<<grid, kBlock, 0, st>>>(keys, n, n_dev, (unsigned long long *)table_keys, table_vals,
                                           (uint64_t)cap - 1, slot_of_row, asc_status);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

// ------------------------------------------------------------------------ kernel map
struct Offsets {
  int d[27 * 3];
};

__global__ __launch_bounds__(kBlock) void kernel_map_kernel(const uint64_t *__restrict__ tkeys,
                                                            const int *__restrict__ tvals, uint64_t mask,
                                                            const int *__restrict__ out_coords, int64_t n_out, int K,
                                                            Offsets off, int *__restrict__ nbr, int *nbr_t) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n_out * K) return;
  const int64_t o = idx / K;
  const int k = (int)(idx - o * K);
  const int4 c = reinterpret_cast<const int4 *>(out_coords)[o];
  uint64_t key;
  int v = -1;
  if (pack_key(c.x, c.y + off.d[3 * k], c.z + off.d[3 * k + 1], c.w + off.d[3 * k + 2], key))
    v = table_find(tkeys, tvals, mask, key);
  nbr[idx] = v;
  if (nbr_t && v >= 0) nbr_t[(int64_t)v * K + k] = (int)o;
}

// ------------------------------------------------------------------------ block index
// Block key of a coordinate at tensor stride ts: cell = coordinate / ts (exact for map rows, floor for safety),
// block = cell >> 2 per axis (on the biased 16-bit value, so negative coordinates floor correctly), packed like a
// voxel key; `local` = position of the cell inside its 4x4x4 block (x fastest).
__device__ __forceinline__ bool block_key(int b, int x, int y, int z, int ts, uint64_t &key, int &local) {
  if (ts > 1) x = floor_to(x, ts) / ts, y = floor_to(y, ts) / ts, z = floor_to(z, ts) / ts;
  const unsigned ux = (unsigned)(x + 32768), uy = (unsigned)(y + 32768), uz = (unsigned)(z + 32768);
  const bool ok = ((unsigned)b <= 65534u) && ux <= 65535u && uy <= 65535u && uz <= 65535u;
  key = ((uint64_t)(unsigned)b << 48) | ((uint64_t)(ux >> 2) << 32) | ((uint64_t)(uy >> 2) << 16) | (uint64_t)(uz >> 2);
  local = (int)((ux & 3u) | ((uy & 3u) << 2) | ((uz & 3u) << 4));
  return ok;
}

// 32-bit multiplicative hash of a block key: the look-up kernels are instruction-bound (splitmix64 alone is ~30 VALU
// instructions in 32-bit hardware), and a block table holds few, well-spread keys
__device__ __forceinline__ uint64_t blk_hash(uint64_t key) {
  unsigned h = (unsigned)key * 0x9E3779B1u ^ (unsigned)(key >> 32) * 0x85EBCA77u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 13;
  return h;
}

// (A table given too few slots for the blocks -- blk_cap is the caller's promise -- must not hang the card: probing stops after
//  one trip round the table, the row is left out (slot -1: the later passes skip it) and *overflow is cleared from its 0xFF fill.)
__device__ __forceinline__ void blk_insert_body(const int *__restrict__ coords, int64_t n, int ts, unsigned long long *table,
                                                uint64_t mask, int *__restrict__ slot_of_row, int *overflow, int *sticky) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;  // (callers drop whole idle workgroups; every lane of a live wave reaches the shuffles)
  const int lane = threadIdx.x & 63;
  const int4 c = reinterpret_cast<const int4 *>(coords)[live ? i : n - 1];
  uint64_t key;
  int local;
  block_key(c.x, c.y, c.z, c.w, ts, key, local);  // rows of a map are always in range
  if (!live) key = kEmptyKey;
  // adjacent lanes in the same block (scan order: the z run of a block, ~4 rows) insert once, with the OR of their cells
  const uint64_t before = shfl_up1_u64(key);
  const bool head = live && (lane == 0 || before != key);
  const unsigned long long head_mask = __ballot(head);
  int s32 = 0;
  {
    // run length of a head = distance to the next head (or to the end of the wave); idle lanes are heads of nothing
    const unsigned long long later = (head_mask | ~__ballot(live)) >> lane >> 1;
    const int len = head ? (later ? __builtin_ctzll(later) + 1 : 64 - lane) : 0;
    unsigned long long bits = 1ull << local;
    int maxlen = len;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, d));
    for (int j = 1; j < maxlen; ++j) {
      const int l2 = __shfl(local, min(lane + j, 63));
      if (j < len) bits |= 1ull << l2;
    }
    if (head) {
      uint64_t s = blk_hash(key) & mask;
      bool placed = false;
      for (uint64_t probes = 0; probes <= mask; ++probes) {
        const unsigned long long prev = atomicCAS(&table[2 * s], (unsigned long long)kEmptyKey, (unsigned long long)key);
        if (prev == kEmptyKey || prev == key) {
          placed = true;
          break;
        }
        s = (s + 1) & mask;
      }
      if (placed) {
        atomicAnd(&table[2 * s + 1], ~bits);  // the mask is kept inverted: the 0xFF fill of the table means "empty"
        s32 = (int)s;
      } else {
        *overflow = 0;
        if (sticky) *sticky = 1;  // (mink_set_overflow_sink: a host-visible word nobody refills -- the caller's next batch sees it)
        s32 = -1;
      }
    }
  }
  s32 = __shfl(s32, live ? run_head_lane(head_mask, lane) : lane);
  if (live) slot_of_row[i] = s32;
}

// One row per block (the one in its lowest occupied cell, the "leader") owns the block's run of `rowids`.  Runs are
// laid out in row order of the leaders: pass 1 counts the cells led by each workgroup, pass 2 sums the counts before
// its own workgroup and hands every leader its start.  No atomics (a single counter word takes ~90 adds per
// microsecond: 70 k leaders on it serialise for longer than the rest of the build), deterministic layout.
template <bool ASSIGN>
__device__ __forceinline__ void blk_leader_body(const int *__restrict__ coords, int64_t n, int ts,
                                                const unsigned long long *__restrict__ table,
                                                const int *__restrict__ slot_of_row, int *__restrict__ base,
                                                int *__restrict__ wg_counts) {
  __shared__ int s_wave[kBlock / 64];
  const int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i0 < n;
  const int64_t i = live ? i0 : n - 1;  // (idle lanes shadow the last row and never lead: whole waves reach the shuffles)
  const int4 c = reinterpret_cast<const int4 *>(coords)[i];
  uint64_t key;
  int local;
  block_key(c.x, c.y, c.z, c.w, ts, key, local);
  const int s = slot_of_row[i];
  if (!live || s < 0) local = -1;
  const unsigned long long m = s < 0 ? 0ull : ~table[2 * (int64_t)s + 1];
  const bool leader = m && local == __builtin_ctzll(m);
  const int cnt = leader ? __popcll(m) : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  if (!ASSIGN) {
    if (threadIdx.x == 0) wg_counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    return;
  }
  // this workgroup's offset = sum of the counts of the workgroups before it (a few thousand ints from L2: cheaper than
  // a scan launch between the two passes, and nothing here can be held up by a single-workgroup kernel)
  __shared__ int s_part[kBlock / 64];
  int part = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += kBlock) part += wg_counts[i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
  if (lane == 0) s_part[wave] = part;
  __syncthreads();
  int before = s_part[0] + s_part[1] + s_part[2] + s_part[3];
  for (int w = 0; w < wave; ++w) before += s_wave[w];
  if (leader) base[s] = before + incl - cnt;
}

__device__ __forceinline__ void blk_fill_body(const int *__restrict__ coords, int64_t n, int ts,
                                              const unsigned long long *__restrict__ table, const int *__restrict__ slot_of_row,
                                              const int *__restrict__ base, int *__restrict__ rowids) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int4 c = reinterpret_cast<const int4 *>(coords)[i];
  uint64_t key;
  int local;
  block_key(c.x, c.y, c.z, c.w, ts, key, local);
  const int s = slot_of_row[i];
  if (s < 0) return;  // (a row that found no slot: blk_insert_body)
  const unsigned long long m = ~table[2 * (int64_t)s + 1];
  rowids[base[s] + __popcll(m & ((1ull << local) - 1ull))] = (int)i;
}

// The block indices of ALL input maps of a batch's plan are built by four launches, not four per map (blockIdx.y = map):
// the builds are independent of each other, and a prepared batch has six of them.
static int *g_overflow_sink = nullptr;  // mink_set_overflow_sink
constexpr int kMaxBatch = 8;
struct BlkBuild {
  const int *coords;
  int64_t n;
  unsigned long long *table;
  uint64_t mask;
  int *slot, *base, *rowids, *overflow;
  int ts;
};
struct BlkBuildBatch {
  BlkBuild e[kMaxBatch];
  int *sticky;  // process-wide overflow sink (device-visible host word), or nullptr
};
__global__ __launch_bounds__(kBlock) void blk_insert_kernel(BlkBuildBatch b) {
  const BlkBuild &e = b.e[blockIdx.y];
  if ((int64_t)blockIdx.x * kBlock >= e.n) return;
  blk_insert_body(e.coords, e.n, e.ts, e.table, e.mask, e.slot, e.overflow, b.sticky);
}
template <bool ASSIGN>
__global__ __launch_bounds__(kBlock) void blk_leader_kernel(BlkBuildBatch b) {
  const BlkBuild &e = b.e[blockIdx.y];
  if ((int64_t)blockIdx.x * kBlock >= e.n) return;  // (whole workgroups: the barriers below are reached by all or none)
  blk_leader_body<ASSIGN>(e.coords, e.n, e.ts, e.table, e.slot, e.base, e.rowids);  // (workgroup counts live in the head of rowids)
}
__global__ __launch_bounds__(kBlock) void blk_fill_kernel(BlkBuildBatch b) {
  const BlkBuild &e = b.e[blockIdx.y];
  if ((int64_t)blockIdx.x * kBlock >= e.n) return;
  blk_fill_body(e.coords, e.n, e.ts, e.table, e.slot, e.base, e.rowids);
}
// 0xFF fill of up to sixteen int32 buffers in one launch (blockIdx.y = buffer): 16-byte stores over the aligned body, single
// words before and behind it (a hipMemsetAsync per buffer is one launch each, two when the size is not a multiple of 16)
__global__ __launch_bounds__(kBlock) void fill_ff_kernel(FillBatch f) {
  unsigned *p = f.ptr[blockIdx.y];
  const int64_t n = f.nwords[blockIdx.y];
  const int64_t head = min(n, (int64_t)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2));
  const int64_t n16 = (n - head) >> 2, tail0 = head + 4 * n16;
  uint4 *body = reinterpret_cast<uint4 *>(p + head);
  const uint4 v = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n16; i += (int64_t)gridDim.x * kBlock) body[i] = v;
  if (blockIdx.x == 0) {
    if ((int64_t)threadIdx.x < head) p[threadIdx.x] = 0xFFFFFFFFu;
    if (tail0 + (int64_t)threadIdx.x < n) p[tail0 + threadIdx.x] = 0xFFFFFFFFu;
  }
}
int FillQueue::flush() {
  if (n == 0) return MINK_OK;
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(cdiv(max16, kBlock), 2048));
  for (int rep = 0; rep < 1 + dup; ++rep) fill_ff_kernel<<<dim3((unsigned)blocks, (unsigned)n), kBlock, 0, st>>>(b);
  MINK_CHECK_LAUNCH();
  n = 0, max16 = 0;
  return MINK_OK;
}
int FillQueue::add(void *ptr, int64_t bytes) {
  if (bytes <= 0) return MINK_OK;
  if (((uintptr_t)ptr & 3) || (bytes & 3)) {  // (not a run of 32-bit words: the runtime's fill)
    MINK_HIP(hipMemsetAsync(ptr, 0xFF, (size_t)bytes, st));
    return MINK_OK;
  }
  b.ptr[n] = (unsigned *)ptr, b.nwords[n] = bytes >> 2;
  max16 = std::max(max16, bytes >> 4);
  if (++n == 16) return flush();
  return MINK_OK;
}

// Same result as kernel_map_kernel, through the block index.  Thread per (output row, offset): the 27 look-ups of a
// row sit in adjacent lanes and hit the same one to eight block entries.
template <class OFF>
__device__ __forceinline__ void kernel_map_blk_body(const unsigned long long *__restrict__ table, const int *__restrict__ base,
                                                    const int *__restrict__ rowids, uint64_t mask, int ts,
                                                    const int *__restrict__ out_coords, int64_t n_out, int K, const OFF &off,
                                                    int *__restrict__ nbr, int *nbr_t) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n_out * K) return;
  const int64_t o = idx / K;
  const int k = (int)(idx - o * K);
  const int4 c = reinterpret_cast<const int4 *>(out_coords)[o];
  uint64_t key;
  int local, v = -1;
  if (block_key(c.x, c.y + off.d[3 * k], c.z + off.d[3 * k + 1], c.w + off.d[3 * k + 2], ts, key, local)) {
    uint64_t s = blk_hash(key) & mask;
    for (uint64_t probes = 0; probes <= mask; ++probes) {  // (bounded: a table without a free slot must not hang the look-up)
      const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(table)[s];
      if (e.x == key) {
        const unsigned long long m = ~e.y;
        if ((m >> local) & 1ull) v = rowids[base[s] + __popcll(m & ((1ull << local) - 1ull))];
        break;
      }
      if (e.x == kEmptyKey) break;
      s = (s + 1) & mask;
    }
  }
  nbr[idx] = v;
  if (nbr_t && v >= 0) nbr_t[(int64_t)v * K + k] = (int)o;
}

// The 3^3 neighbourhood of one output row per THREAD (unit offsets in input cells: every 3x3x3 convolution of the
// network, strided or not).  The 27 cells lie in at most 2x2x2 blocks -- A = block of (cell - 1), B = block of
// (cell + 1) per axis -- so the thread probes eight block entries and answers all 27 look-ups from their masks with
// bit tests and popcounts: ~20 instructions per neighbour instead of ~300 for one probe chain each.  Results are
// staged in LDS and written as one contiguous run per workgroup.
struct __attribute__((packed, aligned(4))) Row27 {
  int v[27];
};
template <bool HAS_T>
__device__ __forceinline__ void kernel_map_blk27_body(const unsigned long long *__restrict__ table, const int *__restrict__ base,
                                                      const int *__restrict__ rowids, uint64_t mask, int ts,
                                                      const int *__restrict__ out_coords, int64_t n_out, int *__restrict__ nbr,
                                                      int *nbr_t) {
  const int64_t o0 = (int64_t)blockIdx.x * kBlock;
  const int64_t o = o0 + threadIdx.x;
  const bool live = o < n_out;
  const int4 c = reinterpret_cast<const int4 *>(out_coords)[live ? o : n_out - 1];
  int cx = c.y, cy = c.z, cz = c.w;
  if (ts > 1) cx = floor_to(cx, ts) / ts, cy = floor_to(cy, ts) / ts, cz = floor_to(cz, ts) / ts;
  const int u[3] = {cx + 32768, cy + 32768, cz + 32768};  // 0..65535 for rows of a map; neighbours may step outside
  const bool b_ok = (unsigned)c.x <= 65534u;
  // block entries: index = ix + 2 iy + 4 iz, i = 0 -> block of (u - 1), 1 -> block of (u + 1)
  unsigned long long M[8];
  int B[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int nx = u[0] + ((q & 1) ? 1 : -1), ny = u[1] + ((q & 2) ? 1 : -1), nz = u[2] + ((q & 4) ? 1 : -1);
    M[q] = 0ull, B[q] = 0;
    if (b_ok && (unsigned)nx <= 65535u && (unsigned)ny <= 65535u && (unsigned)nz <= 65535u) {
      const uint64_t key = ((uint64_t)(unsigned)c.x << 48) | ((uint64_t)((unsigned)nx >> 2) << 32) |
                           ((uint64_t)((unsigned)ny >> 2) << 16) | (uint64_t)((unsigned)nz >> 2);
      uint64_t s = blk_hash(key) & mask;
      for (uint64_t probes = 0; probes <= mask; ++probes) {
        const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(table)[s];
        if (e.x == key) {
          M[q] = ~e.y, B[q] = base[s];
          break;
        }
        if (e.x == kEmptyKey) break;
        s = (s + 1) & mask;
      }
    }
  }
  // the centre cell of an axis shares block A unless it sits on the low face of its block (then it is in B)
  const bool cB[3] = {(u[0] & 3) == 0, (u[1] & 3) == 0, (u[2] & 3) == 0};
  int out[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    const int d[3] = {k % 3 - 1, (k / 3) % 3 - 1, k / 9 - 1};
    // select the block entry: per axis bit = 1 (B) for d = +1, 0 (A) for d = -1, cB for d = 0
    unsigned long long m;
    int bs;
    {
      unsigned long long mx[4];
      int bx[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // x axis resolved: entries over (iy, iz)
        const bool sel = d[0] > 0 || (d[0] == 0 && cB[0]);
        mx[j] = sel ? M[2 * j + 1] : M[2 * j];
        bx[j] = sel ? B[2 * j + 1] : B[2 * j];
      }
      const bool sy = d[1] > 0 || (d[1] == 0 && cB[1]);
      const unsigned long long my0 = sy ? mx[1] : mx[0], my1 = sy ? mx[3] : mx[2];
      const int by0 = sy ? bx[1] : bx[0], by1 = sy ? bx[3] : bx[2];
      const bool sz = d[2] > 0 || (d[2] == 0 && cB[2]);
      m = sz ? my1 : my0;
      bs = sz ? by1 : by0;
    }
    const int local = ((u[0] + d[0]) & 3) | (((u[1] + d[1]) & 3) << 2) | (((u[2] + d[2]) & 3) << 4);
    int v = -1;
    if ((m >> local) & 1ull) v = rowids[bs + __popcll(m & ((1ull << local) - 1ull))];
    out[k] = v;
    if (HAS_T && live && v >= 0) nbr_t[(int64_t)v * 27 + k] = (int)o;
  }
  // the row's 27 entries (108 contiguous bytes, 4-byte aligned) leave as six 16-byte stores and one of 12: no LDS staging --
  // the 27.6 KB per workgroup it took kept up to 138 KB of a CU's LDS away from the convolution kernels this one runs beside
  if (live) {
    Row27 *dst = reinterpret_cast<Row27 *>(nbr + o * 27);
    Row27 r;
#pragma unroll
    for (int k = 0; k < 27; ++k) r.v[k] = out[k];
    *dst = r;
  }
}

__global__ __launch_bounds__(kBlock) void kernel_map_blk_kernel(const unsigned long long *__restrict__ table,
                                                                const int *__restrict__ base,
                                                                const int *__restrict__ rowids, uint64_t mask, int ts,
                                                                const int *__restrict__ out_coords, int64_t n_out, int K,
                                                                Offsets off, int *__restrict__ nbr, int *nbr_t) {
  kernel_map_blk_body(table, base, rowids, mask, ts, out_coords, n_out, K, off, nbr, nbr_t);
}
struct SmallOffsets {  // up to eight offsets (pooling 2^3, 1x1x1)
  int d[24];
};
struct KMapS {
  const unsigned long long *table;
  const int *base, *rowids, *out_coords;
  uint64_t mask;
  int64_t n_out;
  int *nbr, *nbr_t;
  int ts, K;
  SmallOffsets off;
};
struct KMapSBatch {
  KMapS e[kMaxBatch];
};
__global__ __launch_bounds__(kBlock) void kernel_map_blk_small_kernel(KMapSBatch b) {  // blockIdx.y = table
  const KMapS &e = b.e[blockIdx.y];
  if ((int64_t)blockIdx.x * kBlock >= e.n_out * e.K) return;
  kernel_map_blk_body(e.table, e.base, e.rowids, e.mask, e.ts, e.out_coords, e.n_out, e.K, e.off, e.nbr, e.nbr_t);
}
struct KMap27 {
  const unsigned long long *table;
  const int *base, *rowids, *out_coords;
  uint64_t mask;
  int64_t n_out;
  int *nbr, *nbr_t;
  int ts;
};
struct KMap27Batch {
  KMap27 e[kMaxBatch];
};
template <class Q>  // the fields KMap27 and KMapS share
static void kmap_desc(Q &q, const MinkKernelMapDesc &e) {
  q.table = (const unsigned long long *)e.blk_table, q.base = e.blk_base, q.rowids = e.blk_rowids, q.out_coords = e.out_coords;
  q.mask = (uint64_t)e.blk_cap - 1, q.n_out = e.n_out, q.nbr = e.nbr, q.nbr_t = e.nbr_t, q.ts = e.in_ts;
}
template <bool HAS_T>
__global__ __launch_bounds__(kBlock) void kernel_map_blk27_kernel(KMap27Batch b) {  // blockIdx.y = table
  const KMap27 &e = b.e[blockIdx.y];
  if ((int64_t)blockIdx.x * kBlock >= e.n_out) return;
  kernel_map_blk27_body<HAS_T>(e.table, e.base, e.rowids, e.mask, e.ts, e.out_coords, e.n_out, e.nbr, e.nbr_t);
}

}  // namespace mink

using namespace mink;

extern "C" {

int mink_kernel_map(const uint64_t *in_table_keys, const int32_t *in_table_vals, int64_t in_cap,
                    const int32_t *out_coords, int64_t n_out, const int32_t *offsets_host, int32_t K, int32_t *nbr,
                    int32_t *nbr_t, void *stream) {
  MINK_REQUIRE(K >= 1 && K <= 27 && offsets_host, "kernel_map: kernel volume %d unsupported (1..27)", K);
  MINK_REQUIRE(in_cap >= 64 && (in_cap & (in_cap - 1)) == 0, "kernel_map: bad table capacity");
  MINK_REQUIRE(n_out >= 0 && n_out * K < (1ll << 31), "kernel_map: n_out*K overflows int32 indexing");
  if (n_out == 0) return MINK_OK;
  MINK_REQUIRE(in_table_keys && in_table_vals && out_coords && nbr, "kernel_map: NULL pointer");
  MINK_REQUIRE(((uintptr_t)out_coords & 15) == 0, "kernel_map: out_coords misaligned");
  Offsets off;
  memset(&off, 0, sizeof off);
  memcpy(off.d, offsets_host, sizeof(int) * 3 * K);
  kernel_map_kernel<<<dim3((unsigned)cdiv(n_out * K, kBlock)), kBlock, 0, (hipStream_t)stream>>>(
      in_table_keys, in_table_vals, (uint64_t)in_cap - 1, out_coords, n_out, K, off, nbr, nbr_t);
  MINK_CHECK_LAUNCH();
  return MINK_OK;
}

int mink_set_overflow_sink(int32_t *host_word) {
  if (!host_word) {
    g_overflow_sink = nullptr;
    return MINK_OK;
  }
  void *dp = nullptr;
  MINK_REQUIRE(hipHostGetDevicePointer(&dp, host_word, 0) == hipSuccess && dp,
               "set_overflow_sink: the word must live in pinned (device-mapped) host memory");
  g_overflow_sink = (int *)dp;
  return MINK_OK;
}

int mink_kernel_map_batch(int32_t n, const MinkKernelMapDesc *d, void *stream) {
  MINK_REQUIRE(n >= 0 && (n == 0 || d), "kernel_map_batch: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  // One batch's plan is ~6 block indices and ~14 tables over independent maps: the 0xFF fills, the four passes of the
  // index builds and the table kernels are each issued as ONE launch over all of them (blockIdx.y = map), in that order.
  // ---- pass 0: validation, fills
  FillQueue fills{st, (diag_dup() & 64) != 0};
  for (int i = 0; i < n; ++i) {
    const MinkKernelMapDesc &e = d[i];
    if (e.nbr_t && e.n_in > 0)
      if (int rc = fills.add(e.nbr_t, (int64_t)sizeof(int32_t) * e.n_in * e.K)) return rc;
    if (!e.blk_table) continue;
    MINK_REQUIRE(e.K >= 1 && e.K <= 27 && e.n_out >= 0 && e.n_in >= 0 && e.n_out * e.K < (1ll << 31) && e.in_ts >= 1,
                 "kernel_map_batch: bad shape in descriptor %d", i);
    MINK_REQUIRE(e.blk_cap >= 64 && (e.blk_cap & (e.blk_cap - 1)) == 0 && e.blk_base && e.blk_slot &&
                     e.blk_rowids && e.blk_counter && e.in_coords && ((uintptr_t)e.blk_table & 15) == 0,
                 "kernel_map_batch: bad block-index buffers in descriptor %d", i);
    MINK_REQUIRE(e.n_out == 0 || (e.out_coords && e.nbr && ((uintptr_t)e.out_coords & 15) == 0), "kernel_map_batch: NULL/misaligned pointer");
    if (e.blk_build) {
      int rc = fills.add(e.blk_table, (int64_t)sizeof(uint64_t) * 2 * e.blk_cap);
      if (!rc) rc = fills.add(e.blk_counter, sizeof(int32_t));  // (0xFFFFFFFF = every block found a slot)
      if (rc) return rc;
    }
  }
  if (int rc = fills.flush()) return rc;
  // ---- pass 1: block indices (insert, two leader passes, fill)
  for (int i0 = 0; i0 < n;) {
    BlkBuildBatch bb;
    bb.sticky = g_overflow_sink;
    int nb = 0;
    int64_t nmax = 0;
    int i = i0;
    for (; i < n && nb < kMaxBatch; ++i) {
      const MinkKernelMapDesc &e = d[i];
      if (!e.blk_table || !e.blk_build || e.n_in <= 0) continue;
      BlkBuild &q = bb.e[nb++];
      q.coords = e.in_coords, q.n = e.n_in, q.table = (unsigned long long *)e.blk_table, q.mask = (uint64_t)e.blk_cap - 1;
      q.slot = e.blk_slot, q.base = e.blk_base, q.rowids = e.blk_rowids, q.ts = e.in_ts, q.overflow = e.blk_counter;
      nmax = std::max(nmax, e.n_in);
    }
    i0 = i;
    if (nb == 0) continue;
    const dim3 g((unsigned)cdiv(nmax, kBlock), (unsigned)nb);
    const int dup = diag_dup();
    for (int rep = 0; rep < 1 + ((dup & 2) != 0); ++rep) blk_insert_kernel<<<g, kBlock, 0, st>>>(bb);
    MINK_CHECK_LAUNCH();
    for (int rep = 0; rep < 1 + ((dup & 16) != 0); ++rep) blk_leader_kernel<false><<<g, kBlock, 0, st>>>(bb);
    MINK_CHECK_LAUNCH();
    for (int rep = 0; rep < 1 + ((dup & 4) != 0); ++rep) blk_leader_kernel<true><<<g, kBlock, 0, st>>>(bb);
    MINK_CHECK_LAUNCH();
    for (int rep = 0; rep < 1 + ((dup & 32) != 0); ++rep) blk_fill_kernel<<<g, kBlock, 0, st>>>(bb);
    MINK_CHECK_LAUNCH();
  }
  // ---- pass 2: tables.  3x3x3 unit-offset tables (with / without the transposed table) and the small ones (pooling, 1x1x1)
  // in one launch per kind; anything else one launch per table
  KMap27Batch b27[2];
  KMapSBatch bs;
  int n27[2] = {0, 0}, ns = 0;
  int64_t max27[2] = {0, 0}, maxs = 0;
  auto flush27 = [&](int t) -> int {
    if (n27[t] == 0) return MINK_OK;
    const dim3 g((unsigned)cdiv(max27[t], kBlock), (unsigned)n27[t]);
    for (int rep = 0; rep < 1 + ((diag_dup() & 1) != 0); ++rep) {
      if (t) kernel_map_blk27_kernel<true><<<g, kBlock, 0, st>>>(b27[1]);
      else kernel_map_blk27_kernel<false><<<g, kBlock, 0, st>>>(b27[0]);
    }
    MINK_CHECK_LAUNCH();
    n27[t] = 0, max27[t] = 0;
    return MINK_OK;
  };
  auto flush_small = [&]() -> int {
    if (ns == 0) return MINK_OK;
    kernel_map_blk_small_kernel<<<dim3((unsigned)cdiv(maxs, kBlock), (unsigned)ns), kBlock, 0, st>>>(bs);
    MINK_CHECK_LAUNCH();
    ns = 0, maxs = 0;
    return MINK_OK;
  };
  for (int i = 0; i < n; ++i) {
    const MinkKernelMapDesc &e = d[i];
    if (!e.blk_table) {  // per-voxel hash map
      if (int rc = mink_kernel_map(e.in_table_keys, e.in_table_vals, e.in_cap, e.out_coords, e.n_out, e.offsets, e.K, e.nbr,
                                   e.nbr_t, stream))
        return rc;
      continue;
    }
    if (e.n_out == 0) continue;
    Offsets off;
    memset(&off, 0, sizeof off);
    memcpy(off.d, e.offsets, sizeof(int) * 3 * e.K);
    bool unit27 = e.K == 27;  // offsets == {-1,0,1}^3 * in_ts, x fastest: the 3x3x3 convolutions
    for (int k = 0; k < 27 && unit27; ++k)
      unit27 = off.d[3 * k] == (k % 3 - 1) * e.in_ts && off.d[3 * k + 1] == ((k / 3) % 3 - 1) * e.in_ts &&
               off.d[3 * k + 2] == (k / 9 - 1) * e.in_ts;
    if (unit27) {
      const int t = e.nbr_t ? 1 : 0;
      kmap_desc(b27[t].e[n27[t]++], e);
      max27[t] = std::max(max27[t], e.n_out);
      if (n27[t] == kMaxBatch)
        if (int rc = flush27(t)) return rc;
      continue;
    }
    if (e.K <= 8) {
      KMapS &q = bs.e[ns++];
      kmap_desc(q, e);
      q.K = e.K;
      memset(&q.off, 0, sizeof q.off);
      memcpy(q.off.d, e.offsets, sizeof(int) * 3 * e.K);
      maxs = std::max(maxs, e.n_out * e.K);
      if (ns == kMaxBatch)
        if (int rc = flush_small()) return rc;
      continue;
    }
    kernel_map_blk_kernel<<<dim3((unsigned)cdiv(e.n_out * e.K, kBlock)), kBlock, 0, st>>>(
        (const unsigned long long *)e.blk_table, e.blk_base, e.blk_rowids, (uint64_t)e.blk_cap - 1, e.in_ts, e.out_coords, e.n_out,
        e.K, off, e.nbr, e.nbr_t);
    MINK_CHECK_LAUNCH();
  }
  if (int rc = flush27(0)) return rc;
  if (int rc = flush27(1)) return rc;
  return flush_small();
}

}  // extern "C"
