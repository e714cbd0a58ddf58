// What the coordinate-map translation units share: coords.hip (keys, unique, pyramid, the scans), kmap.hip (hash inserts,
// neighbour tables, block index, 0xFF fills), rulebook.hip (rulebook, parity classes) and plenoxel.hip (data.npz decoder).
// Only what MORE THAN ONE of them references lives here; a helper with one user stays with its user.  A kernel is defined
// in one file and reached from the others through the host launchers declared below.
#pragma once
#include "common.h"

namespace mink {

constexpr int kBlock = 256;  // 4 waves

// Hash-map capacity for n keys (mink_table_capacity): in a level chain the row count of a level is only known on
// the device, and so is the capacity of the next level's map -- sized for the rows it really receives, not for the
// field's row count (a 2 M-slot table per level for 173 k / 37 k / 8 k ... rows cost 125 MB of clearing per batch and
// scattered the few keys over 25 MB each).
__host__ __device__ __forceinline__ uint64_t table_capacity(int64_t n) {
  uint64_t cap = 64;
  while (cap < (uint64_t)(2 * n)) cap <<= 1;
  return cap;
}

// Level 0 of a pyramid: rows whose keys are STRICTLY ascending (the order of a voxel grid's `links`, of np.nonzero) are
// their own unique rows, and no hash insert is needed to find that out -- every row compares its key with the row before it
// and the first wave that sees a pair out of order sets MINK_STATUS_NOT_ASCENDING (one coherent look at the word per
// offending wave, one atomic until it is seen set).  The unique kernels of level 0 read the word (asc_fast).
__device__ __forceinline__ bool asc_fast(const uint32_t *asc_status) {
  return asc_status && !(*asc_status & MINK_STATUS_NOT_ASCENDING);
}

// ---- first pass of unique (insert_kernel: kmap.hip, beside the block insert: the two share the run-of-equal-keys helpers,
// and the compiler's code for either depends on the other being in its translation unit).  One thread per row over
// cdiv(max(n, 1), kBlock) workgroups; slot_of_row[n] receives the slot of every row's key; cap = slots of the map.
int launch_insert(const uint64_t *keys, int64_t n, const int *n_dev, uint64_t *table_keys, int32_t *table_vals, int64_t cap,
                  int *slot_of_row, const uint32_t *asc_status, hipStream_t st);

// ---- exclusive scans of int32 (scan_kernel / scan_batch_kernel: coords.hip)
struct ScanBatch {  // one workgroup per array
  const int *in[8];
  int *out[8], *total[8];
  int64_t n[8];
};
int launch_scan(const int *in, int *out, int64_t n, int *total, hipStream_t st);  // total (optional) receives the sum
int launch_scan_batch(const ScanBatch &b, int n, hipStream_t st);                 // the first n arrays of b

// ---- 0xFF fills (fill_ff_kernel: kmap.hip).  Up to sixteen runs of 32-bit words per launch (blockIdx.y = run): add() queues
// a run and launches when sixteen are waiting, flush() launches what is waiting.  A run that is not whole 32-bit words goes
// to hipMemsetAsync at once.  `dup`: the MINK_DIAG_DUP repeat of every launch.
struct FillBatch {
  unsigned *ptr[16];
  int64_t nwords[16];
};
struct FillQueue {
  hipStream_t st;
  bool dup;
  int n = 0;
  int64_t max16 = 0;  // 16-byte stores of the longest waiting run
  FillBatch b;
  int add(void *ptr, int64_t bytes);
  int flush();
};

}  // namespace mink
