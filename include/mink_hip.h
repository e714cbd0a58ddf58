/*
 * mink_hip.h -- C ABI of libmink_hip.so: the MI355X (gfx950) native backend for the
 * sparse-3D-convolution classification hot path of POSTECH-CVLab/NeRF-Downstream
 * (co3d_3d/train.py -> Mink-ResNet14/34 on PeRFception-CO3D plenoxel grids).
 *
 * The reference has no C FFI of its own for this path: its seam is the Python module
 * API of the third-party MinkowskiEngine (ME), whose native backend
 * (`MinkowskiEngineBackend._C`, imported by the reference at
 * co3d_3d/src/models/mink/modules/sparse_conv.py:7-12) is what these entry points
 * replace.  Each declaration cites the reference call site(s) it serves; paths are
 * relative to /root/reference.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless named `*_host`;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *     enqueued asynchronously on it, nothing here synchronises the device;
 *   - the caller owns every buffer (no hidden allocations, no global state) so the
 *     library is safe to call from a graph-captured or multi-stream host; every scratch
 *     buffer is passed WITH ITS SIZE (`workspace_bytes`, ABI version 2): the size a launch needs can depend on a
 *     plan (split factors, row splits), so the library checks it against the plan it is about to launch and returns
 *     MINK_EINVAL instead of writing past the end of a buffer sized for another plan;
 *   - the library writes only the first C columns of the first n rows of an output (the pad columns of a row pitch ld > C, rows
 *     an accumulating or scattering call does not visit and statistics rows past the count a call reports keep their bits) and
 *     only the first `workspace_bytes` it asked for; for the entry points of the training step (convolution, weight gradient,
 *     batch-norm family, pools, head, loss, optimizer) no pad-column or out-of-extent value of an input reaches a result, so
 *     their pad columns may hold anything, NaN included (tests/test_gpu_guard.py holds them to both, bit for bit);
 *   - return value 0 = success, otherwise a negative MINK_E* code and
 *     mink_last_error() (thread-local) describes the failure;
 *   - coordinates are int32 rows (batch, x, y, z); row counts are int64; feature
 *     matrices are row-major fp32 with an explicit leading dimension (`ld*`, in
 *     elements) so channel-padded layouts (e.g. 27 -> 28) need no copy;
 *   - a "neighbour table" nbr[n_out][K] (int32, -1 = no neighbour) is the
 *     output-stationary form of ME's kernel map: nbr[o][k] = input row located at
 *     coordinate(o) + offset(k).  K = kernel volume, offsets enumerated x fastest /
 *     z slowest (k = (dx+1) + 3(dy+1) + 9(dz+1) for a 3^3 kernel; witness
 *     sparse_conv.py:375-379).
 */
#ifndef MINK_HIP_H
#define MINK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MINK_OK 0
#define MINK_EINVAL (-1)   /* bad argument (shape / alignment / NULL) */
#define MINK_ELAUNCH (-2)  /* HIP launch or runtime error */

/* Device-side status word bits (written by the coordinate kernels into `status`). */
#define MINK_STATUS_RANGE 1u     /* a coordinate fell outside the packable range */
#define MINK_STATUS_UNSORTED 2u  /* batch column is not non-decreasing */
#define MINK_STATUS_NOT_ASCENDING 4u /* mink_coords_build_levels, informational: the input rows' keys are not strictly ascending
                                        (when CLEAR the rows were their own unique rows and level 0's hash map was left empty) */

/* ------------------------------------------------------------------ error text and ABI version (csrc/lib.hip) */
const char *mink_last_error(void);
/* 2: every scratch buffer is passed with its size; 3: MinkStem.xb (bf16 storage); 4: mink_net_* (the whole trunk per call).
 * A caller compiled or bound against this header refuses a library that answers another number. */
#define MINK_ABI_VERSION 4
int mink_abi_version(void);

/* ------------------------------------------------------------------ coordinate maps (csrc/coords.hip)
 * Coordinate hash map: open addressing, linear probing, 64-bit packed keys
 * (16 bits each for batch | x+2^15 | y+2^15 | z+2^15), int32 values.
 * Replaces ME's CoordinateMapCPU/GPU (insert_and_map / stride / kernel_map) behind
 * ME.TensorField(...).sparse() (models/mink/base_model.py:10-13, models/mink/resnet.py:164)
 * and behind every MinkowskiConvolution / MinkowskiSumPooling forward
 * (modules/common.py:116-125, resnet.py:62-64).
 */

/* Number of hash slots (power of two) required for `n` keys. */
int64_t mink_table_capacity(int64_t n);

/* Bytes of scratch required by mink_coords_unique for `n` rows. */
int64_t mink_unique_workspace_bytes(int64_t n);

/* Key generation.  mode 0: float field rows (b,x,y,z) -> floor() (ME A1 quantisation);
 * mode 1: int32 rows copied; both then floor each spatial coordinate to a multiple of
 * `out_ts` (>=1; 1 = identity) which is ME's stride map key functor
 * (CoordinateMap::stride, used by sparse_conv.py:403-405).
 * keys[n] receives the packed keys; *status |= MINK_STATUS_RANGE on overflow. */
int mink_coords_make_keys(const void *coords, int mode, int64_t n, int32_t out_ts, uint64_t *keys,
                          uint32_t *status, void *stream);

/* insert_and_map with FIRST-OCCURRENCE row numbering (what ME's CPU insert_and_map
 * yields for TensorField.sparse(); the same order is used for stride maps, see
 * DESIGN.md "row order").
 *   table_keys[cap], table_vals[cap] : the hash map (cap = mink_table_capacity(n));
 *                                      on return vals hold the unique row id
 *   out_coords[n][4]   : coordinates of the unique rows (first n_unique rows valid)
 *   unique_index[n]    : first input row of each unique row
 *   inverse[n]         : unique row of every input row (the stride map in2out)
 *   n_unique           : device int32 scalar
 */
int mink_coords_unique(const uint64_t *keys, int64_t n, uint64_t *table_keys, int32_t *table_vals,
                       int64_t cap, int32_t *out_coords, int32_t *unique_index, int32_t *inverse,
                       int32_t *n_unique, void *workspace, int64_t workspace_bytes, void *stream);

/* The whole coordinate pyramid of one batch in ONE call and with NO host synchronisation:
 * level 0 = insert_and_map of the input rows (mode as in mink_coords_make_keys, floored to
 * out_ts_host[0], normally 1); level l>0 = stride map of level l-1 floored to out_ts_host[l].
 * Row counts of the levels stay on the device (each level's kernels read the previous count
 * from `meta`), so every buffer is sized for the upper bound `n`:
 *   table_keys[l][cap], table_vals[l][cap], out_coords[l][n][4], index_b[l][n] (inverse map /
 *   in2out of level l), index_a[l][n] (first-occurrence rows; may be NULL for l > 0).
 *   meta[nlev+2] (device int32): unique rows per level, then the status word, then the batch
 *   count (batch index of the last row + 1).  The caller reads `meta` back once.
 * Input rows whose packed keys are strictly ascending (the order of a voxel grid's `links`) need no hash insert at
 * level 0: every row is compared with the one before it, and only when a pair is out of order
 * (MINK_STATUS_NOT_ASCENDING in the status word) does level 0 go through its hash map.  In the ascending case that
 * map is left EMPTY (all slots cleared): a caller that wants look-ups through it inserts the level's rows itself
 * (mink_coords_make_keys + mink_coords_unique).
 * The hash map of level l > 0 occupies only the first mink_table_capacity(rows of level l-1) slots of its
 * buffer -- the capacity for the rows it really receives, computed on the device; a later look-up in it
 * (mink_kernel_map) must be given that capacity, which the caller can compute once it has read `meta`.
 * Replaces the chain TensorField.sparse() -> stride() x5 of one forward pass
 * (resnet.py:164-173, sparse_conv.py:403-405). */
int64_t mink_levels_workspace_bytes(int64_t n);
int mink_coords_build_levels(const void *coords, int mode, int64_t n, int32_t nlev,
                             const int32_t *out_ts_host, uint64_t *const *table_keys,
                             int32_t *const *table_vals, int64_t cap, int32_t *const *out_coords,
                             int32_t *const *index_a, int32_t *const *index_b, int32_t *meta,
                             void *workspace, int64_t workspace_bytes, void *stream);

/* Row ranges of each batch index in a coordinate list whose batch column is
 * non-decreasing (guaranteed by ME.utils.sparse_collate, data/utils.py:25-30).
 * batch_offsets[B+1].  Sets MINK_STATUS_UNSORTED otherwise.  (ME origin_map.) */
int mink_batch_offsets(const int32_t *coords, int64_t n, int32_t B, int32_t *batch_offsets,
                       uint32_t *status, void *stream);

/* ------------------------------------------------------------------ neighbour tables (csrc/kmap.hip; the 5^3 / 7^3 cube tables: csrc/conv_bigk.hip) */
/* Kernel map as a neighbour table: for every output row o and offset k probe the INPUT
 * map at out_coords[o] + offsets[k].  offsets_host[K][3] are already scaled by
 * dilation * input tensor stride.  If nbr_t != NULL it must be pre-filled with -1
 * ([n_in][K]) and receives the transposed table nbr_t[i][k] = o (used by dgrad).
 * Replaces CoordinateMapManager::kernel_map (witness for the Python-visible format:
 * sparse_conv.py:90-96,124-143). */
int mink_kernel_map(const uint64_t *in_table_keys, const int32_t *in_table_vals, int64_t in_cap,
                    const int32_t *out_coords, int64_t n_out, const int32_t *offsets_host, int32_t K,
                    int32_t *nbr, int32_t *nbr_t, void *stream);

/* Every kernel map of one forward/backward pass in ONE call (one descriptor per map; same
 * semantics as mink_kernel_map, nbr_t is cleared to -1 here).  Cuts the per-map host cost. */
typedef struct MinkKernelMapDesc {
  const uint64_t *in_table_keys;
  const int32_t *in_table_vals;
  int64_t in_cap;
  const int32_t *out_coords;
  int64_t n_out;
  int64_t n_in;
  int32_t *nbr;
  int32_t *nbr_t; /* may be NULL */
  int32_t K;
  int32_t offsets[81]; /* [K][3], scaled by dilation * input tensor stride */
  /* Optional block index of the INPUT map (blk_table != NULL): neighbour look-ups go through a second, much smaller
   * hash map keyed by the 4x4x4-cell BLOCK of a coordinate instead of through the per-voxel map.  A block entry
   * holds the occupancy mask of its 64 cells and the start of its run in `blk_rowids`; the row of a cell is
   * blk_rowids[base + popcount(mask below the cell)].  The 27 neighbours of a voxel fall into at most 8 blocks and
   * neighbouring voxels share them, so a wave touches a handful of cache lines where the per-voxel map (one random
   * 64-byte line for the key and one for the value, per probe) touched thousands: 1.5 GB of HBM traffic per stem table
   * became the size of the table itself.  Results are identical (bit-exact tables).  Descriptors that share an input
   * map share the buffers; exactly the first of them sets blk_build = 1 and the index is built by that call. */
  const int32_t *in_coords; /* [n_in][4] rows of the input map */
  int32_t in_ts;            /* its tensor stride (cells are coordinates / in_ts) */
  int32_t blk_build;
  uint64_t *blk_table;      /* [blk_cap][2]: block key, inverted occupancy mask */
  int32_t *blk_base;        /* [blk_cap] */
  int32_t *blk_slot;        /* [n_in] scratch: block slot of every input row */
  int32_t *blk_rowids;      /* [max(n_in, 8)] */
  int32_t *blk_counter;     /* [1]: the build fills it with 0xFFFFFFFF (= every block found a slot) and writes 0 if blk_cap was too
                               small (rows of blocks that found no slot are then missing from the tables: the caller's error,
                               reported instead of a hang; see also mink_set_overflow_sink) */
  int64_t blk_cap;          /* power of two >= 2 * the number of occupied blocks (<= n_in; the blocks of the map at tensor stride ts
                               are the cells of the map at 4 ts, so a caller that holds that map knows the number) */
} MinkKernelMapDesc;
int mink_kernel_map_batch(int32_t n, const MinkKernelMapDesc *descs, void *stream);

/* Neighbour table of a centred CUBE of ks^3 offsets, ks = 5 (K = 125) or 7 (K = 343): the sizes beyond the 27 offsets that
 * MinkKernelMapDesc.offsets holds.  Semantics of mink_kernel_map: nbr[o][k] = the input row at out_coords[o] + offset_k or -1, k
 * enumerating x fastest and z slowest, offset_k = (k % ks - r, k / ks % ks - r, k / ks^2 - r) * step with r = (ks - 1) / 2 and
 * step = dilation * input tensor stride; nbr_t[i][k] = o (may be NULL; cleared to -1 here).  A neighbour whose coordinate
 * leaves the packable range (-32768..32767 per axis) is absent.  The entry inserts the input rows (unique, as the rows of a
 * map are) into a per-voxel hash map of its own in `workspace` (>= mink_kernel_map_cube_workspace_bytes(n_in)), so it does not
 * depend on the level's map having been filled (mink_coords_build_levels leaves it empty for ascending rows), and probes it
 * once per (row, offset).  Refuses n_out * K >= 2^31.  Coordinates and workspace on 16 bytes. */
int64_t mink_kernel_map_cube_workspace_bytes(int64_t n_in);
int mink_kernel_map_cube(const int32_t *in_coords, int64_t n_in, const int32_t *out_coords, int64_t n_out, int32_t ks,
                         int32_t step, int32_t *nbr, int32_t *nbr_t, void *workspace, int64_t workspace_bytes, void *stream);

/* Process-wide overflow sink of the block-index builds: a 32-bit word in PINNED host memory (device-mapped; NULL = none), zero
 * initialised by the caller.  A build whose blk_cap was too small writes 1 into it (besides clearing its own blk_counter) and
 * nobody ever refills it, so a caller that looks at the word before queuing its next batch learns of a violated capacity
 * promise without a device synchronisation or a copy -- one batch late at most, instead of silently missing neighbours. */
int mink_set_overflow_sink(int32_t *host_word);

/* ------------------------------------------------------------------ rulebook and parity classes: derived orders of a table or a map (csrc/rulebook.hip) */
/* ME-format rulebook from a neighbour table: per offset k the (in,out) pairs ordered
 * by output row, built with wave64 ballot + prefix sums.
 *   counts[K+1]      : exclusive scan of pairs per offset (device, int32)
 *   pairs_in/out[P]  : concatenated lists (P <= n_out*K), may be NULL to only count
 *   workspace        : >= mink_rulebook_workspace_bytes(n_out, K)
 */
int64_t mink_rulebook_workspace_bytes(int64_t n_out, int32_t K);
int mink_rulebook(const int32_t *nbr, int64_t n_out, int32_t K, int32_t *counts, int32_t *pairs_in,
                  int32_t *pairs_out, void *workspace, int64_t workspace_bytes, void *stream);

/* Parity-class permutation of the rows of a tensor-stride-`ts` map: rows grouped by the parity
 * of (coordinate / ts) per axis (8 classes), each class segment padded to a multiple of `pad`
 * rows with -1.  perm[mink_class_partition_rows(n,pad)].  Used by the input-gradient of
 * stride-2 convolutions (resnet_block.py:29-37 with stride 2): all rows of one class are reached
 * through the same 2^p kernel offsets, so class-pure tiles skip the other offsets. */
int64_t mink_class_partition_rows(int64_t n, int32_t pad);
int64_t mink_class_partition_workspace_bytes(int64_t n);
int mink_class_partition(const int32_t *coords, int64_t n, int32_t ts, int32_t pad, int32_t *perm,
                         void *workspace, int64_t workspace_bytes, void *stream);
/* The same for up to eight maps in four launches (fill, count, scan, place; blockIdx.y = map) instead of four per map:
 * what a prepared batch asks for (one permutation per strided convolution of the network). */
typedef struct MinkClassPartitionDesc {
  const int32_t *coords; /* [n][4] */
  int64_t n;
  int32_t ts, pad;
  int32_t *perm;         /* mink_class_partition_rows(n, pad) entries */
  void *workspace;       /* mink_class_partition_workspace_bytes(n), 256-byte aligned */
  int64_t workspace_bytes;
} MinkClassPartitionDesc;
int mink_class_partition_batch(int32_t n_maps, const MinkClassPartitionDesc *descs, void *stream);

/* ------------------------------------------------------------------ sparse convolution (csrc/conv.hip, csrc/conv_wgrad.hip; kernel volumes above 27: csrc/conv_bigk.hip)
 * Replaces ME ConvolutionForward/BackwardKernel behind ME.MinkowskiConvolution
 * (modules/common.py:116-125; the algorithm is re-stated by the reference at
 * sparse_conv.py:122-144): out[o] = sum_k in[nbr[o][k]] @ W[k]  (+ bias).
 */

/* Output-stationary gather-GEMM on the fp32 matrix cores.
 *   x[n_in][ldx], cin  : gathered operand (every table entry is -1 or < n_in)
 *   w                  : w_transposed == 0:  w[K][cin][cout]   (forward)
 *                        w_transposed == 1:  w[K][cout][cin]   (dgrad: pass the forward
 *                                            kernel and swap cin/cout)
 *   flip_k             : use w[K-1-k] for table column k (dgrad of a stride-1 conv
 *                        re-uses the forward table: nbr_t[i][k] == nbr[i][K-1-k])
 *   nbr[n_out][K]      : neighbour table;  y[n_out][ldy] receives cout columns.  (cin == 28, the flattened-K
 *                        stem path: taken only when n_in < 2^24 - 1 -- its rows are addressed with a 24-bit
 *                        multiply -- and the table has fewer than 2^32 bytes (4 n_out K: it is read through a
 *                        32-bit buffer descriptor); larger inputs and tables take the general path.)
 *   bias[cout] or NULL
 *   row_perm/n_virtual : optional row permutation (NULL/0 = identity): tile row v computes
 *                        output row row_perm[v], -1 entries are padding (mink_class_partition)
 *   ksplit             : >1 splits the K offsets over `ksplit` workgroups per tile and
 *                        reduces through `workspace` (ksplit*n_out*cout floats).  With a class
 *                        permutation of an fp32 mid layer (cin >= 64, K >= 8) the split is over
 *                        the cin/32 channel chunks instead (<= cin/32 slices; a tile of one
 *                        parity class has few live offsets, every slice sees all of them)
 */
/* Test / measurement knob (never needed by a caller): bit 9 = no flattened-K stem path, bit 10 = tiled instead of streaming
 * stem weight gradient, bits 12-15 / 16-27 = force the weight-gradient offset grouping / row-split count (sweeps; this is the
 * plan change the workspace_bytes arguments guard against), bit 28 = bf16 math keeps the fp32 stem weight gradient, bit 29 =
 * plain workgroup order in the streaming weight gradient, bit 30 / 31 = the dense gather-GEMM instead of the row-compacted
 * kernel for the mid layers / the strided data gradients (the tests compare the two).  Returns the previous low byte. */
int mink_conv_set_stagger(int units);

/* Which software pipeline the row-compacted mid-layer kernel (compact_gemm_kernel) runs: bit 0 = the stride-1 forward / data
 * gradient launches, bit 1 = the class-permuted strided data gradients on the THREE-STAGE form (three LDS stages of the gathered-row
 * tile, MFMA operands read one item ahead; three workgroups per CU), 0 = the two-stage form (four workgroups per CU).  Results are
 * bit-identical either way.  Returns the previous mode. */
int mink_conv_set_pipeline(int mode);

/* Measurement only: while `buf` (device memory, 5 x uint64 per workgroup, `capacity_workgroups` of them) is set, the mid-layer
 * forward kernel runs the instantiation that carries the timing switches and every workgroup records the shader clock at its start,
 * at the head of its item loop, at its epilogue and at its end (stores drained), plus its hardware id (scripts/kbench.py ctrace).
 * NULL: off. */
int mink_conv_trace(void *buf, int64_t capacity_workgroups);
/* Matrix-core arithmetic of mink_conv_gather_gemm (forward / input gradient):
 *   0 = exact fp32 MFMA (default), 1 = bf16 operands with fp32 accumulation (BASELINE config
 *   "bf16 mixed precision"), 3 = split-bf16 (hi/lo, three products; ~1e-5 relative).
 * HBM tensors stay fp32 in every mode.  Returns the previous mode. */
int mink_conv_set_math(int mode);
int mink_conv_get_math(void); /* the current mode, unchanged */
/* Split-K factor the library recommends for a layer (1 for large row counts).  row_classes != 0:
 * the launch will pass a class-partitioned row_perm (stride-2 dgrad), n_out = its n_virtual. */
int mink_conv_plan_ksplit(int64_t n_out, int32_t K, int32_t cout, int32_t row_classes);
/* The same with the reduction width known (what the block sequencer and the Python layer ask): for a class-permuted fp32 mid
 * layer (row_classes != 0) the channel-chunk split of the row-compacted kernel, for an fp32 mid layer its offset split (<= 14
 * slabs), otherwise mink_conv_plan_ksplit's answer.  The workspace is 4 * ksplit * n_out * cout bytes in every case.
 * Which kernel a call with that split then reaches: mink_conv_gather_gemm_launch_info below. */
int mink_conv_plan(int64_t n_rows, int32_t K, int32_t cin, int32_t cout, int32_t row_classes);

/* Which launch a convolution call will make, answered by the planner the launch itself runs (host arithmetic, no GPU).
 * kernel = MINK_KERNEL_*, targ = the template arguments of the instantiation in the order given with each family, grid /
 * block / lds_bytes the launch configuration, slabs the slices it writes (row splits for a weight gradient), epilogue =
 * MINK_EPILOGUE_*.  A call with n_out == 0 launches nothing: all zeros. */
enum {
  MINK_KERNEL_GATHER_SCALAR = 1,     /* gather_gemm_kernel {W_T} */
  MINK_KERNEL_GATHER2 = 2,           /* gather_gemm2_kernel {W_T, STAGE, FLAT, MATH} */
  MINK_KERNEL_COMPACT = 3,           /* compact_gemm_kernel {W_T, PERM, ABL, MATH, P3, SK} */
  MINK_KERNEL_WGRAD = 4,             /* wgrad_kernel {G, NARROW, VEC, BUF} */
  MINK_KERNEL_WGRAD16 = 5,           /* wgrad16_kernel {G} */
  MINK_KERNEL_WGRAD_STREAM = 6,      /* wgrad_stream_kernel {D, FUSE, FLAT} */
  MINK_KERNEL_WGRAD_STREAM_BF16 = 7, /* wgrad_stream_bf16_kernel {FUSE, B16} */
  MINK_KERNEL_WGRAD_STREAM_B16T = 8  /* wgrad_stream_b16t_kernel */
};
enum {
  MINK_EPILOGUE_NONE = 0,
  MINK_EPILOGUE_COLSUM = 1,              /* un-split launch with statistics: colsum_f32_kernel over the per-tile partials */
  MINK_EPILOGUE_SPLITK_REDUCE = 2,       /* splitk_reduce_kernel */
  MINK_EPILOGUE_SPLITK_REDUCE_STATS = 3, /* splitk_reduce_stats_kernel */
  MINK_EPILOGUE_SLABS = 4,               /* the slabs are left to the caller (mink_conv_gather_gemm_slabs) */
  MINK_EPILOGUE_SLAB_REDUCE = 5          /* weight gradient: slab_reduce_kernel over the row splits */
};
typedef struct {
  int32_t kernel;
  int32_t targ[6];
  int32_t grid[3];
  int32_t block;
  int32_t lds_bytes;
  int32_t slabs;
  int32_t epilogue;
} MinkConvLaunchInfo;
/* mink_conv_gather_gemm / _slabs / _stats described by scalars: row_perm / bias / stats / slabs != 0 where the call passes
 * that pointer (stats: the three statistics buffers), xw_aligned = x and w on 16 bytes, y_aligned = y, workspace and bias on
 * 16 bytes.  Refuses what the call would refuse for these scalars, with the same message. */
int mink_conv_gather_gemm_launch_info(int64_t n_in, int32_t ldx, int32_t cin, int32_t w_transposed, int32_t flip_k, int64_t n_out,
                                      int32_t K, int32_t row_perm, int64_t n_virtual, int32_t ldy, int32_t cout, int32_t bias,
                                      int32_t ksplit, int32_t stats, int32_t slabs, int32_t xw_aligned, int32_t y_aligned,
                                      MinkConvLaunchInfo *info);
/* mink_conv_wgrad (fuse = 0), mink_conv_wgrad_bn_relu_pool (1; ldy = cout) or mink_conv_wgrad_bn_relu_pool_b16 (2; ldx = 32,
 * ldy = cout) described the same way; aligned = x and dy on 16 bytes, n_pool the pooled rows of a fused call (else 0). */
int mink_conv_wgrad_launch_info(int64_t n_in, int32_t ldx, int32_t cin, int32_t ldy, int32_t cout, int64_t n_out, int32_t K,
                                int32_t fuse, int64_t n_pool, int32_t aligned, MinkConvLaunchInfo *info);
/* flip_k: bit 0 = read the weights of offset K-1-k for offset k (data gradient of a stride-1 convolution through the
 * forward table); bit 1 = ACCUMULATE, y[row] += result instead of y[row] = result -- for an un-split launch whose
 * row_perm visits every output row at most once (rows it does not visit are left untouched): the data gradient of
 * the 1x1x1 strided shortcut convolution is added into the main branch's gradient at the 1/8 of the rows it reaches. */
int mink_conv_gather_gemm(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *w, int32_t w_transposed,
                          int32_t flip_k, const int32_t *nbr, int64_t n_out, int32_t K,
                          const int32_t *row_perm, int64_t n_virtual, float *y, int32_t ldy,
                          int32_t cout, const float *bias, int32_t ksplit, float *workspace,
                          int64_t workspace_bytes, void *stream);
/* mink_conv_gather_gemm that LEAVES a split launch's partial slabs in `workspace`: described with its consumers,
 * mink_bn_small_fwd / mink_bn_small_bwd / mink_bn_bwd_slabs, in the batch-norm section below. */
int mink_conv_gather_gemm_slabs(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *w, int32_t w_transposed,
                                int32_t flip_k, const int32_t *nbr, int64_t n_out, int32_t K, const int32_t *row_perm,
                                int64_t n_virtual, float *y, int32_t ldy, int32_t cout, int32_t ksplit, float *workspace,
                                int64_t workspace_bytes, int32_t *slabs_out, void *stream);
/* Forward convolution that also emits the column statistics of its output for the batch norm that
 * follows (reference resnet_block.py:53-60: every 3x3x3 convolution feeds a norm): the un-split
 * kernel sums its tile in the epilogue, the split-K reduce sums while it adds the slabs -- y is
 * not read again.  stats_out: double [<= 512][2][cout]; *stats_rows (host) = partial rows written,
 * 0 when this launch shape cannot produce them (the caller then calls mink_bn_stats);
 * stats_ws >= mink_conv_stats_workspace_bytes(n_out, cout). */
int64_t mink_conv_stats_workspace_bytes(int64_t n_out, int32_t cout);
int mink_conv_gather_gemm_stats(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *w, const int32_t *nbr,
                                int64_t n_out, int32_t K, float *y, int32_t ldy, int32_t cout,
                                const float *bias, int32_t ksplit, float *workspace, int64_t workspace_bytes,
                                double *stats_out, int32_t *stats_rows, void *stats_ws, int64_t stats_ws_bytes, void *stream);

/* Weight gradient dW[k] = X[nbr[.][k]]^T @ dY, split over row blocks and reduced
 * deterministically (no atomics).  x has n_in rows (every nbr entry is -1 or in [0, n_in)).
 * workspace >= mink_conv_wgrad_workspace_bytes().
 * The tiled kernels read x, dy and the table through 32-bit buffer offsets only when each has fewer than 2^31 bytes,
 * n_in < 2^24, and the "no neighbour" offset those kernels form -- the low 32 bits of 0xFFFFFF * 4 ldx -- lies at or
 * beyond the end of x (for ldx > 64 that product wraps: ldx = 68 puts it at 2^28 - 272); any other call takes the
 * 64-bit addressed instantiation.  Which one: mink_conv_wgrad_launch_info. */
int64_t mink_conv_wgrad_workspace_bytes(int64_t n_out, int32_t K, int32_t cin, int32_t cout);
int mink_conv_wgrad(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *dy, int32_t ldy,
                    int32_t cout, const int32_t *nbr, int64_t n_out, int32_t K, float *dw, void *workspace,
                    int64_t workspace_bytes, void *stream);
/* Weight gradient of a convolution whose output y feeds  pool(relu(bn(y)))  (the stem of the
 * reference ResNets, resnet.py:58-64) and whose input needs no gradient: the gradient with respect
 * to y is recomputed from (y, pooled gradient, batch statistics, dgamma, dbeta -- mink_bn_relu_pool_bwd
 * with dx = NULL) inside the kernel's operand load and never written to memory.
 * Only for shapes the streaming kernel takes (K = 27, cin <= 32, many rows): ask _supported() first. */
int mink_conv_wgrad_bn_relu_pool_supported(int64_t n_in, int32_t ldx, int32_t cin, int64_t n_out, int32_t K,
                                           int32_t cout);
int mink_conv_wgrad_bn_relu_pool(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *y, int32_t cout,
                                 const float *dy_pool, int64_t n_pool, const int32_t *in2out, const float *mean,
                                 const float *invstd, const float *gamma, const float *beta,
                                 const float *dgamma, const float *dbeta, const int32_t *nbr, int64_t n_out,
                                 int32_t K, float *dw, void *workspace, int64_t workspace_bytes, void *stream);

/* Kernel volumes 27 < K <= MINK_BIGK_MAX_K (the 5^3 and 7^3 cubes; csrc/conv_bigk.hip).  Exact fp32 on the matrix cores in
 * EVERY mink_conv_set_math mode; no atomics, fixed summation order (bit-identical runs).  Arguments as mink_conv_gather_gemm
 * (w_transposed, flip_k bit 0, pitches ldx / ldy; any cin, cout >= 1; no alignment beyond 4 bytes) without row_perm and split:
 * ONE launch, a workgroup owns MINK_BIGK_ROW_TILE rows x 64 columns, walks its table in chunks of 32 offsets, drops the offsets
 * no row of the tile has and reduces flattened over (present offset, channel).  The weight gradient works on steps of
 * MINK_BIGK_WGRAD_ROWS rows, skips an offset none of them has, splits the rows over workgroups and sums the splits in order
 * through `workspace` (>= mink_conv_bigk_wgrad_workspace_bytes()). */
#define MINK_BIGK_MAX_K 343
#define MINK_BIGK_ROW_TILE 64
#define MINK_BIGK_WGRAD_ROWS 32
int mink_conv_bigk_gather_gemm(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *w, int32_t w_transposed,
                               int32_t flip_k, const int32_t *nbr, int64_t n_out, int32_t K, float *y, int32_t ldy, int32_t cout,
                               const float *bias, void *stream);
int64_t mink_conv_bigk_wgrad_workspace_bytes(int64_t n_out, int32_t K, int32_t cin, int32_t cout);
int mink_conv_bigk_wgrad(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const float *dy, int32_t ldy, int32_t cout,
                         const int32_t *nbr, int64_t n_out, int32_t K, float *dw, void *workspace, int64_t workspace_bytes,
                         void *stream);

/* ------------------------------------------------------------------ dense GEMM, classifier head and loss (csrc/dense.hip) */
/* Data gradient of a 1x1x1 convolution as a plain GEMM: y[n][N] = x[n][Kd] @ W^T with the FORWARD kernel W[N = cin][Kd = cout]
 * (the `downsample` convolution of a residual block, models/mink/resnet.py:120-128), one fp32 MFMA accumulator chain per
 * element, k ascending -- the same sum mink_conv_gather_gemm forms for a one-column table.  Kd a multiple of 4. */
int mink_dense_xwt(const float *x, const float *w, int64_t n, int32_t Kd, int32_t N, float *y, void *stream);
/* dst[idx[r]][0..C) += src[r][0..C) for every r < n_src with idx[r] >= 0; the idx values must be distinct (no atomics).
 * With idx = the forward table of a kernel-volume-1 strided convolution this adds the shortcut's data gradient into the
 * rows of the block-input gradient it reaches (about one in eight). */
int mink_rows_scatter_add(const float *src, const int32_t *idx, int64_t n_src, int32_t C, float *dst, void *stream);

/* Classifier head in one launch each way: logits[b] = mean_{rows of batch b} x[row] @ W + bias, i.e.
 * MinkowskiGlobalAvgPooling followed by the kernel-volume-1 `final` convolution with bias (models/mink/resnet.py:15-22,
 * 93-99,175-177; W is ME's (Cin, Cout) kernel of a `use_mm` convolution, bias (1, Cout) or NULL).  pooled[B][C] is an
 * output the backward pass reads.  Backward: dx[n][C] (may be NULL), dw[C][ncls], dbias[ncls] (may be NULL). */
int mink_head_forward(const float *x, const int32_t *batch_offsets, int32_t B, int32_t C, const float *w, const float *bias,
                      int32_t ncls, float *pooled, float *logits, void *stream);
int mink_head_backward(const float *dlogits, const float *pooled, const float *w, const int32_t *batch_offsets, int32_t B,
                       int32_t C, int32_t ncls, float *dw, float *dbias, float *dx, void *stream);
/* torch.nn.functional.cross_entropy(logits, labels) with its defaults (mean over the batch; reference
 * modules/classification_training.py:33) as one launch each way.  labels: int64 [B]; prob[B][ncls] (softmax) is kept for
 * backward; *loss a device scalar; a label outside [0, ncls) makes the loss NaN.  grad_loss: device scalar. */
int mink_softmax_ce_forward(const float *logits, const int64_t *labels, int32_t B, int32_t ncls, float *prob, float *loss,
                            void *stream);
int mink_softmax_ce_backward(const float *prob, const int64_t *labels, const float *grad_loss, int32_t B, int32_t ncls,
                             float *dlogits, void *stream);

/* ------------------------------------------------------------------ pooling (csrc/pool.hip)
 * MinkowskiSumPooling(k=2,s=2) (resnet.py:62-64): out[o] = sum_k in[nbr[o][k]] with the
 * 2^3 children table; backward dIn[i] = dOut[in2out[i]].
 */
int mink_pool_sum_fwd(const float *x, int32_t ldx, int32_t C, const int32_t *nbr, int64_t n_out, int32_t K,
                      float *y, void *stream);
int mink_pool_sum_bwd(const float *dy, int32_t C, const int32_t *in2out, int64_t n_in, float *dx,
                      void *stream);

/* MinkowskiGlobalAvgPooling (resnet.py:15-22,175): y[b] = mean of rows
 * [batch_offsets[b], batch_offsets[b+1]); backward dx[i] = dy[b]/N_b. */
int mink_global_avg_fwd(const float *x, int32_t C, const int32_t *batch_offsets, int32_t B, float *y,
                        void *stream);
int mink_global_avg_bwd(const float *dy, int32_t C, const int32_t *batch_offsets, int32_t B, int64_t n,
                        float *dx, void *stream);

/* Max pooling over a neighbour table whose windows may overlap -- the 3x3 stride-2 pooling of the dense 2-D
 * comparison network (torchvision ResNet, reference co3d_2d/src/model/models.py:18-23), which is its only caller: C % 4 == 0,
 * contiguous rows, and a window with no present entry gets -inf.  ME.MinkowskiMaxPooling on sparse tensors goes through
 * mink_pool_local_max_fwd / _bwd below (any C, row pitch, empty windows -> 0).
 * arg[n_out][C] receives the input row of each maximum; backward gathers through the transposed table nbr_t[n_in][K]
 * (the windows containing a row), so there are no atomics. */
int mink_pool_max_fwd(const float *x, int32_t C, const int32_t *nbr, int64_t n_out, int32_t K, float *y, int32_t *arg,
                      void *stream);
int mink_pool_max_bwd(const float *dy, const int32_t *arg, int32_t C, const int32_t *nbr_t, int64_t n_in, int32_t K,
                      float *dx, void *stream);

/* The sparse pooling family.
 * Conventions of mink_pool_sum_* / mink_in_* / mink_ln_*: fp32 features x[n][C] with a row pitch ldx >= C (outputs and
 * gradients are contiguous, pitch C), any 1 <= C <= 4096 -- 16-byte accesses when C % 4 == 0, ldx % 4 == 0 and the pointers are
 * 16-byte aligned, dword accesses otherwise --, no host read-back, no floating-point atomics, sums in a fixed order (two runs
 * are bitwise equal), empty table entries are -1.
 *
 * Local pooling over a neighbour table nbr[n_out][K] whose windows may overlap (1 <= K <= 81), k ascending:
 *   mode 0 (ME.MinkowskiSumPooling beyond kernel_size == stride): y[o] = sum over the present k of x[nbr[o][k]]
 *   mode 1 (ME.MinkowskiAvgPooling):                              y[o] = that sum / cnt[o]
 * cnt[o] (int32 [n_out]; required for mode 1, optional for mode 0) = the number of present entries of row o: the average
 * divides by the number of non-empty inputs, NOT by the kernel volume [ME-recall of MinkowskiAvgPooling; parity unpinned: ME
 * is absent and the reference holds no fixture for this layer].  A row with no present entry gets 0 and cnt 0.
 * Backward gathers through the transposed table nbr_t[n_in][K] (nbr_t[i][k] = o iff nbr[o][k] = i):
 *   dx[i] = sum over the present k of dy[nbr_t[i][k]] (/ cnt[nbr_t[i][k]] for mode 1). */
int mink_pool_local_fwd(const float *x, int32_t ldx, int32_t C, const int32_t *nbr, int64_t n_out, int32_t K, int32_t mode,
                        float *y, int32_t *cnt, void *stream);
int mink_pool_local_bwd(const float *dy, int32_t C, const int32_t *nbr_t, int64_t n_in, int32_t K, int32_t mode,
                        const int32_t *cnt, float *dx, void *stream);
/* ME.MinkowskiMaxPooling: y[o][c] = max over the present k of x[nbr[o][k]][c], arg[o][c] = that input row; the lowest k wins a
 * tie (the first present entry in kernel-offset order), a NaN never replaces a number.  A row with no present entry gets 0
 * and arg -1.  Backward: dx[i][c] = sum over the present k of (arg[o][c] == i ? dy[o][c] : 0), o = nbr_t[i][k]. */
int mink_pool_local_max_fwd(const float *x, int32_t ldx, int32_t C, const int32_t *nbr, int64_t n_out, int32_t K, float *y,
                            int32_t *arg, void *stream);
int mink_pool_local_max_bwd(const float *dy, const int32_t *arg, int32_t C, const int32_t *nbr_t, int64_t n_in, int32_t K,
                            float *dx, void *stream);
/* Global pooling, segmented over batch_offsets (int32 [B+1] on the device, 1 <= B <= 65535; sample b owns rows
 * [batch_offsets[b], batch_offsets[b+1])).  Launch shape of mink_in_fwd: per-workgroup partials in `workspace`
 * (mink_global_pool_workspace_bytes, 8-byte aligned), combined in a fixed order; two launches forward, one backward for any B.
 *   ME.MinkowskiGlobalMaxPooling: y[b][c] = max over the sample's rows, arg[b][c] = the LOWEST row attaining it (row index into
 *     x); an empty sample gives 0 and arg -1.  Backward: dx[i][c] = arg[b][c] == i ? dy[b][c] : 0, one pass over the rows of dx.
 *   ME.MinkowskiGlobalSumPooling: y[b] = sum of the sample's rows, accumulated in double and rounded once; dx[i] = dy[b]. */
int64_t mink_global_pool_workspace_bytes(int64_t n, int32_t C, int32_t B);
int mink_global_max_fwd(const float *x, int64_t n, int32_t ldx, int32_t C, const int32_t *batch_offsets, int32_t B, float *y,
                        int32_t *arg, void *workspace, int64_t workspace_bytes, void *stream);
int mink_global_max_bwd(const float *dy, const int32_t *arg, int64_t n, int32_t C, const int32_t *batch_offsets, int32_t B,
                        float *dx, void *stream);
int mink_global_sum_fwd(const float *x, int64_t n, int32_t ldx, int32_t C, const int32_t *batch_offsets, int32_t B, float *y,
                        void *workspace, int64_t workspace_bytes, void *stream);
int mink_global_sum_bwd(const float *dy, int64_t n, int32_t C, const int32_t *batch_offsets, int32_t B, float *dx, void *stream);

/* ------------------------------------------------------------------ segmentation tail (csrc/seghead.hip)
 * SparseTensor.slice() (reference res16unet.py:435), any C >= 1.  Forward: y[i][:] = x[idx[i]][:], i < n (an index outside
 * [0, n_src) gives a zero row).  Backward (mink_segment_sum, declared beside
 * mink_segment_mean in the field section): y[r][:] = sum of x[members[j]][:] over j in [seg[r], seg[r+1]), in member
 * order (fixed-order fp32 sum: bitwise reproducible), with the (members, seg) pair TensorField.sparse() builds for
 * mink_segment_mean. */
int mink_rows_gather(const float *x, int64_t ldx, int64_t n_src, int32_t C, const int32_t *idx, int64_t n, float *y, void *stream);

/* torch.nn.functional.cross_entropy(z, labels, weight=w, ignore_index=ignore_label) (mean reduction) over per-point logits
 * z[n][C] (fp32, row stride ldz >= C), 2 <= C <= 128, with the prediction, the confusion matrix and the label counts out
 * of the same pass over the logits (reference modules/segmentation_training.py SegLoss :27-44, utils fast_hist).
 *   labels        : int64 [n] (labels_int64 != 0) or int32 [n]
 *   w             : class weights [C], NULL = all ones
 *   a row is VALID when 0 <= label < C and label != ignore_label, IGNORED when label == ignore_label and BAD otherwise;
 *   bad rows are counted and otherwise treated like ignored ones (no device-side assert)
 *   lse[n]        : log sum exp of every row -- all the backward pass needs besides the logits
 *   pred[n]       : int32 argmax (lowest index on ties); NULL to skip
 *   hist[C*C]     : int64, hist[label * C + pred] over the valid rows (zeroed here); NULL to skip
 *   stats         : 40 bytes, 8-byte aligned: double num = sum_valid w[y] * (lse - z[y]); double den = sum_valid w[y];
 *                   int64 n_valid; int64 n_ignored; int64 n_bad -- in this order
 *   loss          : fp32 device scalar num / den (NaN when nothing is valid, as torch gives)
 *   workspace     : >= mink_seg_ce_workspace_bytes(n, C), 8-byte aligned (per-workgroup partial sums)
 * The assignment of rows to workgroups is fixed, every workgroup writes one (num, den) partial in double and a second
 * launch adds the partials in index order: the result is bitwise the same from run to run.  n == 0 writes loss = NaN,
 * a zero histogram and zero stats.
 * Backward: dz[i][j] = g / den * valid_i * w[y_i] * (exp(z[i][j] - lse[i]) - [j == y_i]); g = *grad_loss and den = stats'
 * second double are read on the device; every element of the dense dz[n][C] is written (zeros on ignored / bad rows, and
 * everywhere when den == 0, where torch writes NaN). */
int64_t mink_seg_ce_workspace_bytes(int64_t n, int32_t C);
int mink_seg_ce_forward(const float *z, int64_t ldz, const void *labels, int32_t labels_int64, const float *w, int64_t ignore_label,
                        int64_t n, int32_t C, float *lse, int32_t *pred, int64_t *hist, void *stats, float *loss, void *workspace,
                        int64_t workspace_bytes, void *stream);
int mink_seg_ce_backward(const float *z, int64_t ldz, const void *labels, int32_t labels_int64, const float *w, int64_t ignore_label,
                         const float *lse, const void *stats, const float *grad_loss, int64_t n, int32_t C, float *dz, void *stream);

/* ------------------------------------------------------------------ batch norm (csrc/batchnorm.hip)
 * MinkowskiBatchNorm == torch.nn.BatchNorm1d on the feature matrix
 * (modules/common.py:22-24; witness resnet.py:101-105), MinkowskiReLU (resnet.py:61),
 * residual `out += residual` (modules/resnet_block.py:66).
 */
int64_t mink_bn_workspace_bytes(int64_t n, int32_t C);

/* Batch statistics: mean[C], invstd[C] = 1/sqrt(biased var + eps); if running_mean !=
 * NULL also updates running stats with `momentum` (unbiased variance, torch semantics). */
int mink_bn_stats(const float *x, int64_t n, int32_t C, float eps, float momentum, float *mean,
                  float *invstd, float *running_mean, float *running_var, void *workspace, int64_t workspace_bytes,
                  void *stream);

/* y = [relu]( (x-mean)*invstd*gamma + beta [+ residual] ) */
int mink_bn_apply(const float *x, int64_t n, int32_t C, const float *mean, const float *invstd,
                  const float *gamma, const float *beta, const float *residual, int32_t relu, float *y,
                  void *stream);
/* Training-mode forward in one call: mink_bn_stats followed by mink_bn_apply (mean / invstd are
 * outputs kept for backward).  A single-launch variant for small layers (one workgroup per four
 * channels over all rows) was measured 3-9x slower than the three launches (strided 16-byte
 * column reads) and is not provided. */
int mink_bn_fwd(const float *x, int64_t n, int32_t C, float eps, float momentum, const float *gamma,
                const float *beta, const float *residual, int32_t relu, float *y, float *mean, float *invstd,
                float *running_mean, float *running_var, void *workspace, int64_t workspace_bytes, void *stream);
/* Statistics from column partials [rows][2][C] (sum, sum of squares; double) that the producer of
 * x already computed -- mink_conv_gather_gemm_stats -- instead of a reduction pass over x. */
int mink_bn_stats_from_partials(const double *partial, int32_t rows, int64_t n, int32_t C, float eps,
                                float momentum, float *mean, float *invstd, float *running_mean,
                                float *running_var, void *stream);

/* Backward of the op above.  y (the forward output) is only read when relu != 0.
 * dgamma[C], dbeta[C]; dx[n][C]; dresidual (may be NULL) receives the masked grad. */
int mink_bn_bwd(const float *dy, const float *x, const float *y, int64_t n, int32_t C, const float *mean,
                const float *invstd, const float *gamma, int32_t relu, float *dx, float *dresidual,
                float *dgamma, float *dbeta, void *workspace, int64_t workspace_bytes, void *stream);

/* Split form for MinkowskiSyncBatchNorm (train.py:106-107): per-channel sums stay on the device
 * as doubles so the host can all-reduce them (RCCL) between the passes.
 *   mink_bn_reduce mode 0: sums = [sum x | sum x^2];  mode 1: [sum g | sum g*xhat] (g masked by y>0
 *   when y != NULL).  n_total: device double (rows over all ranks). */
int mink_bn_reduce(int32_t mode, const float *a, const float *b, const float *y, int64_t n, int32_t C,
                   const float *mean, const float *invstd, double *sums, void *workspace, int64_t workspace_bytes, void *stream);
int mink_bn_stats_from_sums(const double *sums, const double *n_total, int32_t C, float eps, float momentum,
                            float *mean, float *invstd, float *running_mean, float *running_var,
                            void *stream);
int mink_bn_bwd_from_sums(const float *dy, const float *x, const float *y, int64_t n, int32_t C,
                          const double *sums, const double *n_total, const float *mean,
                          const float *invstd, const float *gamma, int32_t relu, float *dx,
                          float *dresidual, float *scratch2c, void *stream);

/* Fused tail of the stem: y_pool = SumPool(relu(BN(x))) without materialising the normalised
 * [n,C] tensor (bn1 -> relu -> pool, resnet.py:58-64).  `nbr[n_out][K]` is the 2^3 children
 * table, `in2out[n]` the stride map.  Statistics come from mink_bn_stats; the ReLU mask of the
 * backward pass is recomputed from x. */
int mink_bn_relu_pool_fwd(const float *x, int32_t C, const float *mean, const float *invstd,
                          const float *gamma, const float *beta, const int32_t *nbr, int64_t n_out,
                          int32_t K, float *y, void *stream);
int mink_bn_relu_pool_bwd(const float *dy_pool, const float *x, int64_t n, int32_t C, const float *mean,
                          const float *invstd, const float *gamma, const float *beta,
                          const int32_t *in2out, float *dx, float *dgamma, float *dbeta,
                          void *workspace, int64_t workspace_bytes, void *stream);

/* Batch-norm finalize inside the apply pass.
 * mink_bn_apply_from_partials = mink_bn_stats_from_partials + mink_bn_apply (the reference's MinkowskiBatchNorm forward,
 * co3d_3d/src/models/mink/modules/common.py:22-24) -- as ONE launch when `rows` is at most the fold limit (mink_bn_set_fold; at
 * most 128; DEFAULT 0 = never: see below), re-reading the partials in every workgroup of the pass costs at most ~8 MB in total,
 * and C is a multiple of 64: every workgroup of the apply pass sums the partial rows of its 64 channels itself, in the
 * order of the finalize kernel (results are bit-identical to the two-call sequence; mean / invstd / running statistics are
 * written by the first row chunk).  mink_bn_bwd folds its finalize into its apply pass under the same conditions.  Every
 * workgroup re-reads rows x 1 KB of partials and starts its pass behind that: measured SLOWER than the separate finalize launch
 * in every configuration (B=16: +5 % folding every layer, +-0 with the bytes rule; ResNet34 at B=4: +2.5 % with the bytes rule
 * -- DESIGN.md Appendix A), so it is off by default and kept as a tested, bit-identical option.  mink_bn_set_fold(max_rows) sets the limit (0: never; 1000 + r: r rows
 * without the total-bytes rule, for tests) and returns the previous one. */
int mink_bn_set_fold(int32_t max_rows);
/* mink_bn_bwd whose incoming gradient is still the `nslab` split-K slabs ([nslab][n][C] at dy_slabs) of the data-gradient
 * convolution that produced it (mink_conv_gather_gemm_slabs): the column-reduction pass sums them in slab order -- what
 * splitk_reduce would have written, bit for bit --, adds `addend` behind them (optional [n][C]: the gradient of a residual branch,
 * what mink_eltwise(.., 2, ..) would have added) and stores the sum to dy_sum on the way.  One or two launches and passes over
 * the gradient less per convolution backward.  C <= 1024. */
int mink_bn_bwd_slabs(const float *dy_slabs, int32_t nslab, const float *addend, float *dy_sum, const float *x, const float *y, int64_t n, int32_t C,
                      const float *mean, const float *invstd, const float *gamma, int32_t relu, float *dx, float *dresidual,
                      float *dgamma, float *dbeta, void *workspace, int64_t workspace_bytes, void *stream);
int mink_bn_apply_from_partials(const float *x, int64_t n, int32_t C, const double *partial, int32_t rows, float eps, float momentum,
                                const float *gamma, const float *beta, const float *residual, int32_t relu, float *y, float *mean,
                                float *invstd, float *running_mean, float *running_var, void *stream);

/* Few-row layers: batch norm in one launch.
 * Below mink_bn_small_rows() rows (1024; 0 when switched off with mink_bn_set_small(0)) a batch norm as three dependent launches
 * (column partials, finalize, apply: the reference's MinkowskiBatchNorm = nn.BatchNorm1d, co3d_3d/src/models/mink/modules/
 * common.py:22-24, resnet_block.py:53-69) is launch latency, not bytes.  Here a workgroup owns 16 channels and ALL rows:
 *   mink_conv_gather_gemm_slabs  mink_conv_gather_gemm that LEAVES a split launch's partial slabs in `workspace`
 *                                ([*slabs_out][n_out][cout]; *slabs_out == 1: y is complete) -- no bias
 *   mink_bn_small_fwd            y = sum of `nslab` slabs (nslab == 0: y as given) -> batch statistics (mean, invstd, running
 *                                statistics as mink_bn_stats) -> out = [relu](bn(y) [+ residual])
 *   mink_bn_small_bwd            mink_bn_bwd in one launch; nslab > 0: the incoming gradient is the sum of `nslab` slabs at
 *                                `dy` ([nslab][n][C]) plus `addend` ([n][C], optional: a residual branch's gradient),
 *                                written to dy_sum
 * C must be a multiple of 16.  Results are deterministic; the summation order differs from the three-launch form (last-bit
 * differences), which is why the module-by-module path, the yardstick of the bitwise tests, never takes these. */
int32_t mink_bn_small_rows(void);
int mink_bn_set_small(int32_t on);
int mink_bn_small_fwd(const float *slabs, int32_t nslab, int64_t n, int32_t C, float *y, float eps, float momentum,
                      const float *gamma, const float *beta, const float *residual, int32_t relu, float *out, float *mean,
                      float *invstd, float *running_mean, float *running_var, void *stream);
int mink_bn_small_bwd(const float *dy, int32_t nslab, const float *addend, float *dy_sum, const float *x, const float *y, int64_t n, int32_t C,
                      const float *mean, const float *invstd, const float *gamma, int32_t relu, float *dx, float *dresidual,
                      float *dgamma, float *dbeta, void *stream);

/* ------------------------------------------------------------------ instance norm / layer norm (csrc/norm.hip)
 * MinkowskiInstanceNorm (modules/common.py:25-26): sample b owns rows [batch_offsets[b], batch_offsets[b+1]) of x[n][C]
 * (int32 [B+1] on the device, batch_offsets[B] == n; empty samples are legal) and is normalised per channel by its own
 * mean / biased variance:  y = [relu]( (x - mean_b) * invstd_b * gamma + beta [+ residual] ),  invstd = 1/sqrt(var + eps).
 * Any C in [1, 4096] (16-byte accesses when C % 4 == 0 and every matrix is 16-byte aligned, dword accesses otherwise),
 * 1 <= B <= 65535, n < 2^31.  mean[B][C], invstd[B][C] are outputs kept for backward (0, 0 for an empty sample).
 * Three launches whatever B is, nothing is read back; sum x and sum x^2 are accumulated in double, no floating-point
 * atomics, partials combined in a fixed order: bitwise reproducible.
 *   workspace : >= mink_in_workspace_bytes(n, C, B), 8-byte aligned */
int64_t mink_in_workspace_bytes(int64_t n, int32_t C, int32_t B);
int mink_in_fwd(const float *x, int64_t n, int32_t C, const int32_t *batch_offsets, int32_t B, float eps, const float *gamma,
                const float *beta, const float *residual, int32_t relu, float *y, float *mean, float *invstd, void *workspace,
                int64_t workspace_bytes, void *stream);
/* Backward of the op above (four launches).  y (the forward output) is only read when relu != 0.
 * dx[n][C] per sample from that sample's sum g and sum g*xhat (g = dy masked by y > 0); dgamma[C], dbeta[C] summed over all
 * rows of all samples (samples added in index order); dresidual (may be NULL) receives g. */
int mink_in_bwd(const float *dy, const float *x, const float *y, int64_t n, int32_t C, const int32_t *batch_offsets, int32_t B,
                const float *mean, const float *invstd, const float *gamma, int32_t relu, float *dx, float *dresidual,
                float *dgamma, float *dbeta, void *workspace, int64_t workspace_bytes, void *stream);

/* MinkowskiLayerNorm == torch.nn.LayerNorm(C) on the feature matrix (modules/common.py:27-28): every row is normalised over
 * its C channels, 1 <= C <= 512:  y[r] = [relu]( (x[r] - mean_r) * invstd_r * gamma + beta [+ residual[r]] ).
 * One launch; the row stays in registers between the mean pass and the sum (x - mean)^2 pass (two-pass variance).
 * mean[n], invstd[n] are outputs kept for backward. */
int mink_ln_fwd(const float *x, int64_t n, int32_t C, float eps, const float *gamma, const float *beta, const float *residual,
                int32_t relu, float *y, float *mean, float *invstd, void *stream);
/* Backward (two launches): dx[n][C] per row, dresidual (may be NULL) the masked dy, dgamma[C] / dbeta[C] as per-workgroup
 * column partials (double) added in a fixed order.  workspace: >= mink_ln_workspace_bytes(n, C), 8-byte aligned. */
int64_t mink_ln_workspace_bytes(int64_t n, int32_t C);
int mink_ln_bwd(const float *dy, const float *x, const float *y, int64_t n, int32_t C, const float *mean, const float *invstd,
                const float *gamma, int32_t relu, float *dx, float *dresidual, float *dgamma, float *dbeta, void *workspace,
                int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ PowerNorm (csrc/powernorm.hip)
 * MinkowskiPowerNorm (modules/powernorm.py:246-329; `get_norm("PN")`, modules/common.py:29-30) on x[n][C] with a row pitch
 * ldx >= C (every other matrix -- y, residual, dy, dx, dresidual -- is contiguous, pitch C; the pad columns of x may hold
 * anything, NaN included: no value of them reaches a result), `groups` groups of C / groups channels (groups must divide C):
 *   r[row][g] = 1/sqrt(mean over the group's channels of x^2 + 1e-5)   xh = x * r    (the group scaling; its epsilon is fixed)
 *   training: it = ++iters[0];  var[c] = mean over rows of xh^2;  scale = it <= warmup_iters ? 1/sqrt(var + eps)
 *             : 1/sqrt(running_phi + eps) (running_phi BEFORE this step's update);  then, if it < warmup_iters,
 *             running_phi = running_phi (it-1)/it + var/it;  always running_phi = alpha_fwd running_phi + (1-alpha_fwd) var
 *   eval    : scale = 1/sqrt(running_phi + eps); no buffer changes
 *   y = [relu]( weight * (xh * scale) + bias [+ residual] )
 * Limits: 1 <= C <= 4096 (MINK_PN_MAX_C; refused beyond, before any launch), 1 <= groups <= C, n < 2^31; mink_pn_fwd and
 * mink_pn_bwd refuse n == 0 (an empty batch has no second moment), mink_pn_apply accepts it.  16-byte accesses when
 * (C / groups) % 4 == 0, ldx % 4 == 0 and x, y, residual, dy, dx, dresidual are 16-byte aligned, dword accesses otherwise; the [C] vectors
 * and rscale may have any 4-byte alignment, iters (int64 [1]) is 8-byte aligned.
 * Everything is decided on the device: iters is bumped and read there, the warm-up branch and both running_phi updates
 * happen there, nothing is read back.  Sums are accumulated in double in a fixed order and rounded once; no floating-point
 * atomics; two runs from the same state are bitwise equal.
 * Outputs kept for backward: rscale[n][groups] (r above), var[C], scale[C].  Four launches.
 *   workspace : >= mink_pn_workspace_bytes(n, C, groups), 8-byte aligned (0 from the query = a shape the family refuses) */
#define MINK_PN_MAX_C 4096
int64_t mink_pn_workspace_bytes(int64_t n, int32_t C, int32_t groups);
int mink_pn_fwd(const float *x, int32_t ldx, int64_t n, int32_t C, int32_t groups, float eps, float alpha_fwd, int64_t warmup_iters,
                const float *weight, const float *bias, const float *residual, int32_t relu, float *y, float *rscale, float *var,
                float *scale, float *running_phi, int64_t *iters, void *workspace, int64_t workspace_bytes, void *stream);
/* Eval-mode forward (three launches): rscale[n][groups] and scale[C] are outputs, as above. */
int mink_pn_apply(const float *x, int32_t ldx, int64_t n, int32_t C, int32_t groups, float eps, const float *running_phi, const float *weight,
                  const float *bias, const float *residual, int32_t relu, float *y, float *rscale, float *scale, void *stream);
/* Backward (three launches): PowerNorm's approximate derivative, then the exact one of the group scaling.  With dym = dy
 * masked by y > 0 (y is only read when relu != 0), z = xh * scale:
 *   a = dym weight - (1 - alpha_bkw) ema_gz z   (ema_gz as it is when the call is made);   ema_gz += mean over rows of a z
 *   dxh = a / sqrt(var + eps)   (the BATCH var, also after warm-up);   dx = r (dxh - xh * mean over the group of dxh xh)
 *   dweight = sum over rows of dym z;  dbias = sum over rows of dym;  dresidual (may be NULL) = dym
 * training == 0 (a forward by mink_pn_apply): a = dym weight, dxh = a * scale, ema_gz and var are not touched (may be NULL). */
int mink_pn_bwd(const float *dy, const float *x, int32_t ldx, const float *y, int64_t n, int32_t C, int32_t groups, float eps, float alpha_bkw,
                int32_t training, const float *rscale, const float *var, const float *scale, const float *weight, int32_t relu,
                float *ema_gz, float *dx, float *dresidual, float *dweight, float *dbias, void *workspace, int64_t workspace_bytes,
                void *stream);

/* ------------------------------------------------------------------ trilinear interpolation and splat (csrc/interp.hip)
 * ME.MinkowskiInterpolation (reference co3d_3d/src/data/transforms.py:472,514-521 PerlinNoise; models/mink/fcnn.py:194-208
 * `y.interpolate(x)`) and TensorField.splat (fcnn.py:186) [ME-recall of interpolation_map_weight / TensorField.splat; parity
 * unpinned: ME is absent and the reference holds no fixture for either].  Everything is fp32; conventions of the pooling
 * family above (row pitch, 16-byte or dword lanes, no floating-point atomics, fixed summation order, -1 = absent).
 *
 * A query row (b, x, y, z) of tfield[n][4] (fp32, 16-byte aligned) is read against the map of tensor stride ts whose hash
 * map is (table_keys, table_vals, cap) (values = row ids < n_rows).  Per axis lo = floor(x / ts) * ts with lo <= x < lo + ts
 * exactly, d = (x - lo) / ts; corner c (bit 0 = x, bit 1 = y, bit 2 = z) is at lo + ts with factor d where its bit is set and
 * at lo with factor 1 - d where it is clear; w[q][c] = the product of the three factors, imap[q][c] = the corner's row or -1
 * (a present corner of weight 0 keeps its row).  The batch index is (int)b; one outside 0..65534 finds nothing.  A corner
 * outside the 16-bit key range and a NaN or infinite coordinate set MINK_STATUS_RANGE in *status (a device word the caller
 * zeroes). */
int mink_interp_map_weight(const float *tfield, int64_t n, int32_t ts, const uint64_t *table_keys, const int32_t *table_vals,
                           int64_t cap, int64_t n_rows, int32_t *imap, float *w, uint32_t *status, void *stream);
/* The splat's coordinate rows: corners[8n][4] int32 = the eight corners of floor(tfield row) at tensor stride 1, listed
 * (point 0, corners 0..7), (point 1, ...), and their weights w[8n] (may be NULL).  mink_coords_build_levels /
 * mink_coords_make_keys + mink_coords_unique turn them into the map; the `inverse` they return is the splat's imap. */
int mink_splat_coords(const float *tfield, int64_t n, int32_t *corners, float *w, uint32_t *status, void *stream);
/* y[q][:] = sum over c = 0..7 (ascending, absent entries skipped) of w[q][c] * x[imap[q][c]][:]; x has n_x rows of pitch ldx.
 * Interpolation forward and splat backward. */
int mink_interp_gather(const float *x, int32_t ldx, int64_t n_x, int32_t C, const int32_t *imap, const float *w, int64_t n_q,
                       float *y, void *stream);
/* dx[i][:] = sum over j in [seg[i], seg[i+1]) of w[members[j]] * dy[members[j] >> 3][:], i < n_rows: the pairs (q, c) grouped
 * by target row as a CSR, members[n_pairs] = q * 8 + c ascending inside a segment; dy has n_q rows of pitch ldy.
 * Interpolation backward and splat forward.  A segment is summed by one wave (up to 256 pairs) or one workgroup (longer) in
 * a fixed order: two runs are bitwise equal. */
int mink_interp_segsum(const float *dy, int32_t ldy, int64_t n_q, int32_t C, const float *w, const int32_t *members,
                       const int32_t *seg, int64_t n_rows, int64_t n_pairs, float *dx, void *stream);

/* ------------------------------------------------------------------ point stage of the point classifiers (csrc/field.hip)
 * What happens on a TensorField before and after .sparse() in reference models/mink/fcnn.py:143-165 and pointnet.py:100-109.
 * Conventions of the pooling and interpolation families above (fp32, row pitch, 16-byte or dword lanes, no floating-point
 * atomics, fixed summation order, -1 = absent, a device status word for range errors).
 *
 * `y.slice(x)` at tensor stride ts (reference fcnn.py:158-161: strides 2, 8, 32, 128): idx[i] = the row of the voxel of tensor
 * stride ts that contains the float row (b, x, y, z) of tfield[n][4] (fp32, 16-byte aligned), or -1 when the map
 * (table_keys, table_vals, cap; values = row ids < n_rows) holds none.  The key is floor(floor(x) / ts) * ts per axis (floor
 * towards minus infinity for negative values too), the batch index is (int)b and one outside 0..65534 finds nothing; key
 * packing and probe sequence are those of mink_interp_map_weight.  A key outside the 16-bit range and a NaN or infinite
 * coordinate set MINK_STATUS_RANGE in *status (a device word the caller zeroes).
 * [ME-recall of SparseTensor.slice: ME composes the field's inverse mapping with the stride maps from tensor stride 1 to ts;
 * for a level derived by striding -- every level of a manager here -- that is the voxel containing the point, which is what
 * this computes directly.  Parity unpinned: ME is absent and the reference holds no fixture for it.] */
int mink_field_map(const float *tfield, int64_t n, int32_t ts, const uint64_t *table_keys, const int32_t *table_vals, int64_t cap,
                   int64_t n_rows, int32_t *idx, uint32_t *status, void *stream);
/* `ME.cat(y1.slice(x), ..., y4.slice(x))` (reference fcnn.py:158-163) in one launch, without the [n][C_s] intermediates:
 * y[i][off_s : off_s + C_s] = x_s[idx_s[i]][:], off_s = C_0 + ... + C_(s-1), for 1 <= n_src <= 8 sources; source s has rows[s]
 * rows of pitch ldx[s]; idx_s[i] < 0 (or >= rows[s]) gives zeros in that source's columns.  x, ldx, rows, C, idx are HOST arrays
 * of n_src entries; y has n rows of pitch ldy >= the sum of C.  The backward is mink_segment_sum per source over the column
 * slice dy + off_s (pitch ldy) with a CSR of the field rows grouped by voxel, rows with idx < 0 in no segment. */
int mink_field_gather_cat(int32_t n_src, const float *const *x, const int32_t *ldx, const int64_t *rows, const int32_t *C,
                          const int32_t *const *idx, int64_t n, float *y, int32_t ldy, void *stream);

/* TensorField.sparse() feature averaging (ME UNWEIGHTED_AVERAGE, resnet.py:164):
 * y[u] = mean_{j in [seg[u],seg[u+1])} x[members[j]] (members sorted by input row). */
int mink_segment_mean(const float *x, int32_t ldx, int32_t C, const int32_t *members, const int32_t *seg,
                      int64_t n_out, float *y, void *stream);
/* The plain sum over the same (members, seg) pair, in member order: the backward of SparseTensor.slice()
 * (mink_rows_gather, segmentation tail) and of mink_field_gather_cat. */
int mink_segment_sum(const float *x, int32_t ldx, int32_t C, const int32_t *members, const int32_t *seg,
                     int64_t n_out, float *y, void *stream);
/* Backward of mink_segment_mean (TensorField.sparse() of learned per-point features, reference fcnn.py:143-144,165):
 * dx[members[j]][:] = dy[u][:] / (seg[u+1] - seg[u]) for j in [seg[u], seg[u+1]), u < n_out; members[n_members] are rows of
 * dx (n_in rows of pitch lddx), each written exactly once; a member behind seg[n_out] belongs to no segment. */
int mink_segment_mean_bwd(const float *dy, int32_t ldy, int32_t C, const int32_t *members, const int32_t *seg, int64_t n_out,
                          int64_t n_members, int64_t n_in, float *dx, int32_t lddx, void *stream);

/* ------------------------------------------------------------------ generative decoders: children and pruning (csrc/generate.hip)
 * Coordinate maps a network makes and unmakes (ME.MinkowskiGenerativeConvolutionTranspose, ME.MinkowskiPruning): int32
 * coordinate rows (b, x, y, z), 16-byte aligned; feature rows as in the pooling and field families above (fp32, row pitch,
 * 16-byte lanes when C % 4 == 0 and every pitch and pointer allows, dword lanes otherwise, -1 = absent).  No atomics, and no
 * kernel waits for memory that another workgroup of the same launch writes.
 *
 * Children of the parents coords[n][4] at the even tensor stride ts: children[8 p + k] = (b, x + (k & 1) h, y + ((k >> 1) & 1) h,
 * z + ((k >> 2) & 1) h), h = ts / 2 -- the offsets of a size-2 kernel at tensor stride ts / 2, x fastest.  Parents that are
 * multiples of ts inside the 16-bit key range have children inside it (no status word); children of distinct parents are
 * distinct. */
int mink_generate_children(const int32_t *coords, int64_t n, int32_t ts, int32_t *children, void *stream);

/* Rows one workgroup of mink_prune_compact owns: row counts next to its multiples are where the compaction can go wrong. */
#define MINK_PRUNE_BLOCK 256
/* Stable compaction of the rows i < n with mask[i] != 0 (one byte per row: a torch bool tensor), n >= 1, B samples:
 *   kept[n]          : first *total entries: the kept old rows, ascending
 *   old2new[n]       : the new row of every old row, -1 for a pruned one
 *   out_coords[n][4] : first *total rows: coords of the kept rows
 *   batch_offsets[B + 1] : row ranges of the samples among the KEPT rows (the batch column of coords is non-decreasing); a
 *                      sample that lost every voxel has an empty range, batch_offsets[B] = *total
 *   total            : device int32
 * Three launches -- counts per MINK_PRUNE_BLOCK rows, one workgroup scanning the counts, the scatter -- through `workspace`
 * (mink_prune_workspace_bytes(n), 8-byte aligned). */
int64_t mink_prune_workspace_bytes(int64_t n);
int mink_prune_compact(const uint8_t *mask, const int32_t *coords, int64_t n, int32_t B, int32_t *kept, int32_t *old2new,
                       int32_t *out_coords, int32_t *batch_offsets, int32_t *total, void *workspace, int64_t workspace_bytes,
                       void *stream);
/* Forward of the pruning: y[j][:] = x[kept[j]][:], j < n_out (zeros where kept[j] is outside 0 .. n_in - 1). */
int mink_prune_gather(const float *x, int32_t ldx, int64_t n_in, int32_t C, const int32_t *kept, int64_t n_out, float *y, int32_t ldy,
                      void *stream);
/* Its backward in one pass: dx[i][:] = dy[old2new[i]][:] for a kept row, zeros for a pruned one (old2new[i] < 0), i < n_in --
 * every row of dx is written exactly once. */
int mink_prune_gather_bwd(const float *dy, int32_t ldy, int64_t n_out, int32_t C, const int32_t *old2new, int64_t n_in, float *dx,
                          int32_t lddx, void *stream);

/* ------------------------------------------------------------------ union of tensors on different maps (csrc/union.hip)
 * ME.MinkowskiUnion: the map of the union of k coordinate lists and the sum of the inputs over it (the skip of a U-shaped
 * completion net).  Conventions of the generative section above: int32 coordinate rows (b, x, y, z), 16-byte aligned; fp32
 * feature rows with a row pitch, 16-byte lanes when C % 4 == 0 and every pitch and pointer allows, dword lanes otherwise;
 * -1 = absent; no float atomics, no kernel waits for memory that another workgroup of the same launch writes, and no entry
 * point synchronises with the host. */
/* The most inputs of one union: the length of the host arrays below, not a tuning number. */
#define MINK_UNION_MAX_INPUTS 8
/* Rows one workgroup of mink_union_build's compaction owns: row counts next to its multiples are where it can go wrong. */
#define MINK_UNION_BLOCK 256
/* The union of k coordinate lists (2 <= k <= MINK_UNION_MAX_INPUTS), all at one tensor stride: list i holds n_host[i] >= 1
 * UNIQUE rows coords[i][n_i][4] with a non-decreasing batch column in [0, B) and its batch offsets batch_offsets[i][B + 1] on
 * the device; coords, batch_offsets and in2out are HOST arrays of k device pointers; sum n_i < 2^31.
 * Row order [ME-recall: ME's own union order is unpinned, ME is absent; this is the definition]: sample-major; inside a sample
 * the rows of input 0 in their order, then the rows of input 1 that no earlier input holds, in their order, and so on.
 *   out_coords[sum n_i][4]  : first *total rows: the union
 *   in2out[i][n_i]          : the union row of every row of input i (-1 only for a row the contract above excludes)
 *   out2in[k][out2in_pitch] : first *total entries of row i: the row of input i behind union row u, -1 = input i lacks it;
 *                             out2in_pitch >= sum n_i.  Entries and rows of out_coords past *total are not written.
 *   out_batch_offsets[B + 1]: row ranges of the samples in the union; a sample empty in every input has an empty range,
 *                             out_batch_offsets[B] = *total
 *   total                   : device int32
 * A hash of all sum n_i rows on the packed 64-bit keys, the first occurrence in (input, row) order winning its slot as in
 * mink_coords_unique, then counts per MINK_UNION_BLOCK positions, one workgroup scanning the counts, the scatter, the rows
 * that lost, the offsets: separate launches through `workspace` (mink_union_workspace_bytes, 8-byte aligned; -1 and an
 * error text for counts mink_union_build refuses). */
int64_t mink_union_workspace_bytes(int32_t k, const int64_t *n_host, int32_t B);
int mink_union_build(int32_t k, const int32_t *const *coords, const int32_t *const *batch_offsets, const int64_t *n_host, int32_t B,
                     int32_t *out_coords, int32_t *const *in2out, int32_t *out2in, int64_t out2in_pitch, int32_t *out_batch_offsets,
                     int32_t *total, void *workspace, int64_t workspace_bytes, void *stream);
/* y[u][:] = the sum over the inputs that hold union row u (out2in[i][u] >= 0), u < n_out, taken in ascending input index: the
 * first one present is copied -- a row held by one input comes out bit for bit, -0.0 included -- and the later ones are added
 * to it in fp32, so the result is a pure function of the inputs; NaN and infinities reach only the union rows their input
 * row maps to.  x and ldx_host / n_host are host arrays of k device pointers / row pitches / row counts; pad columns of y are
 * not written; n_out == 0 returns without a launch.  Backward: dx_i[r][:] = dy[in2out[i][r]][:], which is mink_prune_gather
 * with kept = in2out[i]. */
int mink_union_sum(int32_t k, const float *const *x, const int32_t *ldx_host, const int64_t *n_host, int32_t C, const int32_t *out2in,
                   int64_t out2in_pitch, int64_t n_out, float *y, int32_t ldy, void *stream);

/* ------------------------------------------------------------------ elementwise (csrc/elementwise.hip) */
/* Elementwise: mode 0: y = max(x,0); mode 1: dx = (y>0) ? dy : 0 (a=dy,b=y);
 * mode 2: y = a + b. */
int mink_eltwise(const float *a, const float *b, int64_t count, int32_t mode, float *y, void *stream);

/* Pointwise activations beyond ReLU -- ME.MinkowskiLeakyReLU / ELU / CELU / SELU / GELU / PReLU, which the reference's
 * layer factory lists at import time (co3d_3d/src/models/mink/modules/common.py:36-43) and MinkowskiFunctional mirrors
 * (:56-71).  kind: 1 leaky-ReLU (alpha = negative slope), 2 ELU(alpha), 3 CELU(alpha), 4 SELU, 5 GELU (erf form),
 * 6 PReLU (`slope`: C per-channel weights, or one shared weight when C == 1; channels are the fastest axis).
 * gy == NULL: out = f(x) over `count` elements; otherwise out = gy * f'(x). */
int mink_activation(const float *x, const float *gy, const float *slope, int32_t C, int64_t count, int32_t kind,
                    float alpha, float *out, void *stream);

/* Optimizer step over flat buffers.
 * torch.optim.SGD's update with momentum and weight decay (the reference's optimizer: co3d_3d/src/modules/optim.py:12-14,
 * co3d_3d/configs/co3d_cls.gin) for parameters w, gradients g and momentum buffers m that each live in ONE flat fp32 buffer of
 * the same layout (n floats, a multiple of 4; padding elements are zero and stay zero):
 *   g' = g + weight_decay w;  m = momentum m + g';  w = w - lr m        (dampening 0, no Nesterov; a zero m = torch's first step)
 * zero_grad != 0 clears g behind the update (the next step's zero_grad memset).  One pass over 6 n floats. */
int mink_sgd_step(float *w, float *g, float *m, int64_t n, float lr, float momentum, float weight_decay, int32_t zero_grad, void *stream);

/* ------------------------------------------------------------------ dataset front-end (csrc/plenoxel.hip)
 * PeRFception-CO3D `data.npz` batch on the device (reference co3d.py:160-166 de-quantisation,
 * :196-205 links -> coordinates and feature selection): `links[n]` flat indices x*ry*rz + y*rz + z,
 * `density[n]`, `sh_q[n][27]` uint8, per scene b (rows scene_offsets[b] .. scene_offsets[b+1])
 * `sh_scale[b][27]`, `sh_min[b][27]`.  Writes coords int32 [n][4] = (b, x, y, z) and the selected
 * feature columns: density at col_density, the 27 de-quantised SH coefficients at col_sh, ones at
 * col_ones, the three "xyzs" columns at col_xyzs (-1 = not selected; the columns must tile 0..C-1).
 * sh = float(sh_q) * scale + min with separate multiply and add, bit-identical to the numpy expression of
 * the reference.  xyzs (co3d.py:209-214, `configs/feature_coord.gin`): every point minus the mean of its own
 * three coordinates, divided by the largest such norm of its scene -- a per-scene reduction, done in a
 * first pass into scene_scratch[n_scenes] (required when col_xyzs >= 0); every operation rounded separately. */
int mink_decode_plenoxel(const int32_t *links, const float *density, const uint8_t *sh_q,
                         const int32_t *scene_offsets, int32_t n_scenes, const float *sh_scale,
                         const float *sh_min, int64_t n, int32_t reso_y, int32_t reso_z, int32_t col_density,
                         int32_t col_sh, int32_t col_ones, int32_t col_xyzs, float *scene_scratch, int32_t C,
                         int32_t *coords, float *feats, int32_t ldf, void *stream);

/* ------------------------------------------------------------------ scene augmentation (csrc/augment.hip)
 * The reference augments every scene on the CPU in its DataLoader workers (co3d.py:216-219 applies
 * transforms.Compose of the gin-listed classes of transforms.py; configs/co3d_aug3.gin:2-23).  Here
 * the host only DRAWS the per-scene randomness and the whole batch is transformed on the device.
 * Per scene b a row of MINK_AUG_PARAMS floats (all matrices row-major, applied as row-vector * M):
 *     p = c * A + a                          stages before the flip (rotation, affine, ...)
 *     q_j = FLIP[j] ? max_j - p_j : p_j      max over the scene's surviving voxels (over all voxels
 *                                            when FLIP_ALL != 0: dropout listed after the flip)
 *     r = q * B + b + jitter * BJ            jitter_j = JITTER * (u_j - 0.5), u uniform [0,1)
 *     voxel kept iff u >= DROPOUT            (CoordinateDropout; 0 keeps everything)
 *     feats[:, raw column in [FEAT_START, FEAT_START + FEAT_DIM)] += (normal - 0.5) * FEAT_STD
 * (transforms.py: RandomRotation :351-358, RandomAffine :416-427, CoordinateDropout :255-265,
 * RandomHorizontalFlip :444-450, CoordinateUniformTranslation :288-294, CoordinateJitter :276-281,
 * RandomScale :367-373, RandomFeatureJitter :34-41.)  Differences from the reference, by design:
 * the dropout is an independent coin per voxel and keeps the voxel order (the reference draws an
 * exact-size random subset in random order); the per-voxel random numbers are Philox4x32-10 with
 * key = seed, counter = (voxel index in its scene, draw, streams[b], 0): draw 0 -> (dropout u, jitter
 * u_x, u_y, u_z), draw 1+j/4 -> four Box-Muller normals for noise columns 4(j/4)..4(j/4)+3.
 * Coordinates are computed in fp32 with every product and sum rounded separately, in the order
 * ((v0*M0j + v1*M1j) + v2*M2j) + t_j, so a CPU restatement reproduces them bit for bit. */
enum {
  MINK_AUG_A = 0,           /* 9 */
  MINK_AUG_a = 9,           /* 3 */
  MINK_AUG_FLIP = 12,       /* 3 flags */
  MINK_AUG_B = 15,          /* 9 */
  MINK_AUG_b = 24,          /* 3 */
  MINK_AUG_BJ = 27,         /* 9 */
  MINK_AUG_JITTER = 36,     /* 2 * jitter_std, 0 = none */
  MINK_AUG_DROPOUT = 37,    /* dropout ratio, 0 = none */
  MINK_AUG_FEAT_STD = 38,   /* 0 = none */
  MINK_AUG_FEAT_START = 39, /* raw-layout column, co3d.py:205-214: [xyzs 0:3 | density 3 | sh 4:31] */
  MINK_AUG_FEAT_DIM = 40,
  MINK_AUG_FLIP_ALL = 41,
  MINK_AUG_PARAMS = 44,
  MINK_AUG_MAX_CHANNELS = 32
};

int64_t mink_augment_workspace_bytes(int64_t n, int32_t n_scenes);

/* coords [n][4] (batch, x, y, z) sorted by batch, float32 or -- coords_are_int32 -- int32 as written by
 * mink_decode_plenoxel; feats [n][ldf] (C columns used);
 * scene_offsets [n_scenes+1], params [n_scenes][MINK_AUG_PARAMS], streams [n_scenes] on the device.
 * raw_cols[C] is a HOST array: the raw-layout column of every feature column (-1 = never jittered).
 * Writes the survivors, in order, to out_coords [>= n][4] / out_feats [>= n][ldo] and their number
 * to the device int *n_kept (n_kept == n whenever every DROPOUT is 0: no read-back needed then). */
int mink_augment_scenes(const void *coords, int32_t coords_are_int32, const float *feats, int64_t ldf, int32_t C, int64_t n,
                        const int32_t *scene_offsets, int32_t n_scenes, const float *params,
                        const uint32_t *streams, uint64_t seed, const int32_t *raw_cols, float *out_coords,
                        float *out_feats, int64_t ldo, int32_t *n_kept, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ segmentation scene augmentation (csrc/seg_augment.hip)
 * The PeRFception-ScanNet recipe of the reference (configs/scannet_plenoxel.gin: RandomRotation, RandomCrop, RandomAffine,
 * CoordinateDropout, RandomFeatureJitter, RandomHorizontalFlip, RandomTranslation, ElasticDistortion) as one device program
 * per scene.  Its own parameter row: MINK_SEGAUG_PARAMS DOUBLES per scene (matrices row-major, applied as row-vector * M):
 *     p = c * A0 + a0                          stages before the crop
 *     crop (CROP != 0; transforms.py:194-244): n = p - min(p), range = max(max(n) - CROP_SIZE, 0) per axis, over every row
 *         of the scene.  range == 0 on all axes: no crop.  Else box k < CROP_TRIES: lo = CROP_U[k] * range,
 *         hi = lo + CROP_SIZE, keeps the rows with lo < n < hi on every axis; the first box that keeps a row wins; none: no crop
 *     q = p * A1 + a1                          stages between the crop and the flip
 *     kept = in crop && u >= DROPOUT           (the dropout coin u of MINK_AUG; crop first: dropout after the crop)
 *     q_j = FLIP[j] ? max_j - q_j : q_j        max over the rows alive at the flip: in crop && u >= DROPOUT
 *                                              (in crop only when FLIP_ALL != 0: dropout listed after the flip)
 *     r = q * B + b                            stages after the flip
 *     elastic pass e < MINK_SEGAUG_MAX_ELASTIC with g = ELASTIC[2e] > 0, m = ELASTIC[2e+1] (transforms.py:535-594), over the
 *         kept rows: lo = min(r), dim = floor((max(r) - lo) / g) + 3 per axis; noise [dim][3] ~ N(0,1) blurred by
 *         Bx^2 By^2 Bz^2 (B = 3-tap box 1/3, zero outside the grid); r += m * trilinear(noise; node i at lo - g + i g; 0 outside the grid's box)
 *     feats[:, raw column in [FEAT_START, FEAT_START + FEAT_DIM)] += (normal - 0.5) * FEAT_STD     (as MINK_AUG)
 * Coordinates are computed in double -- p, q and r with every product and sum rounded, in the order
 * ((v0*M0j + v1*M1j) + v2*M2j) + t_j, so a float64 restatement reproduces the crop decision exactly -- and written as float.
 * Every min / max is an order-preserving integer atomic: results are bitwise identical run to run.
 * Philox4x32-10 with key = seed.  Per row: counter (row in scene, draw, streams[b], 0), as MINK_AUG (draw 0 -> dropout coin,
 * draw 1+j/4 -> feature noise).  Grid node (ix, iy, iz) of elastic pass e: counter (ix | iy << 16, iz | e << 16, streams[b], 1);
 * words (0,1) -> Box-Muller -> noise x, y; words (2,3) -> noise z (cosine branch); u1 = (w >> 8) + 1 over 2^24, so |noise| <= 5.77.
 * The noise grids live in the workspace at capacities the caller sizes on the host: GRID_BOUND[3] per scene (a bound of dim
 * over the scene's passes), grid_nodes = sum over the scenes of GRID_BOUND[0] * GRID_BOUND[1] * GRID_BOUND[2].  A pass whose
 * dim exceeds its scene's bound stores no grid (nothing is written past the bound): the displacement of each point is then
 * evaluated from the Philox noise of the 6^3 nodes around it -- the same values -- and the pass is counted in status[1].
 * A dim over 65535 (nodes that cannot be keyed) or a non-finite extent: the pass is not applied, counted in status[2].
 * EXTENT (the raw per-axis extent of the scene) is read by the host only, to compute GRID_BOUND. */
enum {
  MINK_SEGAUG_A0 = 0,          /* 9 */
  MINK_SEGAUG_a0 = 9,          /* 3 */
  MINK_SEGAUG_CROP = 12,       /* 1 = RandomCrop drawn */
  MINK_SEGAUG_CROP_SIZE = 13,  /* 3 */
  MINK_SEGAUG_CROP_TRIES = 16, /* boxes drawn, <= MINK_SEGAUG_MAX_TRIES */
  MINK_SEGAUG_CROP_U = 17,     /* [MINK_SEGAUG_MAX_TRIES][3] uniform [0,1) */
  MINK_SEGAUG_A1 = 65,         /* 9 */
  MINK_SEGAUG_a1 = 74,         /* 3 */
  MINK_SEGAUG_DROPOUT = 77,    /* dropout ratio, 0 = none */
  MINK_SEGAUG_FLIP = 78,       /* 3 flags */
  MINK_SEGAUG_FLIP_ALL = 81,
  MINK_SEGAUG_B = 82,          /* 9 */
  MINK_SEGAUG_b = 91,          /* 3 */
  MINK_SEGAUG_FEAT_STD = 94,   /* 0 = none */
  MINK_SEGAUG_FEAT_START = 95, /* raw-layout column; ScanNet: [xyzs 0:3 | dists 3 | density 4 | sh 5:32] */
  MINK_SEGAUG_FEAT_DIM = 96,
  MINK_SEGAUG_ELASTIC = 97,    /* [MINK_SEGAUG_MAX_ELASTIC][2] (granularity, magnitude); granularity 0 = no pass */
  MINK_SEGAUG_GRID_BOUND = 101, /* 3 */
  MINK_SEGAUG_EXTENT = 104,    /* 3, host only */
  MINK_SEGAUG_PARAMS = 108,
  MINK_SEGAUG_MAX_TRIES = 16,
  MINK_SEGAUG_MAX_ELASTIC = 2
};

int64_t mink_augment_seg_workspace_bytes(int64_t n, int32_t n_scenes, int64_t grid_nodes);

/* coords [n][4] (batch, x, y, z) sorted by batch, float32 or (coords_are_int32) int32; feats [n][ldf] (C columns used);
 * scene_offsets [n_scenes+1], params [n_scenes][MINK_SEGAUG_PARAMS] (double), streams [n_scenes] on the device;
 * raw_cols[C] a HOST array as for mink_augment_scenes.  n_elastic = elastic passes to run (the largest over the scenes),
 * grid_nodes as above.  Writes the survivors, in order, to out_coords [>= n][4], out_feats [>= n][ldo] and the source row
 * of every survivor to out_rows [>= n]; the device int32 status[3] receives (survivors, elastic passes evaluated without a
 * stored grid, elastic passes not applied). */
int mink_augment_seg_scenes(const void *coords, int32_t coords_are_int32, const float *feats, int64_t ldf, int32_t C, int64_t n,
                            const int32_t *scene_offsets, int32_t n_scenes, const double *params, const uint32_t *streams,
                            uint64_t seed, const int32_t *raw_cols, int32_t n_elastic, int64_t grid_nodes, float *out_coords,
                            float *out_feats, int64_t ldo, int32_t *out_rows, int32_t *status, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ point-cloud voxel down-sampling (csrc/points.hip)
 * ME.utils.sparse_quantize(xyz, colours, labels=labels, quantization_size=Q, return_index=True, ignore_label=IGNORE) as the
 * reference's ScannetDataset calls it on every scene (co3d_3d/src/data/scannet.py:233-247), for a whole batch.  One parameter
 * row per scene, MINK_VOXDS_PARAMS doubles: Q (quantisation size; 0 = no down-sampling), VOXEL (voxel size), IGNORE (label).
 * Within each scene:
 *     key            (b, floor(f32(x) / f32(Q)), floor(f32(y) / f32(Q)), floor(f32(z) / f32(Q))); Q == 0: every row its own voxel
 *     representative the FIRST row of each voxel in input-row order; the representatives are ordered by that first row
 *     label          the common raw label of the voxel's rows, IGNORE as soon as two of them differ (int32 min / max atomics)
 *     coordinates    (b, f32(x[rep]) / f32(VOXEL), ...)  -- continuous, as scannet.py:244
 * ME leaves the representative and the row order unspecified (its CPU and GPU backends differ); first row, first-row
 * order is this project's convention.  A spatial key outside [-32768, 32767] sets MINK_STATUS_RANGE in status[1] (that
 * voxel's rows are then numbered with the clamped key: the output is not valid). */
enum {
  MINK_VOXDS_Q = 0,
  MINK_VOXDS_VOXEL = 1,
  MINK_VOXDS_IGNORE = 2,
  MINK_VOXDS_PARAMS = 4
};

int64_t mink_voxel_downsample_workspace_bytes(int64_t n);

/* coords [n][4] float32 (batch, x, y, z), sorted by batch; feats [n][ldf] (C columns used); labels [n] int32; scene_offsets
 * [n_scenes+1] and params [n_scenes][MINK_VOXDS_PARAMS] on the device.  Writes the representatives, in order, to
 * out_coords [n][4], out_feats [n][ldo], out_labels [n] and their input rows to out_rows [n]; out_offsets [n_scenes+2]
 * receives the row range of every scene's representatives, with out_offsets[n_scenes+1] = n (the unused tail counts as one
 * more scene); the device int32 status[2] receives (representatives, MINK_STATUS_* bits). */
int mink_voxel_downsample_scenes(const float *coords, const float *feats, int64_t ldf, int32_t C, const int32_t *labels, int64_t n,
                                 const int32_t *scene_offsets, int32_t n_scenes, const double *params, float *out_coords,
                                 float *out_feats, int64_t ldo, int32_t *out_labels, int32_t *out_rows, int32_t *out_offsets,
                                 int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ colour program (csrc/points.hip)
 * The reference's colour stages (co3d_3d/src/data/transforms.py:44-122: ChromaticTranslation, ChromaticJitter,
 * NormalizeColor) as an ordered list of at most MINK_COLORAUG_MAX_OPS ops per scene, applied to the 3 colour columns
 * cols[0..2] of rows [0, scene_offsets[n_scenes]) (scene_offsets [n_scenes+1] on the device; rows past it are not touched).
 * Row of MINK_COLORAUG_PARAMS doubles: COUNT ops, op k at OPS + k * MINK_COLORAUG_OP_STRIDE = (kind, arguments...):
 *     TRANSLATE (t0, t1, t2)             c = f32(clip(c + t_j, 0, 255))          (double sum)
 *     JITTER    (sigma)                  c = f32(clip(c + sigma * N(0,1), 0, 255)) (double), sigma = std * 255
 *     NORMALIZE (m0, m1, m2, s0, s1, s2) c = (c - f32(m_j)) / f32(s_j)            (float)
 * The jitter normals are Philox4x32-10 with key = seed, counter (key_rows[i] - key_offsets[b], k, streams[b], 2) for op k
 * of row i in scene b: words (0,1) -> Box-Muller -> N_0, N_1, words (2,3) -> N_2 (cosine branch), u1 = ((w >> 8) + 1) / 2^24.
 * key_rows [n] (int32) names the row a jitter is keyed by, key_offsets [n_scenes+1] the first key row of every scene. */
enum {
  MINK_COLORAUG_COUNT = 0,
  MINK_COLORAUG_OPS = 1,
  MINK_COLORAUG_OP_STRIDE = 8,
  MINK_COLORAUG_MAX_OPS = 4,
  MINK_COLORAUG_PARAMS = 33,
  MINK_COLORAUG_TRANSLATE = 1,
  MINK_COLORAUG_JITTER = 2,
  MINK_COLORAUG_NORMALIZE = 3
};

int mink_color_augment_scenes(float *feats, int64_t ldf, const int32_t *cols_host, int64_t n, const int32_t *scene_offsets,
                              int32_t n_scenes, const double *params, const uint32_t *streams, uint64_t seed,
                              const int32_t *key_rows, const int32_t *key_offsets, void *stream);

/* ------------------------------------------------------------------ LiDAR scans (csrc/lidar.hip)
 * What the reference's SemanticKITTIDataset (co3d_3d/src/data/semantic_kitti.py:165-222) does to a raw scan around the
 * down-sampling and the recipe, for a whole batch.  Both are row passes: one thread per row, 16-byte row accesses when every
 * pointer and pitch involved is a multiple of 16 bytes and dwords otherwise, every output element written once from its own
 * row's inputs (bitwise repeatable).
 *
 * mink_lidar_decode_scans: scan [n][4] float32 is the .bin file (x, y, z, intensity), raw_labels [n] the .label words, or
 * NULL = every word 0 (a scan without its .label file); scene_offsets [n_scenes+1], lut [lut_size] on the device.  Writes
 *     coords [n][4]   = (scene of the row, x, y, z)
 *     feats  [n][ldo] = x, y, z, intensity in columns 0..3 (ldo >= 4; further columns are not touched)
 *     labels [n]      = lut[word & 0xFFFF]   -- the table comes BEFORE the voxel vote (:183-196), the upper 16 bits (the
 *                       instance id) are dropped; a semantic id >= lut_size gets ignore_label and is counted
 * and the device int32 *status = the number of rows whose semantic id the table does not hold (zeroed by the call; the
 * reference raises an IndexError there).  n == 0 and empty scenes are legal.
 *
 * mink_lidar_finish_rows: the step after the geometric program (:200-209), in place, for every row i < min(n, *n_rows) with
 * n_rows a DEVICE int32 (the survivor count mink_augment_seg_scenes or mink_voxel_downsample_scenes left in its status):
 *     feats[i][c0 .. c0+2] = coords[i][1..3]                  the transformed metric coordinates, as float
 *     coords[i][1..3]      = coords[i][1..3] / voxel_size     one IEEE float division (as mink_voxel_downsample_scenes' VOXEL)
 * Rows at or past the count are neither read nor written.  In the 16-byte form (coords and feats 16-byte aligned, ldf % 4 == 0,
 * c0 % 4 == 0) a row's coords[i][0] and feats[i][c0+3] are stored back with the bits that were read; in the dword form they are
 * not touched.  Both calls refuse (MINK_EINVAL) operands whose byte ranges overlap -- scan / raw_labels against coords [n][4],
 * feats [n][ldo] and labels, and those three against each other; coords, feats [n][ldf] and n_rows here.  The program computes in double and writes float, so the voxel
 * coordinate is f32(r) / f32(voxel_size): without a recipe bit for bit the reference's float32 array / python float; with
 * one the reference divides in double before its single rounding, which can differ by one float ulp. */
int mink_lidar_decode_scans(const float *scan, const uint32_t *raw_labels, int64_t n, const int32_t *scene_offsets, int32_t n_scenes,
                            const int32_t *lut, int32_t lut_size, int32_t ignore_label, float *coords, float *feats, int64_t ldo,
                            int32_t *labels, int32_t *status, void *stream);
int mink_lidar_finish_rows(float *coords, int64_t n, const int32_t *n_rows, float voxel_size, float *feats, int64_t ldf, int32_t c0,
                           void *stream);

/* ------------------------------------------------------------------ images: AugMix chains and the 2-D recipe (csrc/image.hip)
 * What the reference's 2-D loader does to a decoded frame (co3d_2d/src/data/loader.py:100-107, augmix.py:184-215,
 * transforms.py), for a whole batch, with Pillow's arithmetic: every 8-bit result below is the integer Pillow computes, the
 * float result follows torch's float32 operations one by one.  The host decodes and draws; the device applies.
 *
 * A batch: `packed`, the uint8 HWC RGB images of the B samples one after the other (any sizes, any byte alignment);
 * `offsets` [B+1] int64, the BYTE offset of every image in `packed` (offsets[0] = 0, offsets[b+1] - offsets[b] = 3 * w * h,
 * offsets[B] = 3 * total_pixels); `sizes` [B][2] int32 = (w, h), w * h < 2^31; `programs` [B][MINK_IMG_PARAMS] double, all on the device.
 * A sample whose offsets, sizes or boxes do not fit is not read: its chain buffers stay as they are and its output is NaN.
 *
 * The program row of a sample:
 *     [WIDTH]              chains of this sample, 0 .. MINK_IMG_MAX_WIDTH and <= the call's `width` (0: evaluation, out = pre_0)
 *     [M]                  m (a float32), out = (1 - m) * pre_0(x) + m * mix
 *     [WS + i - 1]         ws_i (float32) of chain i = 1 .. WIDTH: mix = ((0 + ws_1 * pre_1) + ws_2 * pre_2) + ..., in that order
 *     [BRANCH + k * BRANCH_STRIDE + ...]  branch k = 0 .. WIDTH; branch 0 is the untouched image, branch i >= 1 chain i:
 *       B_DEPTH            ops of the chain, 0 .. MINK_IMG_MAX_DEPTH (ignored for branch 0)
 *       B_OPS + r * OP_STRIDE = (kind, p0 .. p5) of round r: AUTOCONTRAST, EQUALIZE (no arguments; per-channel tables from the
 *                          histogram), POSTERIZE (p0 = bits kept: v & ~(2^(8-bits) - 1)), SOLARIZE (p0 = t: v < t ? v : 255 - v),
 *                          ROTATE, SHEAR_X/Y, TRANSLATE_X/Y (p0 .. p5 = the affine matrix a0 .. a5 the host built: output pixel
 *                          (x, y) reads xin = a0 (x + .5) + a1 (y + .5) + a2, yin = a3 (x + .5) + a4 (y + .5) + a5, BILINEAR,
 *                          zero outside [0, w) x [0, h), in double, truncated to 8 bits)
 *       B_BOX              x0, y0, w, h of the crop, inside the image
 *       B_TARGET           OW, OH: the crop is resized to OW x OH (BILINEAR, horizontal pass first, 8 bits after each pass, the
 *                          taps clipped to the crop, coefficients of 22 fractional bits) ...
 *       B_WINDOW           wx, wy: ... of which the S x S window at (wx, wy) is kept (RandomResizedCrop: OW = OH = S, window 0, 0;
 *                          CenterCrop: shorter side S, the centred window)
 *       B_ORDER            three slots, each a MINK_IMG_JIT_* or 0: the ColorJitter steps in the drawn order, uint8 to uint8
 *       B_FACTORS          brightness, saturation, hue factor (read by the slots that name them)
 *       B_FLIP             != 0: mirror the columns
 *       B_RGB              r, g, b of the PCA lighting (float32), added after / 255; then (x - mean) / std of the CO3D statistics
 *
 * mink_img_workspace_bytes: the scratch of both calls for a batch of total_pixels pixels, B samples and at most `width` chains
 * per sample (independent of S): histograms [B][width][3][256] int32, tables [B][width][3][256] uint8 and, per chain, two
 * images of the whole batch, A and B.  Round 0 reads `packed` and writes A, round 1 reads A and writes B, round 2 reads B and
 * writes A: mink_img_chain_buffer_offset(total_pixels, B, width, chain i >= 1, depth d >= 1) is the byte offset in the workspace
 * of the batch of chain i after d ops (laid out like `packed`), -1 for arguments outside those ranges.
 *
 * mink_img_chain_round: round r = 0, 1, 2 of every chain of the batch, three launches (histograms of the chains whose op of this
 * round needs one: LDS sub-histograms with equal bins of a wave merged before the atomic, integer sums only; the tables; one
 * apply pass of 16-byte stores with scalar head and tail).  Chains with depth <= r are skipped.  Rounds run in order on one stream.
 *
 * mink_img_finish: out [B][3][S][S] float32, every element written once; one workgroup owns a tile of the output of one sample
 * and walks branch 0 .. WIDTH in order, accumulating in registers (no atomics: two calls agree bit for bit).  `stages`, when
 * not NULL, is uint8 [B][width + 1][S][S][3] and receives the 8-bit image of branch k <= WIDTH after the flip (further
 * branches are not written).  No product of the float and double expressions above is fused with an addition. */
enum {
  MINK_IMG_MAX_WIDTH = 3,
  MINK_IMG_MAX_DEPTH = 3,
  MINK_IMG_OP_AUTOCONTRAST = 1,
  MINK_IMG_OP_EQUALIZE = 2,
  MINK_IMG_OP_POSTERIZE = 3,
  MINK_IMG_OP_ROTATE = 4,
  MINK_IMG_OP_SOLARIZE = 5,
  MINK_IMG_OP_SHEAR_X = 6,
  MINK_IMG_OP_SHEAR_Y = 7,
  MINK_IMG_OP_TRANSLATE_X = 8,
  MINK_IMG_OP_TRANSLATE_Y = 9,
  MINK_IMG_JIT_BRIGHTNESS = 1,
  MINK_IMG_JIT_SATURATION = 2,
  MINK_IMG_JIT_HUE = 3,
  MINK_IMG_WIDTH = 0,
  MINK_IMG_M = 1,
  MINK_IMG_WS = 2,
  MINK_IMG_BRANCH = 5,
  MINK_IMG_BRANCH_STRIDE = 40,
  MINK_IMG_B_DEPTH = 0,
  MINK_IMG_B_OPS = 1,
  MINK_IMG_OP_STRIDE = 7,
  MINK_IMG_B_BOX = 22,
  MINK_IMG_B_TARGET = 26,
  MINK_IMG_B_WINDOW = 28,
  MINK_IMG_B_ORDER = 30,
  MINK_IMG_B_FACTORS = 33,
  MINK_IMG_B_FLIP = 36,
  MINK_IMG_B_RGB = 37,
  MINK_IMG_PARAMS = 165
};

int64_t mink_img_workspace_bytes(int64_t total_pixels, int32_t B, int32_t width, int32_t S);
int64_t mink_img_chain_buffer_offset(int64_t total_pixels, int32_t B, int32_t width, int32_t chain, int32_t depth);
int mink_img_chain_round(const uint8_t *packed, const int64_t *offsets, const int32_t *sizes, const double *programs,
                         int64_t total_pixels, int32_t B, int32_t width, int32_t round, void *workspace, int64_t workspace_bytes,
                         void *stream);
int mink_img_finish(const uint8_t *packed, const int64_t *offsets, const int32_t *sizes, const double *programs,
                    int64_t total_pixels, int32_t B, int32_t width, int32_t S, const void *workspace, int64_t workspace_bytes,
                    float *out, uint8_t *stages, void *stream);

/* ------------------------------------------------------------------ images: background paste (csrc/paste.hip)
 * The reference's BackgroundAug (co3d_2d/src/data/transforms.py:113-159) for a whole batch, IN PLACE in the packed batch of the
 * section above, before its chain rounds: the slot of a pasting sample holds the background frame on entry and the composite on
 * exit.  `packed`, `offsets`, `sizes` as above; `fg`, uint8 [fg_bytes], the HWC RGB frames to paste and `mask`, uint8
 * [mask_bytes], their mask planes (one byte per pixel), both packed at any byte alignment and neither overlapping `packed`;
 * `table` [B][MINK_PASTE_PARAMS] int64 on the device, per sample
 *     FG_OFFSET, MASK_OFFSET   byte offset of its frame in `fg` and of its mask in `mask`
 *     FG_W, FG_H               size of the frame
 *     MASK_W, MASK_H           size of the mask (it need not be the frame's)
 *     RW, RH                   the size both are resized to; RW = 0: the sample does not paste and nothing of it is touched
 * Frame and mask are resized as Image.resize((RW, RH)) does with Pillow's default filter: BICUBIC (a = -0.5, support
 * 2 * max(in / out, 1)), horizontal pass first, 8 bits after each pass, coefficients of 22 fractional bits rounded half away
 * from zero; a pass whose side does not change copies.  With (w, h) the slot's size the rectangle rows [y0, y1) =
 * [max(0, (h - RH) / 2), min(h, (h + RH) / 2)) -- columns alike -- receives
 *     out = (uint8) (fg * m + (1 - m) * bg),   m = mask / 255
 * in double, no product fused with the addition, where fg and mask are read from row RH / 2 - (y1 - y0) / 2 of the resized
 * images on.  Every other byte of `packed` keeps its value.  One workgroup owns a tile of one rectangle and a thread its own
 * pixels: no atomics, two calls agree bit for bit.
 *
 * max_w, max_h: HOST scalars, the largest rectangle extent of the batch per axis (they size the grid; nothing is read back).
 * Either 0: no sample pastes and nothing is launched.  A sample whose row does not fit -- offsets outside `fg` / `mask`, a side
 * outside 1 .. MINK_PASTE_MAX_SIDE, a slot that is not the one `offsets` and `sizes` describe, a rectangle larger than
 * max_w x max_h -- is skipped whole: nothing of it is read or written. */
enum {
  MINK_PASTE_FG_OFFSET = 0,
  MINK_PASTE_MASK_OFFSET = 1,
  MINK_PASTE_FG_W = 2,
  MINK_PASTE_FG_H = 3,
  MINK_PASTE_MASK_W = 4,
  MINK_PASTE_MASK_H = 5,
  MINK_PASTE_RW = 6,
  MINK_PASTE_RH = 7,
  MINK_PASTE_PARAMS = 8,
  MINK_PASTE_MAX_SIDE = 1048576
};

int mink_img_paste(uint8_t *packed, const int64_t *offsets, const int32_t *sizes, int64_t total_pixels, int32_t B, const uint8_t *fg,
                   int64_t fg_bytes, const uint8_t *mask, int64_t mask_bytes, const int64_t *table, int32_t max_w, int32_t max_h,
                   void *stream);

/* ------------------------------------------------------------------ whole residual blocks (csrc/trunk.hip)
 * One call = the complete launch sequence of one stage of the reference network, so the host pays one FFI call per
 * block instead of one per kernel (a Mink-ResNet14 step is ~300 launches; issued one by one from a Python autograd
 * graph the host, not the GPU, was the bottleneck).  Same kernels, same order, same results as the per-operator
 * entry points above -- these functions only sequence them:
 *
 *   mink_stem_forward/backward   conv1 -> bn1 -> relu -> SumPooling(2,2)            (models/mink/resnet.py:58-64,163-166)
 *   mink_block_forward/backward  BasicBlock: conv1-norm1-relu-conv2-norm2 (+downsample(x) or x) -relu
 *                                                                                   (modules/resnet_block.py:53-69)
 *
 * Three streams take part (any two may be the same stream): `compute` runs the chain, `branch` runs the shortcut
 * (1x1x1 strided convolution + norm) beside it, `wgrad` runs the weight gradients beside the data-gradient chain.
 * Cross-stream ordering inside a call uses events owned by the library; on return everything the NEXT call on
 * `compute` needs is ordered on `compute`, EXCEPT the weight gradients (dw of every convolution), which are complete
 * on `wgrad` -- the caller joins `wgrad` once, at the end of the backward pass.  Buffers must stay alive until then.
 * Batch norm runs in training mode (batch statistics; running statistics updated in place when given). */
typedef struct {
  const float *w;        /* [K][cin][cout] */
  float *dw;             /* backward: weight gradient [K][cin][cout] (written, not accumulated) */
  const int32_t *nbr;    /* [n_out][K] neighbour table in -> out */
  const int32_t *nbr_t;  /* backward, stride > 1: transposed table [n_in][K]; NULL for stride 1 (the flipped table) */
  const int32_t *perm;   /* backward, stride > 1: parity-class row order of the input map (mink_class_partition) */
  int64_t n_perm;        /* rows of `perm` (0 without one) */
  int32_t K, cin, cout, stride;
} MinkConvLayer;

typedef struct {
  const float *gamma, *beta;          /* [C] */
  float *running_mean, *running_var;  /* [C] or both NULL */
  float *dgamma, *dbeta;              /* backward: [C] (written) */
  float *mean, *invstd;               /* [C] batch statistics: written by forward, read by backward */
  float momentum, eps;
} MinkNormLayer;

typedef struct {
  void *compute, *branch, *wgrad;     /* hipStream_t */
  void *ws_compute, *ws_branch, *ws_wgrad; /* scratch per stream, 256-byte aligned */
  int64_t ws_bytes;                   /* size of EACH scratch buffer (>= mink_block_workspace_bytes) */
} MinkExec;

typedef struct {
  MinkConvLayer conv;   /* 3^3, stride 1, no bias; cin a multiple of 4 */
  MinkNormLayer norm;
  const int32_t *nbr_pool;  /* [n_pool][8] children table of the 2^3 sum pooling */
  const int32_t *in2out;    /* [n] row -> pooled row */
  int64_t n, n_pool;
  const float *x;  /* [n][cin] */
  float *y;        /* [n][cout] convolution output (kept for backward) */
  float *out;      /* [n_pool][cout] */
  const float *g_out;  /* backward: gradient of `out` */
  void *xb;        /* ABI 3, bf16 storage (needs mink_conv_set_math(1)): [n][32] bf16 copy of x, written by forward and read by
                      backward; `y` is then bf16 [n][cout].  NULL: fp32 storage */
  int32_t xb_ready; /* nonzero: `xb` already holds mink_rows_to_bf16(x) (made ahead of the step, e.g. beside the previous one):
                      forward does not write it */
} MinkStem;

typedef struct {
  MinkConvLayer conv1, conv2, down;   /* down.w == NULL: identity shortcut (then n_in == n_out, cin == cout) */
  MinkNormLayer norm1, norm2, normd;
  int64_t n_in, n_out;
  const float *x;   /* [n_in][cin] */
  float *y1, *h1, *y2, *yd, *sd, *out;  /* [n_out][planes] each: conv1 out, relu(norm1), conv2 out, shortcut conv out,
                                           normalised shortcut, block output (yd, sd unused without a down path) */
  /* backward */
  const float *g_out;  /* [n_out][planes] */
  float *g_x;          /* [n_in][cin], or NULL when the block input needs no gradient */
  float *g_tmp;        /* scratch for the intermediate gradients: mink_block_grad_scratch_floats() floats */
} MinkBasicBlock;

int64_t mink_block_workspace_bytes(int64_t n_in, int64_t n_out, int32_t cin, int32_t cout);
int64_t mink_block_grad_scratch_floats(int64_t n_in, int64_t n_out, int32_t cin, int32_t cout, int32_t has_down);
/* 1 when mink_stem_forward/backward accept this stem (else compose it from the per-operator calls) */
int mink_stem_supported(int64_t n, int32_t cin, int32_t cout, int32_t K);
int mink_stem_forward(const MinkStem *s, const MinkExec *ex);
int mink_stem_backward(const MinkStem *s, const MinkExec *ex);
int mink_block_forward(const MinkBasicBlock *b, const MinkExec *ex);
int mink_block_backward(const MinkBasicBlock *b, const MinkExec *ex);

/* ------------------------------------------------------------------ the whole trunk as one call (csrc/trunk.hip)
 * Stem + every BasicBlock of a Mink-ResNet (the reference's ResNetBase.forward up to layer4:
 * co3d_3d/src/models/mink/resnet.py:107-161 `_make_layer`, :163-175 `forward`) in ONE host call per direction.
 * mink_net_forward / mink_net_backward sequence exactly what mink_stem_* and mink_block_* sequence (they call them),
 * block after block; what they add is the binding of every block to this batch -- rows, neighbour tables, activation
 * and gradient addresses -- from a handful of per-LEVEL records, so the host's per-step work no longer grows with the
 * depth of the network (Mink-ResNet34 at four scenes per GPU, BASELINE config #3's per-GPU shape: 3.6 ms of host per
 * 4.7 ms step with one call per block).
 *
 * Levels: level 0 is the stem's output (tensor stride 2), level l + 1 the map a stride-2 block takes level l to.
 * A block with conv1.stride == 2 goes from its level to the next and must carry a shortcut convolution (kernel
 * volume 1); a block with stride 1 stays on its level with an identity shortcut.
 *
 * The caller fills, once: every block's static fields (w, dw, K, cin, cout, stride of the three convolutions; gamma, beta,
 * running statistics, dgamma, dbeta, momentum, eps of the three norms) and the stem's; per step: the level records, the
 * stem's x / nbr / nbr_pool / in2out / n / n_pool / y / out / norm.mean / norm.invstd (the stem's activations stay
 * caller-owned: their layout depends on the storage type).  The library fills everything else in `blocks`.
 *
 * Activation arena (forward writes, backward reads; mink_net_sizes gives the size): per block, 256-byte aligned,
 * [y1 | h1 | y2 | out | (yd | sd)] [n_out][C] each, then six [C] statistics vectors.  The trunk's output is the last
 * block's `out` (net->out, net->out_rows).  Gradient arena (backward scratch): per block its mink_block_grad_scratch
 * floats and the gradient of its input.
 *
 * done_events (backward, optional; n_blocks entries from mink_event_create, NULL entries skipped): event i is recorded on
 * ex->wgrad once EVERY parameter gradient of block i (weights on `wgrad`, batch-norm scale / shift on `compute` /
 * `branch`) has been queued and ordered before it -- what a data-parallel caller makes a bucket's all-reduce wait for,
 * instead of for the tail of the streams (the whole backward pass is queued by the time this call returns).
 *
 * mink_set_block_done_hook (backward, data parallelism): called ON THE HOST, inside mink_net_backward, at the very point
 * where done_events[i] would be recorded -- block i's kernels are queued and ex->wgrad is ordered after them -- so that the
 * caller can issue that block's collective from ex->wgrad right there (what is queued on that stream so far IS what the
 * collective must wait for): no event, no stream of its own for the launches.  (A fifth busy hardware queue is what the
 * "eight hardware queue cliff" of DESIGN section 6 turned out to be.)  The hook must not call back into mink_net_*.  NULL = off.
 *
 * mink_set_stage_hook: instrumentation (race tests, timelines): called on the host before the stem (stage -1) and before
 * every block (stage i) of forward (backward = 0) and backward (= 1; there the stem comes last).  NULL = off. */
typedef struct {
  int64_t n;               /* rows of this level */
  const int32_t *nbr3;     /* [n][27] 3^3 stride-1 table of the level onto itself */
  const int32_t *down3;    /* [n][27] 3^3 stride-2 table from the finer level into this one (NULL at level 0) */
  const int32_t *down1;    /* [n][1] the shortcut's table (kernel volume 1, stride 2) */
  const int32_t *down3_t;  /* backward: [n_finer][27] transposed `down3` */
  const int32_t *perm;     /* backward: parity-class row order of the finer level (mink_class_partition), or NULL */
  int64_t n_perm;
} MinkLevelMaps;

typedef struct {
  MinkStem stem;
  MinkBasicBlock *blocks;
  int32_t n_blocks;
  int32_t with_stem;       /* 0: the caller runs mink_stem_forward / _backward itself (stem.out / stem.n_pool still describe level 0) */
  float *out;              /* written by mink_net_forward: [out_rows][C of the last block] */
  int64_t out_rows;
  const float *g_stem_out; /* written by mink_net_backward: gradient of the stem's output (in the gradient arena) */
} MinkNet;

typedef void (*MinkStageHook)(int32_t stage, int32_t backward);
int mink_set_stage_hook(MinkStageHook hook);
typedef void (*MinkBlockDoneHook)(int32_t block);
int mink_set_block_done_hook(MinkBlockDoneHook hook);
int mink_event_create(void **event_out);
int mink_event_destroy(void *event);
int mink_stream_wait_event(void *stream, void *event);
int mink_net_sizes(const MinkNet *net, const MinkLevelMaps *levels, int32_t n_levels, int64_t *act_floats, int64_t *grad_floats,
                   int64_t *ws_bytes);
int mink_net_forward(MinkNet *net, const MinkLevelMaps *levels, int32_t n_levels, float *arena, int64_t arena_floats,
                     const MinkExec *ex);
int mink_net_backward(MinkNet *net, const MinkLevelMaps *levels, int32_t n_levels, float *arena, int64_t arena_floats,
                      const float *g_out, float *grad_arena, int64_t grad_floats, const MinkExec *ex, void *const *done_events);

/* ------------------------------------------------------------------ bf16 storage of the full-resolution stage (csrc/stem16.hip, csrc/batchnorm.hip, csrc/conv_wgrad.hip)
 * BASELINE config "bf16 mixed precision", storage form: the network input and the stem convolution's output -- three
 * quarters of the activation bytes of a Mink-ResNet step -- are kept in HBM as bf16; the pooled level and everything
 * below stay fp32.  Arithmetic is that of mink_conv_set_math(1) (bf16 operands, fp32 accumulation); the batch-norm
 * statistics are those of the STORED (rounded) convolution output.
 *   mink_rows_to_bf16     x fp32 [n][c] (pitch ldx) -> xb bf16 [n][32], zero-padded (c <= 32)
 *   mink_stem_conv_bf16s  yb bf16 [n_out][64] = conv over nbr [n_out][27] of xb with w fp32 [27][cin][64];
 *                         stats_out: double [stats_rows][2][64] column (sum, sum of squares) partials for
 *                         mink_bn_stats_from_partials; stats_rows must equal mink_stem_conv_bf16s_stats_rows()
 *                         (one row per workgroup of the persistent launch)
 *   mink_bn_relu_pool_fwd_b16 / _bwd_b16: mink_bn_relu_pool_fwd / _bwd (parameter gradients only) reading that bf16 output
 *   mink_conv_wgrad_bn_relu_pool_b16: mink_conv_wgrad_bn_relu_pool with x = xb (pitch 32) and y bf16 */
int mink_rows_to_bf16(const float *x, int64_t n, int32_t c, int32_t ldx, void *xb, void *stream);
int mink_stem_conv_bf16s_supported(int64_t n_in, int64_t n_out, int32_t K, int32_t cin, int32_t cout);
int32_t mink_stem_conv_bf16s_stats_rows(void);
int mink_stem_conv_bf16s(const void *xb, int64_t n_in, const float *w, int32_t cin, const int32_t *nbr, int64_t n_out, int32_t K,
                         void *yb, int32_t cout, double *stats_out, int32_t stats_rows, void *stream);
int mink_bn_relu_pool_fwd_b16(const void *xb, int32_t C, const float *mean, const float *invstd, const float *gamma,
                              const float *beta, const int32_t *nbr, int64_t n_out, int32_t K, float *y, void *stream);
int mink_bn_relu_pool_bwd_b16(const float *dy_pool, const void *xb, int64_t n, int32_t C, const float *mean, const float *invstd,
                              const float *gamma, const float *beta, const int32_t *in2out, float *dgamma, float *dbeta,
                              void *workspace, int64_t workspace_bytes, void *stream);
int mink_conv_wgrad_bn_relu_pool_b16(const void *xb, int64_t n_in, int32_t cin, const void *yb, int32_t cout, const float *dy_pool,
                                     int64_t n_pool, const int32_t *in2out, const float *mean, const float *invstd,
                                     const float *gamma, const float *beta, const float *dgamma, const float *dbeta,
                                     const int32_t *nbr, int64_t n_out, int32_t K, float *dw, void *workspace,
                                     int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ streams confined to a CU subset (csrc/trunk.hip)
 * A HIP stream whose kernels may only run on compute units [first_cu, first_cu + n_cus) of the device's
 * `total_cus` (hipExtStreamCreateWithCUMask; on a multi-XCD part consecutive mask bits go round the XCDs, so a
 * contiguous range is spread evenly over them).  The training step keeps several streams busy at once -- the
 * data-gradient chain, the weight gradients beside it, the next batch's coordinate maps (ME builds those on the
 * stream it computes on: models/mink/resnet.py:164 -> CoordinateMapManager) -- and an auxiliary stream that may
 * take every CU slows the kernels of the chain it runs beside; confined to a few CUs it still finishes in the
 * shadow of the chain.  The caller owns the stream. */
int mink_stream_create_cu_subset(int32_t first_cu, int32_t n_cus, int32_t total_cus, void **stream_out);
int mink_stream_destroy(void *stream);

/* ------------------------------------------------------------------ kernel timing (measurement only) (csrc/conv.hip)
 * bench.py reports the roofline of the dominant convolution kernel from HIP events recorded on the stream each
 * kernel is launched on.  mode 0: off; 1: every convolution launch; 2: only launches matching (kind, K, cin, cout).
 * kind: 0 forward, 1 data gradient, 2 weight gradient, -1 (mode 2) any of them -- the passes of one layer.  mink_conv_timing_fetch synchronises the recorded events,
 * writes up to `max` entries and clears the list; returns the number written (or the number pending if out == NULL). */
typedef struct {
  int32_t kind, K, cin, cout;
  int64_t n_in, n_out;
  const int32_t *nbr;
  float ms;
} MinkTimingEntry;
int mink_conv_timing(int32_t mode, int32_t kind, int32_t K, int32_t cin, int32_t cout);
int64_t mink_conv_timing_fetch(MinkTimingEntry *out, int64_t max);

/* ------------------------------------------------------------------ dynamic graph layers (csrc/graph.hip)
 * DGCNN (reference co3d_3d/src/models/mink/dgcnn.py:8-38,81-85) on the rows of a field, without an n x n distance matrix
 * and without any edge-sized (n x k x C) tensor.
 *
 * mink_knn: idx[i][0..k) = the global rows of the k rows of the SAME sample (batch_offsets int32 [B + 1], device, never read
 *   by the host) nearest to row i of x[n][C] (row stride ldx floats) in squared Euclidean distance, row i included; ascending
 *   distance, ties to the lower row.  The ranking score is ||x_j||^2 - 2 x_i.x_j in fp32 (inner products on the fp32 matrix
 *   cores).  1 <= C <= MINK_KNN_MAX_C, 1 <= k <= MINK_KNN_MAX_K, samples of any size (empty ones included), n k < 2^31.  The
 *   slots of a row whose sample holds fewer than k rows with a comparable (non-NaN) score are -1.
 *
 * mink_knn_cross: the same search with queries and candidates in two matrices (feature matching between two clouds, reference
 *   co3d_3d/src/utils/geometry.py find_nn_gpu): idx[i][0..k) = the global rows of c, inside the SAME sample, nearest to row i
 *   of q.  q[nq][C] (row stride ldq floats), rows of sample b = q_offsets[b] .. q_offsets[b+1]; c[nc][C] (row stride ldc), rows
 *   of sample b = c_offsets[b] .. c_offsets[b+1]; both offset arrays int32 [B + 1] on the device (entries are clamped to the
 *   row counts).  Ranking as mink_knn: score ||c_j||^2 - 2 q_i.c_j in fp32, ascending, equal scores in ascending row order;
 *   slots beyond the number of comparable (non-NaN score) candidates of the sample are -1.  The launch shape, the tile loop
 *   and the running top-k are mink_knn's (one device function, two instantiations).
 *   dist (may be NULL): dist[i][s] = sum_c (q_i[c] - c_idx[c])^2 recomputed for the chosen pair by direct differences, one
 *   fused multiply-add chain, channels ascending, carried in double and rounded to fp32 once (within one fp32 rounding of the
 *   exact value; an fp32 chain would round every difference too and exceed C u); +inf where idx is -1 (such a slot is never
 *   followed).  This is not the ranking score, so it carries no cancellation -- and neighbouring slots may be out of exact
 *   order by less than the ranking error.  1 <= C <= MINK_KNN_MAX_C, 1 <= k <= MINK_KNN_MAX_K, nq k < 2^31, samples of any size on either side.
 *
 * Edge convolution.  With W = [W1 | W2] the reference's W [x_j - x_i ; x_i] is e[i][j] = P[idx[i][j]] + Q[i], P = X W1^T,
 *   Q = X (W2 - W1)^T, both [n][C] (C = output channels, any C >= 1).  An idx outside [0, n) is clamped, never followed.
 *   mink_edge_stats: per-channel (sum e, sum e^2) over the n k edges as double column partials [mink_edge_stats_rows(n)][2][C]
 *     for mink_bn_stats_from_partials (row count n k).
 *   mink_edge_fwd: y[i][c] = max_j lrelu_0.2(gamma (e - mean) invstd + beta), arg[i][c] = the lowest slot j attaining it.
 *   mink_edge_bwd: with z^ / e^ at the arg slot, g = dy (z^ > 0 ? 1 : 0.2), dbeta = sum_i g, dgamma = sum_i g e^; training != 0:
 *     de[i][j] = gamma invstd ([j = arg] g - dbeta / M - e^[i][j] dgamma / M), M = n k; else only the [j = arg] g term.  dQ[i] sums
 *     de over the k edges leaving row i, dP[r] over the edges arriving at r: (members, seg) = the flat edge ids i k + j grouped
 *     by idx, int32 [n k] / [n + 1], ascending inside a segment.  Fixed-order sums, no atomics: bitwise reproducible. */
#define MINK_KNN_MAX_K 64
#define MINK_KNN_MAX_C 256
int mink_knn(const float *x, int64_t n, int64_t ldx, int32_t C, const int32_t *batch_offsets, int32_t B, int32_t k, int32_t *idx,
             void *stream);
int mink_knn_cross(const float *q, int64_t nq, int64_t ldq, const float *c, int64_t nc, int64_t ldc, int32_t C,
                   const int32_t *q_offsets, const int32_t *c_offsets, int32_t B, int32_t k, int32_t *idx, float *dist, void *stream);
int32_t mink_edge_stats_rows(int64_t n);
int mink_edge_stats(const float *P, const float *Q, const int32_t *idx, int64_t n, int32_t k, int32_t C, double *partial,
                    int64_t partial_bytes, void *stream);
int mink_edge_fwd(const float *P, const float *Q, const int32_t *idx, int64_t n, int32_t k, int32_t C, const float *mean,
                  const float *invstd, const float *gamma, const float *beta, float *y, uint8_t *arg, void *stream);
int64_t mink_edge_bwd_workspace_bytes(int64_t n, int32_t C);
int mink_edge_bwd(const float *dy, const float *P, const float *Q, const int32_t *idx, const uint8_t *arg, int64_t n, int32_t k,
                  int32_t C, const float *mean, const float *invstd, const float *gamma, const float *beta, int32_t training,
                  const int32_t *members, const int32_t *seg, float *dP, float *dQ, float *dgamma, float *dbeta, void *workspace,
                  int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ PAConv (csrc/paconv.hip)
 * Score-weighted neighbour aggregation (reference co3d_3d/src/models/paconv: feat_trans_dgcnn / feat_trans_pointnet followed
 * by assign_score_withk / assign_score_withk_halfkernel, aggregate = sum) with the neighbour sum taken in INPUT space:
 *     A[i][m][:] = sum_j s[i][j][m] x[idx[i][j]][:]     S[i][m] = sum_j s[i][j][m]     CX[i][m][:] = S[i][m] x[i][:]
 *     y[i][:]    = sum_m (A[i][m][:] Wn_m - CX[i][m][:] Wc_m)           one dense GEMM of [A | CX] with [Wn ; -Wc], the caller's
 * with Wn_m = K1_m + K2_m, Wc_m = K1_m (DGCNN flavour, weight bank [2 Cin][M][O] = [K1 ; K2]) or Wn_m = 2 K_m, Wc_m = K_m
 * (PointNet flavour, bank [Cin][M][O]).  No [n][M][O] and no [n][k][.][O] tensor is formed, forward or backward.
 *
 * Layouts: x[n][Cin] contiguous; idx int32 [n][k] of global rows (as mink_knn writes them); s[n][k][M]; A, CX, dA, dCX are
 * [n][M][Cin] with a common row pitch of ldz floats (>= M Cin: the two halves of one [n][2][M][Cin] buffer have ldz = 2 M Cin);
 * S[n][M]; ds[n][k][M]; dx[n][Cin].  1 <= M <= MINK_PACONV_MAX_M, 1 <= k <= MINK_KNN_MAX_K, any Cin >= 1, n k < 2^31.  A slot
 * whose idx lies outside [0, n) contributes nothing to A or S, is never followed, and gets ds = 0.  16-byte accesses where
 * Cin % 4 == 0, ldz % 4 == 0 and the pointers are 16-byte aligned (scores: M % 4 == 0), dwords otherwise.
 *
 *   mink_paconv_gather: A, and where the pointers are given S and CX, in one pass.  A group of G lanes (the power of two in
 *     4..64 covering Cin / VEC) owns a row and a chunk of G VEC channels and holds M accumulators per channel; the k slots
 *     are walked in ascending order as an fp32 fma chain, S by plain additions in the same order.
 *   mink_paconv_score_bwd: with dA = g Wn^T and dCX = -g Wc^T (the gradients of the GEMM's two operands),
 *     ds[i][j][m] = sum_c (dA[i][m][c] x[idx[i][j]][c] + dCX[i][m][c] x[i][c]), c ascending, one lane per slot.
 *   mink_paconv_scatter_bwd: dx[r][:] = sum_{e in list(r)} sum_m s[e][m] dA[e / k][m][:] + sum_m S[r][m] dCX[r][m][:], where
 *     (members, seg) = the flat slot ids e = i k + j grouped by idx[e], int32 [n k] / [n + 1], ascending inside a segment (slots
 *     outside [0, n) behind the last segment): edges ascending, m ascending, then the centre term.
 * Fixed-order sums, no atomics: two runs give the same bits. */
#define MINK_PACONV_MAX_M 16
int mink_paconv_gather(const float *x, const float *s, const int32_t *idx, int64_t n, int32_t k, int32_t M, int32_t Cin, float *A,
                       float *CX, int64_t ldz, float *S, void *stream);
int mink_paconv_score_bwd(const float *dA, const float *dCX, int64_t ldz, const float *x, const int32_t *idx, int64_t n, int32_t k,
                          int32_t M, int32_t Cin, float *ds, void *stream);
int mink_paconv_scatter_bwd(const float *dA, const float *dCX, int64_t ldz, const float *s, const float *S, const int32_t *members,
                            const int32_t *seg, int64_t n, int32_t k, int32_t M, int32_t Cin, float *dx, void *stream);

/* ------------------------------------------------------------------ scene sub-sampling (csrc/sample.hip)
 * Farthest-point sampling of every scene of a batch (reference co3d_3d/src/data/transforms.py FarthestPointSample.sample: a loop
 * of num_points iterations over all voxels of a scene, on the CPU).  Nothing is read back by the call.
 *
 * mink_fps_scenes: xyz[n][ld] row-major fp32, 3 <= ld <= MINK_FPS_MAX_LD, only columns 0..2 are read (a [n][3] matrix, or columns 1..3 of a float
 *   [n][4] coordinate matrix through a pointer one float in: no alignment beyond 4 bytes is asked for).  Scene b = rows
 *   offsets[b] .. offsets[b+1] (int32 [B + 1], device, never read by the host); start[b] (int32 [B], device) = the scene-local
 *   row of its first pick.  idx[b][0..m) (int32 [B][m]) = the GLOBAL rows (offsets[b] + local row) picked, in pick order.  Per scene:
 *       dist[i] = 1e10f;  cur = start[b];
 *       m times:  emit cur;  for every row i: d = ((dx dx) + (dy dy)) + (dz dz) with dx = x_i - x_cur, ..., every difference,
 *                 product and sum rounded to fp32 on its own (no fused multiply-add);  dist[i] = d where d < dist[i];
 *                 cur = the row with the largest dist, ties to the LOWEST row (as torch.argmax).
 *   So with fewer distinct positions than m, once all are taken every distance is 0 and the remaining picks are local row 0; and
 *   a coincident point is never picked while a point at positive distance remains.  m may exceed the scene's size.
 *   One workgroup of MINK_FPS_THREADS threads per scene; no workgroup waits for another.  Where a scene's coordinates and
 *   running distances live depends on its size alone, and the picks do not depend on it:
 *       rows <= MINK_FPS_XYZ_REG_ROWS_SMALL, <= MINK_FPS_XYZ_REG_ROWS : both in registers (2 / 8 rows per thread)
 *       rows <= MINK_FPS_DIST_REG_ROWS : distances in registers (56 per thread), coordinates re-read from memory every pick
 *       larger : distances in `workspace` (n_max floats per scene), coordinates re-read every pick
 *   Each of the four is a launch of its own over the B scenes (a workgroup whose scene belongs to another leaves at once; one that
 *   no scene of at most n_max rows can need is not launched), so scenes of different residencies run one group after the other.
 *   n = rows of xyz (1 <= n < 2^31); n_max = the caller's bound on the largest scene (1 <= n_max <= n; n itself always serves);
 *   workspace_bytes >= mink_fps_workspace_bytes(n_max, B) (0 up to MINK_FPS_DIST_REG_ROWS: workspace may then be NULL); B m < 2^31.
 *   status (int32 [1], device; zeroed by the call, then OR-ed): a scene that is empty or whose offsets leave [0, n]
 *   (MINK_FPS_EMPTY_SCENE), whose start lies outside it (MINK_FPS_BAD_START) or that holds more than n_max rows
 *   (MINK_FPS_SCENE_TOO_LARGE) is not read at all: its m picks are -1 and the bit is set; the other scenes are sampled. */
#define MINK_FPS_THREADS 1024
#define MINK_FPS_MAX_LD 4096
#define MINK_FPS_XYZ_REG_ROWS_SMALL 2048
#define MINK_FPS_XYZ_REG_ROWS 8192
#define MINK_FPS_DIST_REG_ROWS 57344
#define MINK_FPS_EMPTY_SCENE 1
#define MINK_FPS_BAD_START 2
#define MINK_FPS_SCENE_TOO_LARGE 4
int64_t mink_fps_workspace_bytes(int64_t n_max, int32_t B);
int mink_fps_scenes(const float *xyz, int64_t n, int64_t ld, const int32_t *offsets, const int32_t *start, int32_t B, int32_t m,
                    int64_t n_max, int32_t *idx, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ weight-sparse convolution (csrc/wsconv.hip)
 * Inference with pruned kernels (reference co3d_3d/src/models/mink/modules/sparse_conv.py: WeightSparseConvolution(Transpose)
 * .forward -> one `spmm` per kernel offset over the CSR that `sparsify("csr")` keeps).  Forward only, fp32, no atomics:
 *
 *     y[r][0..cout) = bias + sum over the valid offsets k = koffs[v], v ascending, with i = nbr[r][k] >= 0,
 *                            of sum over the nonzeros (ci, co, w) of W[k]:  x[i][ci] * w
 *
 * one fp32 fma chain per output element (offsets ascending, input channels ascending inside an offset), bitwise reproducible.
 * Only products with a STORED weight are formed: an input channel all of whose weights were pruned is never read into a result, so
 * a NaN there does not reach y (mink_conv_gather_gemm on the masked weights would multiply it by zero).  A row without a neighbour
 * at an offset is staged as zeros, so the stored weights must be finite.
 *
 *   x[n_in][ldx], cin <= ldx; y[n_out][ldy], cout <= ldy: pad columns of x are never read, pad columns of y never written.
 *   nbr[n_out][K]: entries -1 or < n_in, as for mink_conv_gather_gemm.  A transposed convolution passes its transposed table.
 *   koffs[n_valid]: the offsets that hold a nonzero, ascending, each < K.  n_valid <= K.
 *   rowptr[n_valid][cout + 1], colidx[nnz], vals[nnz]: CSR of W[koffs[v]]^T per valid offset -- rows are output channels, column
 *     indices input channels, ascending inside a row; rowptr values index the concatenated colidx / vals (rowptr[0][0] = 0, the
 *     last one = nnz, row v+1 begins where row v ends).
 *   cptr[n_valid][cout][nchunks + 1], nchunks = ceil(cin / MINK_WSCONV_CHUNK): derived from the CSR -- cptr[v][co][j] = the first
 *     nonzero of row (v, co) whose column is >= j MINK_WSCONV_CHUNK (the last entry = the row's end).  The kernel stages
 *     MINK_WSCONV_CHUNK input channels at a time; read only when cin > MINK_WSCONV_CHUNK, may be NULL otherwise.
 *   bias[cout] or NULL.
 * n_out == 0: MINK_OK without a launch.  n_valid == 0 or nnz == 0: every row of y is the bias, or zero (no table is read; the
 * sparse operands may be NULL).  Tile: 64 rows (n_out < MINK_WSCONV_WIDE_ROWS) or 256 rows x MINK_WSCONV_COUT_TILE channels per
 * workgroup; 16-byte accesses to x / y where the pointer and the pitch allow, dwords otherwise. */
#define MINK_WSCONV_CHUNK 64
#define MINK_WSCONV_COUT_TILE 64
#define MINK_WSCONV_WIDE_ROWS 32768
int mink_wsconv_fwd(const float *x, int64_t n_in, int32_t ldx, int32_t cin, const int32_t *nbr, int64_t n_out, int32_t K,
                    const int32_t *koffs, int32_t n_valid, const int32_t *rowptr, const int32_t *cptr, const int32_t *colidx,
                    const float *vals, int64_t nnz, float *y, int32_t ldy, int32_t cout, const float *bias, void *stream);

/* ------------------------------------------------------------------ positional encoding (csrc/posenc.hip)
 * MinkowskiPositionalEncoding (reference co3d_3d/src/models/mink/modules/encoding.py:74-209), fp32, no atomics.  With
 * Q = 2 L C encoded columns, column q reads input channel q / (2L):
 *
 *     y[i][q]          = sin(freq[q] * x[i][q / (2L)] + phase[q])      0 <= q < Q   (one fused multiply-add, then sinf)
 *     y[i][Q + c - lo] = x[i][c]                                       lo <= c < hi (the pass-through columns, bit-equal)
 *     dx[i][c]         = sum over q in [2L c, 2L (c + 1)), ascending, of freq[q] * cos(freq[q] * x[i][c] + phase[q]) * dy[i][q]
 *                        (+ dy[i][Q + c - lo] when lo <= c < hi, added last)
 *
 * freq[Q] and phase[Q] are device arrays (the module's `frequencies` and `offset`); which entries hold sines and which
 * cosines is the caller's business.  x[n][ldx], C <= ldx; y and dy have n rows of pitch ldy >= Q + hi - lo and nothing beyond
 * those columns is read or written, so the layer can fill the left columns of a wider matrix; dx[n][lddx], C <= lddx.
 * 1 <= C <= 4096, 1 <= L <= 32, 0 <= lo <= hi <= C, n < 2^28.  n == 0: MINK_OK without a launch.  Forward: one lane per column
 * group; backward: one lane per (row, channel), which owns the channel's 2L contiguous columns, so two runs are bitwise equal.
 * 16-byte accesses to y / dy / freq / phase when 2L % 4 == 0, ldy % 4 == 0 and those pointers are 16-byte aligned, dwords
 * otherwise; x, dx and the pass-through columns always move as dwords. */
int mink_posenc_fwd(const float *x, int64_t n, int32_t C, int32_t ldx, const float *freq, const float *phase, int32_t L, int32_t lo,
                    int32_t hi, float *y, int32_t ldy, void *stream);
int mink_posenc_bwd(const float *dy, int32_t ldy, const float *x, int64_t n, int32_t C, int32_t ldx, const float *freq,
                    const float *phase, int32_t L, int32_t lo, int32_t hi, float *dx, int32_t lddx, void *stream);

/* ------------------------------------------------------------------ multi-head self-attention (csrc/attn.hip)
 * The attention of a Vision Transformer block (timm's Attention.forward between its `qkv` and `proj` linears; the reference
 * builds these networks in co3d_2d/src/model/models.py:37-54), fp32, on token rows: B samples of N tokens, H heads of D channels.
 *
 *     qkv [B N][ldq]  row b N + t is one token; column s H D + h D + d holds q (s = 0), k (s = 1) or v (s = 2) of head h --
 *                     what nn.Linear(dim, 3 dim) writes; ldq >= 3 H D
 *     out [B N][ldo]  column h D + d, what `proj` reads; ldo >= H D:
 *                     out[b N + i][h D + d] = sum_j softmax_j(scale q_i . k_j) v_j[d]        (per sample b and head h)
 *     lse [B][H][N]   max_j s_ij + log sum_j exp(s_ij - max_j s_ij) with s_ij = scale q_i . k_j (scaled-score units)
 *     dout[B N][lddo] the gradient of out, lddo >= H D
 *     dqkv[B N][lddq] the gradient of qkv in qkv's layout, lddq >= 3 H D; every logical element is written exactly once
 *
 * No N x N matrix reaches memory: the backward recomputes P = exp(s - lse).  Every product runs on the fp32 MFMA (an fmaf chain,
 * one rounding per product), the row maximum (forward) or lse (backward) is subtracted before every exponential, `scale` is
 * applied to the finished dot product.  mink_set_conv_math does not reach these entry points.  No atomics, every sum in a fixed
 * order: two calls on the same inputs give the same bits.  mink_attn_bwd launches three kernels: delta = rowsum(dout * out) into
 * the workspace ([B][H][N] floats), then one whose workgroups own 64 keys (dk, dv) and one whose workgroups own 64 queries (dq);
 * both recompute the scores.
 *
 * D == MINK_ATTN_HEAD_DIM, 1 <= N <= MINK_ATTN_MAX_TOKENS, 1 <= H <= MINK_ATTN_MAX_HEADS, B >= 1 with B H N < 2^31 and
 * B N < 2^31 / 192; pointers 4-byte aligned, the workspace 8-byte aligned and of at least mink_attn_bwd_workspace_bytes() bytes.
 * Anything else is MINK_EINVAL before any launch.  Only the logical columns of the logical rows are read or written: pad
 * columns may hold NaN and keep their bits, token rows past N of a tile are neither read nor stored.  16-byte accesses when
 * every matrix pointer of the call is 16-byte aligned and every pitch a multiple of 4, dwords otherwise. */
#define MINK_ATTN_HEAD_DIM 64
#define MINK_ATTN_MAX_TOKENS 4096
#define MINK_ATTN_MAX_HEADS 1024
int64_t mink_attn_bwd_workspace_bytes(int64_t B, int64_t N, int32_t H, int32_t D);
int mink_attn_fwd(const float *qkv, int32_t ldq, int64_t B, int32_t N, int32_t H, int32_t D, float scale, float *out, int32_t ldo,
                  float *lse, void *stream);
int mink_attn_bwd(const float *qkv, int32_t ldq, const float *out, int32_t ldo, const float *lse, const float *dout, int32_t lddo,
                  int64_t B, int32_t N, int32_t H, int32_t D, float scale, float *dqkv, int32_t lddq, void *workspace,
                  int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ multi-head self-attention on bf16 rows (csrc/attn16.hip)
 * The attention of a mixed-precision Vision Transformer: the entry points above with qkv, out, dout and dqkv in bf16 (`void *`,
 * as for mink_stem_conv_bf16s) and the products on v_mfma_f32_16x16x32_bf16.  The row layout, the pitches (in ELEMENTS) and the
 * shape limits are those of mink_attn_fwd / mink_attn_bwd; lse and the delta workspace, both [B][H][N], are fp32.
 *
 * The arithmetic contract (tests/attn16_restate.py derives its bounds from it):
 *   Every product runs on the bf16 MFMA with fp32 accumulation.
 *   Everything else is fp32, except these roundings to bf16 (round to nearest even, relative error <= U16 = 2^-8):
 *     F1: bf16(exp(s - m)) as the operand of P V.  The row sum l, and so lse, use the unrounded fp32 weights.
 *     F2: the stored out.
 *     B1: bf16(exp(s - lse)) as the operand of dV = P^T dO.
 *     B2: bf16(P o (dP - delta)) as the operand of dQ and dK.  It is formed in fp32 from the unrounded P.
 *     B3: the stored dqkv, after the scale.
 *   delta_i = sum_d dO_id out_id is an fp32 sum over the stored, rounded out.
 *   Never rounded to bf16: the scores; dP, delta, m, l and lse; the online-softmax rescale factors; the O, dQ, dK and dV
 *   accumulators before their final store.
 *   The maximum (forward) or lse (backward) is subtracted before every exponential.
 *   `scale` multiplies the finished dot product.
 *
 * No atomics, every sum in a fixed order: two calls on the same inputs give the same bits.  mink_attn_bwd_b16 launches three
 * kernels as mink_attn_bwd does (delta into the workspace, a key-owning kernel for dk and dv, a query-owning kernel for dq).
 *
 * bf16 pointers 2-byte aligned, lse 4-byte aligned, the workspace 8-byte aligned and of at least
 * mink_attn_bwd_b16_workspace_bytes() bytes; anything else, and any shape mink_attn_fwd refuses, is MINK_EINVAL before any
 * launch.  Only the logical columns of the logical rows are read or written: pad columns may hold NaN and keep their bits, token
 * rows past N of a tile are neither read nor stored, every logical output element is written exactly once.  16-byte loads and
 * 8-byte stores when every matrix pointer of the call is 16-byte aligned and every pitch a multiple of 8 elements, 2-byte
 * accesses otherwise, with identical results bit for bit. */
int64_t mink_attn_bwd_b16_workspace_bytes(int64_t B, int64_t N, int32_t H, int32_t D);
int mink_attn_fwd_b16(const void *qkv, int32_t ldq, int64_t B, int32_t N, int32_t H, int32_t D, float scale, void *out, int32_t ldo,
                      float *lse, void *stream);
int mink_attn_bwd_b16(const void *qkv, int32_t ldq, const void *out, int32_t ldo, const float *lse, const void *dout, int32_t lddo,
                      int64_t B, int32_t N, int32_t H, int32_t D, float scale, void *dqkv, int32_t lddq, void *workspace,
                      int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ grouped convolution (csrc/gconv.hip)
 * The 3x3 layers of the ResNeXt networks of the 2-D comparison (torchvision's Bottleneck with groups = 32): a convolution over
 * a neighbour table whose G groups do not mix.  Rows are [n][ld] fp32; group g owns the input columns g cg_in .. (g + 1) cg_in and
 * the output columns g cg_out .. (g + 1) cg_out.
 *
 *     nbr[n_out][K]  entries -1 ("outside") or in [0, n_in), as for mink_conv_gather_gemm; 1 <= K <= MINK_GCONV_MAX_K
 *     w  [K][G][cg_in][cg_out]                                   (the packed layout; also the layout of dw)
 *     mink_gconv_fwd    y[r][g cg_out + o] = sum_k sum_c x[nbr[r][k]][g cg_in + c] * w[k][g][c][o]
 *     mink_gconv_wgrad  dw[k][g][c][o]     = sum_r x[nbr[r][k]][g cg_in + c] * dy[r][g cg_out + o]
 *
 * w_transposed reads `w` as [K][G][cg_out][cg_in] and flip_k (bit 0) uses offset K-1-k: with both, and cg_in / cg_out exchanged,
 * the same entry point is the data gradient through the forward weights, with the meaning the flags have in
 * mink_conv_gather_gemm -- stride 1 through the forward table with flip_k, stride 2 through the transposed table.
 *
 * fp32 in, fp32 accumulate, fp32 out in EVERY mink_conv_set_math mode: the grouped layers do not follow bf16 math.  No atomics,
 * every sum in a fixed order (the weight gradient is split over row blocks whose partials are added in ascending order): two
 * calls on the same inputs give the same bits.  A table entry of -1 contributes nothing: the vector-FMA kernels skip it, the
 * matrix-core kernels (cg_in == cg_out in {16, 32, 64}) feed the row as zeros -- in the weight gradient on both sides, so a NaN of
 * dy stays out of the offsets its row does not reach; non-finite WEIGHTS reach every row of their group there.  Every logical
 * output element is written and nothing else: pad columns beyond G cg_out keep their bits, pad columns of the inputs are not read.
 * Any G, cg_in, cg_out >= 1 with K G cg_in cg_out < 2^31, any pitch >= the logical width, pointers 4-byte aligned (16-byte
 * accesses when x and y are 16-byte aligned and both pitches are multiples of 4); n_in, n_out < 2^31.  The workspace is 8-byte
 * aligned and of at least mink_gconv_wgrad_workspace_bytes() bytes.  Anything else is MINK_EINVAL before any launch.  n_out == 0
 * succeeds without a launch (mink_gconv_wgrad then sets dw to zero). */
#define MINK_GCONV_MAX_K 27
int mink_gconv_fwd(const float *x, int64_t n_in, int32_t ldx, const float *w, int32_t w_transposed, int32_t flip_k, const int32_t *nbr,
                   int64_t n_out, int32_t K, int32_t G, int32_t cg_in, int32_t cg_out, float *y, int32_t ldy, void *stream);
int64_t mink_gconv_wgrad_workspace_bytes(int64_t n_out, int32_t K, int32_t G, int32_t cg_in, int32_t cg_out);
int mink_gconv_wgrad(const float *x, int64_t n_in, int32_t ldx, const float *dy, int32_t ldy, const int32_t *nbr, int64_t n_out, int32_t K,
                     int32_t G, int32_t cg_in, int32_t cg_out, float *dw, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MINK_HIP_H */
