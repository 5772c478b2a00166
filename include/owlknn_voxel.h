/*
 * owlknn_voxel.h -- voxel-grid downsampling per cloud (tknnVoxelGrid), an entry point of libowl_mi355x.so on top of the C ABI of
 * owlknn.h: one point per occupied grid cell, what voxel_down_sample and VoxelGrid of the point-cloud libraries give, and
 * grid_cluster followed by avg_pool.  Plain C99; link and load as owlknn.h says.
 *
 * The call takes an engine for its device, its stream order and its workspace only: it needs NO built tree, and leaves a tree, a
 * halo tree and the state of tknnSolve untouched.  The host reads no array of the caller.
 */
#pragma once
#include "owlknn.h"
#include "owlknn_batch.h" /* TKNN_MAX_BATCHES */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- voxel grid ---------------------------------------------------------------------------------------------------------------------------
 * tknnVoxelGrid bins n rows into cubic cells of edge `voxel` and reduces the rows of every occupied cell of every cloud to one.
 *   inputs     d_points: n packed fp32 triples, 0 <= n < 2^31 - 1; voxel: the cell edge, finite and > 0; origin[3]: finite;
 *              d_batch (may be NULL): n int32 labels in any order, num_batches = B clouds, 1 <= B <= TKNN_MAX_BATCHES (without
 *              d_batch B is 1); d_values (may be NULL): n x C packed fp32, 0 <= C = channels <= TKNN_VOXEL_MAX_CHANNELS.
 *   cell       per axis c = floorf((p - origin) / voxel): the subtraction and the division one IEEE fp32 operation each, the
 *              division a true, correctly rounded one (no reciprocal).  A row is IN THE GRID iff all three c lie in [0, 2^21).
 *   left out   each row that is left out is counted once, by the first of these that holds: a coordinate that is not finite
 *              (info->bad_rows); a label outside [0, B) (info->bad_labels); a finite row outside the grid (info->out_of_grid).
 *              Such a row belongs to no voxel, its d_map entry is -1.  A value entry that is not finite is summed like any other:
 *              the result follows IEEE.
 *   voxels     a voxel is a distinct (label, cx, cy, cz) among the rows in the grid; voxels are numbered ascending by that tuple,
 *              so the numbering does not depend on the order of the rows.  V = info->voxels is their number.
 *   outputs    each may be NULL; the per-voxel ones hold `capacity` entries:
 *              d_cell (V x 3 int32): cx, cy, cz;
 *              d_count (V int32): the rows of the voxel;
 *              d_centroid (V x 3 fp32): per axis the sum of (double)p over the voxel's rows, divided by the count in double, rounded
 *                once to fp32;
 *              d_value_mean (V x C fp32): the same for the value columns;
 *              d_first (V int32): the smallest row of the voxel;
 *              d_nearest (V int32): the row of the voxel with the smallest key (bits of d2, row), d2 = (dx*dx + dy*dy) + dz*dz in
 *                uncontracted fp32 of the row against the ROUNDED fp32 centroid above: "keep an original point";
 *              d_voxel_label (V int32): the voxel's cloud;
 *              d_offsets (B + 1 int64): cloud b owns the voxels [d_offsets[b], d_offsets[b + 1]);
 *              d_map (n int32): the voxel of each row, -1 for a row left out.
 *   capacity   a call with every per-voxel output NULL is the COUNT PASS: it gives info->voxels and, if given, d_map and d_offsets;
 *              of capacity only the range is checked.  Otherwise V > capacity returns TKNN_E_ARG before any output is written.  The host reads
 *              one word of the call's own scratch for that check (none where capacity >= n: V <= n), and the call's counters at
 *              its end; nothing else.
 *   tails      no output word stays stale: entries V .. capacity - 1 are written as count 0, cell -1, label -1, first and nearest
 *              -1, centroid and means NaN.
 *   order      the fp64 sums run in one fixed order that depends on the voxel's rows alone, not on how voxels fall on workgroups:
 *              two calls on the same input agree in every output bit.  Against an fp64 sum in another order a centroid or mean is
 *              equal or an adjacent fp32 value.  A voxel of at most TKNN_VOXEL_LANE_ROWS rows is summed by one lane, a longer one
 *              by a wave, one of more than TKNN_VOXEL_WAVE_ROWS rows by a workgroup.  In the environment, read per call:
 *              TKNN_VOXEL_FORCE_WAVE=1 sends every voxel the lane would take to the wave; TKNN_VOXEL_LANE_ROWS=<rows> and
 *              TKNN_VOXEL_WAVE_ROWS=<rows> move the two thresholds (measurements, and tests of the workgroup's path at small n).
 *              Cells, counts, first, labels, offsets and map do not depend on any of them, centroids and means within the bound
 *              above.
 * info: voxels; rows_in_grid = n - bad_rows - bad_labels - out_of_grid; max_count: the rows of the fullest voxel; wave_voxels,
 * block_voxels: the voxels a wave and a workgroup summed (0 where no centroid, mean or nearest row is asked for); key_ms: cells and counters; sort_ms: the sorts, head flags and scan; reduce_ms: map,
 * offsets, sums and tails; solve_ms: all of it.
 * Errors, in this order, all TKNN_E_ARG:
 *   1. NULL engine / options / info;
 *   2. d_points NULL with n > 0;
 *   3. d_values NULL with channels > 0; d_value_mean given with channels = 0;
 *   4. n negative or >= 2^31 - 1; voxel not finite or not > 0; an origin that is not finite; num_batches outside
 *      1 .. TKNN_MAX_BATCHES, or not 1 without d_batch; channels outside 0 .. TKNN_VOXEL_MAX_CHANNELS; capacity negative or
 *      >= 2^31 - 1; an unknown flag;
 *   5. V > capacity (found on the device, before anything the caller can see is written).
 * A refused call writes nothing, info included.  n = 0 succeeds with V = 0, filled tails and offsets all 0. */
#define TKNN_VOXEL_MAX_CHANNELS 16
#define TKNN_VOXEL_CELL_BITS 21
#define TKNN_VOXEL_LANE_ROWS 24
#define TKNN_VOXEL_WAVE_ROWS 2048
typedef struct {
  int64_t n;                 /* rows */
  const float *d_points;     /* n x 3 */
  const int32_t *d_batch;    /* n, may be NULL: one cloud */
  const float *d_values;     /* n x channels, may be NULL with channels = 0 */
  float voxel;               /* > 0, finite */
  float origin[3];           /* finite */
  int32_t num_batches;       /* 1 .. TKNN_MAX_BATCHES; 1 without d_batch */
  int32_t channels;          /* 0 .. TKNN_VOXEL_MAX_CHANNELS */
  uint32_t flags;            /* no flag is defined: 0 */
  int32_t pad_;
  int64_t capacity;          /* entries of each per-voxel output */
  int32_t *d_cell;           /* capacity x 3, may be NULL */
  int32_t *d_count;          /* capacity, may be NULL */
  float *d_centroid;         /* capacity x 3, may be NULL */
  float *d_value_mean;       /* capacity x channels, may be NULL */
  int32_t *d_first;          /* capacity, may be NULL */
  int32_t *d_nearest;        /* capacity, may be NULL */
  int32_t *d_voxel_label;    /* capacity, may be NULL */
  int64_t *d_offsets;        /* num_batches + 1, may be NULL */
  int32_t *d_map;            /* n, may be NULL */
} tknnVoxelGridOptions;
typedef struct {
  int64_t voxels;
  int64_t rows_in_grid;
  int64_t bad_rows, bad_labels, out_of_grid;
  int64_t wave_voxels, block_voxels;
  int32_t max_count;
  float key_ms, sort_ms, reduce_ms, solve_ms;
  int32_t pad_;
} tknnVoxelGridInfo;
TKNN_API int tknnVoxelGrid(tknnEngine e, const tknnVoxelGridOptions *o, tknnVoxelGridInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
