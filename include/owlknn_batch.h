/*
 * owlknn_batch.h -- many point clouds in one tree (tknnBuildBatched) and the k nearest neighbours inside a query's own cloud
 * (tknnBatchKnn), entry points of libowl_mi355x.so on top of the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a tree over B labelled clouds ------------------------------------------------------------------------------------------
 * tknnBuildBatched is tknnBuildIds for n points of which point i belongs to cloud ("batch") d_batch[i], 0 <= d_batch[i] <
 * num_batches.  Labels need not be sorted or contiguous in the caller's buffer, and a batch may be empty.  All batches share one
 * scene box.
 *   the key    of a point with a NaN coordinate is tknnBuild's (bit 63 alone: it sorts last and is in no batch); of every other
 *              point ((uint64_t)d_batch[i] << (63 - bb)) | (key21 >> bb), key21 its 63-bit key in tknnBuild's tree and bb the
 *              smallest multiple of 3 with 2^bb >= num_batches (0 for one batch, at most 15).  The keys are hierarchical, so
 *              key21 >> bb is the point's cell at level 21 - bb / 3 of the same grid.  Sorted by that key every batch is ONE
 *              contiguous range of sorted slots, in curve order inside; with one batch the tree is tknnBuildIds' word for word.
 *   the rest   of the build is tknnBuild's.  A batched tree is a valid tree for every other call, which treats it as one set
 *              (their rows do not depend on the tree's order); tknnBatchKnn needs one.  A later tknnBuild / tknnBuildIds makes
 *              the engine's tree a plain one again.
 * Errors, in this order: NULL engine / d_xyz / d_batch: TKNN_E_ARG; n as tknnBuild refuses it; num_batches < 1: TKNN_E_ARG;
 * num_batches > TKNN_MAX_BATCHES: TKNN_E_UNSUPPORTED; a label outside [0, num_batches): TKNN_E_ARG, the message says how many
 * there are, and the engine is left without a tree.
 *
 * tknnBatchLayout: what the last tknnBuildBatched made.  num_batches, key_bits (bb) on the host (either may be NULL); d_starts,
 * if given, receives num_batches + 1 int32 ON THE DEVICE: batch b is the sorted slots d_starts[b] .. d_starts[b + 1] - 1, and
 * d_starts[num_batches] is the number of points without a NaN.  TKNN_E_STATE unless the engine's tree is a batched one. */
#define TKNN_MAX_BATCHES 32768
TKNN_API int tknnBuildBatched(tknnEngine e, const float *d_xyz, const int32_t *d_ids /* may be NULL */, const int32_t *d_batch,
                              int32_t num_batches, int64_t n, tknnBuildInfo *info, void *stream);
TKNN_API int tknnBatchLayout(tknnEngine e, int32_t *num_batches, int32_t *key_bits, int32_t *d_starts /* num_batches + 1, device, may be NULL */,
                             void *stream);

/* ---- at most k nearest points of the query's own batch --------------------------------------------------------------------------
 * tknnBatchKnn is tknnKnn and tknnRadiusKnn inside a batch: the at most k nearest points of the built set P (n points) that carry
 * the query's label, as dense rows of k, for m arbitrary labelled points Q or for the points of P themselves.
 *   row j      the points p of P with batch[p] == d_query_batch[j], whose distance d = sqrt((dx*dx + dy*dy) + dz*dz), every
 *              operation fp32 and uncontracted (tknnKnn's, bit for bit), is finite and, when a radius is given, d <= r_j; p is
 *              not the point d_skip_ids[j] names.  Ascending in (d, index) -- ties at the k-th place are decided by the index --,
 *              cut after k; written at d_idx[j * k ..] (and d_dist[j * k ..]), the unused tail of a row is idx = -1, dist = +inf.
 *              A query with a NaN coordinate, with a label outside [0, num_batches) or in an empty batch has an empty row.
 *   d_counts[j] = min(k, the eligible points of row j).
 * An entry names its point by id on trees built with ids, by row otherwise.
 * The radius: `radius` is finite and > 0, FLT_MAX means none; or d_radii, m floats, r_j = d_radii[j] -- a NaN, non-finite or
 * <= 0 entry gives an empty row, and `radius` is then ignored.  The host reads neither the radii nor the labels.
 * External queries (d_queries and d_query_batch given, m rows): nothing is "self" unless d_skip_ids says so; a negative value
 * skips nothing.
 * The set's own points (d_queries == NULL and d_query_batch == NULL): row j answers for the point in row j of the buffer given to
 * tknnBuildBatched, in its own batch; m must equal n and d_skip_ids must be NULL; every point is left out of its own row (by its
 * id on trees built with ids, by its row otherwise), a coinciding duplicate of the same batch stays, at distance 0; d_radii is
 * indexed by row.  A point with a NaN is in no batch: its row is empty.
 * k may exceed the size of a batch.  A halo tree, if set, is ignored; the tree and the state of tknnSolve are not modified;
 * results are addressed by the caller's j whatever order the engine works in.
 * info: as tknnKnnInfo counts them; seed_point_tests is 0 exactly when no seed pass ran (it runs when there is no radius at all:
 * d_radii == NULL and radius == FLT_MAX).  The walk never reads a block of 16 sorted slots that does not touch the query's batch.
 * Errors, in this order: NULL engine / options / d_idx, d_queries NULL with m != n, d_skip_ids given with d_queries NULL, exactly
 * one of d_queries and d_query_batch NULL: TKNN_E_ARG; not built, or built without batches: TKNN_E_STATE; k < 1, m < 0,
 * m >= 2^31 - 1: TKNN_E_ARG; k > TKNN_MAX_K_REGISTERS: TKNN_E_UNSUPPORTED; without d_radii a radius that is NaN, <= 0 or
 * infinite: TKNN_E_ARG.  A refused call writes nothing.  m = 0 with queries given succeeds with a zeroed info. */
typedef struct {
  const float *d_queries;       /* m packed fp32 triples (2-D data: z = 0), or NULL: the set's own points, m = n */
  int64_t m;
  int32_t k;                    /* 1 .. TKNN_MAX_K_REGISTERS; k may exceed the size of a batch (rows are then not full) */
  float radius;                 /* every row's radius if d_radii is NULL: finite and > 0, FLT_MAX = none */
  const float *d_radii;         /* NULL, or m floats (self mode: by row) */
  const int32_t *d_skip_ids;    /* NULL, or (external queries only) m int32; a negative value skips nothing */
  const int32_t *d_query_batch; /* m int32, the queries' labels; NULL exactly when d_queries is */
  int32_t *d_idx;               /* m*k, required */
  float *d_dist;                /* m*k, may be NULL */
  int32_t *d_counts;            /* m, may be NULL */
} tknnBatchKnnOptions;
typedef struct {
  int64_t total;              /* entries over all rows = sum of d_counts */
  int64_t full_rows;          /* rows with k entries */
  int64_t node_tests, point_tests; /* the walk's */
  int64_t seed_point_tests;   /* points read for the seed bounds (0: no seed pass) */
  int64_t tightened_rows;     /* full rows whose final k-th distance is below their radius or seed bound */
  int64_t lane_rows;          /* rows the one-query-per-lane kernel answered */
  float solve_ms, order_ms, seed_ms, walk_ms;
} tknnBatchKnnInfo;
TKNN_API int tknnBatchKnn(tknnEngine e, const tknnBatchKnnOptions *o, tknnBatchKnnInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
