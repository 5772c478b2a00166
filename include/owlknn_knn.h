/*
 * owlknn_knn.h -- exact k nearest neighbours without a radius (tknnKnn), an entry point of libowl_mi355x.so on top of the C ABI
 * of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the k nearest points, exactly, with no radius to choose ------------------------------------------------------------
 * tknnKnn returns the k nearest points of the built set P (n points), as dense rows of k, for m arbitrary points Q or for the
 * points of P themselves.  The caller gives no radius: the points around a query's place on the tree's curve give an upper bound
 * of its k-th distance, and one walk of tknnRadiusKnn's kind, started with that bound, finds the row.
 *   row j  is the row tknnRadiusKnn gives q_j at radius = FLT_MAX, the largest finite float.  Spelled out: the points p of P
 *          whose distance sqrt((dx*dx + dy*dy) + dz*dz), every operation fp32 and uncontracted, is finite, ascending in (fp32
 *          distance, index) -- fully determined, ties at the k-th place are decided by the index --, cut after k.  It is written
 *          at d_idx[j * k ..] (and d_dist[j * k ..]); the unused tail of a row is idx = -1, dist = +inf.
 *   d_counts[j] = min(k, the eligible points of row j).
 * An entry names its point by id on trees built with tknnBuildIds, by row otherwise.
 * External queries (d_queries given, m rows): nothing is "self" unless d_skip_ids says so, exactly as tknnRadiusKnn takes it --
 * the point named d_skip_ids[j] (by id on trees built with tknnBuildIds, by row otherwise) is left out of row j and of its
 * count, a negative value skips nothing.  A query with a NaN coordinate has an empty row; NaN points of P are nobody's
 * neighbour.  Queries may lie anywhere, far outside the box of P included.
 * The set's own points (d_queries == NULL): row j answers for the point in row j of the buffer given to tknnBuild; m must equal
 * n and d_skip_ids must be NULL.  Every point is left out of its own row (by its id on trees built with tknnBuildIds, by its row
 * otherwise), while another point that coincides with it stays, at distance 0: the exact all-kNN of the set in one call, what
 * tknnSolveEx + tknnRepairExact return where their rows are finished and the distances finite.
 * k may exceed the number of eligible points (rows are then not full).  A halo tree, if set, is ignored; the tree and the state
 * of tknnSolve are not modified; results are addressed by the caller's j whatever order the engine works in.
 * info: total = the sum of d_counts, full_rows the rows with k entries, node_tests / point_tests the walk's, as the other calls
 * count them; seed_point_tests the points read around the queries' places on the curve for the bounds; tightened_rows the rows
 * whose final k-th distance lies below their seed bound; lane_rows the rows the one-query-per-lane kernel answered (team stack
 * exhausted, or a tree too small for a box pyramid); solve_ms the whole call, order_ms the ordering of the queries along the
 * tree's curve (external queries only), seed_ms the bounds, walk_ms the traversal kernels.
 * Errors, in this order: NULL engine / options / d_idx, d_queries NULL with m != n, d_skip_ids given with d_queries NULL:
 * TKNN_E_ARG; not built: TKNN_E_STATE; k < 1, m < 0, m >= 2^31 - 1: TKNN_E_ARG; k > TKNN_MAX_K_REGISTERS: TKNN_E_UNSUPPORTED.
 * m = 0 with d_queries given succeeds with a zeroed info. */
typedef struct {
  const float *d_queries;     /* m packed fp32 triples (2-D data: z = 0), or NULL: the set's own points, m = n */
  int64_t m;
  int32_t k;                  /* 1 .. TKNN_MAX_K_REGISTERS; k > n is allowed (rows are then never full) */
  int32_t reserved_;
  const int32_t *d_skip_ids;  /* NULL, or (external queries only) m int32: the point named d_skip_ids[j] (id on trees built
                                 with ids, row otherwise) is left out of row j and of its count; a negative value skips nothing */
  int32_t *d_idx;             /* m*k, required */
  float *d_dist;              /* m*k, may be NULL */
  int32_t *d_counts;          /* m, may be NULL */
} tknnKnnOptions;
typedef struct {
  int64_t total;              /* entries over all rows = sum of d_counts */
  int64_t full_rows;          /* rows with k entries */
  int64_t node_tests, point_tests; /* the walk's */
  int64_t seed_point_tests;   /* points read for the seed bounds */
  int64_t tightened_rows;     /* rows whose final k-th distance is below their seed bound */
  int64_t lane_rows;          /* rows the one-query-per-lane kernel answered */
  float solve_ms, order_ms, seed_ms, walk_ms;
} tknnKnnInfo;
TKNN_API int tknnKnn(tknnEngine e, const tknnKnnOptions *o, tknnKnnInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
