/*
 * owlknn_periodic.h -- the k nearest neighbours in a periodic cell (tknnPeriodicKnn), an entry point of libowl_mi355x.so on top
 * of the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- at most k nearest points under a per-axis periodic metric ----------------------------------------------------------
 * tknnPeriodicKnn is tknnRadiusKnn and tknnKnn in a periodic cell: the at most k nearest points of the built set P (n points),
 * as dense rows of k, for m arbitrary points Q or for the points of P themselves; rows may carry a radius.  The tree is the
 * one tknnBuild made -- no shifted copies, every point is met once.
 *   the cell   lo[3], period[3]; axis a is periodic iff period[a] > 0, 0 means open (2-D data: period[2] = 0).  A value x is
 *              IN the cell on a periodic axis iff x >= lo[a] && fl(x - lo[a]) <= period[a].  The built set must lie in the
 *              cell on every periodic axis; nothing is wrapped for the caller.  (scipy's cKDTree(data, boxsize = L): lo = 0,
 *              period = L.)
 *   the metric for a point p and a query q, every operation fp32 and uncontracted: per axis a = |fl(p_a - q_a)|, w_a = a on an
 *              open axis and min(a, |fl(period[a] - a)|) on a periodic one; d2 = (w_x*w_x + w_y*w_y) + w_z*w_z, d = sqrt(d2).
 *              With no periodic axis this is tknnKnn's distance bit for bit.  A NaN coordinate on either side: no neighbour.
 *   row j      the points p of P that are eligible for q_j, ascending in (d, index) -- fully determined, ties at the k-th place
 *              are decided by the index --, cut after k; written at d_idx[j * k ..] (and d_dist[j * k ..]), the unused tail
 *              of a row is idx = -1, dist = +inf.  Eligible: d is finite and d <= r_j (a distance exactly r_j is inside); p is
 *              not the point d_skip_ids[j] names; q_j is in the cell on every periodic axis -- a query outside the cell, or one
 *              with a NaN, has an empty row.  Every point appears at most once in a row, also where the k-th distance exceeds
 *              half a period (small sets): the row is the literal minimum over the formula.
 *   d_counts[j] = min(k, the eligible points of row j).
 * An entry names its point by id on trees built with tknnBuildIds, by row otherwise.
 * The radius: `radius` is finite and > 0, FLT_MAX means none; or d_radii, m floats, r_j = d_radii[j] -- a NaN, non-finite or
 * <= 0 entry gives an empty row (the host never reads them), and `radius` is then ignored.
 * External queries (d_queries given, m rows): nothing is "self" unless d_skip_ids says so, as tknnRadiusKnn takes it -- a
 * negative value skips nothing.
 * The set's own points (d_queries == NULL): row j answers for the point in row j of the buffer given to tknnBuild; m must equal
 * n and d_skip_ids must be NULL; every point is left out of its own row (by its id on trees built with tknnBuildIds, by its row
 * otherwise), a coinciding duplicate stays, at distance 0; d_radii is indexed by row.
 * k may exceed the number of eligible points.  A halo tree, if set, is ignored; the tree and the state of tknnSolve are not
 * modified; results are addressed by the caller's j whatever order the engine works in.
 * info: as tknnKnnInfo counts them; seed_point_tests is 0 exactly when no seed pass ran (it runs when there is no radius at all:
 * d_radii == NULL and radius == FLT_MAX).
 * Errors, in this order: NULL engine / options / d_idx, d_queries NULL with m != n, d_skip_ids given with d_queries NULL:
 * TKNN_E_ARG; not built: TKNN_E_STATE; k < 1, m < 0, m >= 2^31 - 1: TKNN_E_ARG; k > TKNN_MAX_K_REGISTERS: TKNN_E_UNSUPPORTED;
 * a period[a] that is NaN, negative or infinite, a non-finite lo[a] on a periodic axis, without d_radii a radius that is NaN,
 * <= 0 or infinite: TKNN_E_ARG; the box of the built set (NaN points ignored) not in the cell on a periodic axis: TKNN_E_ARG,
 * the message names the axis.  A refused call writes nothing.  m = 0 with d_queries given succeeds with a zeroed info. */
typedef struct {
  const float *d_queries;     /* m packed fp32 triples (2-D data: z = 0), or NULL: the set's own points, m = n */
  int64_t m;
  int32_t k;                  /* 1 .. TKNN_MAX_K_REGISTERS; k > n is allowed (rows are then never full) */
  float radius;               /* every row's radius if d_radii is NULL: finite and > 0, FLT_MAX = none */
  const float *d_radii;       /* NULL, or m floats (self mode: by row) */
  const int32_t *d_skip_ids;  /* NULL, or (external queries only) m int32; a negative value skips nothing */
  float lo[3];                /* the cell's lower corner (read on periodic axes only) */
  float period[3];            /* the cell's periods; 0 = an open axis */
  int32_t *d_idx;             /* m*k, required */
  float *d_dist;              /* m*k, may be NULL */
  int32_t *d_counts;          /* m, may be NULL */
} tknnPeriodicKnnOptions;
typedef struct {
  int64_t total;              /* entries over all rows = sum of d_counts */
  int64_t full_rows;          /* rows with k entries */
  int64_t node_tests, point_tests; /* the walk's */
  int64_t seed_point_tests;   /* points read for the seed bounds (0: no seed pass) */
  int64_t tightened_rows;     /* full rows whose final k-th distance is below their radius or seed bound */
  int64_t lane_rows;          /* rows the one-query-per-lane kernel answered */
  float solve_ms, order_ms, seed_ms, walk_ms;
} tknnPeriodicKnnInfo;
TKNN_API int tknnPeriodicKnn(tknnEngine e, const tknnPeriodicKnnOptions *o, tknnPeriodicKnnInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
