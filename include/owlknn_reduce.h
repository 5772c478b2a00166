/*
 * owlknn_reduce.h -- weighted sums over the points within a radius of each query, without the lists (tknnRadiusReduce), an entry
 * point of libowl_mi355x.so on top of the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- neighbourhood reduction within a radius ---------------------------------------------------------------------------------------
 * tknnRadiusReduce gives, for every query q_j, sums over the points of the built set P within `radius` of it: how many there are, the
 * sum of a kernel weight of their distance, and the weighted sum of per-point values -- a density or a kernel density estimate, an
 * SPH field, a kernel-weighted mean of features (a mean-shift step, a bilateral filter, Nadaraya-Watson regression).  No (query,
 * neighbour) pair is written to memory.  The tree is any built point tree (tknnBuild, tknnBuildIds, tknnBuildBatched).
 *   queries    d_queries: m packed fp32 triples, addressed by the caller's j, as in tknnRadiusQuery.  d_queries == NULL: the set's
 *              own n points are the queries; then m must equal n and the results are addressed by the caller's row.  (The walk
 *              takes the own points in sorted-slot order; no pass orders them.)
 *   neighbours the points p of P with sqrt((dx*dx + dy*dy) + dz*dz) <= radius, every operation fp32 and uncontracted: the literal
 *              predicate of tknnRadiusQuery, so d_counts[j] is that call's row length.  Nothing is "self": a point of P that
 *              coincides with q_j is a neighbour at distance 0.  flags & TKNN_REDUCE_SKIP_SELF, allowed only with d_queries ==
 *              NULL, leaves the query's own slot out; coinciding duplicates stay in.  A query with a NaN coordinate has no
 *              neighbours; NaN points of P are nobody's neighbour.  On a batched tree the labels are IGNORED, as tknnRadiusQuery
 *              ignores them: the neighbours come from every cloud.  One radius > 0 per call.
 *   weight     with d2 the fp32 ((dx*dx + dy*dy) + dz*dz), d its fp32 root and r the radius, a neighbour's weight w is
 *                TKNN_W_ONE            1
 *                TKNN_W_GAUSS          exp(d2 * c), c = (float)(-0.5 / ((double)h * h)), h = bandwidth (finite, > 0), truncated at r
 *                TKNN_W_EPANECHNIKOV   max(0, 1 - d2 * (float)(1.0 / ((double)r * r)))
 *                TKNN_W_CUBIC_SPLINE   the SPH M4 spline on support r: with s = d * (float)(2.0 / r),
 *                                      1 - 1.5 s^2 + 0.75 s^3 for s <= 1, max(0, 0.25 (2 - s)^3) above
 *              evaluated in fp32.  All four are unnormalised, w <= 1: the constant of the dimension is the caller's to apply.
 *              (A bandwidth so small that c is not finite gives what IEEE arithmetic gives.)
 *   values     d_values: n x channels floats, row-major BY THE CALLER'S ROW -- never by id, also on trees built with ids.
 *              channels = C in 0 .. 16; C = 0 takes no values: only counts and weight sums are produced.
 *   outputs    at least one, all addressed by j (own points: by the caller's row):
 *                d_counts  m int32: the neighbours;
 *                d_wsum    m float: the sum of w;
 *                d_out     m x C float: the sum of w * v_c; required iff C > 0, not written with C = 0.
 *              flags & TKNN_REDUCE_NORMALIZE: d_out holds (sum of w * v_c) / (sum of w), and exactly 0 where the sum of w as the
 *              device has it is 0; d_wsum stays the unnormalised sum.  (Values = the coordinates, a Gauss weight: one mean-shift
 *              step.)
 *   arithmetic accumulation is fp32, its order unspecified: the last bits of a sum may differ between the two kernels named under
 *              info.  No floating-point atomics: a row is summed by the one team, or the one lane, that walks it.
 *              A value is multiplied by its weight only for a point that passed the predicate -- values of points outside the
 *              sphere, of the skipped self and of NaN points never reach an accumulator, whatever they hold --; a NaN or inf
 *              value of a true neighbour propagates by IEEE rules.  With TKNN_W_ONE d_wsum is the count as a float.
 * The host reads no array of the caller.  The tree, the state of tknnSolve and a halo tree are not modified.
 *
 * info: total = the sum of the counts; max_row = the largest; fallback_items = the queries whose sums were made by the
 * one-query-per-lane kernel, which takes the walks whose stack ran out (TKNN_REDUCE_FORCE_FALLBACK=1 in the environment, read per
 * call: every query, so fallback_items = m); node_tests, point_tests (informational); order_ms: ordering the queries along the
 * tree's curve (0 for the own points); stage_ms: gathering d_values into sorted-slot order (0 with C = 0); walk_ms: the walks;
 * solve_ms: all of it.
 * Errors, in this order:
 *   1. NULL engine / options; no output at all (d_counts, d_wsum and d_out all NULL); d_queries NULL with m != n: TKNN_E_ARG;
 *   2. not built, or a box tree: TKNN_E_STATE;
 *   3. radius not > 0 or not finite; weight not one of the four; an unknown flag; with TKNN_W_GAUSS a bandwidth not > 0 or not
 *      finite; channels outside 0 .. 16; channels > 0 without d_values or without d_out; channels = 0 with neither d_counts nor
 *      d_wsum; TKNN_REDUCE_SKIP_SELF with d_queries; m < 0 or m >= 2^31 - 1: TKNN_E_ARG;
 *   4. m = 0 succeeds with a zeroed info.
 * A refused call writes nothing, info included. */
#define TKNN_REDUCE_NORMALIZE 1u
#define TKNN_REDUCE_SKIP_SELF 2u
enum { TKNN_W_ONE = 0, TKNN_W_GAUSS = 1, TKNN_W_EPANECHNIKOV = 2, TKNN_W_CUBIC_SPLINE = 3 };
#define TKNN_REDUCE_MAX_CHANNELS 16
typedef struct {
  int64_t m;                /* queries; with d_queries NULL: n */
  float radius;             /* > 0, finite */
  float bandwidth;          /* TKNN_W_GAUSS: h, > 0, finite; otherwise not read */
  int32_t weight;           /* TKNN_W_* */
  int32_t channels;         /* C, 0 .. 16 */
  uint32_t flags;           /* TKNN_REDUCE_NORMALIZE | TKNN_REDUCE_SKIP_SELF */
  int32_t pad_;
  const float *d_queries;   /* m x 3, or NULL: the set's own points */
  const float *d_values;    /* n x C by the caller's row; NULL with C = 0 */
  int32_t *d_counts;        /* m, may be NULL */
  float *d_wsum;            /* m, may be NULL */
  float *d_out;             /* m x C, required iff C > 0 */
} tknnRadiusReduceOptions;
typedef struct {
  int64_t total;            /* sum of the counts */
  int64_t max_row;          /* largest count */
  int64_t fallback_items;   /* queries summed by the lane kernel */
  int64_t node_tests;       /* informational */
  int64_t point_tests;      /* informational */
  float solve_ms, order_ms, stage_ms, walk_ms;
} tknnRadiusReduceInfo;
TKNN_API int tknnRadiusReduce(tknnEngine e, const tknnRadiusReduceOptions *o, tknnRadiusReduceInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
