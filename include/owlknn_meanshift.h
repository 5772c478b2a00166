/*
 * owlknn_meanshift.h -- mean-shift mode seeking over the built set (tknnMeanShift), an entry point of libowl_mi355x.so on top of
 * the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"
#include "owlknn_reduce.h" /* TKNN_W_* */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- mean shift ------------------------------------------------------------------------------------------------------------------------
 * tknnMeanShift moves every seed to the kernel-weighted mean of the points of the built set P within `radius` of it, again and
 * again, until the seed stops moving: the trajectories of sklearn's MeanShift.  The loop runs inside the call; the seeds that have
 * stopped leave the work list on the device, and no (seed, neighbour) pair is written to memory.  The tree is any built point tree
 * (tknnBuild, tknnBuildIds, tknnBuildBatched).
 *   tree       on a batched tree the labels are IGNORED, as tknnRadiusReduce ignores them: the neighbours come from every cloud.
 *              A tree with ids is fine: no point is looked up by row.  The tree, the state of tknnSolve and a halo tree are not
 *              modified.
 *   seeds      d_seeds: m packed fp32 triples, addressed by the caller's j.  d_seeds == NULL: the set's own n points are the seeds;
 *              then m must equal n and the results are addressed by the caller's row.  Nothing is "self": a seed that is a point
 *              of P has that point among its neighbours, at distance 0.
 *   one step   from the position x: the neighbours are the points p of P with sqrt((dx*dx + dy*dy) + dz*dz) <= radius, d = p - x,
 *              every operation fp32 and uncontracted: the literal predicate of tknnRadiusQuery at q = x, so the count is that
 *              call's row length.  A neighbour's weight w is TKNN_W_ONE, TKNN_W_GAUSS (with `bandwidth`, truncated at `radius`)
 *              or TKNN_W_EPANECHNIKOV exactly as owlknn_reduce.h defines them.  a = (sum w dx, sum w dy, sum w dz) over the fp32
 *              offsets, W = sum w (TKNN_W_ONE: the count as a float); the step is s = a / W, three fp32 divisions; x' = x + s;
 *              shift = sqrt((s.x*s.x + s.y*s.y) + s.z*s.z), fp32 and uncontracted.  The sums are over OFFSETS, not over
 *              coordinates: a cloud far from the origin loses nothing.
 *   arithmetic accumulation is fp32, its order unspecified: the last bits of a sum may differ between the two kernels named under
 *              info, never between two runs or two calls of the same kernel at the same position.  No floating-point atomics: a
 *              row is summed by the one team, or the one lane, that walks it.  A weight and an offset are multiplied only for a
 *              point that passed the predicate: NaN and infinite points of P are nobody's neighbour and reach no sum.
 *   loop       per seed, pass t = 0, 1, ...: walk at x.  A seed with a NaN coordinate: stop, TKNN_MS_INVALID (count 0, W 0).
 *              count = 0: stop, TKNN_MS_EMPTY, x unchanged.  shift is NaN (W underflowed to 0, or the sums overflowed): stop,
 *              TKNN_MS_INVALID, x unchanged, the step does not count, d_shift holds the NaN.  Otherwise x <- x', the step counts;
 *              shift <= tol: stop, TKNN_MS_CONVERGED; max_iterations steps taken: stop, TKNN_MS_RUNNING.  A seed that has stopped
 *              is never walked again.
 *   outputs    each may be NULL, at least one is given; all addressed by j (own points: by the caller's row):
 *                d_modes       m x 3 float: the final position;
 *                d_counts      m int32: the neighbours of the seed's LAST walk;
 *                d_wsum        m float: the W of that walk;
 *                d_shift       m float: the last shift, +inf where no step was taken;
 *                d_iterations  m int32: the steps taken;
 *                d_status      m uint8: TKNN_MS_*.
 * The host reads no array of the caller.
 *
 * info: iterations = the passes run (a pass walks every seed still moving); walks = the seed-walks summed over the passes (m times
 * the passes only if no seed stopped early); converged, empty, running, invalid: the seeds per status; fallback_items = the rows
 * whose sums were made by the one-query-per-lane kernel, which takes the walks whose stack ran out, summed over the passes
 * (TKNN_MEANSHIFT_FORCE_FALLBACK=1 in the environment, read per call: every row, so fallback_items = walks); node_tests,
 * point_tests (informational); order_ms: ordering the seeds along the tree's curve (TKNN_MEANSHIFT_REORDER=R in the environment,
 * read per call: again every R passes, from where the seeds are then; no result depends on it); walk_ms: the walks; compact_ms:
 * taking the stopped seeds out of the work list; solve_ms: all of it.
 * Errors, in this order:
 *   1. NULL engine / options / info; no output at all; d_seeds NULL with m != n: TKNN_E_ARG;
 *   2. not built, or a box tree: TKNN_E_STATE;
 *   3. radius not > 0 or not finite; weight not TKNN_W_ONE, TKNN_W_GAUSS or TKNN_W_EPANECHNIKOV (TKNN_W_CUBIC_SPLINE is refused);
 *      with TKNN_W_GAUSS a bandwidth not > 0 or not finite; tol negative or not finite; max_iterations < 1; an unknown flag;
 *      m < 0 or m >= 2^31 - 1: TKNN_E_ARG;
 *   4. m = 0 succeeds with a zeroed info.
 * A refused call writes nothing, info included. */
enum { TKNN_MS_RUNNING = 0, TKNN_MS_CONVERGED = 1, TKNN_MS_EMPTY = 2, TKNN_MS_INVALID = 3 };
typedef struct {
  int64_t m;                /* seeds; with d_seeds NULL: n */
  const float *d_seeds;     /* m x 3, or NULL: the set's own points */
  float radius;             /* > 0, finite */
  float bandwidth;          /* TKNN_W_GAUSS: h, > 0, finite; otherwise not read */
  float tol;                /* >= 0, finite */
  int32_t weight;           /* TKNN_W_ONE / TKNN_W_GAUSS / TKNN_W_EPANECHNIKOV */
  int32_t max_iterations;   /* >= 1 */
  uint32_t flags;           /* no flag is defined: 0 */
  float *d_modes;           /* m x 3, may be NULL */
  int32_t *d_counts;        /* m, may be NULL */
  float *d_wsum;            /* m, may be NULL */
  float *d_shift;           /* m, may be NULL */
  int32_t *d_iterations;    /* m, may be NULL */
  uint8_t *d_status;        /* m, may be NULL */
} tknnMeanShiftOptions;
typedef struct {
  int64_t iterations;       /* passes run */
  int64_t walks;            /* seed-walks, summed over the passes */
  int64_t converged, empty, running, invalid; /* seeds per status */
  int64_t fallback_items;   /* rows summed by the lane kernel, over the passes */
  int64_t node_tests;       /* informational */
  int64_t point_tests;      /* informational */
  float solve_ms, order_ms, walk_ms, compact_ms;
} tknnMeanShiftInfo;
TKNN_API int tknnMeanShift(tknnEngine e, const tknnMeanShiftOptions *o, tknnMeanShiftInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
