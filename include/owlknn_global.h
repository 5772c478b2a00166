/*
 * owlknn_global.h -- the middle of a registration: nearest and second-nearest rows of feature vectors (tknnFeatureMatch) and RANSAC
 * over the correspondences they give (tknnRansac), two entry points of libowl_mi355x.so on top of the C ABI of owlknn.h.  With them
 * normals (tknnLocalPca) -> descriptors (tknnFpfh) -> match -> ransac -> tknnIcp(init) never leaves the device.  Plain C99; link and
 * load as owlknn.h says.
 *
 * Both calls take an engine for its device, its stream order and its workspace only: they need NO built tree, and leave a tree, a
 * halo tree and the state of tknnSolve untouched.  The host reads no array of the caller.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- feature matching ------------------------------------------------------------------------------------------------------------------
 * tknnFeatureMatch gives every source row its nearest and second-nearest target row in D <= 64 dimensions, by brute force.
 *   inputs     d_source: m rows, d_target: n rows, each D packed fp32 (a row starts D floats after the one before it).
 *   distance   acc = 0; for c = 0 .. D-1: t = a_c - b_c; acc = acc + t*t -- every operation fp32 and rounded on its own, in channel
 *              order.  Not |a|^2 + |b|^2 - 2 a.b: rows of an FPFH sum to 300 and near neighbours differ by little.
 *   left out   a row with an entry that is not finite matches nobody and nobody matches it.
 *   outputs    each may be NULL, at least one must be given:
 *              d_best (m int32): the target row with the smallest acc, ties to the smaller row; -1 for a source row left out, and
 *                when no target row is left;
 *              d_best_d2 (m fp32): that acc, +inf where d_best = -1;
 *              d_second_d2 (m fp32): the smallest acc over the target rows other than d_best[i] -- equal to d_best_d2 when a
 *                duplicate exists, +inf when no other row is left (n = 1) and where d_best = -1.
 * info: pair_tests = (m - bad_source_rows) * (n - bad_target_rows); bad_source_rows, bad_target_rows: the rows left out; chunks: the
 * target is split into that many ranges of rows, a source row's partial results merged over them (TKNN_MATCH_CHUNK=<rows> in the
 * environment, read per call, forces the range's length; no result depends on it); solve_ms: all of it; match_ms: the distances;
 * merge_ms: the merge.  TKNN_MATCH_ROWS=4 in the environment, read per call, selects the register tile of four source rows per lane
 * that was measured against the two in use (D <= 36 only); no result depends on it.
 * Errors, in this order:
 *   1. NULL engine / options / info; no output given; d_source NULL with m > 0; d_target NULL with n > 0: TKNN_E_ARG;
 *   2. D outside 1 .. 64; m or n negative or >= 2^31 - 1; an unknown flag: TKNN_E_ARG;
 *   3. m = 0 succeeds with a zeroed info; n = 0 succeeds with every row -1, +inf, +inf.
 * A refused call writes nothing, info included. */
#define TKNN_MATCH_MAX_D 64
typedef struct {
  int64_t m, n;              /* source rows, target rows */
  const float *d_source;     /* m x D */
  const float *d_target;     /* n x D */
  int32_t D;                 /* 1 .. TKNN_MATCH_MAX_D */
  uint32_t flags;            /* no flag is defined: 0 */
  int32_t *d_best;           /* m, may be NULL */
  float *d_best_d2;          /* m, may be NULL */
  float *d_second_d2;        /* m, may be NULL */
} tknnFeatureMatchOptions;
typedef struct {
  int64_t pair_tests;
  int64_t bad_source_rows, bad_target_rows;
  int32_t chunks;
  float solve_ms, match_ms, merge_ms;
} tknnFeatureMatchInfo;
TKNN_API int tknnFeatureMatch(tknnEngine e, const tknnFeatureMatchOptions *o, tknnFeatureMatchInfo *info, void *stream);

/* ---- RANSAC over correspondences ----------------------------------------------------------------------------------------------------------
 * tknnRansac finds the rigid transform T (4 x 4 row-major double, source frame -> target frame) that most of c correspondences agree
 * with: what registration_ransac_based_on_feature_matching and SampleConsensusPrerejective of the point-cloud libraries give.
 *   inputs     d_source: ms packed fp32 triples, d_target: mt; d_pairs: c x 2 int32 (source row, target row).
 *   staging    record i is (s, p) = (source[pairs[i][0]], target[pairs[i][1]]).  A row outside [0, ms) or [0, mt) refuses the call.
 *   trial t    key = h(seed + 0x9e3779b9 * (uint32)t), with h(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16
 *              (uint32).  Slot s = 0 .. ransac_n-1 draws a = 0 .. 7: u = h(key ^ (0x85ebca6b * (8*s + a + 1))),
 *              index = ((uint64)u * c) >> 32, and takes the first index that differs from every earlier slot's; none of the eight
 *              does: status TKNN_RANSAC_DUPLICATE.
 *   edges      edge_similarity sim > 0: for every pair (i, j) of the sample ds = sqrt(|s_i - s_j|^2), dt = sqrt(|p_i - p_j|^2), fp32
 *              and uncontracted, the square as (x*x + y*y) + z*z; unless ds >= sim*dt and dt >= sim*ds for all: TKNN_RANSAC_EDGE.
 *   solve      Kabsch / Horn on the sample in double, coordinates relative to the centroid of the staged target records, with
 *              tknnIcp's solver and its degenerate rule (owlknn_icp.h): TKNN_RANSAC_DEGENERATE.  The top three rows of T are rounded
 *              to fp32 and applied as tknnIcp applies them: s'.x = ((Tf00*x + Tf01*y) + Tf02*z) + Tf03.
 *   distance   d = sqrt((dx*dx + dy*dy) + dz*dz) of s' and p in fp32.  A sample member with d > max_dist: TKNN_RANSAC_FAR.
 *   score      a trial that is TKNN_RANSAC_OK counts its inliers: the records with d <= max_dist, all c of them.  The best trial
 *              has the most inliers, ties to the smaller trial; nothing float decides it.
 *   batches    trials run in order in batches of TKNN_RANSAC_BATCH; after each, f = best inliers / c and
 *              needed = log(1 - confidence) / log(1 - f^ransac_n) in double (f = 0 or confidence = 1: infinite); the loop stops
 *              once trials_run >= min(max_trials, needed).  A trial's result does not depend on its batch.
 *   refit      up to refit_rounds times: the inliers under T and their fp64 moments (tknnIcp's point-to-point pass, L2), one step
 *              dT of tknnIcp's solver, T' = dT T; kept if its inlier count is not smaller, else (or at a degenerate system) the
 *              refit stops.
 *   evaluation inliers, fitness = inliers / c, inlier_rmse = sqrt(sum d^2 / inliers) under the final T, d^2 of the fp32 values s'
 *              and p in double, summed in a fixed order: two runs agree bit for bit.  (The sum is taken for the final T and for
 *              each refit only, not per trial: no trial's rank needs it.)
 *   outputs    info; and on the device, each may be NULL: d_inlier_mask (c uint8, 1 where d <= max_dist under the final T),
 *              d_trial_status (max_trials int32: the status, -1 where the trial was not run), d_trial_inliers (max_trials int32:
 *              the count, -1 where the trial was not scored or not run).
 *              No trial TKNN_RANSAC_OK (c < ransac_n among the reasons: no trial is run then): transform = identity,
 *              best_trial = -1, inliers = 0, the mask zero, and the call succeeds.
 * info: transform; best_trial; inliers, fitness, inlier_rmse; trials_run, batches; status_counts by status; refits_kept; solve_ms: all
 * of it; sample_ms: the trials' kernel; score_ms: scoring and the best; refit_ms: evaluation and refit.
 * TKNN_RANSAC_SCORE=tile in the environment, read per call, selects the scoring kernel that was measured against the one in use
 * (survivors x record chunks through LDS instead of a wave per survivor; up to 2^26 pairs); no result depends on it.
 * Errors, in this order:
 *   1. NULL engine / options / info; d_source NULL with ms > 0; d_target NULL with mt > 0; d_pairs NULL with c > 0: TKNN_E_ARG;
 *   2. ransac_n not 3 or 4; max_dist not > 0 or not finite; edge_similarity outside [0, 1]; confidence outside (0, 1];
 *      max_trials < 1; refit_rounds outside 0 .. 8; ms, mt or c negative or >= 2^31 - 1; an unknown flag: TKNN_E_ARG;
 *   3. a pair row out of range (found on the device, before anything the caller can see is written): TKNN_E_ARG.
 * A refused call writes nothing, info included. */
#define TKNN_RANSAC_BATCH 4096
#define TKNN_RANSAC_OK 0
#define TKNN_RANSAC_DUPLICATE 1
#define TKNN_RANSAC_EDGE 2
#define TKNN_RANSAC_DEGENERATE 3
#define TKNN_RANSAC_FAR 4
typedef struct {
  int64_t ms, mt, c;          /* source points, target points, correspondences */
  const float *d_source;      /* ms x 3 */
  const float *d_target;      /* mt x 3 */
  const int32_t *d_pairs;     /* c x 2: source row, target row */
  int32_t ransac_n;           /* 3 or 4 */
  float max_dist;             /* > 0 and finite */
  float edge_similarity;      /* 0 .. 1; 0: no edge check */
  int32_t max_trials;         /* >= 1 */
  double confidence;          /* in (0, 1]; 1: never stop early */
  uint32_t seed;
  int32_t refit_rounds;       /* 0 .. 8 */
  uint32_t flags;             /* no flag is defined: 0 */
  int32_t pad_;
  uint8_t *d_inlier_mask;     /* c, may be NULL */
  int32_t *d_trial_status;    /* max_trials, may be NULL */
  int32_t *d_trial_inliers;   /* max_trials, may be NULL */
} tknnRansacOptions;
typedef struct {
  double transform[16];       /* row-major, source frame -> target frame */
  double fitness, inlier_rmse;
  int64_t inliers;
  int64_t status_counts[5];   /* by TKNN_RANSAC_OK .. TKNN_RANSAC_FAR, over the trials run */
  int32_t best_trial;         /* -1: no trial was TKNN_RANSAC_OK */
  int32_t trials_run, batches, refits_kept;
  float solve_ms, sample_ms, score_ms, refit_ms;
} tknnRansacInfo;
TKNN_API int tknnRansac(tknnEngine e, const tknnRansacOptions *o, tknnRansacInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
