/*
 * owlknn_plane.h -- RANSAC plane segmentation of the built point set, scored through the box pyramid (tknnSegmentPlane), an entry point
 * of libowl_mi355x.so on top of the C ABI of owlknn.h: what segment_plane(distance_threshold, ransac_n = 3, num_iterations) and
 * SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE of the point-cloud libraries give.  Plain C99; link and load as
 * owlknn.h says.
 *
 *   tree       a built point tree without ids, as tknnIcp requires (a row is named by the caller's row).  The labels of a batched tree
 *              and a halo tree are ignored.  The tree, the halo tree and the state of tknnSolve are not modified.
 *   active     d_active (n uint8 by the caller's row, may be NULL): row r is active iff (d_active is NULL or d_active[r] != 0) and its
 *              three coordinates are finite.  The active rows ascending are the list A of length c (info.active).  Only active rows
 *              are sampled, scored and reported: a caller takes several planes out of one tree by clearing the rows it has found.
 *   trial t    ransac_sample(seed, t, 3, c, idx) of tknnRansac (owlknn_global.h: "trial t"), unchanged, draws three indices into A;
 *              none among a slot's eight draws: TKNN_PLANE_DUPLICATE.  No trial runs when c < 3.
 *   plane      of the sample (p0, p1, p2) = (A[idx[0]], A[idx[1]], A[idx[2]]), fp32, every operation rounded on its own (no fma):
 *              e1 = p1 - p0, e2 = p2 - p0; g = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x);
 *              l1 = (e1x*e1x + e1y*e1y) + e1z*e1z, l2 likewise of e2, g2 = (gx*gx + gy*gy) + gz*gz;
 *              unless g2 is finite and g2 > 2^-40 * (l1 * l2): TKNN_PLANE_DEGENERATE.  n = (gx / q, gy / q, gz / q) with q = sqrt(g2)
 *              (division and square root correctly rounded), the anchor a = p0.
 *   axis       axis not all zero: the host normalises it in double (x / sqrt((x*x + y*y) + z*z)) and rounds to fp32: A^.  Unless
 *              |(nx*A^x + ny*A^y) + nz*A^z| >= min_cos (fp32, as above): TKNN_PLANE_ANGLE.  An all-zero axis: no constraint, min_cos
 *              is not read.  (min_cos near 1 and axis = up: the ground plane of the perpendicular-plane model.)
 *   distance   of row x = (x, y, z): d = |(nx*(x - ax) + ny*(y - ay)) + nz*(z - az)|, fp32, the three differences rounded first: the
 *              anchor keeps the cancellation local, a cloud far from the origin loses nothing.  x is an inlier iff d <= distance_threshold.
 *   score      a TKNN_PLANE_OK trial's score is its inlier count over all of A.  The best trial has the most inliers, ties to the
 *              smaller trial; nothing float decides it.
 *   batches    trials run in order in batches of TKNN_PLANE_BATCH; after each, f = best inliers / c and
 *              needed = log(1 - confidence) / log(1 - f^3) in double (f = 0 or confidence = 1: infinite); the loop stops once
 *              trials_run >= min(max_trials, needed).  A trial's result does not depend on its batch.
 *   refit      up to refit_rounds times, from the best trial's plane: the inliers of the current plane, their count m, the sums S1
 *              and the sums of products S2 of their coordinates relative to the centre of the scene box -- (double)x - cx with
 *              cx = 0.5 * ((double)lo + (double)hi) of the built set's bounding box (points with a NaN left out), 0 on an axis
 *              where that is not finite --; fp64, summed in a fixed order (per lane in
 *              steps of the grid, the lanes of a wave by xor-shuffles 1, 2, .. 32, the waves of a workgroup and then the workgroups in
 *              index order): two runs on one tree agree bit for bit.  mean = S1 / m; cov_uv = S2_uv / m - mean_u * mean_v.
 *              Eigen-solver (plane_solve.h, host, double, no fma): cyclic Jacobi on the symmetric 3 x 3 cov, V = I, exactly 12
 *              sweeps, each sweep the pairs (p, q) = (0,1), (0,2), (1,2) in this order; a pair with a_pq == 0 is skipped; else
 *              theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta*theta + 1)) (sign(0) = 1), c = 1 / sqrt(t*t + 1),
 *              s = t*c; a_pp -= t*a_pq, a_qq += t*a_pq, a_pq = 0, and for the third index r: (a_rp, a_rq) <- (c*a_rp - s*a_rq,
 *              s*a_rp + c*a_rq); the columns p, q of V are rotated likewise.  The eigenvalues are the diagonal, l0 <= l1 <= l2 by
 *              value (ties to the smaller column).  The refit stops unless every entry is finite and l1 - l0 > 2^-40 * l2.  The new
 *              normal is column l0 of V divided by its length, the new anchor is mean + centre; both rounded to fp32 once.  The
 *              refit plane is scored with the distance expression above; it is kept iff its inlier count is not smaller, else the
 *              refit stops.
 *              Tolerance: the order of the fp64 sums is fixed but is the device's, so a host restatement that sums in another order
 *              sees moments that differ by at most m * 2^-52 * R^2 per entry, R the half diagonal of the scene box (each of m
 *              products is at most R^2 and a sum of m terms carries at most m roundings of 2^-53 relative each, the division and
 *              the subtraction two more); by Davis-Kahan the eigenvector then turns by at most 2 |dC|_F / (l1 - l0), so each
 *              component of the fp32 normal is within 2^-23 + 6 * m * 2^-52 * R^2 / (l1 - l0) of a restatement's, each component
 *              of the anchor within 2^-23 * max(|anchor|, R) + m * 2^-52 * R.  info.normal and info.anchor are the fp32 values used:
 *              everything that follows from them -- inliers, the mask, the rows, inlier_rmse -- is exact under the distance expression.
 *   outputs    info.plane = (a, b, c, d) in double with a*x + b*y + c*z + d = 0 in the caller's frame: (a, b, c) = the fp32 normal
 *              times the sign below, d = -((a*ax + b*ay) + c*az) in double of the fp32 anchor.  Sign: with an axis,
 *              (a*A^x + b*A^y) + c*A^z (double) is made positive; where it is zero, and with no axis, the first nonzero of (a, b, c)
 *              is made positive.  info.normal has the same sign.
 *              On the device, each may be NULL: d_inlier_mask (n uint8 by the caller's row: 1 for an inlier of the final plane,
 *              else 0, inactive rows 0), d_inlier_rows (n int32: the inlier rows ascending, then -1), d_trial_status (max_trials
 *              int32: the status, -1 where the trial was not run), d_trial_inliers (max_trials int32: the count, -1 where the trial
 *              was not scored or not run).
 *              No trial TKNN_PLANE_OK (c < 3 among the reasons): plane, normal, anchor all zero, best_trial = -1, inliers = 0,
 *              fitness = 0, inlier_rmse = 0, the mask zero, the rows -1, and the call succeeds.
 * info: plane; fitness = inliers / c (0 when c = 0); inlier_rmse = sqrt(sum d^2 / inliers), d the fp32 distance squared in double, summed
 * in the fixed order of the refit (within (inliers + 2) * 2^-53 of any other order's, relatively: the terms are not negative);
 * inliers; active = c; status_counts by status over the trials run; node_tests: child boxes put to
 * the slab test; point_tests: active rows put to the distance expression while scoring trials (the fallback: c per trial);
 * boxes_counted: rows a trial's score took from a box wholly inside the slab, by arithmetic; lane_rows: of point_tests, those of the
 * fallback kernel; best_trial; trials_run, batches, refits_kept; solve_ms: all of it; sample_ms: active list and the trials' planes;
 * score_ms: scoring and the best; refit_ms: evaluation, refit and the outputs.
 * The scoring walk is used when the tree has more than 64 points; TKNN_PLANE_FORCE_FALLBACK=1 in the environment, read
 * per call, scores every trial against every active row with no tree; no result but the four work counters depends on it.
 * Errors, in this order:
 *   1. NULL engine / options / info: TKNN_E_ARG;
 *   2. no built point tree (a box tree among the reasons): TKNN_E_STATE; a tree with ids, or one of more than 2^31 - 65 points:
 *      TKNN_E_UNSUPPORTED;
 *   3. distance_threshold not > 0 or not finite; max_trials < 1; confidence outside (0, 1]; refit_rounds outside 0 .. 8; an axis
 *      entry that is not finite; min_cos outside (0, 1] with a nonzero axis; an unknown flag: TKNN_E_ARG, in this order.
 * A refused call writes nothing, info included.  A successful one writes every word of every output it was given and nothing else.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TKNN_PLANE_BATCH 1024
#define TKNN_PLANE_OK 0
#define TKNN_PLANE_DUPLICATE 1
#define TKNN_PLANE_DEGENERATE 2
#define TKNN_PLANE_ANGLE 3
typedef struct {
  const uint8_t *d_active;    /* n by the caller's row, may be NULL: every row */
  float distance_threshold;   /* > 0 and finite */
  float min_cos;              /* in (0, 1]; read with a nonzero axis only */
  float axis[3];              /* all zero: no constraint */
  int32_t max_trials;         /* >= 1 */
  double confidence;          /* in (0, 1]; 1: never stop early */
  uint32_t seed;
  int32_t refit_rounds;       /* 0 .. 8 */
  uint32_t flags;             /* no flag is defined: 0 */
  int32_t pad_;
  uint8_t *d_inlier_mask;     /* n, may be NULL */
  int32_t *d_inlier_rows;     /* n, may be NULL */
  int32_t *d_trial_status;    /* max_trials, may be NULL */
  int32_t *d_trial_inliers;   /* max_trials, may be NULL */
} tknnPlaneOptions;
typedef struct {
  double plane[4];            /* a, b, c, d: a*x + b*y + c*z + d = 0, (a, b, c) of unit length */
  double fitness, inlier_rmse;
  int64_t inliers, active;
  int64_t status_counts[4];   /* by TKNN_PLANE_OK .. TKNN_PLANE_ANGLE, over the trials run */
  int64_t node_tests, point_tests, boxes_counted, lane_rows;
  float normal[3], anchor[3]; /* the fp32 plane the final inliers were taken with */
  int32_t best_trial;         /* -1: no trial was TKNN_PLANE_OK */
  int32_t trials_run, batches, refits_kept;
  float solve_ms, sample_ms, score_ms, refit_ms;
} tknnPlaneInfo;
TKNN_API int tknnSegmentPlane(tknnEngine e, const tknnPlaneOptions *o, tknnPlaneInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
