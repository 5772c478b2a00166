/*
 * owlknn_icp.h -- rigid registration of a cloud to the built set by iterated closest points (tknnIcp), an entry point of
 * libowl_mi355x.so on top of the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- iterated closest points -----------------------------------------------------------------------------------------------------------
 * tknnIcp aligns a source cloud to the points of the built set P (n points, the target): what registration_icp and
 * evaluate_registration of the point-cloud libraries give.  The loop -- transform, search, moments, solve -- runs inside the call; no
 * list and no per-pair array leaves it unless asked for, and the sums run in fp64.
 *   source     d_source: m packed fp32 triples.  The result is a rigid transform T, a 4 x 4 row-major double matrix that maps the
 *              source frame to the target frame.  init: a HOST pointer to 16 doubles, the T the loop starts from; NULL: the identity.
 *   tree       a built point tree WITHOUT ids (tknnBuild, tknnBuildBatched): a partner is named by the caller's row, and the step
 *              fetches its coordinates and its normal by that row.  On a batched tree the labels are IGNORED, as tknnKnn ignores
 *              them.  A halo tree is ignored.  The tree and the state of tknnSolve are not modified.
 *   applying T the top three rows of T are rounded to fp32 (Tf); s'_j.x = ((Tf00*x + Tf01*y) + Tf02*z) + Tf03, every operation
 *              fp32 and uncontracted, y and z likewise.  Every iteration applies the cumulative T to the ORIGINAL source.
 *   partner    c(j) is the row tknnRadiusKnn gives s'_j at k = 1 and radius = max_dist: the point of P with the smallest fp32
 *              distance sqrt((dx*dx + dy*dy) + dz*dz) <= max_dist, ties to the smaller row; -1 when no point lies within max_dist
 *              or a coordinate of s'_j is NaN.
 *   evaluation N = the j with a partner; fitness = N / m; inlier_rmse = sqrt(sum d^2 / N), 0 when N = 0, with d^2 the squared
 *              distance of the fp32 values s'_j and p_c(j), computed in double.
 *   one step   e_j is the residual, w_j its weight: TKNN_ICP_L2 w = 1; TKNN_ICP_HUBER w = 1 for e <= c, else c / e;
 *              TKNN_ICP_TUKEY w = (1 - (e/c)^2)^2 for e <= c, else 0; c = robust_scale (read only with Huber or Tukey).
 *              TKNN_ICP_POINT_TO_POINT: e = d; mu_s, mu_p the weighted centroids; H = sum w (s' - mu_s)(p - mu_p)^T = U S V^T;
 *                dR = V diag(1, 1, det(V U^T)) U^T, dt = mu_p - dR mu_s (the solver is Horn's quaternion form, which gives this dR).
 *                Degenerate: fewer than 3 pairs with w > 0, or the second-largest singular value of H not above 2^-40 times the
 *                largest (0 up to the rounding of the sums).
 *              TKNN_ICP_POINT_TO_PLANE: d_target_normals, n x 3 floats by the caller's row, is required; r = (s' - p) . n,
 *                e = |r|, J = [(s' - c) x n, n] with c the centre of P's scene box: the step turns about c, not about the origin,
 *                so its condition does not depend on where the cloud sits.  (sum w J^T J) x = -sum w J^T r is solved by Cholesky
 *                in double, x = (alpha, beta, gamma, t); dR = Rz(gamma) Ry(beta) Rx(alpha) and dT maps x to dR (x - c) + c + t.
 *                Degenerate: a pivot that is not finite or not above 2^-40 times its diagonal entry of the matrix (<= 0, up to the
 *                rounding of the sums).  A partner whose normal has a component that is not finite is left out of the system and
 *                counted in skipped_pairs; it stays in fitness and inlier_rmse.
 *              The sums of both methods are taken in double with the coordinates relative to c.  Then T <- dT T, in double.
 *   loop       1. search at T;  2. one moment pass: fitness, inlier_rmse and the step's system, from the same pairs;  3. not the
 *              first pass, |fitness - previous| < rel_fitness and |inlier_rmse - previous| < rel_rmse: stop, converged = 1;
 *              4. max_iterations steps taken: stop;  5. the system is degenerate: stop, degenerate = 1, T unchanged;  6. solve,
 *              update T, go to 1.  iterations = the steps taken (searches = iterations + 1); max_iterations = 0 is the evaluation
 *              at init.
 *   outputs    info; and on the device, each may be NULL: d_corr (m int32, c(j) of the last search), d_corr_dist (m floats, the
 *              fp32 distance, +inf where c(j) = -1), d_aligned (m x 3, the s' of the last search).
 * info: transform; fitness, inlier_rmse, correspondences (N), skipped_pairs of the last search; iterations, searches, converged, degenerate;
 * node_tests, point_tests, lane_rows (the rows the one-query-per-lane kernel answered: walks whose stack ran out, trees too small
 * for a box pyramid, every row under TKNN_ICP_FORCE_FALLBACK=1 in the environment, read per call) summed over the searches;
 * solve_ms: all of it; search_ms: transform, order, seed bounds and walks; moment_ms: the moment passes.
 * Errors, in this order:
 *   1. NULL engine / options / info; d_source NULL with m > 0: TKNN_E_ARG;
 *   2. not built, or a box tree: TKNN_E_STATE;
 *   3. a tree built with ids (tknnBuildIds with d_ids): TKNN_E_UNSUPPORTED;
 *   4. max_dist not > 0 or not finite; an unknown method, robust kind or flag; TKNN_ICP_POINT_TO_PLANE without d_target_normals;
 *      robust_scale not > 0 or not finite with Huber or Tukey; max_iterations < 0; rel_fitness or rel_rmse negative or not finite;
 *      init with an entry that is not finite; m < 0 or m >= 2^31 - 1: TKNN_E_ARG;
 *   5. m = 0 succeeds: transform = init, everything else zero.
 * A refused call writes nothing, info included. */
#define TKNN_ICP_POINT_TO_POINT 0
#define TKNN_ICP_POINT_TO_PLANE 1
#define TKNN_ICP_L2 0
#define TKNN_ICP_HUBER 1
#define TKNN_ICP_TUKEY 2
typedef struct {
  int64_t m;                      /* source points */
  const float *d_source;          /* m x 3 */
  const float *d_target_normals;  /* n x 3 by the caller's row; TKNN_ICP_POINT_TO_PLANE only */
  const double *init;             /* HOST: 16 doubles, row-major; NULL: the identity */
  float max_dist;                 /* > 0 and finite */
  float robust_scale;             /* > 0 and finite; read only with TKNN_ICP_HUBER / TKNN_ICP_TUKEY */
  int32_t method;                 /* TKNN_ICP_POINT_TO_POINT / TKNN_ICP_POINT_TO_PLANE */
  int32_t robust;                 /* TKNN_ICP_L2 / TKNN_ICP_HUBER / TKNN_ICP_TUKEY */
  int32_t max_iterations;         /* >= 0; 0: evaluate at init */
  uint32_t flags;                 /* no flag is defined: 0 */
  double rel_fitness, rel_rmse;   /* >= 0 and finite */
  int32_t *d_corr;                /* m, may be NULL */
  float *d_corr_dist;             /* m, may be NULL */
  float *d_aligned;               /* m x 3, may be NULL */
} tknnIcpOptions;
typedef struct {
  double transform[16];           /* row-major, source frame -> target frame */
  double fitness, inlier_rmse;
  int64_t correspondences;        /* N of the last search */
  int64_t skipped_pairs;          /* point-to-plane: partners of the last search whose normal is not finite */
  int64_t node_tests, point_tests, lane_rows; /* summed over the searches */
  int32_t iterations, searches, converged, degenerate;
  float solve_ms, search_ms, moment_ms;
  int32_t pad_;
} tknnIcpInfo;
TKNN_API int tknnIcp(tknnEngine e, const tknnIcpOptions *o, tknnIcpInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
