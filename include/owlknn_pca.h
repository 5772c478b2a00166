/*
 * owlknn_pca.h -- the covariance of each query's neighbourhood, its eigenvalues, its normal and its surface variation, without the
 * lists (tknnLocalPca), an entry point of libowl_mi355x.so on top of the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h
 * says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- local principal components ------------------------------------------------------------------------------------------------------
 * tknnLocalPca fits a plane to the neighbourhood N_j of every query q_j among the points of the built set P: the number of
 * neighbours, their centroid, their population covariance, its eigenvalues and eigenvectors, the normal and the surface variation
 * lambda0 / (lambda0 + lambda1 + lambda2) -- what estimate_normals of the point-cloud libraries gives.  No (query, neighbour)
 * pair is written to memory.  The tree is any built point tree (tknnBuild, tknnBuildIds, tknnBuildBatched).
 *   queries    d_queries: m packed fp32 triples, addressed by the caller's j.  d_queries == NULL: the set's own n points are the
 *              queries; then m must equal n and the results are addressed by the caller's row.
 *   N_j        a set of points of P, defined by the calls that exist; at least one of radius and k is given (0: not given):
 *                radius only   the row of tknnRadiusQuery at that radius: sqrt((dx*dx + dy*dy) + dz*dz) <= radius, every
 *                              operation fp32 and uncontracted.  With the set's own points the point itself is in, unless
 *                              flags & TKNN_PCA_SKIP_SELF; coinciding duplicates always stay.
 *                k, external   the entries of tknnKnn's row at k; with a radius as well those with distance <= radius
 *                              (tknnRadiusKnn's row).
 *                k, own        the point itself plus the own-points tknnKnn row at k - 1, clipped by radius if one is given: the
 *                              k nearest including itself (k >= 2).  With TKNN_PCA_SKIP_SELF: the own-points row at k, the
 *                              point itself out.
 *              A query with a NaN coordinate has an empty neighbourhood; NaN points of P are nobody's neighbour.  On a batched
 *              tree the labels are IGNORED, as tknnRadiusReduce ignores them.  Ids only decide ties, as they do in tknnKnn.
 *   moments    fp32, the order of the additions unspecified.  With len = |N_j| and d = p - q_j per component in fp32:
 *              S1 = sum of d, S2 = sum of d d^T (six sums); mean = S1 / len; centroid = q_j + mean;
 *              cov_ab = S2_ab / len - mean_a * mean_b, the population covariance.  A term enters a sum only for a point that
 *              passed the predicate.  (The offsets are bounded by the neighbourhood's radius: nothing of the size |p|^2 is
 *              ever subtracted.)
 *   eigen      from the fp32 covariance: eigenvalues ascending and NOT clamped (a last-bit negative lambda0 is allowed),
 *              eigenvectors of unit length.  The normal is the eigenvector of lambda0; its sign:
 *                without TKNN_PCA_ORIENT  flipped so that its component of largest magnitude (the first among equals) is
 *                                         positive;
 *                with TKNN_PCA_ORIENT     v = viewpoint - q_j per component in fp32, s = (n_x v_x + n_y v_y) + n_z v_z,
 *                                         uncontracted; flipped iff s < 0.
 *              Row 0 of d_eigenvectors is the normal as written; the signs of rows 1 and 2 are unspecified.
 *              curvature = max(lambda0, 0) / ((lambda0 + lambda1) + lambda2), 0 where that sum is not > 0.
 *   degenerate rows with len < min_points (0: 3): the count is written, centroid and covariance by the formulas above (all zeros
 *              with len = 0), eigenvalues, eigenvectors, normal and curvature are all 0.  Rows with len >= min_points whose
 *              points are collinear or coincide are solved as they are: the normal is some unit vector of the null space.
 *   outputs    all addressed by j (own points: by the caller's row), any may be NULL, at least one is given:
 *                d_counts m int32; d_centroid m x 3; d_cov m x 6 (xx, xy, xz, yy, yz, zz); d_eigenvalues m x 3 ascending;
 *                d_eigenvectors m x 9 (row i of the 3 x 3 belongs to lambda_i); d_normals m x 3; d_curvature m.
 * The host reads no array of the caller.  The tree, the state of tknnSolve and a halo tree are not modified.
 *
 * info: total = the sum of the counts; max_row = the largest; degenerate_rows = the rows with len < min_points;
 * fallback_items = the rows summed by the one-query-per-lane kernel, which takes the walks whose stack ran out and trees too small
 * for a box pyramid (TKNN_PCA_FORCE_FALLBACK=1 in the environment, read per call: every query, so fallback_items = m);
 * node_tests, point_tests (informational: the moment walk's); solve_ms: all of it; bound_ms: the tknnKnn call and the bounds made
 * of its rows (0 with radius only); order_ms: ordering the queries along the tree's curve (0 for the own points); walk_ms: the
 * walks; finish_ms: centroid, covariance and the eigen-solver.
 * Errors, in this order:
 *   1. NULL engine / options; no output at all; d_queries NULL with m != n: TKNN_E_ARG;
 *   2. not built, or a box tree: TKNN_E_STATE;
 *   3. neither radius nor k; radius negative or not finite; k < 0; own points without TKNN_PCA_SKIP_SELF and k == 1; an unknown
 *      flag; TKNN_PCA_SKIP_SELF with d_queries; TKNN_PCA_ORIENT with a viewpoint that is not finite; min_points < 0; m < 0 or
 *      m >= 2^31 - 1: TKNN_E_ARG;
 *   4. k > TKNN_MAX_K_REGISTERS: TKNN_E_UNSUPPORTED;
 *   5. m = 0 succeeds with a zeroed info.
 * A refused call writes nothing, info included. */
#define TKNN_PCA_SKIP_SELF 1u
#define TKNN_PCA_ORIENT 2u
typedef struct {
  int64_t m;                /* queries; with d_queries NULL: n */
  float radius;             /* > 0 and finite, or 0: none */
  int32_t k;                /* 1 .. TKNN_MAX_K_REGISTERS, or 0: none */
  int32_t min_points;       /* rows with fewer neighbours are degenerate; 0: 3 */
  uint32_t flags;           /* TKNN_PCA_SKIP_SELF | TKNN_PCA_ORIENT */
  float viewpoint[3];       /* read only with TKNN_PCA_ORIENT */
  int32_t pad_;
  const float *d_queries;   /* m x 3, or NULL: the set's own points */
  int32_t *d_counts;        /* m, may be NULL */
  float *d_centroid;        /* m x 3, may be NULL */
  float *d_cov;             /* m x 6: xx, xy, xz, yy, yz, zz; may be NULL */
  float *d_eigenvalues;     /* m x 3, ascending; may be NULL */
  float *d_eigenvectors;    /* m x 9, row i of the 3 x 3 belongs to lambda_i; may be NULL */
  float *d_normals;         /* m x 3, may be NULL */
  float *d_curvature;       /* m, may be NULL */
} tknnLocalPcaOptions;
typedef struct {
  int64_t total;            /* sum of the counts */
  int64_t max_row;          /* largest count */
  int64_t degenerate_rows;  /* rows with len < min_points */
  int64_t fallback_items;   /* rows summed by the lane kernel */
  int64_t node_tests;       /* informational */
  int64_t point_tests;      /* informational */
  float solve_ms, order_ms, bound_ms, walk_ms, finish_ms;
  int32_t pad_;
} tknnLocalPcaInfo;
TKNN_API int tknnLocalPca(tknnEngine e, const tknnLocalPcaOptions *o, tknnLocalPcaInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
