/*
 * owlknn_fpfh.h -- the 33-bin Fast Point Feature Histogram (Rusu, Blodow, Beetz 2009) of every point of the built set, without the
 * lists (tknnFpfh), an entry point of libowl_mi355x.so on top of the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- FPFH ----------------------------------------------------------------------------------------------------------------------------
 * tknnFpfh describes the surface around each of the built set's own n points by three histograms of 11 bins over the angles between
 * its normal and its neighbours' normals, and then blends each point's histograms with its neighbours': what compute_fpfh_feature
 * and FPFHEstimation of the point-cloud libraries give, the descriptor a global registration matches before tknnIcp refines it.  No
 * (point, neighbour) pair is written to memory.  The tree is any built point tree (tknnBuild, tknnBuildIds, tknnBuildBatched); on a
 * batched tree the labels are IGNORED, as tknnRadiusReduce ignores them.  Every array is addressed by the caller's row.
 *   d_normals  n x 3 fp32 by the caller's row, required; read as given and NOT normalised (TrueKNN.normals() gives unit normals).
 *   N_i        the row of tknnRadiusQuery at `radius` for point i -- sqrt((dx*dx + dy*dy) + dz*dz) <= radius, every operation fp32
 *              and uncontracted -- with the point itself left out BY SLOT, as TKNN_PCA_SKIP_SELF leaves it out: coinciding
 *              duplicates stay in.  d_counts[i] = |N_i|.  NaN points are nobody's neighbour and their own rows are all zero.
 *   pair       for source i and neighbour j in N_i, every operation fp32 and rounded on its own, a dot product is
 *              (x*x' + y*y') + z*z' (owlraytracing_amd/csrc/fpfh_pair.h is this text as code):
 *                1. dp = p_j - p_i per component; f4 = sqrt(d2), d2 = (dp_x*dp_x + dp_y*dp_y) + dp_z*dp_z;
 *                2. a1 = (n_i . dp) / f4, a2 = (n_j . dp) / f4;
 *                3. |a1| < |a2|: n1 = n_j, n2 = n_i, dp = -dp, f3 = -a2; otherwise n1 = n_i, n2 = n_j, f3 = a1;
 *                4. v = dp x n1, vn = sqrt(v . v), v = v / vn per component;
 *                5. w = n1 x v;
 *                6. f2 = v . n2;
 *                7. f1 = atan2f(w . n2, n1 . n2).
 *   bins       b1 = clamp(floor((11 * (f1 + pi)) / (2 pi)), 0, 10), pi and 2 pi rounded to fp32;
 *              b2 = clamp(floor((11 * (f2 + 1)) * 0.5), 0, 10); b3 = clamp(floor((11 * (f3 + 1)) * 0.5), 0, 10).
 *              The pair adds 1 to c_i[b1], c_i[11 + b2] and c_i[22 + b3]: d_spfh_counts, n x 33 int32.
 *   degenerate a pair with d2 == 0, with vn == 0, with a component of n_i or n_j that is not finite, or with a feature that is not
 *              finite adds nothing and counts into info.skipped_pairs.  (Open3D, for one, enters a pair with d2 == 0 or vn == 0 as
 *              three features of value 0 instead of leaving it out.)
 *              valid_i = the pairs that entered = c_i[0] + .. + c_i[10].
 *   SPFH       d_spfh, n x 33: SPFH_i[b] = c_i[b] * (100 / valid_i), 0 where valid_i == 0.
 *   FPFH       d_fpfh, n x 33: A_i[b] = the sum over j in N_i of SPFH_j[b] * (1 / d2_ij), a pair entering only where d2_ij > 0 and
 *              the weight is finite (the squared-distance weight both libraries use); the order of the additions is unspecified.
 *              S_i[f] = the sum of A_i over the 11 bins of feature f;
 *              FPFH_i[b] = (S_i[f] > 0 ? A_i[b] * (100 / S_i[f]) : 0) + SPFH_i[b].
 *              With TKNN_FPFH_NO_SELF_TERM the last term is dropped: PCL's form instead of Open3D's.
 *   outputs    d_fpfh, d_spfh, d_spfh_counts, d_counts: any may be NULL, at least one is given.  Without d_fpfh the second pass
 *              over the pairs does not run.
 * No parity with either library is claimed: this text and tests/fpfh_spec.py are the definition.  The host reads no array of the
 * caller.  The tree, the state of tknnSolve and a halo tree are not modified.
 *
 * info: total = the sum of d_counts; max_row = the largest; skipped_pairs = the degenerate pairs; fallback_items = the rows the
 * one-query-per-lane kernel made, of both passes together: it takes the walks whose stack ran out and trees too small for a box
 * pyramid (TKNN_FPFH_FORCE_FALLBACK=1 in the environment, read per call: every row of both passes); node_tests, point_tests
 * (informational, both passes); solve_ms: all of it; stage_ms: the normals into the tree's order; spfh_ms: the first pass and
 * the rows of d_spfh and d_spfh_counts; fpfh_ms: the second pass, 0 without d_fpfh; finish_ms: 0 in this version, the normalisation
 * per feature and the self term run at the end of each row of the second pass.
 * Errors, in this order:
 *   1. NULL engine / options; no output at all; d_normals NULL: TKNN_E_ARG;
 *   2. not built, or a box tree: TKNN_E_STATE;
 *   3. radius not > 0 or not finite; an unknown flag: TKNN_E_ARG;
 *   4. n = 0 succeeds with a zeroed info.
 * A refused call writes nothing, info included. */
#define TKNN_FPFH_NO_SELF_TERM 1u
#define TKNN_FPFH_BINS 33
typedef struct {
  float radius;             /* > 0 and finite */
  uint32_t flags;           /* TKNN_FPFH_NO_SELF_TERM */
  const float *d_normals;   /* n x 3, required */
  float *d_fpfh;            /* n x 33, may be NULL */
  float *d_spfh;            /* n x 33, may be NULL */
  int32_t *d_spfh_counts;   /* n x 33, may be NULL */
  int32_t *d_counts;        /* n, may be NULL */
} tknnFpfhOptions;
typedef struct {
  int64_t total;            /* sum of the counts */
  int64_t max_row;          /* largest count */
  int64_t skipped_pairs;    /* degenerate pairs */
  int64_t fallback_items;   /* rows made by the lane kernel, both passes */
  int64_t node_tests;       /* informational */
  int64_t point_tests;      /* informational */
  float solve_ms, stage_ms, spfh_ms, fpfh_ms, finish_ms;
  int32_t pad_;
} tknnFpfhInfo;
TKNN_API int tknnFpfh(tknnEngine e, const tknnFpfhOptions *o, tknnFpfhInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
