/*
 * owlknn_fps.h -- farthest point sampling inside each cloud of a built point tree (tknnFps), an entry point of libowl_mi355x.so on
 * top of the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- farthest point sampling, per cloud ---------------------------------------------------------------------------------------
 * tknnFps picks, in every cloud of the engine's tree, up to num_samples points so that each one is the point farthest from those
 * picked before it (torch-cluster's fps).  The tree is any built point tree: a plain one (tknnBuild, tknnBuildIds) is ONE cloud,
 * the sorted slots [0, n - nan), B = 1; a batched one (tknnBuildBatched, owlknn_batch.h) has B = num_batches clouds, cloud b the
 * sorted slots [starts[b], starts[b + 1]).
 *   eligible   the points of cloud b without a NaN coordinate, n_b of them.  A point's NAME is its id on trees built with ids, its
 *              row in the caller's buffer otherwise.
 *   d2(p, s)   (dx*dx + dy*dy) + dz*dz, every operation fp32 and uncontracted: the arithmetic under tknnKnn's square root.
 *   w_b        the samples wanted of cloud b: min(S, n_b), with d_num min(max(d_num[b], 0), S, n_b).  S = num_samples >= 1 is
 *              also the row stride of the outputs.
 *   sample 0   the eligible point of the cloud with the smallest name; if d_start_rows[b] is a row of the caller's buffer that
 *              is an eligible point of cloud b, that point instead.  A negative value means "the default"; a row of another cloud,
 *              of a NaN point or out of range also gives the default and is counted in info->bad_starts.
 *   later      D[p] = the minimum of d2(p, s) over the samples s chosen so far (a minimum of fp32 values: exact, order-free).
 *              Chosen points are out of the running.  The next sample is the unchosen eligible point with the largest D; among
 *              equal D, compared as fp32 bits, the smallest name wins.  A cloud so yields exactly w_b distinct points; coinciding
 *              duplicates of a sample are chosen last, at D = 0, in name order.
 *   row b      d_idx[b * S ..]: the names in the order chosen, the tail -1.  d_dist[b * S ..] (optional): sqrtf(D) at the moment of
 *              choice -- the covering radius so far --, +inf for sample 0 and in the tail.  d_counts[b] = w_b (optional).  An
 *              empty cloud has an empty row.
 * The host reads none of d_num, d_start_rows or any device result before or during the work.  The tree, the state of tknnSolve
 * and a halo tree are not modified.
 *
 * The pruning rule (info->point_tests is exactly what it says).  The tree's 64-ary pyramid of boxes over blocks of 16 sorted slots
 * is the walk's: child c of level l covers the slots [c << sh, (c + 1) << sh), sh = 4 + 6 l, and touches the cloud [s, e) iff
 * (s >> sh) <= c <= ((e - 1) >> sh) (boxes and blocks may straddle a cloud boundary).  Per box and cloud the call keeps M, the
 * largest key (D bits, smallest name) over the box's unchosen eligible slots OF THE CLOUD (D = 0 where there is none).  For a new
 * sample s the boxes are walked top-down from the lowest level at which the cloud touches at most 64 boxes: child c is entered
 * iff it touches the cloud and box_min_dist2(box, s) < M_D[c] -- M as it was before this sample's updates --, or c holds s's own
 * slot (s must leave the running, even when only duplicates at D = 0 remain around it).  At an entered block of level 0
 * D = min(D, d2) for the 16 slots, the block's M is recomputed, then its ancestors', bottom-up; the cloud's next sample is the
 * maximum over its top boxes.  box_min_dist2 is the squared distance of s to the box, gaps clamped at 0, in d2's association:
 * fp32 subtraction, multiplication and addition round monotonically, so it is <= d2(p, s) for every point under the box without
 * any margin, a box that is not entered holds no point whose D the sample lowers, and, a child's box lying inside its parent's
 * and a child's M not above it, a block is visited exactly when ITS OWN box passes the test (or it is s's block): the visits do
 * not depend on the levels above.  Every sample, the last one included, is walked.
 *   flags & TKNN_FPS_NO_PRUNE: every block that touches the cloud is visited for every sample; the outputs are identical (the A/B
 *   switch, and a test handle).
 * info: samples = the sum of w_b; point_tests = 16 per visited block; node_tests = pyramid boxes tested (informational);
 * bad_starts; lds_clouds = the clouds worked on from a copy in LDS (0: this library has no such path); init_ms: D, the boxes' keys
 * and the starts; walk_ms: the sampling; solve_ms: both.
 * Errors, in this order: NULL engine / options / d_idx: TKNN_E_ARG; not built, or a box tree: TKNN_E_STATE; num_samples < 1 or
 * B * num_samples >= 2^31: TKNN_E_ARG.  A refused call writes nothing. */
#define TKNN_FPS_NO_PRUNE 1u
typedef struct {
  int32_t num_samples;          /* S >= 1: at most that many samples per cloud, and the row stride of the outputs */
  uint32_t flags;               /* TKNN_FPS_NO_PRUNE */
  const int32_t *d_num;         /* NULL, or B int32: the samples wanted of each cloud (clipped to 0 .. min(S, n_b)) */
  const int32_t *d_start_rows;  /* NULL, or B int32: the row of the caller's buffer to start cloud b with; negative: the default */
  int32_t *d_idx;               /* B*S, required */
  float *d_dist;                /* B*S, may be NULL */
  int32_t *d_counts;            /* B, may be NULL */
} tknnFpsOptions;
typedef struct {
  int64_t samples;              /* sum of d_counts */
  int64_t point_tests;          /* 16 per visited block */
  int64_t node_tests;           /* pyramid boxes tested */
  int64_t bad_starts;           /* entries of d_start_rows >= 0 that did not name an eligible point of their cloud */
  int64_t lds_clouds;           /* clouds worked on from LDS (always 0 here) */
  float solve_ms, init_ms, walk_ms;
} tknnFpsInfo;
TKNN_API int tknnFps(tknnEngine e, const tknnFpsOptions *o, tknnFpsInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
