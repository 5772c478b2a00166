/*
 * owlknn_nms.h -- greedy suppression within a radius inside each cloud of a built point tree (tknnRadiusNms), an entry point of
 * libowl_mi355x.so on top of the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- suppression within a radius, per cloud ------------------------------------------------------------------------------------
 * tknnRadiusNms selects, in every cloud of the engine's tree, a subset K of its points so that no two selected points lie within
 * `radius` of each other and every other point has a stronger selected point within `radius`: non-maximum suppression of scored
 * points, a maximal Poisson-disk subset, radius thinning.  The tree is any built point tree: a plain one (tknnBuild, tknnBuildIds)
 * is ONE cloud, the sorted slots [0, n - nan), B = 1; a batched one (tknnBuildBatched, owlknn_batch.h) has B = num_batches clouds,
 * cloud b the sorted slots [starts[b], starts[b + 1]).  A point's NAME is its id on trees built with ids, its row in the caller's
 * buffer otherwise.
 *   eligible   a point without a NaN coordinate and, where d_scores is given, without a NaN score.  info->bad_scores counts the
 *              NaN entries of d_scores.
 *   within r   p is within r of q iff sqrt((dx*dx + dy*dy) + dz*dz) <= radius, every operation fp32 and uncontracted: the literal
 *              predicate of tknnRadiusQuery.  It is symmetric; coinciding duplicates are within r of each other.  One radius > 0
 *              per call.
 *   key        the pair (strength, name): the larger strength wins, among equal strengths the smaller name (compared as int32).
 *              The strength is a uint32:
 *                d_scores given (n floats, indexed by the row of the caller's buffer): the order-preserving image of the score's
 *                  bits u -- ~u if u & 0x80000000, u | 0x80000000 otherwise.  The image orders the bits, so -0 < +0 here, where
 *                  a float compare calls them equal;
 *                no scores: murmur3's fmix32 of the name's 32 bits (h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35;
 *                  h ^= h >> 16): a blue-noise subset that does not depend on the order of the input, and short chains;
 *                flags & TKNN_NMS_BY_NAME (not together with d_scores): every strength is equal, the smallest name wins -- what a
 *                  sequential loop over the caller's rows keeps.
 *              q DOMINATES p iff q's key beats p's.  Names are expected to be distinct; equal keys are decided by the sorted slot,
 *              so the call always ends, but which of several points with one id is kept is unspecified.
 *   K          the unique set with: an eligible p is in K iff no q in K of p's own cloud dominates p and is within r of p.
 *              (Well-defined by induction down the key order; it is what the sequential greedy loop over the keys keeps.)
 *   d_keep     n uint8, by the caller's row, required: 1 for the points of K, 0 otherwise.
 *   d_cover    n int32, by the caller's row, optional: the point's representative.  A kept point: its own name.  An eligible point
 *              that is not kept: the name of the kept point of its cloud within r with the smallest (distance bits, name) -- one
 *              exists.  A point that is not eligible: -1.
 *   d_counts   B int32, optional: the kept points of each cloud.
 * The host reads no array of the caller.  The tree, the state of tknnSolve and a halo tree are not modified.
 *
 * The work goes in rounds, each one launch: a point whose dominators within r are all decided is decided; the others wait for
 * the next round.  No kernel waits for another workgroup.  A round may see decisions of the same launch, which changes how many
 * rounds a call takes and never its result: info->rounds, point_tests and node_tests are NOT reproducible from call to call.
 * A point is decided at the latest in the round that is the length of the longest chain of dominators within r that ends in it
 * (scores that rise along a line of points: the line's length).  max_rounds > 0 ends the call after that many rounds with
 * TKNN_E_STATE and no output written; its info holds the rounds, the points left undecided, eligible, bad_scores, the counters
 * and the times so far (kept = 0, cover_ms = 0).  0: no limit.
 * info: kept = the sum of d_counts; eligible; bad_scores; rounds; undecided (above; otherwise 0); fallback_items = the points whose decision was made by the
 * one-item-per-lane kernel, which takes the walks whose stack ran out (TKNN_NMS_FORCE_FALLBACK=1 in the environment, read per call:
 * every walk, so fallback_items = eligible; the cover pass's are not counted); point_tests, node_tests (informational);
 * init_ms: keys and states; rounds_ms: the rounds; cover_ms: the cover pass and the outputs; solve_ms: all of it.
 * Errors, in this order: NULL engine / options / d_keep: TKNN_E_ARG; not built, or a box tree: TKNN_E_STATE; radius not > 0 or
 * not finite, d_scores together with TKNN_NMS_BY_NAME, an unknown flag, max_rounds < 0: TKNN_E_ARG.  A refused call writes
 * nothing, info included. */
#define TKNN_NMS_BY_NAME 1u
typedef struct {
  float radius;             /* > 0, finite */
  uint32_t flags;           /* TKNN_NMS_BY_NAME */
  int32_t max_rounds;       /* 0: no limit */
  int32_t pad_;
  const float *d_scores;    /* NULL, or n floats by the caller's row */
  uint8_t *d_keep;          /* n, required */
  int32_t *d_cover;         /* n, may be NULL */
  int32_t *d_counts;        /* B, may be NULL */
} tknnRadiusNmsOptions;
typedef struct {
  int64_t kept;             /* sum of d_counts */
  int64_t eligible;
  int64_t bad_scores;       /* NaN entries of d_scores */
  int64_t rounds;
  int64_t fallback_items;   /* points decided by the lane kernel */
  int64_t undecided;        /* 0; after a call that max_rounds ended: the points its last round left undecided */
  int64_t point_tests;      /* informational, not reproducible */
  int64_t node_tests;       /* informational, not reproducible */
  float solve_ms, init_ms, rounds_ms, cover_ms;
} tknnRadiusNmsInfo;
TKNN_API int tknnRadiusNms(tknnEngine e, const tknnRadiusNmsOptions *o, tknnRadiusNmsInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
