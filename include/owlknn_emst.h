/*
 * owlknn_emst.h -- the minimum spanning tree of the built point set under the Euclidean or the mutual-reachability distance
 * (tknnEmst), an entry point of libowl_mi355x.so on top of the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the minimum spanning forest of the set, for every eps at once --------------------------------------------------------
 * P is the built set (n points), E its eligible points: a point is eligible if it has no NaN coordinate and, when d_core_dist
 * is given, its core_dist[row] is finite and >= 0 (-0 counts as 0).
 *   weight  of {i, j}: d(i, j) = sqrt((dx*dx + dy*dy) + dz*dz), every operation fp32 and uncontracted -- the distance of
 *           every other call, bitwise symmetric; with core distances w = fmaxf(fmaxf(d, core[i]), core[j]), the
 *           mutual-reachability distance HDBSCAN builds on.  An edge whose distance is not finite is no edge: an
 *           overflowing distance is excluded, the rule tknnKnn has for neighbours (and so is inf - inf).
 *   order   edges are ordered by the strict key (bits of w as uint32, min(name_i, name_j), max(name_i, name_j)); name is the
 *           id on trees built with tknnBuildIds, the row otherwise: ties are decided by index as everywhere in this library.
 *   result  with a strict order the minimum spanning forest of E is unique, and the call returns exactly it:
 *           edges = |E| - components records (u, v, w), u < v (names), ascending by the key, in d_u[0 .. edges), d_v, d_w;
 *           the unused tail up to n - 1 is u = v = -1, w = +inf.  The output is fully determined, bit for bit.
 *           d_component (by row): the smallest row of the point's component, -1 for a point that is not eligible.
 * Cutting the Euclidean tree at eps gives single linkage (DBSCAN with min_pts = 1); the tree under core distances taken from
 * tknnKnn is the input of HDBSCAN's linkage step.
 * A halo tree, if set, is ignored, and so are batch labels; the tree and the state of tknnSolve are not modified; n = 1 gives
 * 0 edges and 1 component.  The host never reads the points or the core distances.
 * The work is done in Boruvka rounds: in each, every point finds its nearest point in another component, every component
 * takes the smallest of those edges, and the components so joined become one.  Under the strict key every component that has
 * an outgoing edge merges with another in each round, so ceil(log2 n) + 1 rounds suffice: the default of max_rounds and its
 * cap.
 * info: edges, components and excluded (n - |E|) as above; node_tests / point_tests the walks' over all rounds, as the other
 * calls count them; skipped_subtrees the subtrees stepped over because they lay wholly inside the walking point's own
 * component; rounds the rounds run; solve_ms the whole call, walk_ms the nearest-foreign-point walks, merge_ms the uniform
 * marks, component minima, unions and relabelling, sort_ms the ordering of the records and the components' rows.
 * Errors, in this order: NULL engine / options, NULL d_u / d_v with n > 1: TKNN_E_ARG; not built: TKNN_E_STATE;
 * n >= 2^31 - 1: TKNN_E_ARG; max_rounds reached with components still merging: TKNN_E_ROUNDS (a guard: it cannot happen
 * with max_rounds <= 0; no output is written then, info holds the work done so far).  A refused call writes nothing. */
typedef struct {
  const float *d_core_dist;  /* NULL: plain Euclidean. else n floats by row */
  int32_t *d_u, *d_v;        /* n-1 each, required (n = 1: may be NULL) */
  float *d_w;                /* n-1, may be NULL */
  int32_t *d_component;      /* n, may be NULL */
  int32_t max_rounds;        /* <= 0: ceil(log2 n) + 1, which is also the most that is taken */
  int32_t reserved_;
} tknnEmstOptions;
typedef struct {
  int64_t edges, components, excluded;
  int64_t node_tests, point_tests, skipped_subtrees;
  int32_t rounds, reserved_;
  float solve_ms, walk_ms, merge_ms, sort_ms;
} tknnEmstInfo;
TKNN_API int tknnEmst(tknnEngine e, const tknnEmstOptions *o, tknnEmstInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
