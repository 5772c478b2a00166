/*
 * owlknn_orient.h -- consistent orientation of the built set's normals without a viewpoint (tknnOrientNormals), an entry point of
 * libowl_mi355x.so on top of the C ABI of owlknn.h: Hoppe's propagation along the minimum spanning tree of a neighbour graph, what
 * orient_normals_consistent_tangent_plane(k) of the point-cloud libraries does.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one sign per normal, agreed along a spanning tree ------------------------------------------------------------------------
 * P is the built set (n points, any point tree); d_normals holds n x 3 fp32 by the caller's row, read as given, not normalised.
 *   eligible   a point is eligible if it has no NaN coordinate and its three normal components are finite.  A zero normal is
 *              eligible: it takes part and stays zero.  A point that is not eligible is in no edge; its output normal is the
 *              input bit for bit, its flip 0, its component -1.
 *   graph G    on the eligible points: {i, j} is an edge if j is in i's row of tknnKnn at k for the set's own points (the point
 *              itself is left out of its row, ids decide ties as there), or i in j's.  Both ends must be eligible: an edge to a
 *              point that is not is dropped and not replaced.  Unless TKNN_ORIENT_NO_EMST is set, the records of the plain
 *              Euclidean tknnEmst over P are edges as well, where both ends are eligible: G is then connected wherever the
 *              Euclidean forest is.  Batch labels and a halo tree are ignored, as in tknnEmst.
 *   weight     c = (nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j, every operation fp32 and uncontracted (bitwise symmetric);
 *              w = fmaxf(1.0f - fabsf(c), 0.0f) with fmaxf's rule for NaN (a NaN gives 0), -0 written as +0; the edge's sign bit
 *              is s = (c < 0), false for a NaN.
 *   order      the strict key (bits of w as uint32, min(name_i, name_j), max(name_i, name_j)); name is the id on trees built with
 *              tknnBuildIds, the row otherwise.  Duplicates of one edge are one edge.
 *   tree T     the minimum spanning forest of G under that key: unique.
 *   root       of a component C: with t(p) = (px*dx + py*dy) + pz*dz, fp32 and uncontracted, d = direction, a NaN t counting as
 *              -inf, the point of C with the largest t, among equals (as floats: -0 equals +0) the smallest row.  The root is flipped iff
 *              (nx*dx + ny*dy) + nz*dz < 0, computed the same way.  d = (0, 0, 1) is the rule of the point-cloud libraries; with
 *              d = 0 the root is the component's smallest row and is not flipped.
 *   flips      flip[v] = flip[root] XOR the parity of the number of tree edges with s = 1 on the path root .. v, s from the INPUT
 *              normals: the depth-first rule "flip the child iff its dot with the oriented parent is < 0" without an order of
 *              traversal (negation is exact: the dot with a flipped parent is -c, bit for bit).  Where c is +-0 or a NaN that rule
 *              has no sign to go on; s = 0 then says that the child takes its parent's flip.  Where no c along T and no root's
 *              dot with the direction is zero, the output does not depend on the signs the input normals came with.
 *   output     d_out_normals[v] = the input with the sign bit of all three components toggled iff flip[v]: negation is exact,
 *              every output bit is determined.  d_out_normals MAY equal d_normals (in place, the same bits).  d_flip: n uint8.
 *              d_component (by row): the smallest row of the point's component of G, -1 for a point that is not eligible.
 *              d_u, d_v (int32), d_w (fp32), n - 1 each: T's records, u < v by name, ascending by the key; the tail behind
 *              info->tree_edges is u = v = -1, w = +inf, as tknnEmst fills it.  Any output may be NULL; d_out_normals or d_flip is
 *              given.
 * The work: tknnKnn and tknnEmst through the engine, one candidate per kNN entry and per EMST record, one sort by the key -- an
 * edge's place in the sorted list is its rank, and every later comparison of two edges is one of two uint32 ranks --, Boruvka rounds
 * over the list with the sign parity carried through the merges, then the roots and the flips.  Under the strict key every
 * component that has an outgoing edge merges in a round: ceil(log2 n) + 1 rounds suffice, the default of max_rounds and its cap.
 * info: candidates, the edge slots emitted before the sort (n * k, and n - 1 more with the EMST's); tree_edges = |T|; components =
 * eligible points - tree_edges; excluded = n - eligible points; flipped, the rows with flip = 1; rounds, the rounds run; solve_ms
 * the whole call, knn_ms and emst_ms the two inner calls, sort_ms candidates, sort, duplicates and ranks, forest_ms the rounds,
 * apply_ms roots, flips and outputs.
 * The host reads no array of the caller.  The tree, the state of tknnSolve and a halo tree are not modified.
 * Errors, in this order: NULL engine / options, neither d_out_normals nor d_flip, NULL d_normals: TKNN_E_ARG; not built, or a box
 * tree: TKNN_E_STATE; k outside 1 .. TKNN_MAX_K_REGISTERS, an unknown flag, a direction that is not finite: TKNN_E_ARG;
 * n * (k + 1) >= 2^31: TKNN_E_UNSUPPORTED; max_rounds reached with components still merging: TKNN_E_ROUNDS.  A refused call
 * writes nothing, info included.  n = 1 gives no edges and one component, the point its own root. */
#define TKNN_ORIENT_NO_EMST 1u /* the kNN graph alone: G may fall into more components than the Euclidean forest has */
typedef struct {
  const float *d_normals; /* n x 3, required */
  int32_t k;              /* 1 .. TKNN_MAX_K_REGISTERS */
  uint32_t flags;         /* TKNN_ORIENT_NO_EMST */
  float direction[3];     /* finite */
  int32_t max_rounds;     /* <= 0: ceil(log2 n) + 1, which is also the most that is taken */
  float *d_out_normals;   /* n x 3, may be NULL, may equal d_normals */
  uint8_t *d_flip;        /* n, may be NULL */
  int32_t *d_component;   /* n, may be NULL */
  int32_t *d_u, *d_v;     /* n - 1 each, may be NULL */
  float *d_w;             /* n - 1, may be NULL */
} tknnOrientOptions;
typedef struct {
  int64_t candidates, tree_edges, components, excluded, flipped;
  int32_t rounds, reserved_;
  float solve_ms, knn_ms, emst_ms, sort_ms, forest_ms, apply_ms;
} tknnOrientInfo;
TKNN_API int tknnOrientNormals(tknnEngine e, const tknnOrientOptions *o, tknnOrientInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
