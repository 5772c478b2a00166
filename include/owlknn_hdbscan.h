/*
 * owlknn_hdbscan.h -- what follows the minimum spanning tree of owlknn_emst.h on the device: the single-linkage dendrogram of a
 * sorted forest (tknnLinkage), HDBSCAN's labels of such a forest (tknnHdbscanLabels) and the whole pipeline on the built set
 * (tknnHdbscan).  Entry points of libowl_mi355x.so on top of the C ABI of owlknn.h.  Plain C99; link and load as owlknn.h says.
 */
#pragma once
#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the single-linkage dendrogram of a sorted forest ------------------------------------------------------------------------
 * The input is what tknnEmst writes: `edges` records (d_u[i], d_v[i]) that form a forest over the vertices 0 .. n-1, ascending
 * by the strict key of owlknn_emst.h; record i has rank i, and the order of the records is all that is read (d_w is not).
 * The nodes of the dendrogram are the leaves 0 .. n-1 and the node n + i of record i: Kruskal's algorithm, taking the records in
 * order, joins two trees with record i and names the joined tree n + i.
 *   d_parent[x], x < n + edges: the node that absorbs x, -1 for a root (a vertex in no record is a root);
 *   d_left[i] < d_right[i]:     the two children of node n + i;
 *   d_size[i]:                  the leaves below node n + i.
 * For a spanning tree (left, right, w, size) is scipy's linkage matrix Z, row for row.  The output is fully determined.
 * The engine lends its workspace and its stream; no tree needs to be built, and one that is built is not touched.
 * The dendrogram is built in contraction rounds: every supervertex (a Kruskal cluster found so far) takes its smallest record,
 * the records so chosen form groups, and of every group the records below the smallest record that leaves the group are
 * absorbed as one chain of merges.  A handful of rounds does for every input tried (6 - 11 at 200 000 vertices); no bound is
 * proven, so after max_rounds rounds the records still alive are finished on the host by a sequential union-find over the
 * supervertices, with the same result (info.host_edges says how many there were).
 * Malformed input -- records that are no forest or not in [0, n) -- gives unspecified values, but the call ends and writes only
 * inside its buffers.
 * info: rounds the rounds run, absorbed the records they absorbed, host_edges those left to the host, roots the nodes without a
 * parent (n - edges), solve_ms the whole call.
 * Errors, in this order: NULL engine / options, NULL d_u / d_v with edges > 0, all four outputs NULL: TKNN_E_ARG;
 * n < 1, n >= 2^30, edges < 0, edges > n - 1: TKNN_E_ARG.  A refused call writes nothing. */
typedef struct {
  int64_t n, edges;
  const int32_t *d_u, *d_v; /* edges each */
  const float *d_w;         /* edges; not read by tknnLinkage (may be NULL there), the weights of tknnHdbscanLabels */
  int32_t *d_parent;        /* n + edges, may be NULL */
  int32_t *d_left, *d_right; /* edges each, may be NULL */
  int32_t *d_size;          /* edges, may be NULL */
  int32_t max_rounds;       /* <= 0: 64 */
  int32_t reserved_;
} tknnLinkageOptions;
typedef struct {
  int64_t absorbed, host_edges, roots;
  int32_t rounds, reserved_;
  float solve_ms, pad_;
} tknnLinkageInfo;
TKNN_API int tknnLinkage(tknnEngine e, const tknnLinkageOptions *o, tknnLinkageInfo *info, void *stream);

/* ---- HDBSCAN's labels of a sorted forest -------------------------------------------------------------------------------------
 * The forest is tknnLinkage's input with its weights d_w (>= 0, ascending with the records).  Every tree of the forest is
 * handled on its own; mcs is min_cluster_size.
 *   sizes      size(x) = the leaves below node x; big(x): size(x) >= mcs.  An internal node is a split iff both children are big.
 *   lambda     lambda(x) = 1 / (double) w(x), with w = 0 replaced by FLT_MIN (2^-126): finite, so no inf - inf arises (sklearn
 *              has an infinity here; the two differ on duplicate points only).
 *   clusters   a cluster head is a big root or a big child of a split; its cluster is the head and the chain below it that follows
 *              the only big child, down to a split or to a node without a big child.  birth(h) = lambda(parent(h)), 0 for a root.
 *   points     a point p leaves the cluster of a(p), its lowest big strict ancestor, at lambda_p = lambda(a(p)); a point without
 *              such an ancestor (a tree smaller than mcs) is noise.
 *   stability  of a cluster C, in fp64: the sum over the points that leave C of (lambda_p - birth(C)), plus, if a split s ends C,
 *              size(s) * (lambda(s) - birth(C)).  Every term is >= 0; the order of the additions is not fixed, so the relative
 *              error is at most n * 2^-53.
 *   selection  excess of mass, children before parents: S(C) = max(stability(C), S(c1) + S(c2)); C wins iff it has no children
 *              or stability(C) >= S(c1) + S(c2) (sklearn gives the tie to the children); a root cluster never wins
 *              (sklearn's allow_single_cluster = False).
 *   labels     a point's cluster is the highest winning ancestor-or-self of the cluster it left; none: -1.  Clusters are numbered
 *              by the ascending smallest vertex among their points, as tknnDbscan numbers by smallest core row.
 * d_lambda[p] = lambda_p, 0 for a point that is noise from the start.  d_stability[i] = the stability of the cluster whose head is
 * node n + i, 0 for a node that heads none.  The linkage arrays are tknnLinkage's.
 * The excess-of-mass pass reads one record per cluster (at most 2n / mcs) on the host; everything per point or per node runs on
 * the device.
 * info: clusters the labels given, noise the points labelled -1, condensed_clusters the cluster heads; rounds, absorbed and
 * host_edges tknnLinkage's; solve_ms the whole call, linkage_ms the dendrogram, condense_ms the points' ancestors, the clusters
 * of the nodes and the stabilities, select_ms the excess-of-mass pass with its copies, label_ms labels and numbering.
 * Errors, in this order: NULL engine / options / d_labels, NULL d_u / d_v / d_w with edges > 0: TKNN_E_ARG; n < 1, n >= 2^30,
 * edges < 0, edges > n - 1, min_cluster_size < 2: TKNN_E_ARG.  A refused call writes nothing. */
typedef struct {
  int64_t n, edges;
  const int32_t *d_u, *d_v;
  const float *d_w;
  int32_t min_cluster_size; /* >= 2 */
  int32_t max_rounds;       /* tknnLinkage's */
  int32_t *d_labels;        /* n, required */
  int32_t *d_parent, *d_left, *d_right, *d_size; /* as tknnLinkage's, each may be NULL */
  double *d_lambda;         /* n, may be NULL */
  double *d_stability;      /* edges, may be NULL */
} tknnHdbscanLabelsOptions;
typedef struct {
  int64_t clusters, noise, condensed_clusters;
  int64_t absorbed, host_edges;
  int32_t rounds, reserved_;
  float solve_ms, linkage_ms, condense_ms, select_ms, label_ms, pad_;
} tknnHdbscanLabelsInfo;
TKNN_API int tknnHdbscanLabels(tknnEngine e, const tknnHdbscanLabelsOptions *o, tknnHdbscanLabelsInfo *info, void *stream);

/* ---- HDBSCAN of the built set ------------------------------------------------------------------------------------------------
 * tknnKnn over the set's own points for the core distances, tknnEmst under them, tknnHdbscanLabels of its records: one call.
 *   core distance  the distance to the (min_samples - 1)-th nearest other point, the last column of tknnKnn(k = min_samples - 1):
 *                  sklearn's convention, where a point counts itself.  min_samples = 1: no core distances, the Euclidean tree.
 *   records        d_u, d_v, d_w are tknnEmst's, in its order and by name (the id on trees built with tknnBuildIds), the unused
 *                  tail filled as there; info.edges of them are records.
 *   rows           labels, lambdas and the leaves of the dendrogram are by row, also on trees built with ids: the call maps the
 *                  names of the records back to rows itself.
 * A point that is not eligible for tknnEmst (a NaN coordinate, a core distance that is not finite: fewer than min_samples - 1
 * other points in reach) is in no record: it gets label -1 and is counted in info.excluded.  The linkage arrays hold
 * n + info.edges, info.edges, ... entries; what lies behind them is not written.
 * A halo tree, if set, is ignored, and so are batch labels; the tree and the state of tknnSolve are not modified.  The host
 * never reads the points, the core distances or the records.
 * info: tknnHdbscanLabels' fields; edges and excluded tknnEmst's; knn_ms and emst_ms the two calls in front.
 * Errors, in this order: NULL engine / options / d_labels: TKNN_E_ARG; not built: TKNN_E_STATE; n >= 2^30,
 * min_cluster_size < 2, min_samples < 1: TKNN_E_ARG; min_samples - 1 > TKNN_MAX_K_REGISTERS: TKNN_E_UNSUPPORTED.
 * A refused call writes nothing. */
typedef struct {
  int32_t min_cluster_size; /* >= 2 */
  int32_t min_samples;      /* >= 1, min_samples - 1 <= TKNN_MAX_K_REGISTERS */
  int32_t max_rounds;       /* tknnLinkage's; tknnEmst runs with its default */
  int32_t reserved_;
  int32_t *d_labels;        /* n, required */
  float *d_core_dist;       /* n, may be NULL (not written with min_samples = 1) */
  int32_t *d_u, *d_v;       /* n - 1 each, may be NULL */
  float *d_w;               /* n - 1, may be NULL */
  int32_t *d_parent;        /* 2n - 1, may be NULL */
  int32_t *d_left, *d_right, *d_size; /* n - 1 each, may be NULL */
  double *d_lambda;         /* n, may be NULL */
  double *d_stability;      /* n - 1, may be NULL; 0 behind info.edges: no node there heads a cluster */
} tknnHdbscanOptions;
typedef struct {
  tknnHdbscanLabelsInfo labels; /* solve_ms in here: the whole call */
  int64_t edges, excluded;
  float knn_ms, emst_ms;
} tknnHdbscanInfo;
TKNN_API int tknnHdbscan(tknnEngine e, const tknnHdbscanOptions *o, tknnHdbscanInfo *info, void *stream);

#ifdef __cplusplus
}
#endif
