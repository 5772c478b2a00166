/*
 * owlknn.h -- C-ABI of the MI355X-native TrueKNN engine (libowl_mi355x.so).
 *
 * This is the hot path of vani-nag/OWLRayTracing's samples/s01-trueknn, taken as ONE unit:
 *
 *   reference                                               here
 *   ------------------------------------------------------  --------------------------------
 *   owlDeviceBufferCreate(Sphere[n])  hostCode.cpp:165-166   tknnBuild: points already in HBM
 *   owlUserGeomGroupCreate + owlGroupBuildAccel (+ instance  tknnBuild: HIP LBVH (curve-key sort +
 *     group)  hostCode.cpp:201-206 -> bounds program           radix tree) over the centres; the
 *     deviceCode.cu:38-56 + optixAccelBuild                    radius is applied at test time
 *     (owl/UserGeomGroup.cpp:161-217)
 *   while(!foundKNN){ owlLaunch2D; scan fb; radius*=2;       tknnSolve: the whole radius-doubling
 *     owlGeomSet1f; owlGroupRefitAccel x2 }                    solve, rounds resolved on the device
 *     hostCode.cpp:285-340 around __raygen__rayGen /
 *     __intersection__Spheres  deviceCode.cu:62-153
 *   frameBuffer of Neigh[n*k]  GeomTypes.h:22-28             d_fb (same 24-byte records) and/or
 *                                                            compact idx/dist/intersections
 *
 * The same library also exports the reference's own owl* entry points (include/owl/owl_host.h),
 * which run user raygen / intersect / bounds programs over the same LBVH; the tknn* calls are the
 * fused form of the loop above and give bit-identical rows (modulo the order of exact ties inside
 * one round, which the reference leaves to traversal order; tknn* orders ties by the round in which a
 * candidate was first seen -- the reference's lists persist over rounds -- and then by index).
 *
 * Conventions: plain C, pointers and sizes only.  `d_` pointers are device (HBM) addresses valid
 * on the engine's device.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Every call returns 0 on success or a negative TKNN_E_* code; tknnLastError() gives the text.
 * Nothing here falls back to the CPU.
 */
#ifndef OWLKNN_H
#define OWLKNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TKNN_API __attribute__((visibility("default")))

typedef struct tknnEngine_t *tknnEngine;

/* GeomTypes.h:22-28: 24-byte result record; only slot [q*k+0] carries numNeighbors/intersections */
typedef struct {
  int32_t ind;
  float dist;
  int32_t numNeighbors;
  int32_t pad_;
  int64_t intersections;
} tknnNeigh;

enum {
  TKNN_OK = 0,
  TKNN_E_ARG = -1,      /* bad argument (null pointer, n <= k, radius not finite-positive, ...)  */
  TKNN_E_HIP = -2,      /* a HIP call failed; no device, out of memory, launch failure           */
  TKNN_E_STATE = -3,    /* call order: solve before build, ...                                   */
  TKNN_E_ROUNDS = -4,   /* max_rounds reached with unfinished queries (reference: endless loop)  */
  TKNN_E_UNSUPPORTED = -5 /* k above TKNN_MAX_K; a kernel asked for by name that does not serve this k  */
};

/* The reference takes any k from its command line (samples/s01-trueknn/hostCode.cpp:111) and keeps the lists in global
 * memory (deviceCode.cu:77-134).  Here k <= 64 is served from registers (TKNN_KERNEL_LANE / _WAVE / _TEAM); 64 < k <=
 * TKNN_MAX_K by the team walk with the lists in memory (TKNN_KERNEL_AUTO or _TEAM). */
#define TKNN_MAX_K 1024
#define TKNN_MAX_K_REGISTERS 64

/* which traversal kernel tknnSolve uses */
enum {
  TKNN_KERNEL_AUTO = 0,
  TKNN_KERNEL_LANE = 1,  /* one query per lane, stackless rope traversal, one launch per round    */
  TKNN_KERNEL_WAVE = 2,  /* one 64-query packet per wave, persistent, all rounds in one launch    */
  TKNN_KERNEL_TEAM = 3,  /* 16-lane teams, lanes = candidates of one query's leaf blocks           */
  TKNN_KERNEL_QUERY = 4  /* reported by tknnQuery in info->kernel_used; not a selector tknnSolve takes */
};

typedef struct {
  int32_t rounds;              /* radius levels needed = rounds of the reference loop             */
  float final_radius;          /* radius of the last round                                        */
  int64_t total_intersections; /* sum of Neigh.intersections = intersection-program calls         */
  int64_t node_tests;          /* box tests against BVH nodes (wave kernel: per packet)           */
  int64_t point_tests;         /* exact point-in-box tests executed (>= total_intersections)      */
  int64_t total_active_rounds; /* sum over queries of the rounds in which the query traced a ray  */
  float solve_ms;              /* device time of the traversal launches, HIP events on `stream`   */
  float dominant_kernel_ms;    /* average duration of one launch of the dominant kernel           */
  int32_t dominant_kernel_launches;
  int32_t kernel_used;         /* TKNN_KERNEL_*                                                   */
  int32_t list_capacity;       /* register k-list size the kernel was instantiated with           */
  int64_t unfinished;          /* queries left without k neighbours (only with allow_unfinished)  */
  int64_t tie_rows;            /* rows with bit-identical fp32 distances among their k + 1 best,   */
                               /* redone in the reference's tie order (first round, then index;    */
                               /* deviceCode.cu:77-85: lists persist over rounds)                  */
  int64_t tie_rows_left;       /* ... of which kept (dist, index) order: walk stack exhausted     */
  float tie_ms;                /* device time of that pass (included in solve_ms)                 */
  int32_t reserved_;
} tknnSolveInfo;

typedef struct {
  float build_ms;        /* device time of the LBVH build                                         */
  int64_t device_bytes;  /* HBM held by the tree                                                  */
  int32_t n;
} tknnBuildInfo;

TKNN_API const char *tknnLastError(void);
TKNN_API int tknnDeviceCount(void);

/* engine on the current HIP device (hipSetDevice before the call picks it) */
TKNN_API int tknnCreate(tknnEngine *out);
TKNN_API void tknnDestroy(tknnEngine e);

/* Build the LBVH over n points.  d_xyz: n packed fp32 triples (the Sphere buffer, 12 B each; 2-D
 * data carries z = 0 as in hostCode.cpp:115-118).  The engine keeps its own curve-ordered copy;
 * d_xyz may be freed afterwards. */
TKNN_API int tknnBuild(tknnEngine e, const float *d_xyz, int64_t n, tknnBuildInfo *info, void *stream);

/* Solve TrueKNN for every point (queries = points, deviceCode.cu:140-153).
 *   k, start_radius   as argv[5], argv[4] of the sample; n > k and 0 < start_radius < inf required
 *   max_rounds        give up (TKNN_E_ROUNDS) after this many radius levels; <= 0 means 64, more than 127 means 127
 *   d_idx, d_dist     n*k each, row q = neighbours of point q (caller's index), ascending
 *                     (dist, index); either may be NULL
 *   d_intersections   n, Neigh.intersections of slot 0 of each row; may be NULL
 *   d_fb              n*k tknnNeigh records in the state the reference's frameBuffer has after its
 *                     last round; may be NULL
 */
TKNN_API int tknnSolve(tknnEngine e, int k, float start_radius, int kernel, int max_rounds,
                       int32_t *d_idx, float *d_dist, int64_t *d_intersections, tknnNeigh *d_fb,
                       tknnSolveInfo *info, void *stream);

/* ---- sharded use: one engine per GPU owns a tile of a larger point set ----
 * tknnBuildIds: like tknnBuild, but point i is reported as d_ids[i] (a global index) in neighbour
 *   lists and excluded as "self" by that id; rows are still addressed by the local position i.  Ids are distinct
 *   and non-negative (any int32 from 0 up); exact-distance ties order by id as they do by index without ids.
 * tknnSetHalo: a second, read-only point set (border points received from neighbouring tiles, with
 *   their global ids) that every query also searches; m = 0 removes it.
 * tknnSolveEx: tknnSolve with options: d_levels (n, may be NULL) receives the 0-based radius level at
 *   which each query finished, or -1; with allow_unfinished != 0 reaching max_rounds is not an
 *   error: unfinished queries keep level -1, their rows are not written and info->unfinished counts
 *   them (the caller widens the halo and solves again).
 * tknnHaloSelect: the send side of the exchange.  d_boxes: nboxes x {lo xyz, hi xyz} fp32 closed
 *   boxes (the peers' tile cells widened by the halo radius, rounded outward by the caller);
 *   d_box_peer: the peer (0 <= peer < npeers <= 64) each box belongs to -- the caller's responsibility: the
 *   entries live on the device and are not checked, the kernels shift a 64-bit mask by them, and an entry
 *   outside that range gives unspecified counts and rows.  Count pass (d_rows NULL):
 *   d_counts[npeers] = my points inside at least one box of each peer.  Write pass: d_rows receives
 *   16-byte rows {x, y, z, id bits}, peer p's rows contiguous from row d_offsets[p] (the caller's
 *   exclusive scan of the counts); the order inside a segment is unspecified. */
typedef struct {
  int32_t k;
  float start_radius;
  int32_t kernel;
  int32_t max_rounds;
  int32_t allow_unfinished;
  int32_t phase; /* 0: every query.  1: only the queries NO point of another tile can reach within the radius the last
                    tknnHaloSelect count pass was given boxes for ("interior"), searched in the own tree alone -- the call may
                    run on its own stream and host thread while the halo is exchanged and tknnSetHalo builds its tree.
                    2: the other ("boundary") queries, own + halo tree; rows and levels of a phase-1 call are kept.
                    3: only the queries an earlier call with allow_unfinished left without a row (d_levels[row] == -1; d_levels
                    required), from level 0 over own + halo tree; rows and levels of the others are kept -- the sharded
                    driver's straggler rounds: the halo has been widened by the shell the next radius level needs.
                    Team kernels only (TKNN_KERNEL_AUTO / _TEAM; any k up to TKNN_MAX_K). */
  int32_t *d_idx;
  float *d_dist;
  int64_t *d_intersections;
  tknnNeigh *d_fb;
  int32_t *d_levels;
  const float *d_start_radii; /* NULL, or n floats: row q starts with d_start_radii[q] instead of start_radius and doubles from
                                 there -- a per-query radius schedule (opt-in: the reference has ONE
                                 radius, samples/s01-trueknn/hostCode.cpp:185,325).  Row q is what the reference's loop gives
                                 for q when started at that radius; every value must be finite and > 0.  Team kernels only
                                 (any k up to TKNN_MAX_K), no halo tree.  info->final_radius then refers to start_radius. */
} tknnSolveOptions;
TKNN_API int tknnBuildIds(tknnEngine e, const float *d_xyz, const int32_t *d_ids, int64_t n,
                          tknnBuildInfo *info, void *stream);
TKNN_API int tknnSetHalo(tknnEngine e, const float *d_xyz, const int32_t *d_ids, int64_t m, void *stream);
TKNN_API int tknnSolveEx(tknnEngine e, const tknnSolveOptions *options, tknnSolveInfo *info, void *stream);
TKNN_API int tknnHaloSelect(tknnEngine e, const float *d_boxes, const int32_t *d_box_peer, int32_t nboxes,
                            int32_t npeers, int64_t *d_counts, const int64_t *d_offsets, float *d_rows,
                            void *stream);

/* The same in ONE pass, for a caller that knows how many rows each peer's segment may hold (both ends of a pair agree on the
 * size of their message from the pair's last exchange): rows are written at d_offsets[peer] .. + d_caps[peer], rows that do not fit
 * are dropped (which ones is unspecified), d_counts[peer] receives the exact number of rows selected (> d_caps[peer]: the caller
 * must fall back to tknnHaloSelect for that peer).  The rows of a segment past min(d_counts[peer], d_caps[peer]) are left
 * untouched, as is everything outside the segments.  No count pass, no host round trip before the rows exist.  Marks the boundary queries like the
 * count pass of tknnHaloSelect. */
TKNN_API int tknnHaloSelectFixed(tknnEngine e, const float *d_boxes, const int32_t *d_box_peer, int32_t nboxes, int32_t npeers,
                                 const int64_t *d_caps, const int64_t *d_offsets, float *d_rows, int64_t *d_counts, void *stream);

/* ---- exact kNN on request ---------------------------------------------------
 * tknnSolve reproduces the reference, whose rows are box-candidate kNN, not exact kNN: a query
 * that finished with box half-width r_q never saw points outside that box, although its k-th
 * distance d_k may exceed r_q (15-20 % of rows on uniform data); and candidates at bit-identical
 * distances keep the reference's order (first round seen, then index), which at the k-th place can
 * keep another point than (dist, index) order does, whatever d_k and r_q are.
 * tknnRepairExact walks every row with d_levels[row] >= 0 once more, over the box of half-width
 * d_k * 1.000001 + 2^-74, and rewrites it with the true k nearest neighbours of the engine's points
 * (own and halo) in (dist, index) order -- index = id on trees built with ids; distances are the
 * solve's fp32 formula.  That holds where squared offsets are subnormal or flush to zero as well
 * (coordinates closer than about 1e-19): the 2^-74 covers their rounding.  Rows with level -1 and
 * rows whose d_k is not finite (squared distances that overflow fp32) are left as they are.  The walk
 * does not depend on r_q: start_radius is only checked (finite, > 0), and rows of a solve with
 * per-query start radii are served the same way.  *repaired (may be NULL) receives the number of rows
 * whose contents changed.
 * Opt-in post-processing: it is never applied by tknnSolve, so parity with the reference is
 * unaffected.  Inputs: the rows and d_levels of a tknnSolveEx call (k <= 64); intersections and
 * frameBuffer images are not touched. */
TKNN_API int tknnRepairExact(tknnEngine e, int k, float start_radius, const int32_t *d_levels,
                             int32_t *d_idx, float *d_dist, int64_t *repaired, void *stream);

/* ---- queries that are not in the set ------------------------------------------------------------------
 * tknnSolve answers for the points of the built set P.  tknnQuery answers for m arbitrary points Q (any fp32
 * triples, any order, inside the bounds of P or not) against the tree of P, built once.
 * Row j is the row the reference's loop gives to q_j in the set P + {q_j}, q_j being the query there: at level L
 * the radius is start_radius doubled L times in fp32; the candidates are the points p of P with
 * fl(p - r) <= q_j <= fl(p + r) on every axis; the query finishes at the first level with at least k candidates;
 * its row is the k best candidates of that level in the order (fp32 distance, level at which the candidate was
 * first a candidate, index) -- index = id on trees built with ids.  There is no self to skip: a point of P that
 * coincides with q_j is an ordinary neighbour at distance 0, so n >= k is enough.
 *   d_levels[j]        that level (0-based), -1 if unfinished
 *   d_intersections[j] candidates summed over the levels the query traced (the reference's counter for q_j in
 *                      P + {q_j} also counts the query's own box once per level: that is left out)
 *   exact != 0         every finished row is rewritten with the true k nearest points of P in (dist, index)
 *                      order, as tknnRepairExact does for the points of the set (levels and intersections stay)
 * Rows are addressed by the caller's index j whatever order the engine works in; d_queries is not referred to
 * after the call returns; the tree and the state of tknnSolve are not modified.  info is filled as for a solve
 * (kernel_used = TKNN_KERNEL_QUERY; dominant_kernel_ms = the traversal of the ordered queries, solve_ms - that
 * - tie_ms = ordering them (plus the exact pass); tie_rows = rows redone for the order of bit-identical distances).
 * Errors, in this order: NULL engine / options / d_queries with m > 0: TKNN_E_ARG; not built: TKNN_E_STATE;
 * k < 1, k > n, radius not finite-positive, m < 0, allow_unfinished without d_levels: TKNN_E_ARG; k >
 * TKNN_MAX_K_REGISTERS: TKNN_E_UNSUPPORTED; a halo tree is set: TKNN_E_UNSUPPORTED (queries over tiles are not
 * served yet); max_rounds reached without allow_unfinished: TKNN_E_ROUNDS.  m = 0 succeeds with a zeroed info.
 * A query with a NaN coordinate never finishes (and NaN points of P are nobody's candidates). */
typedef struct {
  const float *d_queries;   /* m packed fp32 triples (2-D data: z = 0) */
  int64_t m;
  int32_t k;                /* 1 .. TKNN_MAX_K_REGISTERS, and k <= n */
  float start_radius;       /* finite, > 0 */
  int32_t max_rounds;       /* as tknnSolve */
  int32_t allow_unfinished; /* as tknnSolveEx: level -1, row not written, info->unfinished counts */
  int32_t exact;            /* 0: the reference's semantics above.  1: rows rewritten as exact kNN */
  int32_t reserved_;
  int32_t *d_idx;           /* m*k, may be NULL */
  float *d_dist;            /* m*k, may be NULL */
  int64_t *d_intersections; /* m, may be NULL */
  int32_t *d_levels;        /* m, may be NULL (required with allow_unfinished) */
} tknnQueryOptions;
TKNN_API int tknnQuery(tknnEngine e, const tknnQueryOptions *options, tknnSolveInfo *info, void *stream);

/* ---- RT-DBSCAN over the same tree -------------------------------------
 * The reference tree holds no RT-DBSCAN source (README.md:8-9 mentions the method only), so the
 * semantics are this build's own spec (oracle/dbscan_oracle.c): N(p) = {q : dist <= eps} with p
 * included and the TrueKNN fp32 distance arithmetic; core iff |N(p)| >= min_pts; clusters =
 * components of core points, numbered by ascending smallest core index; a border point joins the
 * lowest-numbered adjacent cluster; noise = -1 (sklearn.cluster.DBSCAN's labelling).
 *   d_labels n int32 (required) | d_core n uint8 (may be NULL) | d_counts n int32 |N(p)| (may be
 *   NULL; asking for it disables the early exit of the core test).  Call tknnBuild first. */
typedef struct {
  int32_t clusters;
  float solve_ms;    /* HIP events around all launches of the call */
  float core_ms;     /* the three traversal kernels (events on the launch stream): core flags, */
  float union_ms;    /* unions of neighbouring groups of core points: all launches of the union kernel, */
  float label_ms;    /* labels of border points (tknnDbscanAssign: its one traversal)         */
  int32_t union_launches; /* launches union_ms covers (2: groups that nearly touch, then the rest) */
  int64_t node_tests;         /* tree-node box tests over the three traversals */
  int64_t point_tests;        /* points whose distance to a query was computed (12 algorithmic bytes each) */
  int64_t core_point_tests;   /* ... per traversal */
  int64_t union_point_tests;
  int64_t label_point_tests;
  int64_t union_node_tests;   /* node boxes (32 bytes each) the union kernel's walks looked at */
  int64_t groups;             /* maximal tight nodes with a core point: the vertices of the union pass */
} tknnDbscanInfo;
TKNN_API int tknnDbscan(tknnEngine e, float eps, int min_pts, int32_t *d_labels, uint8_t *d_core,
                        int32_t *d_counts, tknnDbscanInfo *info, void *stream);
/* Labels, core flags and counts are indexed by ROW (position of the point in the buffer given to
 * tknnBuild / tknnBuildIds), also for engines built with ids; clusters are numbered by ascending
 * smallest core row.
 * tknnDbscanAssign: the last step alone, with labels decided by the caller (sharded use: labels
 * agreed between tiles).  d_core_label[row] >= 0: the point is core and has that label; < 0: it is
 * not core.  d_labels[row] = that label for core points, the smallest label among the core points
 * within eps for the others, -1 if there is none.  Core points within eps of each other must carry
 * the same label (true of any DBSCAN clustering). */
TKNN_API int tknnDbscanAssign(tknnEngine e, float eps, const int32_t *d_core_label, int32_t *d_labels,
                              tknnDbscanInfo *info, void *stream);

/* ---- cluster labels for points that are not in the set ---------------------------------------------------------
 * tknnDbscan and tknnDbscanAssign answer for the points of the built set P.  tknnDbscanQuery answers for m arbitrary
 * points Q against the tree of P and a clustering of P the caller hands in as d_core_label (by row, as
 * tknnDbscanAssign takes it: >= 0 core with that label, < 0 not core; core points within eps of each other must carry
 * the same label).  With dist the fp32 formula sqrt((dx*dx + dy*dy) + dz*dz) of every RT-DBSCAN kernel:
 *   d_labels[j]  the smallest d_core_label[p] over the core points p of P with dist(p, q_j) <= eps, -1 if there is
 *                none (the rule by which a border point joins the lowest-numbered adjacent cluster)
 *   d_counts[j]  the number of points p of P, core or not, with dist(p, q_j) <= eps.  Whether q_j would be core itself
 *                (d_counts[j] + 1 >= min_pts) is the caller's to decide: the call takes no min_pts.
 * There is no self: a point of P that coincides with q_j is an ordinary neighbour at distance 0, so with Q = P the
 * labels are tknnDbscan's labels and the counts its d_counts.  A query with a NaN coordinate gets label -1 and count 0;
 * NaN points of P are nobody's neighbour.  Rows of P are rows, not ids; results are addressed by the caller's j
 * whatever order the engine works in.  The tree, the state of tknnSolve and d_core_label are not modified; a halo tree,
 * if set, is ignored as by the other RT-DBSCAN calls.  info is filled as tknnDbscanAssign fills it (clusters = -1,
 * node_tests, point_tests, label_point_tests); label_ms is the traversal kernel alone, solve_ms the whole call with
 * the ordering of the queries along the tree's curve.
 * Errors, in this order: NULL engine / options / d_core_label / d_labels / d_queries with m > 0: TKNN_E_ARG; not
 * built: TKNN_E_STATE; eps not finite-positive, m < 0 or m >= 2^31 - 1: TKNN_E_ARG.  m = 0 succeeds with a zeroed info. */
typedef struct {
  const float *d_queries;       /* m packed fp32 triples (2-D data: z = 0) */
  int64_t m;
  float eps;                    /* finite, > 0 */
  int32_t reserved_;
  const int32_t *d_core_label;  /* n, by row, as tknnDbscanAssign */
  int32_t *d_labels;            /* m, required */
  int32_t *d_counts;            /* m, may be NULL; asking for it adds the counted walk */
} tknnDbscanQueryOptions;
TKNN_API int tknnDbscanQuery(tknnEngine e, const tknnDbscanQueryOptions *options, tknnDbscanInfo *info, void *stream);

/* ---- fixed-radius neighbour lists for points that are not in the set ------------------------------------------------
 * tknnRadiusQuery returns, for m arbitrary points Q, the points of the built set P within `radius` of each, as CSR rows.
 * Row j holds the points p of P with sqrt((dx*dx + dy*dy) + dz*dz) <= radius, every operation fp32 and uncontracted -- the
 * predicate of the RT-DBSCAN calls, so a row's length is tknnDbscanQuery's d_counts[j] at eps = radius.  Distance exactly
 * `radius` is inside.  Nothing is "self": a point of P that coincides with q_j is a neighbour at distance 0.  A query with a
 * NaN coordinate has an empty row; NaN points of P are nobody's neighbour.  An entry names its point by id on trees built with
 * tknnBuildIds, by row otherwise.  A halo tree, if set, is ignored as by the RT-DBSCAN calls; the tree and the state of
 * tknnSolve are not modified; results are addressed by the caller's j whatever order the engine works in.
 * Two passes, as tknnHaloSelect's:
 *   count pass (d_idx = d_dist = NULL): d_offsets[0 .. m] receives the exclusive scan of the row lengths; d_offsets[m] and
 *     info->total are the number of entries the fill pass needs room for.
 *   fill pass  (d_idx given): row j is written at d_offsets[j] .. d_offsets[j + 1] of d_idx (and of d_dist, if given) and
 *     never outside that segment.  The host reads d_offsets[m] once: if it exceeds `capacity`, TKNN_E_ARG before anything is
 *     launched.  A row whose true length differs from its segment (stale offsets, another radius) is counted in
 *     info->mismatched, and the call then returns TKNN_E_STATE (text: tknnLastError); what it has written lies inside the
 *     segments.  sort = 1: every row ascending in (fp32 distance, index) -- fully determined; sort = 0: the order inside a
 *     row is unspecified, the sort is skipped.
 * info: total and max_row over the rows, node_tests / point_tests as the other calls count them (the count pass adds boxes
 * wholly inside the sphere without reading their points), solve_ms the whole call, order_ms the ordering of the queries
 * along the tree's curve, walk_ms the traversal kernels, sort_ms the fill pass's row sort.
 * Errors, in this order: NULL engine / options / d_offsets / d_queries with m > 0: TKNN_E_ARG; not built: TKNN_E_STATE;
 * radius not finite-positive, m < 0, m >= 2^31 - 1, d_dist without d_idx, or capacity < 0: TKNN_E_ARG; 2^31 or more
 * neighbours in one call: TKNN_E_UNSUPPORTED (split the queries).  m = 0 succeeds with d_offsets[0] = 0 (count pass) and a
 * zeroed info. */
typedef struct {
  const float *d_queries;  /* m packed fp32 triples (2-D data: z = 0), any points, in the set or not */
  int64_t m;
  float radius;            /* finite, > 0 */
  int32_t sort;            /* 1: every row in (dist, index) order; 0: order inside a row unspecified */
  int64_t *d_offsets;      /* m + 1, required. count pass: written; fill pass: read */
  int32_t *d_idx;          /* NULL (with d_dist NULL) = count pass; else >= capacity entries */
  float *d_dist;           /* may be NULL in a fill pass */
  int64_t capacity;        /* entries d_idx / d_dist hold (fill pass) */
} tknnRadiusOptions;
typedef struct {
  int64_t total;           /* neighbours over all rows = d_offsets[m] */
  int64_t max_row;         /* longest row */
  int64_t mismatched;      /* fill pass: rows whose length differs from their segment in d_offsets */
  int64_t node_tests, point_tests;
  float solve_ms, order_ms, walk_ms, sort_ms;
} tknnRadiusInfo;
TKNN_API int tknnRadiusQuery(tknnEngine e, const tknnRadiusOptions *o, tknnRadiusInfo *info, void *stream);

/* ---- at most k nearest within a radius, for points that are not in the set ------------------------------------------------
 * tknnRadiusKnn returns, for m arbitrary points Q, the at most k nearest points of the built set P that are no farther than a
 * radius, as dense rows of k: radius(.., max_num_neighbors = k), hybrid search, neighbour lists with a cap.  One pass, no host
 * read of device data before the walk.  With r_j = d_radii[j] where d_radii is given, `radius` otherwise:
 *   row j  is the first min(k, len_j) entries of the row tknnRadiusQuery gives q_j at radius r_j with sort = 1, after the skipped
 *          point, if any, is removed.  Spelled out: the points p of P with sqrt((dx*dx + dy*dy) + dz*dz) <= r_j, every operation
 *          fp32 and uncontracted (the predicate of the RT-DBSCAN calls; distance exactly r_j is inside), ascending in (fp32
 *          distance, index) -- fully determined, ties at the k-th place included --, cut after k.  It is written at
 *          d_idx[j * k ..] (and d_dist[j * k ..]); the unused tail of a row is idx = -1, dist = +inf.
 *   d_counts[j] = min(k, len_j).
 * Nothing is "self" unless d_skip_ids says so: the point named d_skip_ids[j] (by id on trees built with tknnBuildIds, by row
 * otherwise) is left out of row j and of its count -- for Q = P, d_skip_ids[j] = j gives neighbour lists without the point
 * itself, while another point that coincides with it stays, at distance 0.  A negative value skips nothing.  A query with a NaN
 * coordinate has an empty row; NaN points of P are nobody's neighbour.  With d_radii, a row whose radius is NaN, not finite or
 * <= 0 is empty; the host never reads the radii.  An entry names its point by id on trees built with tknnBuildIds, by row
 * otherwise.  k may exceed the size of the set (rows are then never full).  A halo tree, if set, is ignored; the tree and the
 * state of tknnSolve are not modified; results are addressed by the caller's j whatever order the engine works in.
 * info: total = the sum of d_counts, full_rows the rows with k entries, node_tests / point_tests as the other calls count them,
 * lane_rows the rows the one-query-per-lane kernel answered (team stack exhausted, or a tree too small for a box pyramid),
 * solve_ms the whole call, order_ms the ordering of the queries along the tree's curve, walk_ms the traversal kernels.
 * Errors, in this order: NULL engine / options / d_idx / d_queries with m > 0: TKNN_E_ARG; not built: TKNN_E_STATE; k < 1,
 * m < 0, m >= 2^31 - 1, or, without d_radii, a radius that is not finite-positive: TKNN_E_ARG; k > TKNN_MAX_K_REGISTERS:
 * TKNN_E_UNSUPPORTED.  m = 0 succeeds with a zeroed info. */
typedef struct {
  const float *d_queries;     /* m packed fp32 triples (2-D data: z = 0) */
  int64_t m;
  int32_t k;                  /* 1 .. TKNN_MAX_K_REGISTERS; k > n is allowed (rows are then never full) */
  float radius;               /* finite, > 0; ignored for row j where d_radii is given */
  const float *d_radii;       /* NULL, or m floats: row j uses d_radii[j] */
  const int32_t *d_skip_ids;  /* NULL, or m int32: the point named d_skip_ids[j] (id on trees built with ids, row otherwise)
                                 is left out of row j and of its count -- "self" for Q = P; a negative value skips nothing */
  int32_t *d_idx;             /* m*k, required */
  float *d_dist;              /* m*k, may be NULL */
  int32_t *d_counts;          /* m, may be NULL */
} tknnRadiusKnnOptions;
typedef struct {
  int64_t total;              /* entries over all rows = sum of d_counts */
  int64_t full_rows;          /* rows with k entries */
  int64_t node_tests, point_tests;
  int64_t lane_rows;          /* rows the one-query-per-lane kernel answered */
  float solve_ms, order_ms, walk_ms;
  int32_t reserved_;
} tknnRadiusKnnInfo;
TKNN_API int tknnRadiusKnn(tknnEngine e, const tknnRadiusKnnOptions *o, tknnRadiusKnnInfo *info, void *stream);

/* ---- RT-DBSCAN with an auto-grown eps (BASELINE.json configs[4]) ----------------------------------------------
 * No counterpart in the reference (it has no RT-DBSCAN source; BASELINE.md section 4: "spec TBD"), so the rule is this
 * build's own spec (oracle/dbscan_oracle.c, dbref_dbscan_auto), built on the reference's one growth rule, the radius
 * doubling of samples/s01-trueknn/hostCode.cpp:310-330: eps starts at eps0 and doubles (fp32) until at most
 * floor(max_noise * n) points are noise; the labelling returned is tknnDbscan's at that eps.  Growth rounds only
 * count noise (core flags are kept from round to round: neighbourhoods only grow), one full clustering follows.
 * TKNN_E_ROUNDS if max_rounds rounds do not get there (labels then hold the last round's). */
typedef struct {
  tknnDbscanInfo last; /* the full clustering at the final eps */
  int32_t rounds;      /* growth rounds run (1 = eps0 was enough) */
  float eps;           /* the final eps = eps0 * 2^(rounds-1) */
  int64_t noise;       /* points labelled -1 at the final eps */
  float probe_ms;      /* all growth rounds (HIP events) */
  int32_t pad_;
} tknnDbscanAutoInfo;
TKNN_API int tknnDbscanAuto(tknnEngine e, float eps0, int min_pts, double max_noise, int max_rounds, int32_t *d_labels,
                            uint8_t *d_core, tknnDbscanAutoInfo *info, void *stream);
/* One growth round's question alone, for a caller that runs the loop itself (the sharded driver: the tiles' halos grow with
 * eps): d_noise[row] = 1 if the point would be labelled -1 by tknnDbscan(eps, min_pts) -- it is not core and has no core
 * point within eps --, 0 otherwise; no clusters are built.  *noise_count (may be NULL) = how many. */
/* Sharded RT-DBSCAN (owlraytracing_amd/distributed.py): d_out[d_segment[i]] = min(d_out[d_segment[i]], d_value[i])
 * over the n elements with d_segment[i] >= 0; d_out is preset by the caller.  The one per-point step of the label
 * propagation over tiles: the smallest global id of every local cluster.  On the engine's device. */
TKNN_API int tknnSegmentMin(tknnEngine e, const int32_t *d_segment, const int64_t *d_value, int64_t n, int64_t *d_out, void *stream);

TKNN_API int tknnDbscanNoise(tknnEngine e, float eps, int min_pts, uint8_t *d_noise, int64_t *noise_count, void *stream);

/* Test / debug export of the tree to host memory (any pointer may be NULL):
 *   nodes      (n-1) x 8 dwords {lo[3], split, hi[3], other}   (include/owl/lbvh_device.h)
 *   rope_node  n-1, rope_leaf n, prim_id n (caller index of sorted slot)            */
TKNN_API int tknnExportTree(tknnEngine e, void *nodes, int32_t *rope_node, int32_t *rope_leaf,
                            int32_t *prim_id, void *stream);

/* Test hook: the builder's two side tables of a point tree with n > 1 (host buffers).
 *   split_owner  n-1: the internal node that splits its range after sorted position s -- an internal node i is a left
 *                child iff i is the LAST position of its range (parent = split_owner[i]), else a right child (parent =
 *                split_owner[i-1]); RT-DBSCAN climbs with it (owlraytracing_amd/csrc/dbscan_union.hip, db_uniform_kernel)
 *   block_paths  ceil(n/64) x 5: per block of 64 sorted slots the deepest internal node whose range holds the whole block
 *                (last word) and its four nearest ancestors, farthest first, the root where the path is shorter            */
TKNN_API int tknnExportTreeTables(tknnEngine e, int32_t *split_owner, int32_t *block_paths, void *stream);

/* Test / debug export of everything else the readers of a point tree rely on (tests/lbvh_spec.py restates each array from the
 * headers; tests/test_lbvh_gpu.py compares them word for word).  which = 0: the tree of tknnBuild / tknnBuildIds; which = 1: the
 * halo tree of tknnSetHalo.  n is the tree's point count; every pointer is a HOST buffer and may be NULL:
 *   keys         n uint64: the sorted 63-bit curve keys (curve_point_key of owlraytracing_amd/csrc/curve_key.h with 21 levels over
 *                the scene box below; bit 63 alone for a point with a NaN coordinate), ascending, equal keys in input order
 *   points       ceil(n/16)*16 + 16 records {x, y, z, id} of 16 bytes: the points in that order (a point with a NaN coordinate
 *                stored as all-NaN; id = d_ids[row], or the row without ids), then sentinels {NaN, NaN, NaN, -1} that fill the
 *                last block of 16 and one whole block after it
 *   row_slot     n: the sorted slot of each input row (the inverse of prim_id)
 *   wide_boxes   the 64-ary box pyramid the team kernels descend (LbvhWideView, include/owl/lbvh_device.h): the wide_levels
 *                live levels one after the other, level l with wide_count[l] boxes {lo[3], hi[3]}; level 0 = the boxes of the
 *                blocks of 16 sorted points, level l = the boxes of 64 consecutive entries of level l-1, levels added while
 *                the top one has more than 64 entries.  wide_capacity = the boxes the buffer holds (TKNN_E_HIP if too few;
 *                ceil(n/16) * 33/32 + 6 always suffice)
 *   nodes, rope_node, rope_leaf, prim_id, split_owner   as tknnExportTree / tknnExportTreeTables give them for the own tree
 *   scene        lo xyz, hi xyz of the points (NaN coordinates ignored); nan_count: the points with a NaN coordinate, the last
 *                of the order; curve: 0 Hilbert, 1 Morton (TKNN_CURVE at build time)
 * TKNN_E_STATE when the tree asked for is not built: before tknnBuild, and for which = 1 while no halo is set. */
typedef struct {
  int32_t which;         /* in */
  int32_t curve;         /* out, as everything down to scene */
  int64_t n;
  int32_t nan_count;
  int32_t wide_levels;
  int32_t wide_count[6];
  float scene[6];
  int64_t wide_capacity; /* in */
  uint64_t *keys;
  void *points;
  int32_t *row_slot;
  void *wide_boxes;
  void *nodes;
  int32_t *rope_node;
  int32_t *rope_leaf;
  int32_t *prim_id;
  int32_t *split_owner;
} tknnTreeExport;
TKNN_API int tknnExportTreeEx(tknnEngine e, tknnTreeExport *x, void *stream);

/* Test hook for the builder's box trees (what the owl* entry points build over a bounds program's output), without an engine.
 * mode 0: a private tree is built from the n device boxes d_boxes ({lo[3], hi[3]}, 24 bytes each; sorted by the curve key of
 * the centres 0.5f*lo + 0.5f*hi); if d_boxes_refit is not NULL, the tree is then refitted to those n boxes (same topology and
 * order, new node boxes); then nodes (n-1), rope_node (n-1), rope_leaf (n), prim_id (n) and sorted_boxes (n x 6 floats: the
 * boxes last given, in sorted order) are copied to the HOST buffers given (any may be NULL).
 * mode 1: no tree is built, mode 2: a POINT tree is built (d_boxes read as 2 n points), and a refit is asked of it: the refit
 * is refused with TKNN_E_STATE, nothing is launched for it and nothing is copied. */
TKNN_API int tknnDebugBoxTree(const float *d_boxes, int64_t n, const float *d_boxes_refit, int mode, void *nodes,
                              int32_t *rope_node, int32_t *rope_leaf, int32_t *prim_id, float *sorted_boxes, void *stream);

/* Test hook for the wave kernel's candidate test.  For each pair (q[i], r[i]) writes lo[i], hi[i]
 * such that, for every fp32 c,   lo <= c <= hi   <=>   fl(c - r) <= q <= fl(c + r)
 * (the box the bounds program of deviceCode.cu:38-56 writes, tested against the query point). */
TKNN_API int tknnDebugThresholds(const float *d_q, const float *d_r, int64_t n, float *d_lo,
                                 float *d_hi, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OWLKNN_H */
