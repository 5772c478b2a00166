// periodic_knn.hip -- at most k nearest points in a cell that is periodic along some of its axes, with or without a radius, for
// query points that are not in the tree or for the tree's own points (tknnPeriodicKnn, include/owlknn_periodic.h).
//
// tknnRadiusKnn and tknnKnn with the wrapped distance of periodic_metric.h.  The tree is the open-space one: a periodic metric is
// a matter of the query side.  The walk needs a lower bound of the wrapped distance from the query to a box
// (periodic_box_min_dist2, which looks at the query and its two shifted images per periodic axis) and the leaf test the wrapped
// distance itself (periodic_dist2).  ONE walk covers a query -- there is no loop over images --, so every point is met once and no
// point can enter a row twice, also where the k-th distance exceeds half a period.
//   1. external queries: query_order (query_order.h); without any radius also rknn_slots, a query's place in the tree's order
//      (knn_seed.hip).  The tree's own points are their slots and come in curve order: neither pass.
//   2. without any radius (d_radii == NULL, radius == FLT_MAX): rknn_seed_kernel<NREG, PeriodicRule> (radius_knn_walk.h), the
//      window around the slot with periodic_dist2.
//   3. rknn_walk_kernel<NREG, PeriodicRule> and rknn_lane_kernel<K, PeriodicRule>, with an unbounded query box; every query goes
//      to the lane kernel under TKNN_PERIODIC_KNN_FORCE_FALLBACK=1 (read per call).
#include "owlknn_periodic.h"
#include "periodic_metric.h"
#include "query_order.h"
#include "radius_knn_walk.h"

#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

struct PeriodicKnnArgs {
  LbvhView bvh;
  LbvhWideView wide;
  PeriodicCell cell;
  const float *queries;     // external: m packed triples, by the caller's j; null: the tree's own points, an item is a sorted slot
  const uint32_t *order;    // external: the query worked on at sorted position i
  const int32_t *slots;     // external, seed pass: its place in the tree's order, by sorted position (0 .. n)
  int32_t m;
  int k;
  float radius;             // every row's radius if radii and bounds are null (FLT_MAX: none)
  const float *radii;       // m, by the caller's j (may be null)
  float *bounds;            // the seed pass's r_j, by item (null: no seed pass)
  const int32_t *skip_ids;  // external: m, by the caller's j (may be null)
  int force_redo;           // TKNN_PERIODIC_KNN_FORCE_FALLBACK (tests): the walk leaves every query to the lane kernel
  int32_t *out_idx;         // m*k
  float *out_dist;          // m*k (may be null)
  int32_t *out_counts;      // m (may be null)
  int32_t *redo;            // m: items left to the lane kernel
  unsigned long long *ws;   // kRknnWsWords counters
};

// The box rule: a child box is declined if the wrapped distance to every in-cell point of it lies beyond the gate.  The bound
// carries its own absolute slack for the roundings of the shifted images (periodic_metric.h); it and beyond_gate's margin can only
// keep a box the exact rule would decline.  The query box of walk_tree is unbounded (r_wide = FLT_MAX, as tknnKnn's is without a
// seed): a box across a face is as near as one next door.
struct PeriodicRule {
  using Args = PeriodicKnnArgs;
  struct Query {
    LbvhPoint q;
    float r;       // the predicate's radius: the caller's, or the seed bound (which may be 0: k duplicates of the query)
    float r_wide;  // FLT_MAX
    float gate_r;  // the squared-distance gate of an empty list: every d2 whose rounded root can be <= r passes
    int32_t skip;  // the point left out of the row (no point has a negative id)
    int32_t row;   // the caller's j
    bool valid;    // a radius the call takes and a query in the cell without a NaN (a row without: empty)
  };
  static __device__ __forceinline__ int32_t item_at(const Args &a, int32_t pos) { return a.queries ? (int32_t)a.order[pos] : pos; }
  // the point, skipped id and row of an item: the caller's query j, or (the tree's own points) the point of a sorted slot
  static __device__ __forceinline__ void point(const Args &a, int32_t item, bool has_q, Query &s) {
    s.q = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
    s.skip = -1, s.row = item;
    if (!has_q) return;
    if (a.queries) {
      s.q.x = a.queries[3 * (int64_t)item], s.q.y = a.queries[3 * (int64_t)item + 1], s.q.z = a.queries[3 * (int64_t)item + 2];
      s.skip = a.skip_ids ? a.skip_ids[item] : -1;
    } else {
      s.q = a.bvh.points[item];
      s.skip = s.q.id;
      s.row = a.bvh.prim_id[item];
    }
  }
  static __device__ __forceinline__ Query query(const Args &a, int32_t item, bool has_q) {
    Query s;
    point(a, item, has_q, s);
    s.r = !has_q ? 0.f : a.bounds ? a.bounds[item] : a.radii ? a.radii[s.row] : a.radius;
    const bool in_cell = periodic_in_cell(s.q.x, a.cell.lo[0], a.cell.period[0]) & periodic_in_cell(s.q.y, a.cell.lo[1], a.cell.period[1]) &
                         periodic_in_cell(s.q.z, a.cell.lo[2], a.cell.period[2]);
    const bool no_nan = (s.q.x == s.q.x) & (s.q.y == s.q.y) & (s.q.z == s.q.z);
    s.valid = has_q && (s.r > 0.f || (a.bounds && s.r == 0.f)) && s.r <= FLT_MAX && in_cell && no_nan;  // (a NaN radius: neither)
    s.r_wide = FLT_MAX;
    s.gate_r = knn_gate_from_worst(s.r);
    return s;
  }
  static __device__ __forceinline__ bool keep_box(const Args &a, const Query &s, const LbvhBox &bx, int32_t, int, float tau2) {
    return !beyond_gate(periodic_box_min_dist2(bx, s.q.x, s.q.y, s.q.z, a.cell), tau2);
  }
  static __device__ __forceinline__ float dist2(const Args &a, const Query &s, const LbvhPoint &p) {
    return periodic_dist2(p.x, p.y, p.z, s.q.x, s.q.y, s.q.z, a.cell);
  }
  static __device__ __forceinline__ bool slot_ok(const Query &, int32_t) { return true; }
  static __device__ __forceinline__ LaneStep lane_node(const Args &a, const Query &s, int32_t, const LbvhNode &nd, float gate) {
    return beyond_gate(periodic_box_min_dist2(nd, s.q.x, s.q.y, s.q.z, a.cell), gate) ? lane_rope() : lane_descend();
  }
  // every block that holds a point without a NaN (a query at a face has half of its neighbours elsewhere on the curve: that costs
  // a wider walk, nothing else)
  static __device__ __forceinline__ void seed_range(const Args &a, const Query &, int32_t pos, bool has_q, int32_t clean_blocks, int32_t &blk_lo,
                                                    int32_t &blk_hi, int32_t &slot) {
    blk_lo = 0, blk_hi = clean_blocks;
    slot = min(has_q ? (a.queries ? a.slots[pos] : pos) : 0, a.bvh.n - 1);
  }
  static __device__ __forceinline__ void seed_store(const Args &a, const Query &, int32_t item, float bound) { a.bounds[item] = bound; }
};

}  // namespace

void Engine::periodic_knn(const tknnPeriodicKnnOptions &o, tknnPeriodicKnnInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const bool self = o.d_queries == nullptr;
  const bool seeded = !o.d_radii && o.radius == FLT_MAX;
  // the call's workspace: counters | lane list, bounds | external: codes, order (+ the sort's second halves), sort space
  const size_t sort_bytes = self ? 0 : query_order_sort_bytes(m, s);
  RknnWorkspace w(m, 6, sort_bytes);
  w.base = (char *)workspace(w.bytes);
  uint32_t *codes = w.column<uint32_t>(2), *codes_alt = w.column<uint32_t>(3), *order_in = w.column<uint32_t>(4), *order = w.column<uint32_t>(5);
  int32_t *slots = w.column<int32_t>(2);  // (over the codes: the sort is through when the slots are written)

  PeriodicKnnArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.wide = bvh_.wide_view();
  for (int ax = 0; ax < 3; ax++) a.cell.lo[ax] = o.period[ax] > 0.f ? o.lo[ax] : 0.f, a.cell.period[ax] = o.period[ax] > 0.f ? o.period[ax] : 0.f;
  a.queries = o.d_queries;
  a.order = self ? nullptr : order;
  a.slots = self ? nullptr : slots;
  a.m = (int32_t)m;
  a.k = o.k;
  a.radius = o.radius;
  a.radii = o.d_radii;
  a.bounds = seeded ? w.column<float>(1) : nullptr;
  a.skip_ids = o.d_skip_ids;
  if (const char *e = getenv("TKNN_PERIODIC_KNN_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.out_idx = o.d_idx;
  a.out_dist = o.d_dist;
  a.out_counts = o.d_counts;
  a.redo = w.column<int32_t>(0);
  a.ws = w.words();

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kRknnWsWords * sizeof(unsigned long long), s));
  if (!self) query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, w.column<void>(6), sort_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  if (seeded) {
    if (!self) rknn_slots(o.d_queries, order, (int32_t)m, bvh_.scene_device(), bvh_.curve(), bvh_.keys_device(), a.bvh.n, slots, s);
    rknn_seed<PeriodicRule>(a, cu_count_, s);
  }
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  const unsigned long long n_redo = rknn_walks<PeriodicRule>(a, cu_count_, h_counters_, s);
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  rknn_fill_info(info, h_counters_, n_redo, ev_a_, ev_b_, ev_c_, ev_d_);
}

}  // namespace owlmi
