// radius_knn.hip -- at most k nearest points within a radius, for query points that are NOT in the tree (tknnRadiusKnn,
// include/owlknn.h).
//
// Row j is the row tknnRadiusQuery gives q_j at its radius r_j with sort = 1 -- the points p of the built set with
// knn_sqrt(knn_dist2(..)) <= r_j, ascending in (fp32 distance, index) --, without the point d_skip_ids names, cut after k entries
// and padded with (-1, +inf) to k.  One pass over the tree: the list's gate starts at r_j instead of infinity and shrinks as the
// list fills, so a row costs the walk at r_j or the walk of a k-nearest query, whichever is less.
//   1. query_order (query_order.h): the queries along the tree's own curve, as the other query calls order them;
//   2. rknn_walk_kernel<NREG, EuclidRule> (radius_knn_walk.h): the team walk with radius_query.hip's box of half-width
//      r * (1 + 1e-6) and the sphere predicate;
//   3. rknn_lane_kernel<K, EuclidRule>: one query per lane, for the queries whose team stack overflowed (a redo list whose length
//      lives on the device) and for trees too small for a box pyramid.
// The Euclidean rule's walk and lane hooks are here, and with them the kernels that tknnKnn (knn_seed.hip) launches through
// radius_knn_walks with the bounds its seed pass found.
#include "query_order.h"
#include "radius_knn_walk.h"

#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

struct EuclidRule {
  using Args = RadiusKnnKernelArgs;
  struct Query {
    LbvhPoint q;
    float r;       // the sphere predicate's radius
    float r_wide;  // r * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts (radius_query.hip)
    float gate_r;  // the squared-distance gate of an empty list: every d2 whose rounded root can be <= r passes
    int32_t skip;  // the point left out of the row (no point has a negative id)
    int32_t row;   // the row of the output the answer goes to
    bool valid;    // a finite positive radius, or a zero one where the call takes it (a row without one is empty)
  };
  static __device__ __forceinline__ int32_t item_at(const Args &a, int32_t pos) { return a.order ? (int32_t)a.order[pos] : pos; }
  static __device__ __forceinline__ Query query(const Args &a, int32_t qi, bool has_q) {
    Query s;
    s.q.x = a.queries[3 * (int64_t)qi], s.q.y = a.queries[3 * (int64_t)qi + 1], s.q.z = a.queries[3 * (int64_t)qi + 2];
    s.q.id = -1;
    s.r = a.radii ? (has_q ? a.radii[qi] : 0.f) : a.radius;
    s.skip = a.skip_ids && has_q ? a.skip_ids[qi] : -1;
    s.row = a.out_row && has_q ? a.out_row[qi] : qi;
    s.valid = (s.r > 0.f || (a.zero_radius_ok && s.r == 0.f)) && s.r <= FLT_MAX;  // (NaN: neither)
    s.r_wide = s.r * 1.000001f;
    s.gate_r = knn_gate_from_worst(s.r);
    return s;
  }
  static __device__ __forceinline__ bool keep_box(const Args &, const Query &s, const LbvhBox &bx, int32_t, int, float tau2) {
    return !beyond_gate(box_min_dist2(bx, s.q), tau2);
  }
  static __device__ __forceinline__ float dist2(const Args &, const Query &s, const LbvhPoint &p) { return knn_dist2(p.x, p.y, p.z, s.q.x, s.q.y, s.q.z); }
  static __device__ __forceinline__ bool slot_ok(const Query &, int32_t) { return true; }
  static __device__ __forceinline__ LaneStep lane_node(const Args &, const Query &s, int32_t, const LbvhNode &nd, float gate) {
    return rknn_lane_box(nd, s.q, s.r_wide, gate);
  }
};

}  // namespace

unsigned long long radius_knn_walks(const RadiusKnnKernelArgs &a, int cu_count, unsigned long long *h_words, hipStream_t s) {
  return rknn_walks<EuclidRule>(a, cu_count, h_words, s);
}

void Engine::radius_knn(const tknnRadiusKnnOptions &o, tknnRadiusKnnInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  // the call's workspace: counters | codes, order (+ the sort's second halves), lane list | sort space
  const size_t sort_bytes = query_order_sort_bytes(m, s);
  RknnWorkspace w(m, 5, sort_bytes);
  w.base = (char *)workspace(w.bytes);
  uint32_t *codes = w.column<uint32_t>(0), *codes_alt = w.column<uint32_t>(1), *order_in = w.column<uint32_t>(2), *order = w.column<uint32_t>(3);

  RadiusKnnKernelArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.wide = bvh_.wide_view();
  a.queries = o.d_queries;
  a.order = order;
  a.m = (int32_t)m;
  a.k = o.k;
  a.radius = o.radius;
  a.radii = o.d_radii;
  a.skip_ids = o.d_skip_ids;
  if (const char *e = getenv("TKNN_RADIUS_KNN_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.out_idx = o.d_idx;
  a.out_dist = o.d_dist;
  a.out_counts = o.d_counts;
  a.redo = w.column<int32_t>(4);
  a.ws = w.words();

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kRknnWsWords * sizeof(unsigned long long), s));
  query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, w.column<void>(5), sort_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  const unsigned long long n_redo = radius_knn_walks(a, cu_count_, h_counters_, s);
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  rknn_fill_info(info, h_counters_, n_redo, ev_a_, ev_b_, ev_b_, ev_c_);
}

}  // namespace owlmi
