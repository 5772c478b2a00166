// lane_walk.h -- ONE LANE's stackless rope walk of the binary LBVH for one query, and the box arithmetic around it, shared by the
// kernels that walk one query per lane: lane_round_kernel and repair_kernel (trueknn.hip), query_lane_kernel (trueknn_query.hip),
// and RT-DBSCAN's for_each_core_group (unions, border, label, assign, query) and db_count_from (db_core_body's neighbour count) in
// db_device.h and db_has_core_neighbour in dbscan_core.hip.
// What a walk does at a node and at a point comes in as two callables; every function is inlined into its caller.  The box tests
// below, their parenthesisation and the counting rule's margin are what make rows equal the reference's bit for bit: they are
// written here once.  (The 16-lane team walk of the box pyramid is team_walk.h; the wave-uniform walks keep their own loops.)
#pragma once
#include <hip/hip_runtime.h>

#include "owl/lbvh_device.h"

namespace owlmi {
namespace {

constexpr int kCountedSubtree = 32;  // smallest subtree a lane walk tries to count instead of walking (lane_counts_subtree)

// the tree's slots before its NaN points (they sort last): a range of slots that ends before it holds finite points only
__device__ __forceinline__ int32_t lane_clean_end(const LbvhView &tv) { return tv.n - (tv.nan_count ? *tv.nan_count : 0); }

// ---- the box arithmetic ------------------------------------------------------------------------------------------------
// Can the node hold a point p whose box [c_p - r, c_p + r] holds q (deviceCode.cu:38-56, knn_in_box)?  Conservative: any point of the
// node has lo <= c_p <= hi, and fp32 rounding is monotone, so fl(c_p - r) >= fl(lo - r) and fl(c_p + r) <= fl(hi + r).
__device__ __forceinline__ bool lane_box_hit(const LbvhNode &nd, const LbvhPoint &q, float r) {
  return (nd.lo[0] - r <= q.x) & (q.x <= nd.hi[0] + r) & (nd.lo[1] - r <= q.y) & (q.y <= nd.hi[1] + r) & (nd.lo[2] - r <= q.z) &
         (q.z <= nd.hi[2] + r);
}
// The same monotonicity the other way round: if even the largest centre passes the lower test and the smallest the upper one,
// EVERY point of the node is a candidate (deviceCode.cu:74 would count each).
__device__ __forceinline__ bool lane_box_inside(const LbvhNode &nd, const LbvhPoint &q, float r) {
  return (nd.hi[0] - r <= q.x) & (q.x <= nd.lo[0] + r) & (nd.hi[1] - r <= q.y) & (q.y <= nd.lo[1] + r) & (nd.hi[2] - r <= q.z) &
         (q.z <= nd.lo[2] + r);
}
// squared distances from q to the farthest and to the nearest point of the node's box (near2 <= every point's, up to rounding)
__device__ __forceinline__ void lane_box_dist2(const LbvhNode &nd, const LbvhPoint &q, float &far2, float &near2) {
  const float ax = fmaxf(fabsf(q.x - nd.lo[0]), fabsf(q.x - nd.hi[0])), ay = fmaxf(fabsf(q.y - nd.lo[1]), fabsf(q.y - nd.hi[1])),
              az = fmaxf(fabsf(q.z - nd.lo[2]), fabsf(q.z - nd.hi[2]));
  const float gx = fmaxf(fmaxf(nd.lo[0] - q.x, q.x - nd.hi[0]), 0.f), gy = fmaxf(fmaxf(nd.lo[1] - q.y, q.y - nd.hi[1]), 0.f),
              gz = fmaxf(fmaxf(nd.lo[2] - q.z, q.z - nd.hi[2]), 0.f);
  far2 = (ax * ax + ay * ay) + az * az;
  near2 = (gx * gx + gy * gy) + gz * gz;
}
// The count-instead-of-walk rule of the TrueKNN lane kernels, for a node that passed lane_box_hit: if every point of its subtree is
// a candidate and none of them can enter the list any more, or tie with its last entry -- the node lies beyond `gate`, the list's
// squared-distance gate (knn_gate_from_worst) --, the subtree is counted (`count` points), not walked: a query whose box has grown
// over a whole cluster costs O(log n) instead of O(cluster).  The margin of 5e-6 covers the roundings of near2 and of the points'
// own distance arithmetic; a node that holds the query itself has near2 = 0 and is never counted, so a self-solve's count of the
// OTHER points stays right.  Subtrees that reach into the NaN points (they are no candidates) are walked.  Only tried from
// kCountedSubtree points on: near the leaves the test would cost as much as the node test itself and save nothing.
__device__ __forceinline__ bool lane_counts_subtree(int32_t ref, const LbvhNode &nd, const LbvhPoint &q, float r, float gate, int32_t clean_end,
                                                    int32_t &count) {
  const int32_t last = lbvh_last(ref, nd.other);
  count = last - lbvh_first(ref, nd.other) + 1;
  if (!(count >= kCountedSubtree && lane_box_inside(nd, q, r))) return false;
  float far2, near2;
  lane_box_dist2(nd, q, far2, near2);
  return near2 * 0.999995f > gate && last < clean_end;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------
struct LaneStep {  // what a callable answers: where the walk goes next
  enum Kind : int32_t { kDescend, kRope, kGoto, kStop } kind;
  int32_t ref;  // kGoto
};
__device__ __forceinline__ LaneStep lane_descend() { return {LaneStep::kDescend, 0}; }        // to the node's left child (nodes only)
__device__ __forceinline__ LaneStep lane_rope() { return {LaneStep::kRope, 0}; }              // past the subtree / the point
__device__ __forceinline__ LaneStep lane_goto(int32_t ref) { return {LaneStep::kGoto, ref}; }  // on at a reference the callable kept
__device__ __forceinline__ LaneStep lane_stop() { return {LaneStep::kStop, 0}; }              // the walk is over

// When a step's rope is loaded: after the callable has asked for it, or together with the node (or the point) -- a walk is a chain of
// dependent loads, this halves it for four more bytes per step.  Measured per walk: the caller's compile-time choice, not to be unified.
enum class LaneRope { kWhenTaken, kWithNode };

// Depth-first, left-first, from reference `from` until the walk would arrive at `until`: the rope of the subtree's root, so a walk
// of a whole tree goes from tv.root until LBVH_END, and `from` may be a leaf (a tree of one point).  The subtree rooted at `skip` is
// stepped over through `skip_rope`, its rope, before anything of it is loaded (LBVH_END: none -- with both constant the test costs
// nothing).  at_node(ref, node, rope) and at_leaf(slot, point) answer with a LaneStep; `rope` is the node's under kWithNode (a walk
// that comes back later to where it leads has it without a second load), 0 otherwise.  True if a callable stopped the walk.
template <LaneRope ROPE, class NodeFn, class LeafFn>
__device__ __forceinline__ bool lane_walk(const LbvhView &tv, int32_t from, int32_t until, int32_t skip, int32_t skip_rope, NodeFn at_node,
                                          LeafFn at_leaf) {
  constexpr bool kEarly = ROPE == LaneRope::kWithNode;
  int32_t ref = from;
  while (ref != until) {
    if (ref == skip) {
      ref = skip_rope;
      continue;
    }
    if (ref >= 0) {
      const LbvhNode nd = tv.nodes[ref];
      const int32_t rope = kEarly ? tv.rope_node[ref] : 0;
      const LaneStep s = at_node(ref, nd, rope);
      if (s.kind == LaneStep::kStop) return true;
      ref = s.kind == LaneStep::kDescend ? lbvh_left_ref(ref, nd) : s.kind == LaneStep::kGoto ? s.ref : kEarly ? rope : tv.rope_node[ref];
    } else {
      const int32_t slot = ~ref;
      const LbvhPoint p = tv.points[slot];
      const int32_t rope = kEarly ? tv.rope_leaf[slot] : 0;
      const LaneStep s = at_leaf(slot, p);
      if (s.kind == LaneStep::kStop) return true;
      ref = s.kind == LaneStep::kGoto ? s.ref : kEarly ? rope : tv.rope_leaf[slot];
    }
  }
  return false;
}
template <LaneRope ROPE, class NodeFn, class LeafFn>  // the whole tree
__device__ __forceinline__ bool lane_walk(const LbvhView &tv, NodeFn at_node, LeafFn at_leaf) {
  return lane_walk<ROPE>(tv, tv.root, LBVH_END, LBVH_END, LBVH_END, at_node, at_leaf);
}

}  // namespace
}  // namespace owlmi
