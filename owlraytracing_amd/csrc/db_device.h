// db_device.h -- what RT-DBSCAN's kernel files share (dbscan.hip has the algorithm and the map of the files): DbArgs, the
// kernels' argument block, and the device helpers more than one kernel family uses -- the work counters, the tight-node test,
// the union-find, the two neighbour walks.  Engine::DbCall carries a DbArgs across those files (db_call.h), so it is not in an
// anonymous namespace; the helpers are, and every one is inlined into its caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knn_device.h"
#include "lane_walk.h"

#ifndef TKNN_DIAG_BUILD
#define TKNN_DIAG_BUILD 0  // make DIAG=1 -> libowl_mi355x_diag.so: TKNN_DB_DIAG switches parts of the union pass off (times only)
#endif

namespace owlmi {

struct DbArgs {
  LbvhView bvh;
  float eps;
  float eps_wide;  // eps * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts
  int min_pts;
  int want_counts;
  int keep_core;         // tknnDbscanAuto: slots already flagged core by a round with a smaller eps stay core (N(p) only grows)
  uint8_t *core_sorted;  // per sorted slot
  uint8_t *core;         // per caller index (may be null)
  int32_t *counts;       // per caller index (may be null)
  int32_t *parent;       // union-find over SORTED SLOTS (the smaller slot stays root): neighbours in space are neighbours in memory
  int32_t *min_row;      // per slot, meaningful at roots: the smallest row (caller index) among the cluster's core points
  int32_t *rank;         // per caller index: cluster label of the cluster whose smallest core row it is
  int32_t *labels;       // per caller index
  const int32_t *next_core;  // per sorted slot (+1 sentinel): first core slot at or after it, n if none
  float eps_in2, eps_out2;   // eps^2 (1 -+ 1e-5): below / above these, fp32 distance arithmetic cannot disagree
  // work counters, per traversal kernel (kDbStatCore, kDbStatUnion, kDbStatLabel: knn_device.h): tree nodes
  // tested, then points whose distance to a query was computed (12 algorithmic bytes each)
  unsigned long long *stats;
  int32_t *group_of;  // per sorted slot, written by the core-flag kernel (see db_group_kernel); null: not wanted
  int32_t *near_node;  // per sorted slot, or null: the node a few levels above the point's group (written by the core-flag kernel for the noise probe)
  int short_way;  // db_group_union_kernel's settle: 0: the long way only (measurements)
  int chunk;  // packets per chunk dealt to an XCD (db_group_union_kernel)
  int scan_budget;  // steps the quick scan of a probe may take before the subtrees are asked (db_group_union_kernel)
  float reach, near_lo2, near_hi2;  // this pass of db_group_union_kernel: groups whose nearest faces are near_lo2 < d^2 <= near_hi2 apart, reach >= sqrt(near_hi2)
  // second pass of db_group_union_kernel: uni[node] >= 0: every core point under the node is in the set that slot was the root
  // of when the first pass had ended (db_uniform_kernel); negative: not known to be one set
  const int32_t *block_paths;  // Lbvh::block_paths_device(), or null: where a slot's walk down to its group may start
  const int32_t *split_owner;  // Lbvh::split_owner_device()
  int32_t *uni;       // per internal node
  int32_t *uni_leaf;  // per sorted slot, written for the listed groups that are single points only
  int32_t *pk_diag;  // diagnostic library, TKNN_DB_DIAG & 512: per packet of the timed pass: ticks, extent (1e-6), rounds, settles
  unsigned long long *diag_out;  // diagnostic library, TKNN_DB_DIAG & 512: the group-union kernel's wave time by part ([0] loads [1] tests [2] settles [3] pushes [4] packet set-up, s_memtime ticks) and [5] rounds [6] settles [7] packets
  int diag;  // TKNN_DB_DIAG, diagnostic library only (results are wrong when set): 1 = no probes, 2 = no unions between groups, 4 = none inside groups, 8 = walk lengths on stderr, 16 = report a stack overflow (the result is right: the call falls back), 32 = probes by scanning only (the result is right)
};

// consecutive slots (or rows) per thread of the kernels that move four words as one 16-byte load or store (db_flatten_kernel
// says why; db_label_kernel, db_rows_from_slots_kernel); the host sizes their grids by it
constexpr int kDbPer = 4;

namespace {

// a workgroup's counts into the kernel's two counters: wave sums, one LDS atomic per wave, one global
// atomic per workgroup (every thread of the workgroup must call it).  `stats` = a.stats + the kernel's kDbStat.. word: the
// counters are kept in kDbStripes stripes, a workgroup adds to the stripe of its index, the host sums them (knn_device.h).
__device__ __forceinline__ void db_add_stats(unsigned long long *stats, unsigned long long *blk, uint32_t nodes, uint32_t points) {
  stats += (blockIdx.x & (kDbStripes - 1)) * kDbStripeWords;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nodes += __shfl_xor(nodes, off);
    points += __shfl_xor(points, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&blk[0], (unsigned long long)nodes);
    atomicAdd(&blk[1], (unsigned long long)points);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&stats[0], blk[0]);
    atomicAdd(&stats[1], blk[1]);
  }
}

// the same for a kernel whose waves are independent and whose LDS is counted in waves per CU: one global atomic per wave
__device__ __forceinline__ void db_add_stats_wave(unsigned long long *stats, uint32_t nodes, uint32_t points) {
  stats += ((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (kDbStripes - 1)) * kDbStripeWords;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nodes += __shfl_xor(nodes, off);
    points += __shfl_xor(points, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&stats[0], (unsigned long long)nodes);
    atomicAdd(&stats[1], (unsigned long long)points);
  }
}

__device__ __forceinline__ bool node_is_tight(const LbvhNode &nd, float eps_in2) {
  const float ex = nd.hi[0] - nd.lo[0], ey = nd.hi[1] - nd.lo[1], ez = nd.hi[2] - nd.lo[2];
  return ex * ex + ey * ey + ez * ez <= eps_in2;  // NaN boxes (none: fit ignores NaN points) would be "not tight"
}

__device__ __forceinline__ int32_t uf_load(int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t x) {
  for (;;) {
    int32_t p = uf_load(parent + x);
    if (p == x) return x;
    int32_t g = uf_load(parent + p);
    if (g == p) return p;  // p is a root
    __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // path halving
    x = g;
  }
}
__device__ __forceinline__ void uf_unite(int32_t *parent, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    // hook the larger root under the smaller; fails if `hi` stopped being a root meanwhile
    if (atomicCAS(parent + hi, hi, lo) == hi) return;
  }
}

// Walks the tree for the CORE neighbours of q, tight nodes settled as a whole: calls
// f(representative's slot) for every tight node that has a core point within eps of q (its first core
// point stands for all of them) and for every core point within eps reached as a leaf.  `own_slot`
// (or -1) names q's own sorted slot: the tight node holding it is skipped.
// `settled(slot)` may say that the group a tight node's first core point stands for needs no look
// (the union kernel: already in my set), sparing the distance tests and the probe.
template <typename S, typename F>
__device__ __forceinline__ void for_each_core_group(const DbArgs &a, const LbvhPoint &q, int32_t own_slot, S settled, F f,
                                                    uint32_t &node_tests, uint32_t &point_tests) {
  const LbvhView &bvh = a.bvh;
  const float r = a.eps_wide;
  // A tight node the sphere cuts through is PROBED, not scanned: the walk goes on below it (its
  // descendants are tight too: inside -> hit, outside -> skipped) and leaves the subtree through the
  // node's own rope at the first core point found within eps -- one is enough, the node is one group.
  int32_t probe_rep = -1, probe_exit = LBVH_END;
  auto arrive = [&](int32_t ref) { probe_rep = ref == probe_exit ? -1 : probe_rep; };  // left the probed subtree without a hit
  auto found = [&]() {  // the probe's answer: its group is within eps, on behind its subtree
    f(probe_rep);
    probe_rep = -1;
    return lane_goto(probe_exit);
  };
  // (the rope with the node, and at a leaf three independent loads at once -- nearly every leaf reached is core)
  lane_walk<LaneRope::kWithNode>(bvh,
      [&](int32_t ref, const LbvhNode &nd, int32_t rope) {
        arrive(ref);
        node_tests++;
        if (!lane_box_hit(nd, q, r)) return lane_rope();
        const bool probing = probe_rep >= 0;
        if (probing || node_is_tight(nd, a.eps_in2)) {
          const int32_t first = lbvh_first(ref, nd.other), last = lbvh_last(ref, nd.other);
          const int32_t s = a.next_core[first];
          if (s > last || (first <= own_slot && own_slot <= last)) return lane_rope();  // no core point here / my own group
          if (!probing && settled(s)) return lane_rope();
          float far2, near2;
          lane_box_dist2(nd, q, far2, near2);
          if (far2 <= a.eps_in2) {  // every point of the node is within eps
            if (probing) return found();
            f(s);
            return lane_rope();
          }
          if (near2 > a.eps_out2) return lane_rope();  // none is
          if (!probing) probe_rep = s, probe_exit = rope;
        }
        return lane_descend();
      },
      [&](int32_t slot, const LbvhPoint &p) {
        arrive(~slot);
        if (a.core_sorted[slot] && slot != own_slot) {
          point_tests++;
          if (knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z)) <= a.eps) {
            if (probe_rep >= 0) return found();
            f(slot);
          }
        }
        return lane_rope();
      });
}

// The counted neighbour walk: adds to `cnt` the points within eps of q over the subtree `from` .. `until`, the subtree `skip`
// stepped over (lane_walk); it ends at stop_at neighbours (every call starts below that).  `own_slot`: q's sorted slot, or -1
// for a q that is not in the tree.  The rope is fetched WITH the node, not after the box test has asked for it.
__device__ __forceinline__ void db_count_from(const DbArgs &a, const LbvhPoint &q, int32_t own_slot, int32_t clean_end, int32_t stop_at, int32_t from,
                                              int32_t until, int32_t skip, int32_t skip_rope, int32_t &cnt, uint32_t &node_tests, uint32_t &point_tests) {
  const float r = a.eps_wide;
  auto on = [&]() { return cnt < stop_at ? lane_rope() : lane_stop(); };
  lane_walk<LaneRope::kWithNode>(a.bvh, from, until, skip, skip_rope,
      [&](int32_t at, const LbvhNode &nd, int32_t) {
        node_tests++;
        if (!lane_box_hit(nd, q, r)) return lane_rope();
        // a node inside the sphere is counted, not walked
        float far2, near2;
        lane_box_dist2(nd, q, far2, near2);
        const int32_t first = lbvh_first(at, nd.other), last = lbvh_last(at, nd.other);
        // (a node that holds my own slot while a subtree is being stepped over is an ANCESTOR of that subtree -- the subtree
        // itself is stepped over before it gets here, its descendants are never reached --: its points were counted in part
        // already, so it is walked, not added whole)
        const bool over_skipped = skip != LBVH_END && first <= own_slot && own_slot <= last;
        if (far2 <= a.eps_in2 && last < clean_end && !over_skipped) {
          cnt += last - first + 1;
          return on();
        }
        return lane_descend();
      },
      [&](int32_t, const LbvhPoint &p) {
        point_tests++;
        if (knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z)) <= a.eps) cnt++;
        return on();
      });
}

}  // namespace
}  // namespace owlmi
