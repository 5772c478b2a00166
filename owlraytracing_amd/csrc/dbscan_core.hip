// dbscan_core.hip -- RT-DBSCAN, what is known before any union: the core flags, next_core (the first core slot at or after each
// slot), the core flags a caller's labels decide, and the noise probe of the growth rounds.  dbscan.hip has the algorithm and
// the map of the files.
#include "db_call.h"

namespace owlmi {
namespace {

// Core flags.  Every point first looks at its GROUP, the first tight node on its own root path (db_group_kernel): its
// points are pairwise within eps, so if it holds minPts of them the point is core without looking any further.  (Listing the
// points that do have to look and walking for them with full waves, as the label pass does, was tried: on BASELINE config 3
// they are a fifth of all points, a full wave waits for the longest of 64 walks instead of the longest of a dozen, and the
// pass took 2.2 ms instead of 1.45.)
__device__ __forceinline__ void db_core_body(const DbArgs &a, int32_t t, uint32_t &node_tests, uint32_t &point_tests) {
  const LbvhView &bvh = a.bvh;
  if (a.parent) a.parent[t] = t;
  if (a.keep_core && a.core_sorted[t]) return;
  const LbvhPoint q = bvh.points[t];
  int32_t cnt = 0;
  const int stop_at = a.want_counts ? 0x7fffffff : a.min_pts;
  const int32_t clean_end = lane_clean_end(bvh);
  int32_t ref = bvh.root;
  // the last nodes above my group on my root path (anc[0]: kNear levels above it).  A point whose group is too small to
  // decide looks for its minPts neighbours there FIRST: they are next to it, a walk from the root spends two dozen steps
  // getting near (BASELINE config 3: a fifth of the points walk, nearly all of them core, 0.9 of the pass's 1.4 ms).
  constexpr int kNear = 4;
  static_assert(kNear == LBVH_PATH_WORDS - 1, "the block paths hold the ring's ancestors");
  int32_t anc[kNear];
#pragma unroll
  for (int j = 0; j < kNear; j++) anc[j] = bvh.root;
  if (!a.want_counts || a.group_of) {
    int32_t node = bvh.root, first = t;
    if (a.block_paths) {
      // Not from the root: from the deepest node that holds the wave's 64 slots (a table of the tree, LBVH_PATH_BLOCK), with
      // that node's four nearest ancestors in the ring -- if it is not tight none of its ancestors is (a parent's box holds
      // the child's), and the walk from the root would have come through here with exactly this ring (config 3: 16 of a
      // point's 23 steps).  If it is tight, the group is that node or one of the ancestors: the highest tight one among the
      // four the table has -- unless the fourth is tight too, then the walk starts at the root after all.
      const int32_t *bp = a.block_paths + (size_t)(t / LBVH_PATH_BLOCK) * LBVH_PATH_WORDS;
      const int32_t a4 = bp[0], a3 = bp[1], a2 = bp[2], a1 = bp[3], lca = bp[4];
      if (!node_is_tight(bvh.nodes[lca], a.eps_in2)) {
        node = lca;
        anc[0] = a4, anc[1] = a3, anc[2] = a2, anc[3] = a1;
      } else {
        const bool t1 = node_is_tight(bvh.nodes[a1], a.eps_in2), t2 = node_is_tight(bvh.nodes[a2], a.eps_in2),
                   t3 = node_is_tight(bvh.nodes[a3], a.eps_in2), t4 = node_is_tight(bvh.nodes[a4], a.eps_in2);
        node_tests += 4;
        if (!t4) node = t3 ? a3 : t2 ? a2 : t1 ? a1 : lca;  // (the ring stays at the root: no subtree to count in first)
      }
      node_tests++;
    }
    if (TKNN_DIAG_BUILD && (a.diag & 128)) node = -1;  // (times only) no descent to the group
    while (node >= 0) {
      const LbvhNode nd = bvh.nodes[node];
      node_tests++;
      if (node_is_tight(nd, a.eps_in2)) {
        first = lbvh_first(node, nd.other);
        const int32_t last = lbvh_last(node, nd.other);
        if (!a.want_counts && last < clean_end && last - first + 1 >= a.min_pts) {
          cnt = last - first + 1;
          ref = LBVH_END;
        }
        break;
      }
#pragma unroll
      for (int j = 0; j + 1 < kNear; j++) anc[j] = anc[j + 1];
      anc[kNear - 1] = node;
      node = t <= nd.split ? lbvh_left_ref(node, nd) : lbvh_right_ref(node, nd);
    }
    // the group's first slot keeps the group's reference (a node, or ~t for a point by itself), the others ~first
    if (a.group_of) a.group_of[t] = t == first ? (node >= 0 ? node : ~t) : ~first;
    if (a.near_node) a.near_node[t] = anc[0];
  }
  if (TKNN_DIAG_BUILD && (a.diag & 64)) ref = LBVH_END;  // (times only) no neighbour count
  auto count_from = [&](int32_t from, int32_t until, int32_t skip, int32_t skip_rope) {
    db_count_from(a, q, t, clean_end, stop_at, from, until, skip, skip_rope, cnt, node_tests, point_tests);
  };
  if (ref != LBVH_END) {
    const int32_t near = anc[0];
    if (!a.want_counts && near != bvh.root && near >= 0) {
      // enough neighbours in the subtree around me: core, whatever else the sphere holds.  Not enough: the count goes on
      // over the rest of the tree (the walk from the root steps over that subtree).
      const int32_t near_rope = bvh.rope_node[near];
      count_from(near, near_rope, LBVH_END, LBVH_END);
      if (cnt < a.min_pts) count_from(bvh.root, LBVH_END, near, near_rope);  // the rest of the tree
    } else {
      count_from(bvh.root, LBVH_END, LBVH_END, LBVH_END);
    }
  }
  const uint8_t is_core = cnt >= a.min_pts;
  a.core_sorted[t] = is_core;
  // results are indexed by ROW (the point's position in the caller's buffer, prim_id of the sorted
  // slot), not by the id an engine built with tknnBuildIds reports; the union-find by sorted slot
  const int32_t row = bvh.prim_id[t];
  if (a.core && !(TKNN_DIAG_BUILD && (a.diag & 256))) a.core[row] = is_core;
  if (a.counts) a.counts[row] = cnt;
}

// (`block_count`, or null: the workgroup's number of core slots, which the kernels behind this one place their lists by --
// a launch of its own over all the flags otherwise, db_flag_count_kernel)
__global__ void __launch_bounds__(kDbBlock) db_core_kernel(DbArgs a, int32_t *block_count) {
  __shared__ unsigned long long blk_stats[2];
  __shared__ int32_t wave_count[kDbBlock / 64];
  if (threadIdx.x < 2) blk_stats[threadIdx.x] = 0ull;
  __syncthreads();
  uint32_t node_tests = 0, point_tests = 0;
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  if (t < a.bvh.n) db_core_body(a, t, node_tests, point_tests);
  if (block_count) {  // (a lane reads the flag it has just written)
    const unsigned long long m = __ballot(t < a.bvh.n && a.core_sorted[t] != 0);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(m);
  }
  db_add_stats(a.stats + kDbStatCore, blk_stats, node_tests, point_tests);  // (a barrier inside)
  if (block_count && threadIdx.x == 0) {
    int32_t total = 0;
    for (int w = 0; w < kDbBlock / 64; w++) total += wave_count[w];
    block_count[blockIdx.x] = total;
  }
}

// next_core[s] = first core slot >= s (n if none): with rank[s] = number of core slots before s and pos[r] = slot of the
// r-th core point, next_core[s] = pos[rank[s]].  No rank per slot is kept (a library sum over the n flags took 0.05 ms and a
// 40 MB array was written once and read twice): a count of the core flags per workgroup of 256 slots (db_core_kernel, or
// db_flag_count_kernel), a sum over those n / 256 counts, and the two kernels below find a slot's rank as its workgroup's place
// + the core slots before it in the workgroup.
// (and, if asked: the slots that are NOT core, listed in slot order for the label pass -- slot t is the (t - rank[t])-th of
// them, no atomics -- with their number)
__device__ __forceinline__ int32_t db_rank_in_block(bool flag, int32_t block_place, int32_t *wave_count, int32_t &block_total) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_count[wave] = __popcll(m);
  __syncthreads();
  int32_t r = block_place;
  block_total = 0;
  for (int w = 0; w < kDbBlock / 64; w++) {
    if (w < wave) r += wave_count[w];
    block_total += wave_count[w];
  }
  return r + __popcll(m & ((1ull << lane) - 1ull));
}
__global__ void __launch_bounds__(kDbBlock) db_flag_count_kernel(DbArgs a, int32_t *block_count) {
  __shared__ int32_t wave_count[kDbBlock / 64];
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  int32_t total;
  (void)db_rank_in_block(t < a.bvh.n && a.core_sorted[t] != 0, 0, wave_count, total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}
__global__ void __launch_bounds__(kDbBlock) db_core_pos_blocks_kernel(DbArgs a, const int32_t *block_place, int32_t *pos, int32_t *others,
                                                                      unsigned long long *n_others) {
  __shared__ int32_t wave_count[kDbBlock / 64];
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  const bool in = t < a.bvh.n, is_core = in && a.core_sorted[t] != 0;
  int32_t total;
  const int32_t r = db_rank_in_block(is_core, block_place[blockIdx.x], wave_count, total);
  if (!in) return;
  if (is_core)
    pos[r] = t;
  else if (others)
    others[t - r] = t;
  if (t == a.bvh.n - 1) {
    const int32_t n_core = r + (is_core ? 1 : 0);
    pos[n_core] = 0x7f7f7f7f;  // "none" (clamped below): the one place a slot behind the last core point looks at
    if (others) *n_others = (unsigned long long)(a.bvh.n - n_core);
  }
}
__global__ void __launch_bounds__(kDbBlock) db_next_core_blocks_kernel(DbArgs a, const int32_t *block_place, const int32_t *pos, int32_t *next_core) {
  __shared__ int32_t wave_count[kDbBlock / 64];
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  const bool in = t < a.bvh.n;
  int32_t total;
  const int32_t r = db_rank_in_block(in && a.core_sorted[t] != 0, block_place[blockIdx.x], wave_count, total);
  if (!in) return;
  const int32_t v = pos[r];  // a slot after the last core point has rank = number of core points: pos[] holds "none" there
  next_core[t] = v < a.bvh.n ? v : a.bvh.n;
  if (t == a.bvh.n - 1) next_core[a.bvh.n] = a.bvh.n;
}

// tknnDbscanAssign, tknnDbscanQuery: the caller has decided the label of every core point (>= 0; < 0: not core)
__global__ void __launch_bounds__(kDbBlock) db_core_from_labels_kernel(DbArgs a, const int32_t *core_label) {
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  if (t < a.bvh.n) a.core_sorted[t] = core_label[a.bvh.prim_id[t]] >= 0;
}

// ---- "eps auto-grown" (tknnDbscanAuto; spec: oracle/dbscan_oracle.c, dbref_dbscan_auto) ----------------------------
// A round of the growth loop only has to COUNT the noise points: is there a core point within eps of a point that is
// not core itself?  One traversal with an early exit; a subtree without a core point (next_core) is skipped, a node
// wholly inside the sphere that holds one settles the question.  Points found not to be noise never are again (a core
// point stays core as eps grows), so later rounds probe the remaining noise only.
__device__ __forceinline__ bool db_has_core_neighbour(const DbArgs &a, const LbvhPoint &q, int32_t from, int32_t until, int32_t skip,
                                                      int32_t skip_rope, uint32_t &node_tests, uint32_t &point_tests) {
  const LbvhView &bvh = a.bvh;
  const float r = a.eps_wide;
  // (the rope with the node: half the chain of dependent loads; the walk stops at the first core neighbour)
  return lane_walk<LaneRope::kWithNode>(bvh, from, until, skip, skip_rope,
      [&](int32_t ref, const LbvhNode &nd, int32_t) {
        node_tests++;
        // out of reach, or no core point below
        if (!lane_box_hit(nd, q, r) || a.next_core[lbvh_first(ref, nd.other)] > lbvh_last(ref, nd.other)) return lane_rope();
        float far2, near2;
        lane_box_dist2(nd, q, far2, near2);
        if (far2 <= a.eps_in2) return lane_stop();  // all of it within eps, and a core point among it
        return near2 > a.eps_out2 ? lane_rope() : lane_descend();
      },
      [&](int32_t slot, const LbvhPoint &p) {
        if (a.core_sorted[slot]) {
          point_tests++;
          if (knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z)) <= a.eps) return lane_stop();
        }
        return lane_rope();
      });
}
// ... first in the subtree a few levels above the point's own group (the core-flag kernel has left its root in near_node): a
// point that is not noise has its core neighbour next to it, and a walk from the root spends two dozen steps getting there
__device__ __forceinline__ bool db_has_core_neighbour(const DbArgs &a, const LbvhPoint &q, int32_t t, uint32_t &node_tests, uint32_t &point_tests) {
  const LbvhView &bvh = a.bvh;
  const int32_t near = a.near_node ? a.near_node[t] : bvh.root;
  if (near < 0 || near == bvh.root) return db_has_core_neighbour(a, q, bvh.root, LBVH_END, LBVH_END, LBVH_END, node_tests, point_tests);
  const int32_t near_rope = bvh.rope_node[near];
  if (db_has_core_neighbour(a, q, near, near_rope, LBVH_END, LBVH_END, node_tests, point_tests)) return true;
  return db_has_core_neighbour(a, q, bvh.root, LBVH_END, near, near_rope, node_tests, point_tests);  // the rest of the tree
}

// noise[slot] (per sorted slot): in, unless first_round: 1 = was noise in the round before; out: 1 = is noise now.
// stats: kDbStatCore += node / point tests, kDbStatNoise += points still noise.
__global__ void __launch_bounds__(kDbBlock) db_noise_probe_kernel(DbArgs a, uint8_t *noise, int first_round) {
  __shared__ unsigned long long blk_stats[2], blk_noise[2];
  if (threadIdx.x < 2) blk_stats[threadIdx.x] = blk_noise[threadIdx.x] = 0ull;
  __syncthreads();
  uint32_t node_tests = 0, point_tests = 0, still = 0;
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  if (t < a.bvh.n) {
    if (a.core_sorted[t]) {
      noise[t] = 0;
    } else if (first_round || noise[t]) {
      still = db_has_core_neighbour(a, a.bvh.points[t], t, node_tests, point_tests) ? 0u : 1u;
      noise[t] = (uint8_t)still;
    }
  }
  db_add_stats(a.stats + kDbStatCore, blk_stats, node_tests, point_tests);
  db_add_stats(a.stats + kDbStatNoise, blk_noise, still, 0u);
}

}  // namespace

// next_core from a.core_sorted: the core slots of each workgroup (block_places, counted by db_core_kernel; `count`: by a
// launch of its own) -> their exclusive sum -> slot of the r-th core point (pos: where a.rank goes later) -> first core
// slot at or after each slot; and, if asked, the list of the slots that are not core with its length in counters_[kDbNotCore]
void Engine::DbCall::build_next_core(bool count, int32_t *not_core) {
  int32_t *pos = a.rank;
  if (count) hipLaunchKernelGGL(db_flag_count_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, block_places);
  exclusive_sum(block_places, block_places + blocks, (int)blocks);
  hipLaunchKernelGGL(db_core_pos_blocks_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, block_places + blocks, pos, not_core, e.counters_ + kDbNotCore);
  hipLaunchKernelGGL(db_next_core_blocks_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, block_places + blocks, pos, next_core);
}

// a growth round: core flags (with a.keep_core, those of the rounds before stand), next_core, the noise probe of
// every point that is not core (later rounds: of those that still were noise), the statistics read back.  Returns the
// number of noise points; `noise` is per slot.
int64_t Engine::DbCall::probe_round(float eps, bool first_round) {
  set_eps(eps);
  reset_counters();
  hipLaunchKernelGGL(db_core_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, block_places);
  build_next_core(false, nullptr);
  hipLaunchKernelGGL(db_noise_probe_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, noise, first_round ? 1 : 0);
  OWLMI_HIP(hipGetLastError());
  e.db_read_stats(s);
  return (int64_t)e.h_counters_[kDbStatNoise];
}

void Engine::DbCall::core_flags() {
  // the flags BY ROW are written by the label kernel, which scatters to the rows anyway: a one-byte store at the
  // caller's row from this kernel cost a partial sector per point (rocprofv3: 426 MB written for 10 M points)
  DbArgs c = a;
  c.core = nullptr;
  hipLaunchKernelGGL(db_core_kernel, dim3(blocks), dim3(kDbBlock), 0, s, c, block_places);
  OWLMI_HIP(hipEventRecord(e.ev_c_, s));  // end of the core-flag traversal
}

// tknnDbscanAssign, tknnDbscanQuery: the caller's labels decide the core flags
void Engine::DbCall::core_from_labels(const int32_t *core_label) {
  hipLaunchKernelGGL(db_core_from_labels_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, core_label);
}
}  // namespace owlmi
