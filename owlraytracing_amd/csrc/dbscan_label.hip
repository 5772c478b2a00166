// dbscan_label.hip -- RT-DBSCAN from "the roots are final" to the caller's rows: roots and cluster numbers, the walks of the
// points that are not core, labels by slot and by row, the assignment to given labels (tknnDbscanAssign, tknnDbscanQuery),
// and tknnSegmentMin.  dbscan.hip has the algorithm and the map of the files.
#include "db_call.h"

namespace owlmi {
namespace {

// min_row[root] = min(min_row[root], row).  The value only falls, so a read that finds it at or below `row` settles the matter
// without an atomic: a cluster of millions of points would otherwise queue an atomic per wave on ONE address (50 M 2-D
// points, one giant cluster: 6 ms for the pass; with the read first, a handful of atomics get through).
__device__ __forceinline__ void db_min_row(int32_t *cell, int32_t row) {
  if (__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > row) atomicMin(cell, row);
}

// after the unions: every core slot points at its root, and the root learns the smallest ROW of its cluster -- clusters are
// numbered by that (the spec: ascending smallest core index).  A wave's slots mostly share one root: one atomic per wave
// and root, not per point.
// Four consecutive slots per thread, their words fetched as one 16-byte load per array: a thread with one slot has one
// 4-byte load in flight per step of its chain (flag -> parent -> parent's parent -> row), and half a million such threads on
// the device do not fill the memory system (0.15 ms for 0.2 GB).
__global__ void __launch_bounds__(kDbBlock) db_flatten_kernel(DbArgs a, int32_t *zero) {
  const int32_t n = a.bvh.n;
  const long long t0 = ((long long)blockIdx.x * kDbBlock + threadIdx.x) * kDbPer;
  int32_t par[kDbPer], prim[kDbPer];
  bool core[kDbPer];
  if (t0 + kDbPer <= n) {
    const int4 p4 = *reinterpret_cast<const int4 *>(a.parent + t0), r4 = *reinterpret_cast<const int4 *>(a.bvh.prim_id + t0);
    const uchar4 c4 = *reinterpret_cast<const uchar4 *>(a.core_sorted + t0);
    par[0] = p4.x, par[1] = p4.y, par[2] = p4.z, par[3] = p4.w;
    prim[0] = r4.x, prim[1] = r4.y, prim[2] = r4.z, prim[3] = r4.w;
    core[0] = c4.x != 0, core[1] = c4.y != 0, core[2] = c4.z != 0, core[3] = c4.w != 0;
#pragma unroll
    for (int k = 0; k < kDbPer; k++) zero[t0 + k] = 0;  // the root flags of the next launch (the group list lived here; its place is 16-byte aligned only if n is a multiple of four)
  } else {
#pragma unroll
    for (int k = 0; k < kDbPer; k++) {
      const bool in = t0 + k < n;
      const long long t = in ? t0 + k : 0;
      par[k] = a.parent[t], prim[k] = a.bvh.prim_id[t], core[k] = in && a.core_sorted[t] != 0;
      if (in) zero[t] = 0;
    }
  }
  // (plain loads and stores: the unions are over -- what this launch reads is final or, where another lane's store below has
  // or has not arrived, a root or an older ancestor in the same tree: the walk ends at the root either way)
  int32_t up[kDbPer], root[kDbPer];
#pragma unroll
  for (int k = 0; k < kDbPer; k++) up[k] = a.parent[core[k] ? par[k] : 0];
#pragma unroll
  for (int k = 0; k < kDbPer; k++) {
    root[k] = par[k];
    if (core[k] && up[k] != par[k]) {
      int32_t x = up[k], p = a.parent[x];
      while (p != x) x = p, p = a.parent[x];
      root[k] = x;
    }
    if (core[k] && root[k] != par[k]) a.parent[t0 + k] = root[k];
  }
  // the thread's slots of its first core slot's root as one (root, smallest row); the others (a boundary between clusters
  // inside four slots) send their own
  int32_t my_root = -1, row = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < kDbPer; k++) {
    if (!core[k]) continue;
    if (my_root < 0) my_root = root[k];
    if (root[k] == my_root)
      row = min(row, prim[k]);
    else
      db_min_row(a.min_row + root[k], prim[k]);
  }
  const int lane = threadIdx.x & 63;
  // the wave's two most common cases first -- one root for all its slots, or two -- as one atomic each; slots of further
  // roots (sparse regions: many small clusters per wave, hardly two slots on one address) send their own
  bool pending = my_root >= 0;
  for (int round = 0; round < 2; round++) {
    const unsigned long long todo = __ballot(pending);
    if (!todo) break;
    const int j = __ffsll((long long)todo) - 1;
    const int32_t r_j = __shfl(my_root, j);
    const bool same = pending && my_root == r_j;
    int32_t m = same ? row : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off));
    if (lane == j) db_min_row(a.min_row + r_j, m);
    pending = pending && !same;
  }
  if (pending) db_min_row(a.min_row + my_root, row);
}
// roots flag their cluster's smallest row; an exclusive scan over the rows then numbers the clusters
__global__ void __launch_bounds__(kDbBlock) db_root_kernel(DbArgs a, int32_t *is_first_row) {
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  if (t < a.bvh.n && a.core_sorted[t] && a.parent[t] == t) is_first_row[a.min_row[t]] = 1;
}

// The points that are not core (few -- BASELINE config 3: 0.13 % --, scattered over the waves, listed in slot order since the
// core flags were known: db_core_pos_blocks_kernel) take the lowest-numbered cluster among their core neighbours.  Finding those
// neighbours needs the core flags only, not the clusters: the walks -- chains of dependent loads by a few hundred waves, 0.25 ms
// on config 3 -- run BESIDE the group unions on a stream of their own and leave, per listed point, the core neighbours they met
// (one per tight node, db for_each_core_group; a point that is not core has fewer than minPts - 1 of them: `per` - 1 places, and
// a count of -1 if that should ever not be enough).  Lists that would not fit the room (`capacity` words; a set that is mostly
// noise) are not written: the label kernel then walks itself, as it does for a count of -1.
__global__ void __launch_bounds__(kDbBlock) db_border_walk_kernel(DbArgs a, const int32_t *pending, const unsigned long long *n_pending, int32_t *lists,
                                                                  int per, long long capacity) {
  __shared__ unsigned long long blk_stats[2];
  if (threadIdx.x < 2) blk_stats[threadIdx.x] = 0ull;
  __syncthreads();
  uint32_t node_tests = 0, point_tests = 0;
  const long long total = (long long)*n_pending;
  if (total * per <= capacity) {
    for (long long i = (long long)blockIdx.x * kDbBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kDbBlock) {
      const LbvhPoint q = a.bvh.points[pending[i]];
      int32_t *mine = lists + i * per;
      int32_t cnt = 0;
      for_each_core_group(
          a, q, -1, [](int32_t) { return false; },
          [&](int32_t other) {
            if (cnt < per - 1) mine[1 + cnt] = other;
            cnt++;
          },
          node_tests, point_tests);
      mine[0] = cnt <= per - 1 ? cnt : -1;
    }
  }
  db_add_stats(a.stats + kDbStatLabel, blk_stats, node_tests, point_tests);
}

// Labels: core points take their cluster's number (and every point's core flag goes to its row); the listed points take the
// smallest number among the core neighbours db_border_walk_kernel has left them (or walk now).  ONE launch: the first
// `walk_blocks` workgroups serve the list (grid-stride), the rest stream -- two scattered stores per point.
// `by_slot` (or null): the labels stay BY SLOT -- a core slot's number (>= 0; four consecutive slots one 16-byte store), a
// listed slot's -1 (noise) or -3 - label (border) -- and db_rows_from_slots_kernel carries them to the caller's rows through the
// tree's inverse permutation with coalesced stores.  The scatter wrote a partial sector per point and array: rocprofv3 counted
// 648 MB written for 50 MB of output at BASELINE config 3.
__global__ void __launch_bounds__(kDbBlock) db_label_kernel(DbArgs a, const int32_t *pending, const unsigned long long *n_pending, int walk_blocks,
                                                            const int32_t *lists, int per, long long capacity, int32_t *by_slot) {
  __shared__ unsigned long long blk_stats[2];
  if (threadIdx.x < 2) blk_stats[threadIdx.x] = 0ull;
  __syncthreads();
  uint32_t node_tests = 0, point_tests = 0;
  if ((int)blockIdx.x >= walk_blocks) {
    // four consecutive slots per thread (db_flatten_kernel: 16-byte loads, four chains in flight); a core slot's parent IS its
    // root since that kernel
    const int32_t n = a.bvh.n;
    const long long t0 = ((long long)(blockIdx.x - walk_blocks) * kDbBlock + threadIdx.x) * kDbPer;
    int32_t row[kDbPer], root[kDbPer];
    bool in[kDbPer], core[kDbPer];
    if (t0 + kDbPer <= n) {
      const int4 p4 = *reinterpret_cast<const int4 *>(a.parent + t0), r4 = *reinterpret_cast<const int4 *>(a.bvh.prim_id + t0);
      const uchar4 c4 = *reinterpret_cast<const uchar4 *>(a.core_sorted + t0);
      root[0] = p4.x, root[1] = p4.y, root[2] = p4.z, root[3] = p4.w;
      row[0] = r4.x, row[1] = r4.y, row[2] = r4.z, row[3] = r4.w;
      core[0] = c4.x != 0, core[1] = c4.y != 0, core[2] = c4.z != 0, core[3] = c4.w != 0;
      in[0] = in[1] = in[2] = in[3] = true;
    } else {
#pragma unroll
      for (int k = 0; k < kDbPer; k++) {
        in[k] = t0 + k < n;
        const long long t = in[k] ? t0 + k : 0;
        root[k] = a.parent[t], row[k] = a.bvh.prim_id[t], core[k] = in[k] && a.core_sorted[t] != 0;
      }
    }
    int32_t first_row[kDbPer], number[kDbPer];
#pragma unroll
    for (int k = 0; k < kDbPer; k++) first_row[k] = a.min_row[core[k] ? root[k] : 0];
#pragma unroll
    for (int k = 0; k < kDbPer; k++) number[k] = a.rank[core[k] ? first_row[k] : 0];
    if (by_slot) {
      // (a slot that is not core belongs to the list part of this launch: not touched here)
      if (t0 + kDbPer <= n && core[0] && core[1] && core[2] && core[3]) {
        *reinterpret_cast<int4 *>(by_slot + t0) = make_int4(number[0], number[1], number[2], number[3]);
      } else {
#pragma unroll
        for (int k = 0; k < kDbPer; k++)
          if (in[k] && core[k]) by_slot[t0 + k] = number[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < kDbPer; k++) {
        if (!in[k]) continue;
        if (a.core) a.core[row[k]] = core[k];
        if (core[k]) a.labels[row[k]] = number[k];
      }
    }
  } else {
    const long long total = (long long)*n_pending;
    const bool listed = lists != nullptr && total * per <= capacity;
    for (long long i = (long long)blockIdx.x * kDbBlock + threadIdx.x; i < total; i += (long long)walk_blocks * kDbBlock) {
      const int32_t t = pending[i];
      int32_t first_row = -1;  // of my cluster: the smallest over the clusters of my core neighbours (the lowest label)
      auto take = [&](int32_t other) {
        const int32_t m = a.min_row[uf_find(a.parent, other)];
        if (first_row < 0 || m < first_row) first_row = m;
      };
      const int32_t cnt = listed ? lists[i * per] : -1;
      if (cnt >= 0) {
        for (int32_t j = 0; j < cnt; j++) take(lists[i * per + 1 + j]);
      } else {
        const LbvhPoint q = a.bvh.points[t];
        for_each_core_group(a, q, -1, [](int32_t) { return false; }, take, node_tests, point_tests);
      }
      const int32_t label = first_row < 0 ? -1 : a.rank[first_row];
      if (by_slot)
        by_slot[t] = label < 0 ? -1 : -3 - label;
      else
        a.labels[a.bvh.prim_id[t]] = label;
    }
  }
  db_add_stats(a.stats + kDbStatLabel, blk_stats, node_tests, point_tests);
}
// rows <- slots: four consecutive ROWS per thread; their slots come from the tree's inverse permutation (one 16-byte load), the
// slots' words are four scattered 4-byte reads of an array the launch before has just written (40 MB at 10 M points: it sits
// in the 256 MB of cache in front of the memory), the rows' labels and core flags leave as one 16-byte and one 4-byte store
__global__ void __launch_bounds__(kDbBlock) db_rows_from_slots_kernel(DbArgs a, const int32_t *row_slot, const int32_t *by_slot) {
  const int32_t n = a.bvh.n;
  const long long r0 = ((long long)blockIdx.x * kDbBlock + threadIdx.x) * kDbPer;
  if (r0 >= n) return;
  int32_t v[kDbPer];
  if (r0 + kDbPer <= n) {
    const int4 s4 = *reinterpret_cast<const int4 *>(row_slot + r0);
    v[0] = by_slot[s4.x], v[1] = by_slot[s4.y], v[2] = by_slot[s4.z], v[3] = by_slot[s4.w];
    int32_t lab[kDbPer];
#pragma unroll
    for (int k = 0; k < kDbPer; k++) lab[k] = v[k] >= -1 ? v[k] : -3 - v[k];
    *reinterpret_cast<int4 *>(a.labels + r0) = make_int4(lab[0], lab[1], lab[2], lab[3]);
    if (a.core) *reinterpret_cast<uchar4 *>(a.core + r0) = make_uchar4(v[0] >= 0, v[1] >= 0, v[2] >= 0, v[3] >= 0);
  } else {
    for (long long r = r0; r < n; r++) {
      const int32_t w = by_slot[row_slot[r]];
      a.labels[r] = w >= -1 ? w : -3 - w;
      if (a.core) a.core[r] = w >= 0;
    }
  }
}

// tknnDbscanAssign: the caller has decided the label of every core point (>= 0; < 0: not core); a
// core point keeps it, any other point takes the smallest label among its core neighbours, or -1
__global__ void __launch_bounds__(kDbBlock) db_assign_kernel(DbArgs a, const int32_t *core_label) {
  __shared__ unsigned long long blk_stats[2];
  if (threadIdx.x < 2) blk_stats[threadIdx.x] = 0ull;
  __syncthreads();
  uint32_t node_tests = 0, point_tests = 0;
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  if (t < a.bvh.n) {
    const LbvhPoint q = a.bvh.points[t];
    const int32_t row = a.bvh.prim_id[t];
    int32_t best = core_label[row];
    if (best < 0) {
      best = -1;
      for_each_core_group(
          a, q, -1, [](int32_t) { return false; },
          [&](int32_t other) {
            const int32_t l = core_label[a.bvh.prim_id[other]];  // a tight node's core points share one label: its first stands for all
            if (best < 0 || l < best) best = l;
          },
          node_tests, point_tests);
    }
    a.labels[row] = best;
  }
  db_add_stats(a.stats + kDbStatLabel, blk_stats, node_tests, point_tests);
}

// tknnDbscanQuery: the same two questions for points that are NOT in the tree.  One query per lane, the lanes of a wave = 64
// queries that follow each other on the tree's curve (query_order.h); results go to the caller's index order[i].  The label:
// the smallest caller-decided label among the core points within eps (for_each_core_group without a slot of its own: nothing is
// "self", a point of the set that coincides with the query is a neighbour at distance 0); a tree without a core point is not
// walked.  The count, if asked for: db_count_from over the whole tree, no early stop.  A query with a NaN coordinate fails every
// box test and every distance test: label -1, count 0.
struct DbQueryArgs {
  const float *queries;   // m packed triples, caller order
  const uint32_t *order;  // m: the query worked on at sorted position i
  int32_t m;
  const int32_t *core_label;  // n, by row
  int32_t *labels;            // m
  int32_t *counts;            // m, or null
};
__global__ void __launch_bounds__(kDbBlock) db_query_kernel(DbArgs a, DbQueryArgs qa) {
  __shared__ unsigned long long blk_stats[2];
  if (threadIdx.x < 2) blk_stats[threadIdx.x] = 0ull;
  __syncthreads();
  uint32_t node_tests = 0, point_tests = 0;
  const int64_t i = (int64_t)blockIdx.x * kDbBlock + threadIdx.x;
  if (i < (int64_t)qa.m) {
    const int64_t j = (int64_t)qa.order[i];
    const LbvhPoint q = {qa.queries[3 * j], qa.queries[3 * j + 1], qa.queries[3 * j + 2], -1};
    int32_t best = -1;
    if (a.next_core[0] < a.bvh.n)
      for_each_core_group(
          a, q, -1, [](int32_t) { return false; },
          [&](int32_t other) {
            const int32_t l = qa.core_label[a.bvh.prim_id[other]];  // a tight node's core points share one label: its first stands for all
            if (best < 0 || l < best) best = l;
          },
          node_tests, point_tests);
    qa.labels[j] = best;
    if (qa.counts) {
      int32_t cnt = 0;
      db_count_from(a, q, -1, lane_clean_end(a.bvh), 0x7fffffff, a.bvh.root, LBVH_END, LBVH_END, LBVH_END, cnt, node_tests, point_tests);
      qa.counts[j] = cnt;
    }
  }
  db_add_stats(a.stats + kDbStatLabel, blk_stats, node_tests, point_tests);
}

// per-slot flags to the caller's rows
__global__ void __launch_bounds__(kDbBlock) db_rows_kernel(DbArgs a, const uint8_t *by_slot, uint8_t *by_row) {
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  if (t < a.bvh.n) by_row[a.bvh.prim_id[t]] = by_slot[t];
}

}  // namespace

// tknnSegmentMin (sharded RT-DBSCAN, owlraytracing_amd/distributed.py): out[seg[i]] = min(out[seg[i]], val[i]) over the
// elements with seg[i] >= 0 -- the smallest global id of every local cluster, the one per-point step of the label propagation
// (everything after it works on clusters and halo rows).  Few segments and ten million elements is the hard case -- a
// scatter-reduce queues its atomics on a few dozen addresses (two ranks, BASELINE config 3: 160 ms of a 174 ms step) --; as in
// db_min_row the value only falls, so an element that reads a smaller or equal one is done, and a wave first settles the two
// segments most of its lanes hold with one atomic each.
__global__ void __launch_bounds__(kDbBlock) db_segment_min_kernel(const int32_t *seg, const long long *val, long long n, long long *out) {
  const long long i = (long long)blockIdx.x * kDbBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t my_seg = -1;
  long long my_val = 0x7fffffffffffffffll;
  if (i < n) {
    my_seg = seg[i];
    if (my_seg >= 0) my_val = val[i];
  }
  bool pending = my_seg >= 0;
  if (pending && __hip_atomic_load(out + my_seg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= my_val) pending = false;
  for (int round = 0; round < 2; round++) {
    const unsigned long long todo = __ballot(pending);
    if (!todo) break;
    const int j = __ffsll((long long)todo) - 1;
    const int32_t s_j = __shfl(my_seg, j);
    const bool same = pending && my_seg == s_j;
    long long m = same ? my_val : 0x7fffffffffffffffll;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const long long o = __shfl_xor(m, off);
      m = o < m ? o : m;
    }
    if (lane == j) atomicMin(out + s_j, m);
    pending = pending && !same;
  }
  if (pending) atomicMin(out + my_seg, my_val);
}
void db_segment_min(const int32_t *d_seg, const int64_t *d_val, int64_t n, int64_t *d_out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(db_segment_min_kernel, dim3((unsigned)((n + kDbBlock - 1) / kDbBlock)), dim3(kDbBlock), 0, s, d_seg, (const long long *)d_val, (long long)n,
                     (long long *)d_out);
  OWLMI_HIP(hipGetLastError());
}

// the walks of the points that are not core, on the side stream beside everything up to the label kernel
void Engine::DbCall::border_walk() {
  if (!side) return;
  OWLMI_HIP(hipEventRecord(e.ev_side_a_, s));
  OWLMI_HIP(hipStreamWaitEvent(e.db_side_, e.ev_side_a_, 0));
  hipLaunchKernelGGL(db_border_walk_kernel, dim3(walk_grid), dim3(kDbBlock), 0, e.db_side_, a, not_core, e.counters_ + kDbNotCore, border_lists, border_per, (long long)n);
  OWLMI_HIP(hipEventRecord(e.ev_side_b_, e.db_side_));
  e.db_side_pending_ = true;  // (until some stream waits for it: labels(), or the top of the next call if this one throws in between)
}
// every core slot to its root, the roots' smallest rows, the clusters numbered by them
void Engine::DbCall::number_clusters() {
  int32_t *is_root = roots;
  hipLaunchKernelGGL(db_flatten_kernel, dim3(blocks_per), dim3(kDbBlock), 0, s, a, is_root);
  hipLaunchKernelGGL(db_root_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, is_root);
  OWLMI_HIP(hipGetLastError());
  exclusive_sum(is_root, a.rank, (int)n);
  // number of clusters = rank[n-1] + is_root[n-1]
  OWLMI_HIP(hipMemcpyAsync(&last[0], a.rank + (n - 1), 4, hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipMemcpyAsync(&last[1], is_root + (n - 1), 4, hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipEventRecord(e.ev_f_, s));
}
// labels by slot first and a gather to the rows (default), or scattered straight to the rows (TKNN_DB_LABEL=scatter: A/B).
// The caller's arrays must allow 16-byte stores for the gather (hipMalloc'd ones do).
void Engine::DbCall::labels() {
  if (side) {  // the border walk's lists
    OWLMI_HIP(hipStreamWaitEvent(s, e.ev_side_b_, 0));
    e.db_side_pending_ = false;
  }
  const int32_t *row_slot = e.bvh_.row_slot_device();
  const bool gather = row_slot && !knobs.scatter && ((uintptr_t)a.labels % 16 == 0) && (!a.core || (uintptr_t)a.core % 4 == 0);
  int32_t *by_slot = gather ? roots : nullptr;  // (the root flags have been summed: their place is free)
  hipLaunchKernelGGL(db_label_kernel, dim3(walk_grid + blocks_per), dim3(kDbBlock), 0, s, a, not_core, e.counters_ + kDbNotCore, (int)walk_grid,
                     side ? border_lists : (const int32_t *)nullptr, border_per, (long long)n, by_slot);
  if (gather) hipLaunchKernelGGL(db_rows_from_slots_kernel, dim3(blocks_per), dim3(kDbBlock), 0, s, a, row_slot, by_slot);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(e.ev_b_, s));
}
// tknnDbscanAssign: a core point keeps the caller's label, any other point takes the smallest among its core neighbours
void Engine::DbCall::assign_labels(const int32_t *core_label) {
  hipLaunchKernelGGL(db_assign_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, core_label);
  OWLMI_HIP(hipGetLastError());
}
// tknnDbscanQuery: one traversal for the labels (and counts) of the m queries, taken in `order`
void Engine::DbCall::query_labels(const float *d_queries, const uint32_t *order, int64_t m, const int32_t *core_label, int32_t *d_labels, int32_t *d_counts) {
  const DbQueryArgs qa = {d_queries, order, (int32_t)m, core_label, d_labels, d_counts};
  hipLaunchKernelGGL(db_query_kernel, dim3((unsigned)((m + kDbBlock - 1) / kDbBlock)), dim3(kDbBlock), 0, s, a, qa);
  OWLMI_HIP(hipGetLastError());
}
// tknnDbscanNoise: the round's noise flags, kept per slot, to the caller's rows
void Engine::DbCall::noise_rows(uint8_t *d_noise) {
  hipLaunchKernelGGL(db_rows_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, noise, d_noise);
  OWLMI_HIP(hipGetLastError());
}
}  // namespace owlmi
