// radius_knn.hip -- at most k nearest points within a radius, for query points that are NOT in the tree (tknnRadiusKnn,
// include/owlknn.h).
//
// Row j is the row tknnRadiusQuery gives q_j at its radius r_j with sort = 1 -- the points p of the built set with
// knn_sqrt(knn_dist2(..)) <= r_j, ascending in (fp32 distance, index) --, without the point d_skip_ids names, cut after k entries
// and padded with (-1, +inf) to k.  One pass over the tree: the list's gate starts at r_j instead of infinity and shrinks as the
// list fills, so a row costs the walk at r_j or the walk of a k-nearest query, whichever is less.
//   1. query_order (query_order.h): the queries along the tree's own curve, as the other query calls order them;
//   2. radius_knn_walk_kernel<NREG>: persistent, one 16-lane team per query, four teams per wave, walk_tree (team_walk.h) with
//      radius_query.hip's box of half-width r * (1 + 1e-6); the lanes of a team test the 16 points of a leaf block with the sphere
//      predicate, the survivors wait in the team's LDS buffer and are merged sixteen at a time into the sorted register list
//      (t_merge_rows, team_lanes.h) -- query_walk_kernel's loop (trueknn_query.hip) with a single level;
//   3. radius_knn_lane_kernel<K>: one query per lane on the rope walk (lane_walk.h) with knn_device.h's list, for the queries
//      whose team stack overflowed (a redo list whose length lives on the device) and for trees too small for a box pyramid.
// Both kernels write the same rows: (distance, index) order is total, the sphere predicate is the literal one in both, and the
// gates only ever drop what cannot be among a row's first k.
#include "knn_thresholds.h"  // knn_gate_from_worst
#include "lane_walk.h"
#include "query_order.h"
#include "radius_knn_walk.h"
#include "team_lanes.h"
#include "team_walk.h"
#include "trueknn_engine.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kRknnBlock = 64;        // one wave per workgroup, four teams
constexpr int kRknnBlocksPerCu = 16;  // 7.3 KB of LDS each
constexpr int kRknnLaneBlock = 256;

// ---- a query's radius, gate and skipped point ----------------------------------------------------------------------------------
struct RknnQuery {
  LbvhPoint q;
  float r;       // the sphere predicate's radius
  float r_wide;  // r * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts (radius_query.hip)
  float gate_r;  // the squared-distance gate of an empty list: every d2 whose rounded root can be <= r passes
  int32_t skip;  // the point left out of the row (no point has a negative id)
  bool valid;    // a finite positive radius, or a zero one where the call takes it (a row without one is empty)
};
__device__ __forceinline__ RknnQuery rknn_query(const RadiusKnnKernelArgs &a, int32_t qi, bool has_q) {
  RknnQuery s;
  s.q.x = a.queries[3 * (int64_t)qi], s.q.y = a.queries[3 * (int64_t)qi + 1], s.q.z = a.queries[3 * (int64_t)qi + 2];
  s.q.id = -1;
  s.r = a.radii ? (has_q ? a.radii[qi] : 0.f) : a.radius;
  s.skip = a.skip_ids && has_q ? a.skip_ids[qi] : -1;
  s.valid = (s.r > 0.f || (a.zero_radius_ok && s.r == 0.f)) && s.r <= FLT_MAX;  // (NaN: neither)
  s.r_wide = s.r * 1.000001f;
  s.gate_r = knn_gate_from_worst(s.r);
  return s;
}
// ---- 2. the walk -------------------------------------------------------------------------------------------------------------
// The box rule.  A child box that overlaps the query's box is declined if its near corner lies beyond the list's gate tau2:
// near2 * 0.999995 > tau2 (beyond_gate, the margin lane_counts_subtree keeps).  The margin's direction: near2 is at most every
// point's squared distance up to the roundings of both, a few 1e-7 relative; shrinking it by 5e-6 before the compare can only
// keep a box the exact rule would decline, so the rule can only walk more.  No box is ever taken "inside" without reading its
// points: unlike a count, every entry needs its distance.
// The leaf test.  Lane tl takes point tl of the block: d2 = knn_dist2, and where some lane's d2 passes the gate, d = knn_sqrt(d2)
// and the literal d <= r decide (the gate passes every d2 whose root can be <= r, so it drops nothing the literal test accepts).
// The gate.  tau2 starts at knn_gate_from_worst(r); after each merge that leaves k entries it is the smaller of that and
// knn_gate_from_worst(k-th distance).  Teams of a wave loop in lock step: no __syncthreads, only t_wave_sync.
template <int NREG>
__global__ void __launch_bounds__(kRknnBlock) __attribute__((amdgpu_waves_per_eu(4))) radius_knn_walk_kernel(RadiusKnnKernelArgs a) {
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[LBVH_WIDE_LEVELS];
  __shared__ unsigned long long cand_mem[4 * kCandCapacity];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  unsigned long long *my_cand = cand_mem + team * kCandCapacity;
  walk_fill_levels<1>(levels, &a.wide, lane);
  t_wave_sync();
  const LbvhWideView &wv = a.wide;
  unsigned long long node_tests = 0, point_tests = 0, total = 0, full_rows = 0, tightened = 0;
  for (;;) {
    int got = 0;
    if (lane == 0) got = (int)atomicAdd(&a.ws[kRknnWsCursor], 4ull);
    const int base = __builtin_amdgcn_readfirstlane(got);
    if (base >= a.m) break;
    const bool has_q = base + team < a.m;
    const int32_t qi = has_q ? (a.order ? (int32_t)a.order[base + team] : base + team) : 0;
    const RknnQuery s = rknn_query(a, qi, has_q);
    const LbvhPoint &q = s.q;
    const bool active = has_q && s.valid && !a.force_redo;
    const WalkBox qb(q, s.r_wide);
    uint32_t bd[NREG], bi[NREG];  // register j of lane t holds list entry 16 j + t
#pragma unroll
    for (int j = 0; j < NREG; j++) {
      bd[j] = 0x7f7fffffu;  // KNN_EMPTY_KEY = {FLT_MAX, 0}
      bi[j] = 0u;
    }
    float tau2 = s.gate_r;
    uint32_t left_out = 0xffffffffu;  // (not tracked: a row's ties are ordered by index, nothing is looked up afterwards)
    uint32_t fill_n = 0;
    auto merge_buffer = [&]() __attribute__((always_inline)) {
      t_wave_sync();
      t_merge_rows<NREG>(bd, bi, left_out, false, my_cand, fill_n, tl);
      t_wave_sync();
      fill_n = 0;
      tau2 = rknn_gate(s.gate_r, rknn_kth_dist<NREG>(bd, a.k, team));
    };
    bool overflow = wv.levels <= 0;
    if (wv.levels > 0)
      walk_tree<false>(
          levels, wv, stack, kWalkStack, active, q, qb, team, tl, node_tests,
          [&](const LbvhBox &bx, int32_t, int) { return !beyond_gate(box_min_dist2(bx, q), tau2); },
          [&](int32_t b, bool has_b) {
            LbvhPoint p = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
            if (has_b) p = a.bvh.points[(int64_t)b * LBVH_BLOCK + tl];
            point_tests += has_b ? 1u : 0u;
            const float d2 = knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z);
            const bool near = has_b && d2 <= tau2 && p.id != s.skip;  // (a NaN on either side: not a neighbour)
            if (__ballot(near) == 0ull) return;
            const unsigned long long pm = __ballot(near && knn_sqrt(d2) <= s.r);
            if (pm) {
              const uint32_t mine16 = (uint32_t)(pm >> (team << 4)) & 0xffffu;  // my team's lanes with a candidate
              if ((mine16 >> tl) & 1u) my_cand[fill_n + __popc(mine16 & ((1u << tl) - 1u))] = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)p.id;
              fill_n += __popc(mine16);
              if (__ballot(fill_n >= 16u) != 0ull) merge_buffer();
            }
          },
          [&]() {  // a tighter gate for what comes next as soon as a handful of candidates wait
            if (__ballot(fill_n >= (uint32_t)TKNN_MERGE_AT) != 0ull) merge_buffer();
          }, overflow);
    if (__ballot(fill_n > 0u) != 0ull) merge_buffer();
    // ---- the row: k entries, sixteen lanes at a time (64 contiguous bytes per array), the tail padded ----
    const bool redo = has_q && (overflow || a.force_redo);  // left to the lane kernel, which starts the row again
    const bool write = has_q && !redo;
    const int32_t row = write && a.out_row ? a.out_row[qi] : qi;
    uint32_t cnt = 0;
#pragma unroll
    for (int reg = 0; reg < NREG; reg++) {
      const int j = tl + 16 * reg;
      const bool real = j < a.k && !(bd[reg] == 0x7f7fffffu && bi[reg] == 0u);
      cnt += __popc((uint32_t)(__ballot(real) >> (team << 4)) & 0xffffu);
      if (write && j < a.k) {
        const int64_t o = (int64_t)row * a.k + j;
        a.out_idx[o] = real ? (int32_t)bi[reg] : -1;
        if (a.out_dist) a.out_dist[o] = real ? __uint_as_float(bd[reg]) : INFINITY;
      }
    }
    if (tl == 0 && redo) a.redo[atomicAdd(&a.ws[kRknnWsRedo], 1ull)] = qi;
    const float kth = rknn_kth_dist<NREG>(bd, a.k, team);
    if (tl == 0 && write) {
      if (a.out_counts) a.out_counts[row] = (int32_t)cnt;
      total += cnt;
      full_rows += cnt == (uint32_t)a.k ? 1u : 0u;
      tightened += cnt == (uint32_t)a.k && kth < s.r ? 1u : 0u;
    }
  }
  rknn_add_stats(a.ws, lane, total, full_rows, node_tests, point_tests, tightened);
}

// ---- 3. one query per lane: the queries of the redo list ---------------------------------------------------------------------------
// The same predicate, the same gate (a node whose near corner lies beyond it is stepped over through its rope), a sorted list of
// (distance, index) keys in registers: K >= k entries, of which the first k are the row.
template <int K>
__global__ void __launch_bounds__(kRknnLaneBlock) radius_knn_lane_kernel(RadiusKnnKernelArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kRknnLaneBlock + threadIdx.x;
  const bool has_q = t < (int64_t)a.ws[kRknnWsRedo];
  const int32_t qi = has_q ? a.redo[t] : 0;
  const RknnQuery s = rknn_query(a, qi, has_q);
  const LbvhPoint &q = s.q;
  KList<K> list;
  list.clear();
  float gate = s.gate_r;
  unsigned long long node_tests = 0, point_tests = 0;
  if (has_q && s.valid)
    lane_walk<LaneRope::kWithNode>(a.bvh,
        [&](int32_t, const LbvhNode &nd, int32_t) {
          node_tests++;
          if (!lane_box_hit(nd, q, s.r_wide)) return lane_rope();
          float far2, near2;
          lane_box_dist2(nd, q, far2, near2);
          return near2 * 0.999995f > gate ? lane_rope() : lane_descend();
        },
        [&](int32_t, const LbvhPoint &p) {
          point_tests++;
          const float d = knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z));
          if (d <= s.r && p.id != s.skip) {
            list.insert(knn_key(d, p.id));
            uint64_t kth = list.key[0];  // entry k - 1
#pragma unroll
            for (int j = 1; j < K; j++) kth = j == a.k - 1 ? list.key[j] : kth;
            gate = rknn_gate(s.gate_r, knn_key_dist(kth));
          }
          return lane_rope();
        });
  uint32_t cnt = 0;
  bool tightened = false;
  if (has_q) {
    const int32_t row = a.out_row ? a.out_row[qi] : qi;
    const int64_t base = (int64_t)row * a.k;
    uint64_t kth = list.key[0];  // entry k - 1
#pragma unroll
    for (int j = 1; j < K; j++) kth = j == a.k - 1 ? list.key[j] : kth;
#pragma unroll
    for (int j = 0; j < K; j++)
      if (j < a.k) {
        const bool real = list.key[j] != KNN_EMPTY_KEY;
        a.out_idx[base + j] = knn_key_prim(list.key[j]);
        if (a.out_dist) a.out_dist[base + j] = real ? knn_key_dist(list.key[j]) : INFINITY;
        cnt += real ? 1u : 0u;
      }
    if (a.out_counts) a.out_counts[row] = (int32_t)cnt;
    tightened = cnt == (uint32_t)a.k && knn_key_dist(kth) < s.r;
  }
  // (all lanes of the wave are here)
  rknn_add_stats(a.ws, threadIdx.x & 63, cnt, has_q && cnt == (uint32_t)a.k ? 1u : 0u, node_tests, point_tests, tightened ? 1u : 0u);
}

using RknnWalkEntry = void (*)(RadiusKnnKernelArgs);
const RknnWalkEntry kRknnWalks[4] = {radius_knn_walk_kernel<1>, radius_knn_walk_kernel<2>, radius_knn_walk_kernel<3>, radius_knn_walk_kernel<4>};

}  // namespace

// the walk, then the lane kernel for what the walk left
unsigned long long radius_knn_walks(const RadiusKnnKernelArgs &a, int cu_count, unsigned long long *h_words, hipStream_t s) {
  const int blocks = (int)std::min<int64_t>(((int64_t)a.m + 3) / 4, (int64_t)cu_count * kRknnBlocksPerCu);
  void *kargs[] = {(void *)&a};
  OWLMI_HIP(hipLaunchKernel((const void *)kRknnWalks[query_nreg(a.k) - 1], dim3(blocks), dim3(kRknnBlock), kargs, 0, s));
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kRknnWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));  // the call's one host sync before its last: the redo list's length
  const unsigned long long n_redo = h_words[kRknnWsRedo];
  if (n_redo) {
    const unsigned lane_blocks = (unsigned)((n_redo + kRknnLaneBlock - 1) / kRknnLaneBlock);
    ListCapacities::dispatch(list_capacity_for(a.k), [&](auto cap) {
      hipLaunchKernelGGL(radius_knn_lane_kernel<decltype(cap)::value>, dim3(lane_blocks), dim3(kRknnLaneBlock), 0, s, a);
    });
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kRknnWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  }
  return n_redo;
}

void Engine::radius_knn(const tknnRadiusKnnOptions &o, tknnRadiusKnnInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  // the call's workspace: counters | codes, order (+ the sort's second halves) | lane list | sort space
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t sort_bytes = query_order_sort_bytes(m, s);
  const size_t words_b = align(kRknnWsWords * sizeof(unsigned long long)), col_b = align((size_t)m * sizeof(uint32_t));
  char *ws = (char *)workspace(words_b + 5 * col_b + align(sort_bytes));
  unsigned long long *d_words = (unsigned long long *)ws;
  uint32_t *codes = (uint32_t *)(ws + words_b), *codes_alt = (uint32_t *)(ws + words_b + col_b), *order_in = (uint32_t *)(ws + words_b + 2 * col_b),
           *order = (uint32_t *)(ws + words_b + 3 * col_b);
  int32_t *redo = (int32_t *)(ws + words_b + 4 * col_b);
  void *sort_tmp = ws + words_b + 5 * col_b;

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
  a.redo = redo;
  a.ws = d_words;

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(d_words, 0, kRknnWsWords * sizeof(unsigned long long), s));
  query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, sort_tmp, sort_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  unsigned long long *h_words = h_counters_;
  const unsigned long long n_redo = radius_knn_walks(a, cu_count_, h_words, s);
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->total = (int64_t)h_words[kRknnWsTotal];
    info->full_rows = (int64_t)h_words[kRknnWsFullRows];
    info->node_tests = (int64_t)h_words[kRknnWsNodeTests];
    info->point_tests = (int64_t)h_words[kRknnWsPointTests];
    info->lane_rows = (int64_t)n_redo;
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_c_));
    OWLMI_HIP(hipEventElapsedTime(&info->order_ms, ev_a_, ev_b_));
    OWLMI_HIP(hipEventElapsedTime(&info->walk_ms, ev_b_, ev_c_));
  }
}

}  // namespace owlmi
