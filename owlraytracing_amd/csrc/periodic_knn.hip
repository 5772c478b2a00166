// periodic_knn.hip -- at most k nearest points in a cell that is periodic along some of its axes, with or without a radius, for
// query points that are not in the tree or for the tree's own points (tknnPeriodicKnn, include/owlknn_periodic.h).
//
// tknnRadiusKnn and tknnKnn with the wrapped distance of periodic_metric.h.  The tree is the open-space one: a periodic metric is
// a matter of the query side.  The walk needs a lower bound of the wrapped distance from the query to a box
// (periodic_box_min_dist2, which looks at the query and its two shifted images per periodic axis) and the leaf test the wrapped
// distance itself (periodic_dist2).  ONE walk covers a query -- there is no loop over images --, so every point is met once and no
// point can enter a row twice, also where the k-th distance exceeds half a period.
//   1. external queries: query_order (query_order.h); without any radius also periodic_slot_kernel, a query's place in the tree's
//      order (knn_seed.hip's search).  The tree's own points are their slots and come in curve order: neither pass.
//   2. without any radius (d_radii == NULL, radius == FLT_MAX): periodic_seed_kernel<NREG>, knn_seed.hip's window around the slot
//      with periodic_dist2.  The seeds are a subset of the eligible points, so their k-th wrapped distance bounds the row's.
//   3. periodic_walk_kernel<NREG>: radius_knn_walk_kernel's loop (radius_knn.hip) -- persistent, a 16-lane team per query,
//      walk_tree (team_walk.h) with an unbounded query box, the LDS candidate buffer and t_merge_rows, the gate from
//      knn_gate_from_worst, the row written sixteen lanes at a time.
//   4. periodic_lane_kernel<K>: one query per lane on the rope walk (lane_walk.h), for the queries whose team stack overflowed,
//      for trees too small for a box pyramid, and for every query under TKNN_PERIODIC_KNN_FORCE_FALLBACK=1 (read per call).
// Both kernels write the same rows: (distance, index) order is total, the predicate is the literal knn_sqrt(d2) <= r in both, and
// the gates only ever drop what cannot be among a row's first k.
#include "curve_key.h"
#include "knn_thresholds.h"  // knn_gate_from_worst
#include "lane_walk.h"
#include "owlknn_periodic.h"
#include "periodic_metric.h"
#include "query_order.h"
#include "radius_knn_walk.h"  // the counter words, rknn_gate, rknn_add_stats, rknn_kth_dist
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

constexpr int kPknnBlock = 64;         // one wave per workgroup, four teams
constexpr int kPknnBlocksPerCu = 16;   // 7.3 KB of LDS each
constexpr int kPknnSeedBlocksPerCu = 32;  // 1 KB of LDS each
constexpr int kPknnLaneBlock = 256;

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

// ---- a query's point, row, radius, gate and skipped point ----------------------------------------------------------------------
struct PknnQuery {
  LbvhPoint q;
  float r;       // the predicate's radius: the caller's, or the seed bound (which may be 0: k duplicates of the query)
  float gate_r;  // the squared-distance gate of an empty list: every d2 whose rounded root can be <= r passes
  int32_t skip;  // the point left out of the row (no point has a negative id)
  int32_t row;   // the caller's j
  bool valid;    // a radius the call takes and a query in the cell without a NaN (a row without: empty)
};
// the point, skipped id and row of an item: the caller's query j, or (the tree's own points) the point of a sorted slot
__device__ __forceinline__ void pknn_point(const PeriodicKnnArgs &a, int32_t item, bool has_q, LbvhPoint &q, int32_t &skip, int32_t &row) {
  q = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
  skip = -1, row = item;
  if (!has_q) return;
  if (a.queries) {
    q.x = a.queries[3 * (int64_t)item], q.y = a.queries[3 * (int64_t)item + 1], q.z = a.queries[3 * (int64_t)item + 2];
    skip = a.skip_ids ? a.skip_ids[item] : -1;
  } else {
    q = a.bvh.points[item];
    skip = q.id;
    row = a.bvh.prim_id[item];
  }
}
__device__ __forceinline__ PknnQuery pknn_query(const PeriodicKnnArgs &a, int32_t item, bool has_q) {
  PknnQuery s;
  pknn_point(a, item, has_q, s.q, s.skip, s.row);
  s.r = !has_q ? 0.f : a.bounds ? a.bounds[item] : a.radii ? a.radii[s.row] : a.radius;
  const bool in_cell = periodic_in_cell(s.q.x, a.cell.lo[0], a.cell.period[0]) & periodic_in_cell(s.q.y, a.cell.lo[1], a.cell.period[1]) &
                       periodic_in_cell(s.q.z, a.cell.lo[2], a.cell.period[2]);
  const bool no_nan = (s.q.x == s.q.x) & (s.q.y == s.q.y) & (s.q.z == s.q.z);
  s.valid = has_q && (s.r > 0.f || (a.bounds && s.r == 0.f)) && s.r <= FLT_MAX && in_cell && no_nan;  // (a NaN radius: neither)
  s.gate_r = knn_gate_from_worst(s.r);
  return s;
}

// ---- 1. a query's place in the tree's order --------------------------------------------------------------------------------------
// knn_slot_kernel's search (knn_seed.hip): the first slot whose 21-level key is not below the query's.
__global__ void __launch_bounds__(kPknnLaneBlock) periodic_slot_kernel(const float *__restrict__ queries, const uint32_t *__restrict__ order, int32_t m,
                                                                       const float *__restrict__ scene, int curve, const uint64_t *__restrict__ keys,
                                                                       int32_t n, int32_t *__restrict__ slots) {
  const int32_t i = blockIdx.x * kPknnLaneBlock + threadIdx.x;
  if (i >= m) return;
  const int64_t qi = order[i];
  const float ext = fmaxf(fmaxf(scene[3] - scene[0], scene[4] - scene[1]), scene[5] - scene[2]);
  const uint64_t key = curve_point_key(curve, queries[3 * qi], queries[3 * qi + 1], queries[3 * qi + 2], scene[0], scene[1], scene[2], ext, 21);
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  slots[i] = lo;
}

// ---- 2. the seed bound -----------------------------------------------------------------------------------------------------------
// knn_seed_kernel's window (knn_seed.hip) with the wrapped distance: lane tl takes point tl of a block of the window; a seed is a
// point the row could list -- d2 finite, not the skipped point --, so the k-th smallest of the seeds' distances is an upper bound
// of the row's k-th, whatever the place on the curve is worth (a query at a face has half of its neighbours elsewhere on the
// curve: that costs a wider walk, nothing else).  With fewer than k seeds the bound is FLT_MAX.  The window is the same number of
// blocks for every query of a launch, so the teams of a wave loop in lock step.
template <int NREG>
__global__ void __launch_bounds__(kPknnBlock) periodic_seed_kernel(PeriodicKnnArgs a) {
  __shared__ unsigned long long cand_mem[4 * kCandCapacity];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  unsigned long long *my_cand = cand_mem + team * kCandCapacity;
  const int32_t n = a.bvh.n;
  const int32_t clean_blocks = __builtin_amdgcn_readfirstlane((n - *a.bvh.nan_count + LBVH_BLOCK - 1) / LBVH_BLOCK);  // blocks with a point that has no NaN
  const int32_t window = min((a.k + LBVH_BLOCK - 1) / LBVH_BLOCK + 1, clean_blocks);
  const bool self = a.queries == nullptr;
  unsigned long long seed_tests = 0;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < (int64_t)a.m; base += (int64_t)gridDim.x * 4) {
    const int64_t pos = base + team;
    const bool has_q = pos < (int64_t)a.m;
    const int32_t item = has_q ? (self ? (int32_t)pos : (int32_t)a.order[pos]) : 0;
    LbvhPoint q;
    int32_t skip, row;
    pknn_point(a, item, has_q, q, skip, row);
    const int32_t slot = has_q ? (self ? (int32_t)pos : a.slots[pos]) : 0;
    // the window's first block: the slot's block in the middle, clipped at both ends of the order
    const int32_t first = max(0, min((min(slot, n - 1) >> 4) - (window - 1) / 2, clean_blocks - window));
    uint32_t bd[NREG], bi[NREG];  // register j of lane t holds list entry 16 j + t
#pragma unroll
    for (int j = 0; j < NREG; j++) {
      bd[j] = 0x7f7fffffu;  // KNN_EMPTY_KEY = {FLT_MAX, 0}
      bi[j] = 0u;
    }
    uint32_t left_out = 0xffffffffu;  // (not tracked)
    uint32_t fill_n = 0;
    auto merge_buffer = [&]() __attribute__((always_inline)) {
      t_wave_sync();
      t_merge_rows<NREG>(bd, bi, left_out, false, my_cand, fill_n, tl);
      t_wave_sync();
      fill_n = 0;
    };
    for (int32_t w = 0; w < window; w++) {
      LbvhPoint p = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
      if (has_q) p = a.bvh.points[(int64_t)(first + w) * LBVH_BLOCK + tl];
      seed_tests += has_q ? 1u : 0u;
      const float d2 = periodic_dist2(p.x, p.y, p.z, q.x, q.y, q.z, a.cell);
      const bool seed = has_q && d2 <= FLT_MAX && p.id != skip;  // (NaN: not a seed)
      const uint32_t mine16 = (uint32_t)(__ballot(seed) >> (team << 4)) & 0xffffu;
      if (seed) my_cand[fill_n + __popc(mine16 & ((1u << tl) - 1u))] = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)p.id;
      fill_n += __popc(mine16);
      if (__ballot(fill_n >= 16u) != 0ull) merge_buffer();
    }
    if (__ballot(fill_n > 0u) != 0ull) merge_buffer();
    // the list holds rounded roots (t_sorted_row); an empty entry k - 1 is FLT_MAX: fewer than k seeds
    const float bound = fminf(rknn_kth_dist<NREG>(bd, a.k, team), FLT_MAX);
    if (has_q && tl == 0) a.bounds[item] = bound;
  }
  const unsigned long long st = t_wave_sum(seed_tests);
  if (lane == 0 && st) atomicAdd(&a.ws[kRknnWsSeedTests], st);
}

// ---- 3. the walk -----------------------------------------------------------------------------------------------------------------
// The box rule.  A child box is declined if the wrapped distance to every in-cell point of it lies beyond the list's gate tau2:
// periodic_box_min_dist2 * 0.999995 > tau2 (beyond_gate).  The bound carries its own absolute slack for the roundings of the
// shifted images (periodic_metric.h); both margins can only keep a box the exact rule would decline.  The query box of walk_tree
// is unbounded (r = FLT_MAX, as tknnKnn's is without a seed): a box across a face is as near as one next door.
// The leaf test.  Lane tl takes point tl of the block: d2 = periodic_dist2, and where some lane's d2 passes the gate,
// d = knn_sqrt(d2) and the literal d <= r decide.  The gate: tau2 starts at knn_gate_from_worst(r); after each merge that leaves k
// entries it is the smaller of that and knn_gate_from_worst(k-th distance).
template <int NREG>
__global__ void __launch_bounds__(kPknnBlock) __attribute__((amdgpu_waves_per_eu(4))) periodic_walk_kernel(PeriodicKnnArgs a) {
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[LBVH_WIDE_LEVELS];
  __shared__ unsigned long long cand_mem[4 * kCandCapacity];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  unsigned long long *my_cand = cand_mem + team * kCandCapacity;
  walk_fill_levels<1>(levels, &a.wide, lane);
  t_wave_sync();
  const LbvhWideView &wv = a.wide;
  const bool self = a.queries == nullptr;
  unsigned long long node_tests = 0, point_tests = 0, total = 0, full_rows = 0, tightened = 0;
  for (;;) {
    int got = 0;
    if (lane == 0) got = (int)atomicAdd(&a.ws[kRknnWsCursor], 4ull);
    const int base = __builtin_amdgcn_readfirstlane(got);
    if (base >= a.m) break;
    const bool has_q = base + team < a.m;
    const int32_t item = has_q ? (self ? base + team : (int32_t)a.order[base + team]) : 0;
    const PknnQuery s = pknn_query(a, item, has_q);
    const LbvhPoint &q = s.q;
    const bool active = s.valid && !a.force_redo;
    const WalkBox qb(q, FLT_MAX);
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
          [&](const LbvhBox &bx, int32_t, int) { return !beyond_gate(periodic_box_min_dist2(bx, q.x, q.y, q.z, a.cell), tau2); },
          [&](int32_t b, bool has_b) {
            LbvhPoint p = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
            if (has_b) p = a.bvh.points[(int64_t)b * LBVH_BLOCK + tl];
            point_tests += has_b ? 1u : 0u;
            const float d2 = periodic_dist2(p.x, p.y, p.z, q.x, q.y, q.z, a.cell);
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
    uint32_t cnt = 0;
#pragma unroll
    for (int reg = 0; reg < NREG; reg++) {
      const int j = tl + 16 * reg;
      const bool real = j < a.k && !(bd[reg] == 0x7f7fffffu && bi[reg] == 0u);
      cnt += __popc((uint32_t)(__ballot(real) >> (team << 4)) & 0xffffu);
      if (write && j < a.k) {
        const int64_t o = (int64_t)s.row * a.k + j;
        a.out_idx[o] = real ? (int32_t)bi[reg] : -1;
        if (a.out_dist) a.out_dist[o] = real ? __uint_as_float(bd[reg]) : INFINITY;
      }
    }
    if (tl == 0 && redo) a.redo[atomicAdd(&a.ws[kRknnWsRedo], 1ull)] = item;
    const float kth = rknn_kth_dist<NREG>(bd, a.k, team);
    if (tl == 0 && write) {
      if (a.out_counts) a.out_counts[s.row] = (int32_t)cnt;
      total += cnt;
      full_rows += cnt == (uint32_t)a.k ? 1u : 0u;
      tightened += cnt == (uint32_t)a.k && kth < s.r ? 1u : 0u;
    }
  }
  rknn_add_stats(a.ws, lane, total, full_rows, node_tests, point_tests, tightened);
}

// ---- 4. one query per lane: the items of the redo list -----------------------------------------------------------------------------
// The same predicate, the same gate (a node whose box lies beyond it is stepped over through its rope), a sorted list of
// (distance, index) keys in registers: K >= k entries, of which the first k are the row.
template <int K>
__global__ void __launch_bounds__(kPknnLaneBlock) periodic_lane_kernel(PeriodicKnnArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kPknnLaneBlock + threadIdx.x;
  const bool has_q = t < (int64_t)a.ws[kRknnWsRedo];
  const int32_t item = has_q ? a.redo[t] : 0;
  const PknnQuery s = pknn_query(a, item, has_q);
  const LbvhPoint &q = s.q;
  KList<K> list;
  list.clear();
  float gate = s.gate_r;
  unsigned long long node_tests = 0, point_tests = 0;
  if (s.valid)
    lane_walk<LaneRope::kWithNode>(a.bvh,
        [&](int32_t, const LbvhNode &nd, int32_t) {
          node_tests++;
          return beyond_gate(periodic_box_min_dist2(nd, q.x, q.y, q.z, a.cell), gate) ? lane_rope() : lane_descend();
        },
        [&](int32_t, const LbvhPoint &p) {
          point_tests++;
          const float d = knn_sqrt(periodic_dist2(p.x, p.y, p.z, q.x, q.y, q.z, a.cell));
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
    const int64_t base = (int64_t)s.row * a.k;
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
    if (a.out_counts) a.out_counts[s.row] = (int32_t)cnt;
    tightened = cnt == (uint32_t)a.k && knn_key_dist(kth) < s.r;
  }
  // (all lanes of the wave are here)
  rknn_add_stats(a.ws, threadIdx.x & 63, cnt, has_q && cnt == (uint32_t)a.k ? 1u : 0u, node_tests, point_tests, tightened ? 1u : 0u);
}

using PknnEntry = void (*)(PeriodicKnnArgs);
const PknnEntry kPknnSeeds[4] = {periodic_seed_kernel<1>, periodic_seed_kernel<2>, periodic_seed_kernel<3>, periodic_seed_kernel<4>};
const PknnEntry kPknnWalks[4] = {periodic_walk_kernel<1>, periodic_walk_kernel<2>, periodic_walk_kernel<3>, periodic_walk_kernel<4>};

}  // namespace

void Engine::periodic_knn(const tknnPeriodicKnnOptions &o, tknnPeriodicKnnInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const bool self = o.d_queries == nullptr;
  const bool seeded = !o.d_radii && o.radius == FLT_MAX;
  // the call's workspace: counters | lane list, bounds | external: codes, order (+ the sort's second halves), sort space
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t sort_bytes = self ? 0 : query_order_sort_bytes(m, s);
  const size_t words_b = align(kRknnWsWords * sizeof(unsigned long long)), col_b = align((size_t)m * sizeof(uint32_t));
  char *ws = (char *)workspace(words_b + 6 * col_b + align(sort_bytes));
  unsigned long long *d_words = (unsigned long long *)ws;
  auto column = [&](int c) { return ws + words_b + (size_t)c * col_b; };
  int32_t *redo = (int32_t *)column(0);
  float *bounds = (float *)column(1);
  uint32_t *codes = (uint32_t *)column(2), *codes_alt = (uint32_t *)column(3), *order_in = (uint32_t *)column(4), *order = (uint32_t *)column(5);
  int32_t *slots = (int32_t *)column(2);  // (over the codes: the sort is through when the slots are written)
  void *sort_tmp = column(6);

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
  a.bounds = seeded ? bounds : nullptr;
  a.skip_ids = o.d_skip_ids;
  if (const char *e = getenv("TKNN_PERIODIC_KNN_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.out_idx = o.d_idx;
  a.out_dist = o.d_dist;
  a.out_counts = o.d_counts;
  a.redo = redo;
  a.ws = d_words;

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(d_words, 0, kRknnWsWords * sizeof(unsigned long long), s));
  if (!self) query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, sort_tmp, sort_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  if (seeded) {
    if (!self) {
      hipLaunchKernelGGL(periodic_slot_kernel, dim3((unsigned)((m + kPknnLaneBlock - 1) / kPknnLaneBlock)), dim3(kPknnLaneBlock), 0, s, o.d_queries,
                         (const uint32_t *)order, (int32_t)m, bvh_.scene_device(), bvh_.curve(), bvh_.keys_device(), a.bvh.n, slots);
      OWLMI_HIP(hipGetLastError());
    }
    const int blocks = (int)std::min<int64_t>((m + 3) / 4, (int64_t)cu_count_ * kPknnSeedBlocksPerCu);
    void *kargs[] = {(void *)&a};
    OWLMI_HIP(hipLaunchKernel((const void *)kPknnSeeds[query_nreg(o.k) - 1], dim3(blocks), dim3(kPknnBlock), kargs, 0, s));
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  // the walk, then the lane kernel for what the walk left
  unsigned long long *h_words = h_counters_;
  {
    const int blocks = (int)std::min<int64_t>((m + 3) / 4, (int64_t)cu_count_ * kPknnBlocksPerCu);
    void *kargs[] = {(void *)&a};
    OWLMI_HIP(hipLaunchKernel((const void *)kPknnWalks[query_nreg(o.k) - 1], dim3(blocks), dim3(kPknnBlock), kargs, 0, s));
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipMemcpyAsync(h_words, d_words, kRknnWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));  // the call's one host sync before its last: the redo list's length
  const unsigned long long n_redo = h_words[kRknnWsRedo];
  if (n_redo) {
    const unsigned lane_blocks = (unsigned)((n_redo + kPknnLaneBlock - 1) / kPknnLaneBlock);
    ListCapacities::dispatch(list_capacity_for(o.k), [&](auto cap) {
      hipLaunchKernelGGL(periodic_lane_kernel<decltype(cap)::value>, dim3(lane_blocks), dim3(kPknnLaneBlock), 0, s, a);
    });
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipMemcpyAsync(h_words, d_words, kRknnWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  }
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->total = (int64_t)h_words[kRknnWsTotal];
    info->full_rows = (int64_t)h_words[kRknnWsFullRows];
    info->node_tests = (int64_t)h_words[kRknnWsNodeTests];
    info->point_tests = (int64_t)h_words[kRknnWsPointTests];
    info->seed_point_tests = (int64_t)h_words[kRknnWsSeedTests];
    info->tightened_rows = (int64_t)h_words[kRknnWsTightened];
    info->lane_rows = (int64_t)n_redo;
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_d_));
    OWLMI_HIP(hipEventElapsedTime(&info->order_ms, ev_a_, ev_b_));
    OWLMI_HIP(hipEventElapsedTime(&info->seed_ms, ev_b_, ev_c_));
    OWLMI_HIP(hipEventElapsedTime(&info->walk_ms, ev_c_, ev_d_));
  }
}

}  // namespace owlmi
