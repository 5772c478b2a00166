// radius_knn_walk.h -- the one walk, seed and lane kernel of the four calls that return at most k nearest points within a radius
// per row: tknnRadiusKnn (radius_knn.hip), tknnKnn (knn_seed.hip), tknnPeriodicKnn (periodic_knn.hip), tknnBatchKnn (batch_knn.hip),
// and the host steps they share.  A call differs from the next in its RULE, a struct of static device functions next to its
// argument block Args and its per-query record Query (point q, radius r, query-box half-width r_wide, empty-list gate gate_r,
// skipped id skip, output row, valid):
//   item_at(a, pos)                      the item worked on at sorted position pos (a query index, or a sorted slot)
//   point(a, item, has_q, s)             fills what the seed pass needs of s: point, skipped id, row (and the batch's range)
//   query(a, item, has_q)                the whole record
//   keep_box(a, s, box, c, lvl, tau2)    may child c at pyramid level lvl hold a point within the gate tau2?
//   dist2(a, s, p)                       the squared distance of point p
//   slot_ok(s, slot)                     may the point at this sorted slot enter the row at all?
//   lane_node(a, s, ref, node, gate)     the lane walk at a node: its rope or its left child
//   seed_range(a, s, pos, has_q, clean_blocks, blk_lo, blk_hi, slot)   the blocks a query's seeds may come from, and its slot
//   seed_store(a, s, item, bound)        keeps the seed bound
// The Euclidean rule is in two halves, since tknnKnn's seed pass has an argument block of its own: walk and lane hooks in
// radius_knn.hip (where the kernels of tknnRadiusKnn and tknnKnn are instantiated, once), seed hooks in knn_seed.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <type_traits>

#include "knn_thresholds.h"  // knn_gate_from_worst
#include "lane_walk.h"
#include "owl/lbvh_device.h"
#include "team_lanes.h"  // t_lane_read, t_wave_sum, t_merge_rows
#include "team_walk.h"
#include "trueknn_engine.h"

namespace owlmi {

// words of a call's own counters (in the workspace, zeroed per call)
enum {
  kRknnWsCursor = 0,
  kRknnWsRedo = 1,
  kRknnWsTotal = 2,
  kRknnWsFullRows = 3,
  kRknnWsNodeTests = 4,
  kRknnWsPointTests = 5,
  kRknnWsTightened = 6,  // full rows whose k-th distance ended below their radius
  kRknnWsSeedTests = 7,  // the seed kernel's point tests
  kRknnWsWords = 8
};

constexpr int kRknnBlock = 64;            // walk and seed: one wave per workgroup, four teams
constexpr int kRknnBlocksPerCu = 16;      // walk: 7.3 KB of LDS each
constexpr int kRknnSeedBlocksPerCu = 32;  // seed: 1 KB of LDS each
constexpr int kRknnLaneBlock = 256;       // lane and slot passes

struct RadiusKnnKernelArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const float *queries;     // m packed triples, by query index
  const uint32_t *order;    // m: the query worked on at sorted position i (null: query i)
  int32_t m;
  int k;
  float radius;             // every row's radius if radii is null
  const float *radii;       // m, by query index (may be null)
  const int32_t *skip_ids;  // m, by query index (may be null)
  const int32_t *out_row;   // m: the row of the output a query's answer goes to (null: the query's own index)
  int force_redo;           // TKNN_RADIUS_KNN_FORCE_FALLBACK / TKNN_KNN_FORCE_FALLBACK (tests): the walk leaves every query to the lane kernel
  int zero_radius_ok;       // a radius of 0 is a row's radius like any other (tknnKnn: k duplicates of the query); else such a row is empty
  int32_t *out_idx;         // m*k
  float *out_dist;          // m*k (may be null)
  int32_t *out_counts;      // m (may be null)
  int32_t *redo;            // m: queries left to the lane kernel
  unsigned long long *ws;   // kRknnWsWords counters
};

// radius_knn.hip: rknn_walks with the Euclidean rule, for tknnRadiusKnn with the caller's radii and for tknnKnn with the bounds
// its seed kernel found.
unsigned long long radius_knn_walks(const RadiusKnnKernelArgs &a, int cu_count, unsigned long long *h_words, hipStream_t s);

// knn_seed.hip: rknn_slot_kernel over m queries in sorted order -- a query's place among the tree's n sorted keys, or, with
// query_batch (labels by query index), starts, num_batches and key_bits, inside its batch's range of them.
void rknn_slots(const float *queries, const uint32_t *order, int32_t m, const float *scene, int curve, const uint64_t *keys, int32_t n, int32_t *slots,
                hipStream_t s, const int32_t *query_batch = nullptr, const int32_t *starts = nullptr, int32_t num_batches = 0, int key_bits = 0);

// ---- the host steps ----------------------------------------------------------------------------------------------------------------
// A call's workspace: counters | `columns` columns of m words | sort space, each part aligned to 256 bytes.
struct RknnWorkspace {
  static size_t align(size_t b) { return (b + 255) & ~(size_t)255; }
  RknnWorkspace(int64_t m, int columns, size_t sort_bytes)
      : words_b(align(kRknnWsWords * sizeof(unsigned long long))), col_b(align((size_t)m * sizeof(uint32_t))), bytes(words_b + columns * col_b + align(sort_bytes)) {}
  unsigned long long *words() const { return (unsigned long long *)base; }
  template <class T>
  T *column(int c) const { return (T *)(base + words_b + (size_t)c * col_b); }  // (column `columns`: the sort space)
  const size_t words_b, col_b, bytes;
  char *base = nullptr;  // `bytes` of device memory
};

// The info record from the counters as read back, the redo list's length and the call's events; tknnRadiusKnnInfo has no seed
// pass (seeded is ordered there).
template <class Info>
void rknn_fill_info(Info *info, const unsigned long long *h_words, unsigned long long n_redo, hipEvent_t start, hipEvent_t ordered, hipEvent_t seeded,
                    hipEvent_t done) {
  if (!info) return;
  info->total = (int64_t)h_words[kRknnWsTotal];
  info->full_rows = (int64_t)h_words[kRknnWsFullRows];
  info->node_tests = (int64_t)h_words[kRknnWsNodeTests];
  info->point_tests = (int64_t)h_words[kRknnWsPointTests];
  info->lane_rows = (int64_t)n_redo;
  OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, start, done));
  OWLMI_HIP(hipEventElapsedTime(&info->order_ms, start, ordered));
  OWLMI_HIP(hipEventElapsedTime(&info->walk_ms, seeded, done));
  if constexpr (!std::is_same<Info, tknnRadiusKnnInfo>::value) {
    info->seed_point_tests = (int64_t)h_words[kRknnWsSeedTests];
    info->tightened_rows = (int64_t)h_words[kRknnWsTightened];
    OWLMI_HIP(hipEventElapsedTime(&info->seed_ms, ordered, seeded));
  }
}

namespace {

// The gate of a list whose k-th entry lies at distance `kth` (FLT_MAX: fewer than k entries, the gate stays the radius's).  A
// candidate beyond it is farther than r or farther than the k-th entry; one AT the k-th distance passes, the index decides.
__device__ __forceinline__ float rknn_gate(float gate_r, float kth) { return fminf(gate_r, knn_gate_from_worst(kth)); }

__device__ __forceinline__ void rknn_add_stats(unsigned long long *ws, int lane, unsigned long long total, unsigned long long full_rows,
                                               unsigned long long node_tests, unsigned long long point_tests, unsigned long long tightened) {
  const unsigned long long tsum = t_wave_sum(total), fsum = t_wave_sum(full_rows), nt = t_wave_sum(node_tests), pt = t_wave_sum(point_tests),
                           tight = t_wave_sum(tightened);
  if (lane == 0) {
    if (tsum) atomicAdd(&ws[kRknnWsTotal], tsum);
    if (fsum) atomicAdd(&ws[kRknnWsFullRows], fsum);
    if (nt) atomicAdd(&ws[kRknnWsNodeTests], nt);
    if (pt) atomicAdd(&ws[kRknnWsPointTests], pt);
    if (tight) atomicAdd(&ws[kRknnWsTightened], tight);
  }
}

// t_kth_dist (team_walk.h) with the register picked by masks instead of a chain of selects: the compiler turns that chain into a load
// through a selected address, which keeps registers 1 .. NREG - 1 of the list in scratch (16 / 32 bytes for NREG = 3 / 4 in
// query_walk_kernel); picked this way the list stays in registers for every NREG.
template <int NREG>
__device__ __forceinline__ float rknn_kth_dist(const uint32_t (&bd)[NREG], int k, int team) {
  const uint32_t sel = (uint32_t)(k - 1) >> 4;
  uint32_t reg = 0u;
#pragma unroll
  for (int j = 0; j < NREG; j++) reg |= bd[j] & (0u - (uint32_t)(sel == (uint32_t)j));
  return __uint_as_float(t_lane_read(reg, (team << 4) + ((k - 1) & 15)));
}

// ---- the seed bound --------------------------------------------------------------------------------------------------------------
// The tree's points are sorted along a space-filling curve, so the blocks of 16 around a query's slot are real points close to it.
// One 16-lane team per query, four teams per wave; the team reads a window of ceil(k / 16) + 1 blocks around the slot's block,
// clipped to the blocks [blk_lo, blk_hi) the rule names (seed_range), a 16-byte load per lane and block.  Lane tl takes point tl
// of a block: a seed is a point the row could list -- its slot allowed by the rule, d2 finite (a NaN point, a sentinel or a NaN
// query make it NaN), not the skipped point.  Seeds wait in the team's LDS buffer as (d2, id) and are merged sixteen at a time into
// the sorted register list (t_merge_rows, team_lanes.h), as the walk's candidates are.  The k-th smallest of the seeds' distances
// is an upper bound of the row's k-th, whatever the place on the curve is worth: the row's entries are the k smallest distances of
// ALL eligible points, of which the seeds are a subset.  With fewer than k seeds the bound is FLT_MAX.  The loop runs the same
// number of times for every team of a launch, so the teams of a wave stay in lock step: no __syncthreads, only t_wave_sync.
template <int NREG, class Rule>
__global__ void __launch_bounds__(kRknnBlock) rknn_seed_kernel(typename Rule::Args a) {
  __shared__ unsigned long long cand_mem[4 * kCandCapacity];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  unsigned long long *my_cand = cand_mem + team * kCandCapacity;
  const int32_t clean_blocks = __builtin_amdgcn_readfirstlane((a.bvh.n - *a.bvh.nan_count + LBVH_BLOCK - 1) / LBVH_BLOCK);  // blocks with a point that has no NaN
  const int32_t window = (a.k + LBVH_BLOCK - 1) / LBVH_BLOCK + 1;
  unsigned long long seed_tests = 0;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < (int64_t)a.m; base += (int64_t)gridDim.x * 4) {
    const int32_t pos = (int32_t)(base + team);
    const bool has_q = pos < a.m;
    const int32_t item = has_q ? Rule::item_at(a, pos) : 0;
    typename Rule::Query s;
    Rule::point(a, item, has_q, s);
    int32_t blk_lo, blk_hi, slot;
    Rule::seed_range(a, s, pos, has_q, clean_blocks, blk_lo, blk_hi, slot);
    const int32_t mine = has_q ? min(window, blk_hi - blk_lo) : 0;  // 0: nothing to seed from
    // the window's first block: the slot's block in the middle, clipped at both ends of the range
    const int32_t first = max(blk_lo, min((slot >> 4) - (mine - 1) / 2, blk_hi - mine));
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
      const bool has_b = w < mine;
      const int32_t at = (first + w) * LBVH_BLOCK + tl;  // my slot
      LbvhPoint p = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
      if (has_b) p = a.bvh.points[(int64_t)(first + w) * LBVH_BLOCK + tl];
      seed_tests += has_b ? 1u : 0u;
      const float d2 = Rule::dist2(a, s, p);
      const bool seed = has_b && Rule::slot_ok(s, at) && d2 <= FLT_MAX && p.id != s.skip;  // (NaN: not a seed)
      const uint32_t mine16 = (uint32_t)(__ballot(seed) >> (team << 4)) & 0xffffu;
      if (seed) my_cand[fill_n + __popc(mine16 & ((1u << tl) - 1u))] = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)p.id;
      fill_n += __popc(mine16);
      if (__ballot(fill_n >= 16u) != 0ull) merge_buffer();
    }
    if (__ballot(fill_n > 0u) != 0ull) merge_buffer();
    // the list holds rounded roots (t_sorted_row); an empty entry k - 1 is FLT_MAX: fewer than k seeds
    const float bound = fminf(rknn_kth_dist<NREG>(bd, a.k, team), FLT_MAX);
    if (has_q && tl == 0) Rule::seed_store(a, s, item, bound);
  }
  const unsigned long long st = t_wave_sum(seed_tests);
  if (lane == 0 && st) atomicAdd(&a.ws[kRknnWsSeedTests], st);
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
// Persistent, one 16-lane team per query, four teams per wave; a cursor hands out groups of four sorted positions.  walk_tree
// (team_walk.h) with the query's box of half-width r_wide -- query_walk_kernel's loop (trueknn_query.hip) with a single level.
// The box rule (keep_box).  A child box that overlaps the query's box is declined if the rule's lower bound of the distance to
// its points lies beyond the list's gate tau2: bound * 0.999995 > tau2 (beyond_gate, the margin lane_counts_subtree keeps).  The
// margin's direction: the bound is at most every point's squared distance up to the roundings of both, a few 1e-7 relative;
// shrinking it by 5e-6 before the compare can only keep a box the exact rule would decline, so the rule can only walk more.  No
// box is ever taken "inside" without reading its points: unlike a count, every entry needs its distance.
// The leaf test.  Lane tl takes point tl of the block: d2 = dist2, and where some lane's d2 passes the gate, d = knn_sqrt(d2) and
// the literal d <= r decide (the gate passes every d2 whose root can be <= r, so it drops nothing the literal test accepts).  The
// survivors wait in the team's LDS buffer and are merged sixteen at a time into the sorted register list (t_merge_rows).
// The gate.  tau2 starts at knn_gate_from_worst(r); after each merge that leaves k entries it is the smaller of that and
// knn_gate_from_worst(k-th distance).  Teams of a wave loop in lock step: no __syncthreads, only t_wave_sync.
template <int NREG, class Rule>
__global__ void __launch_bounds__(kRknnBlock) __attribute__((amdgpu_waves_per_eu(4))) rknn_walk_kernel(typename Rule::Args a) {
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
    const int32_t item = has_q ? Rule::item_at(a, base + team) : 0;
    const typename Rule::Query s = Rule::query(a, item, has_q);
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
          [&](const LbvhBox &bx, int32_t c, int lvl) { return Rule::keep_box(a, s, bx, c, lvl, tau2); },
          [&](int32_t b, bool has_b) {
            LbvhPoint p = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
            if (has_b) p = a.bvh.points[(int64_t)b * LBVH_BLOCK + tl];
            point_tests += has_b ? 1u : 0u;
            const float d2 = Rule::dist2(a, s, p);
            const bool near = has_b && Rule::slot_ok(s, b * LBVH_BLOCK + tl) && d2 <= tau2 && p.id != s.skip;  // (a NaN on either side: not a neighbour)
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

// ---- one query per lane: the items of the redo list -------------------------------------------------------------------------------
// For the queries whose team stack overflowed, for trees too small for a box pyramid, and for every query under the call's
// TKNN_*_FORCE_FALLBACK=1.  The rope walk (lane_walk.h) with the same predicate and the same gate (lane_node steps over a node
// whose box lies beyond it through its rope), a sorted list of (distance, index) keys in registers (knn_device.h): K >= k entries,
// of which the first k are the row.  Walk and lane kernel write the same rows: (distance, index) order is total, the predicate is
// the literal knn_sqrt(d2) <= r in both, and the gates only ever drop what cannot be among a row's first k.
template <int K, class Rule>
__global__ void __launch_bounds__(kRknnLaneBlock) rknn_lane_kernel(typename Rule::Args a) {
  const int64_t t = (int64_t)blockIdx.x * kRknnLaneBlock + threadIdx.x;
  const bool has_q = t < (int64_t)a.ws[kRknnWsRedo];
  const int32_t item = has_q ? a.redo[t] : 0;
  const typename Rule::Query s = Rule::query(a, item, has_q);
  KList<K> list;
  list.clear();
  float gate = s.gate_r;
  unsigned long long node_tests = 0, point_tests = 0;
  if (has_q && s.valid)
    lane_walk<LaneRope::kWithNode>(a.bvh,
        [&](int32_t ref, const LbvhNode &nd, int32_t) {
          node_tests++;
          return Rule::lane_node(a, s, ref, nd, gate);
        },
        [&](int32_t slot, const LbvhPoint &p) {
          point_tests++;
          const float d = knn_sqrt(Rule::dist2(a, s, p));
          if (Rule::slot_ok(s, slot) && d <= s.r && p.id != s.skip) {
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

// the open-space lane_node: the query's box, then the gate on the node's near corner
__device__ __forceinline__ LaneStep rknn_lane_box(const LbvhNode &nd, const LbvhPoint &q, float r_wide, float gate) {
  if (!lane_box_hit(nd, q, r_wide)) return lane_rope();
  float far2, near2;
  lane_box_dist2(nd, q, far2, near2);
  return near2 * 0.999995f > gate ? lane_rope() : lane_descend();
}

// ---- the launches ------------------------------------------------------------------------------------------------------------------
template <class Rule>
void rknn_seed(const typename Rule::Args &a, int cu_count, hipStream_t s) {
  using Entry = void (*)(typename Rule::Args);
  const Entry seeds[4] = {rknn_seed_kernel<1, Rule>, rknn_seed_kernel<2, Rule>, rknn_seed_kernel<3, Rule>, rknn_seed_kernel<4, Rule>};
  const int blocks = (int)std::min<int64_t>(((int64_t)a.m + 3) / 4, (int64_t)cu_count * kRknnSeedBlocksPerCu);
  void *kargs[] = {(void *)&a};
  OWLMI_HIP(hipLaunchKernel((const void *)seeds[query_nreg(a.k) - 1], dim3(blocks), dim3(kRknnBlock), kargs, 0, s));
  OWLMI_HIP(hipGetLastError());
}

// The walk over the m items of `a`, then the lane kernel over what the walk left; one host sync before the caller's last -- the
// redo list's length, which is returned.  h_words: kRknnWsWords words of pinned host memory, the counters as they stand once the
// stream has been synchronised again.
template <class Rule>
unsigned long long rknn_walks(const typename Rule::Args &a, int cu_count, unsigned long long *h_words, hipStream_t s) {
  using Entry = void (*)(typename Rule::Args);
  const Entry walks[4] = {rknn_walk_kernel<1, Rule>, rknn_walk_kernel<2, Rule>, rknn_walk_kernel<3, Rule>, rknn_walk_kernel<4, Rule>};
  const int blocks = (int)std::min<int64_t>(((int64_t)a.m + 3) / 4, (int64_t)cu_count * kRknnBlocksPerCu);
  void *kargs[] = {(void *)&a};
  OWLMI_HIP(hipLaunchKernel((const void *)walks[query_nreg(a.k) - 1], dim3(blocks), dim3(kRknnBlock), kargs, 0, s));
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kRknnWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));  // the call's one host sync before its last: the redo list's length
  const unsigned long long n_redo = h_words[kRknnWsRedo];
  if (n_redo) {
    const unsigned lane_blocks = (unsigned)((n_redo + kRknnLaneBlock - 1) / kRknnLaneBlock);
    ListCapacities::dispatch(list_capacity_for(a.k), [&](auto cap) {
      hipLaunchKernelGGL((rknn_lane_kernel<decltype(cap)::value, Rule>), dim3(lane_blocks), dim3(kRknnLaneBlock), 0, s, a);
    });
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kRknnWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  }
  return n_redo;
}

}  // namespace

}  // namespace owlmi
