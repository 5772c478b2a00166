// batch_knn.hip -- many labelled point clouds in one tree (tknnBuildBatched) and at most k nearest points inside the query's own
// cloud, with or without a radius, for labelled query points that are not in the tree or for the tree's own points (tknnBatchKnn,
// include/owlknn_batch.h).
//
// The tree is the ordinary one, sorted by a key that carries the label above the curve key (lbvh.hip, batch_key_kernel), so batch b
// is ONE range [starts[b], starts[b + 1]) of sorted slots.  Child c at level lvl of the 64-ary pyramid covers the slots
// [c * span, (c + 1) * span), span = LBVH_BLOCK << (6 * lvl) (walk_count_box's arithmetic, team_walk.h): "this box holds nothing of
// my batch" is two integer compares, no label is ever gathered in a walk, and nothing of the batch is dropped, because a slot of
// the range lies under exactly the children whose slot range holds it.  Boxes and blocks may straddle a batch boundary; the leaf
// test then takes only the lanes whose slot is in the range.
//   build. batch_label_check_kernel counts the labels outside [0, B) (one word read back), Engine::build builds with the labels,
//      batch_starts_kernel finds starts[b] as the lower bound of b << (63 - bb) in the sorted keys, one thread per batch.
//   1. external queries: batch_query_code_kernel and the radix sort of query_order.h's width -- the code is the label above the
//      leading 30 - bb bits of query_order's curve code, so the four teams of a wave walk the same batch and, inside it, neighbouring
//      nodes; without any radius also batch_slot_kernel, knn_slot_kernel's search (knn_seed.hip) of the batched key of (label,
//      query) inside the batch's range.  The tree's own points are their slots and come in (label, curve) order: neither pass.
//   2. without any radius (d_radii == NULL, radius == FLT_MAX): batch_seed_kernel<NREG>, knn_seed_kernel's window of
//      ceil(k / 16) + 1 blocks around the slot, clipped to the blocks that touch the range; a seed has its slot inside the range.
//   3. batch_walk_kernel<NREG>: radius_knn_walk_kernel's loop (radius_knn.hip) with the range rule in keep_box and at the leaf.
//   4. batch_lane_kernel<K>: one query per lane on the rope walk (lane_walk.h), nodes pruned by their slot range, for the queries
//      whose team stack overflowed, and for every query under TKNN_BATCH_KNN_FORCE_FALLBACK=1 (read per call).
// Both kernels write the same rows: (distance, index) order is total, the predicate is the literal knn_sqrt(d2) <= r in both, and
// the gates only ever drop what cannot be among a row's first k.
#include "curve_key.h"
#include "knn_thresholds.h"  // knn_gate_from_worst
#include "lane_walk.h"
#include "owlknn_batch.h"
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

constexpr int kBknnBlock = 64;            // one wave per workgroup, four teams
constexpr int kBknnBlocksPerCu = 16;      // 7.3 KB of LDS each
constexpr int kBknnSeedBlocksPerCu = 32;  // 1 KB of LDS each
constexpr int kBknnLaneBlock = 256;

struct BatchKnnArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const uint64_t *keys;        // the tree's sorted keys: the batch of a slot is keys[slot] >> (63 - key_bits)
  const int32_t *starts;       // num_batches + 1: batch b is the sorted slots starts[b] .. starts[b + 1] - 1
  int32_t num_batches;
  int key_bits;
  const float *queries;        // external: m packed triples, by the caller's j; null: the tree's own points, an item is a sorted slot
  const int32_t *query_batch;  // external: m labels, by the caller's j
  const uint32_t *order;       // external: the query worked on at sorted position i
  const int32_t *slots;        // external, seed pass: its place in its batch's range, by sorted position
  int32_t m;
  int k;
  float radius;                // every row's radius if radii and bounds are null (FLT_MAX: none)
  const float *radii;          // m, by the caller's j (may be null)
  float *bounds;               // the seed pass's r_j, by item (null: no seed pass)
  const int32_t *skip_ids;     // external: m, by the caller's j (may be null)
  int force_redo;              // TKNN_BATCH_KNN_FORCE_FALLBACK (tests): the walk leaves every query to the lane kernel
  int32_t *out_idx;            // m*k
  float *out_dist;             // m*k (may be null)
  int32_t *out_counts;         // m (may be null)
  int32_t *redo;               // m: items left to the lane kernel
  unsigned long long *ws;      // kRknnWsWords counters
};

// ---- the build's two kernels ---------------------------------------------------------------------------------------------------------
// how many labels lie outside [0, num_batches): one word
__global__ void __launch_bounds__(kBknnLaneBlock) batch_label_check_kernel(const int32_t *__restrict__ batch, int64_t n, int32_t num_batches,
                                                                           unsigned long long *__restrict__ bad) {
  unsigned long long mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBknnLaneBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBknnLaneBlock)
    mine += (uint32_t)batch[i] >= (uint32_t)num_batches ? 1u : 0u;
  mine = t_wave_sum(mine);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(bad, mine);
}
// starts[b], 0 <= b <= num_batches: the first sorted slot whose key is not below b << (63 - key_bits); for b = num_batches that is
// the first slot of a point with a NaN (bit 63 alone is above every label), n if there is none
__global__ void __launch_bounds__(kBknnLaneBlock) batch_starts_kernel(const uint64_t *__restrict__ keys, int32_t n, int32_t num_batches, int key_bits,
                                                                      int32_t *__restrict__ starts) {
  const int32_t b = blockIdx.x * kBknnLaneBlock + threadIdx.x;
  if (b > num_batches) return;
  const uint64_t key = (uint64_t)b << (63 - key_bits);
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  starts[b] = lo;
}

// ---- a query's point, row, batch range, radius, gate and skipped point ---------------------------------------------------------------
struct BknnQuery {
  LbvhPoint q;
  float r;       // the predicate's radius: the caller's, or the seed bound (which may be 0: k duplicates of the query)
  float r_wide;  // r * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts (radius_knn.hip)
  float gate_r;  // the squared-distance gate of an empty list: every d2 whose rounded root can be <= r passes
  int32_t skip;  // the point left out of the row (no point has a negative id)
  int32_t row;   // the caller's j
  int32_t s, e;  // the batch's sorted slots [s, e) (0, 0: a label no batch has)
  bool valid;    // a radius the call takes, a query without a NaN and a batch with a point in it (a row without: empty)
};
// the point, skipped id, row and batch range of an item: the caller's query j, or (the tree's own points) the point of a sorted slot
__device__ __forceinline__ void bknn_point(const BatchKnnArgs &a, int32_t item, bool has_q, LbvhPoint &q, int32_t &skip, int32_t &row, int32_t &s,
                                           int32_t &e) {
  q = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
  skip = -1, row = item, s = 0, e = 0;
  if (!has_q) return;
  uint32_t label;
  if (a.queries) {
    q.x = a.queries[3 * (int64_t)item], q.y = a.queries[3 * (int64_t)item + 1], q.z = a.queries[3 * (int64_t)item + 2];
    skip = a.skip_ids ? a.skip_ids[item] : -1;
    label = (uint32_t)a.query_batch[item];
  } else {
    q = a.bvh.points[item];
    skip = q.id;
    row = a.bvh.prim_id[item];
    label = (uint32_t)(a.keys[item] >> (63 - a.key_bits));  // (a NaN point: 2^key_bits, no batch)
  }
  if (label < (uint32_t)a.num_batches) s = a.starts[label], e = a.starts[label + 1];
}
__device__ __forceinline__ BknnQuery bknn_query(const BatchKnnArgs &a, int32_t item, bool has_q) {
  BknnQuery t;
  bknn_point(a, item, has_q, t.q, t.skip, t.row, t.s, t.e);
  t.r = !has_q ? 0.f : a.bounds ? a.bounds[item] : a.radii ? a.radii[t.row] : a.radius;
  const bool no_nan = (t.q.x == t.q.x) & (t.q.y == t.q.y) & (t.q.z == t.q.z);
  t.valid = has_q && (t.r > 0.f || (a.bounds && t.r == 0.f)) && t.r <= FLT_MAX && no_nan && t.e > t.s;  // (a NaN radius: neither)
  t.r_wide = t.r * 1.000001f;
  t.gate_r = knn_gate_from_worst(t.r);
  return t;
}

// ---- 1. the order of the queries, and a query's place in its batch's range -----------------------------------------------------------
// query_code_kernel's code (query_order.h) under the label: (label << (30 - key_bits)) | (code >> key_bits), as the tree's key is made
// from its 21 levels.  A query with a NaN or with a label no batch has sorts last (bit 30), as NaN queries do there.
__global__ void __launch_bounds__(kBknnLaneBlock) batch_query_code_kernel(const float *__restrict__ queries, const int32_t *__restrict__ query_batch, int32_t m,
                                                                          const float *__restrict__ scene, int curve, int32_t num_batches, int key_bits,
                                                                          uint32_t *__restrict__ codes, uint32_t *__restrict__ order) {
  const int32_t i = blockIdx.x * kBknnLaneBlock + threadIdx.x;
  if (i >= m) return;
  const float ext = fmaxf(fmaxf(scene[3] - scene[0], scene[4] - scene[1]), scene[5] - scene[2]);
  uint32_t code = (uint32_t)curve_point_key(curve, queries[3 * (int64_t)i], queries[3 * (int64_t)i + 1], queries[3 * (int64_t)i + 2], scene[0], scene[1],
                                            scene[2], ext, kCodeBits / 3);
  const uint32_t label = (uint32_t)query_batch[i];
  if (label >= (uint32_t)num_batches) code = 1u << kCodeBits;
  if (!(code >> kCodeBits)) code = (label << (kCodeBits - key_bits)) | (code >> key_bits);
  codes[i] = code;
  order[i] = (uint32_t)i;
}
// knn_slot_kernel's search (knn_seed.hip) inside the batch's range: the first slot of [s, e) whose key is not below the batched
// key of (label, query).  A query without a batch or with a NaN gets slot 0: it has no seed pass.
__global__ void __launch_bounds__(kBknnLaneBlock) batch_slot_kernel(const float *__restrict__ queries, const int32_t *__restrict__ query_batch,
                                                                    const uint32_t *__restrict__ order, int32_t m, const float *__restrict__ scene, int curve,
                                                                    const uint64_t *__restrict__ keys, const int32_t *__restrict__ starts, int32_t num_batches,
                                                                    int key_bits, int32_t *__restrict__ slots) {
  const int32_t i = blockIdx.x * kBknnLaneBlock + threadIdx.x;
  if (i >= m) return;
  const int64_t qi = order[i];
  const uint32_t label = (uint32_t)query_batch[qi];
  const float ext = fmaxf(fmaxf(scene[3] - scene[0], scene[4] - scene[1]), scene[5] - scene[2]);
  const uint64_t key21 = curve_point_key(curve, queries[3 * qi], queries[3 * qi + 1], queries[3 * qi + 2], scene[0], scene[1], scene[2], ext, 21);
  int32_t lo = 0, hi = 0;
  if (label < (uint32_t)num_batches && !(key21 >> 63)) lo = starts[label], hi = starts[label + 1];
  const uint64_t key = ((uint64_t)label << (63 - key_bits)) | (key21 >> key_bits);
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
// knn_seed_kernel's window (knn_seed.hip) inside the batch: the blocks that touch [s, e) are blk_lo .. blk_hi - 1, the window is
// min(ceil(k / 16) + 1, blk_hi - blk_lo) of them around the slot's block.  Lane tl takes point tl of a block; a seed is a point the
// row could list -- its slot in [s, e) (edge blocks hold neighbours from other batches), d2 finite, not the skipped point --, so
// the k-th smallest of the seeds' distances is an upper bound of the row's k-th.  A window that does not hold the whole batch has
// at most one edge block, so at least 16 * ceil(k / 16) + 1 slots of the batch, one of which may be the skipped point: k seeds.
// With fewer (a batch of fewer than k eligible points) the bound is FLT_MAX, which costs a walk of the batch's range and no more.
// The loop runs ceil(k / 16) + 1 times for every team of a launch, so the teams of a wave stay in lock step.
template <int NREG>
__global__ void __launch_bounds__(kBknnBlock) batch_seed_kernel(BatchKnnArgs a) {
  __shared__ unsigned long long cand_mem[4 * kCandCapacity];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  unsigned long long *my_cand = cand_mem + team * kCandCapacity;
  const int32_t window = (a.k + LBVH_BLOCK - 1) / LBVH_BLOCK + 1;
  const bool self = a.queries == nullptr;
  unsigned long long seed_tests = 0;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < (int64_t)a.m; base += (int64_t)gridDim.x * 4) {
    const int64_t pos = base + team;
    const bool has_q = pos < (int64_t)a.m;
    const int32_t item = has_q ? (self ? (int32_t)pos : (int32_t)a.order[pos]) : 0;
    LbvhPoint q;
    int32_t skip, row, s, e;
    bknn_point(a, item, has_q, q, skip, row, s, e);
    const int32_t slot = has_q ? (self ? (int32_t)pos : a.slots[pos]) : 0;
    const bool in_batch = e > s;
    const int32_t blk_lo = s >> 4, blk_hi = in_batch ? ((e - 1) >> 4) + 1 : blk_lo;
    const int32_t mine = min(window, blk_hi - blk_lo);  // 0: no batch, no seeds
    // the window's first block: the slot's block in the middle, clipped at both ends of the batch's blocks
    const int32_t first = max(blk_lo, min((min(slot, e - 1) >> 4) - (mine - 1) / 2, blk_hi - mine));
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
      if (has_b) p = a.bvh.points[at];
      seed_tests += has_b ? 1u : 0u;
      const float d2 = knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z);
      const bool seed = has_b && at >= s && at < e && d2 <= FLT_MAX && p.id != skip;  // (NaN: not a seed)
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
// The range rule.  Child c of level lvl covers the slots [c << sh, (c + 1) << sh), sh = 4 + 6 lvl; it meets [s, e) iff
// (s >> sh) <= c <= ((e - 1) >> sh).  A child that does not is declined before its box is looked at; one that does goes through
// radius_knn_walk_kernel's gate rule.  The rule drops no point of the batch: slot t lies under child t >> sh of every level, and
// s <= t < e gives (s >> sh) <= (t >> sh) <= ((e - 1) >> sh).  (Above level 4, sh exceeds 31; every slot is below 2^31, so a shift
// by 31 gives the same zeros.)
// The leaf test.  Lane tl of block b is slot 16 b + tl: a candidate only if that lies in [s, e); then radius_knn_walk_kernel's --
// d2 = knn_dist2, and where some lane's d2 passes the gate, d = knn_sqrt(d2) and the literal d <= r decide.
template <int NREG>
__global__ void __launch_bounds__(kBknnBlock) __attribute__((amdgpu_waves_per_eu(4))) batch_walk_kernel(BatchKnnArgs a) {
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
    const BknnQuery s = bknn_query(a, item, has_q);
    const LbvhPoint &q = s.q;
    const bool active = s.valid && !a.force_redo;
    const WalkBox qb(q, s.r_wide);
    const int32_t rs = s.s, re_last = s.e - 1;  // the batch's first and last slot
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
          [&](const LbvhBox &bx, int32_t c, int lvl) {
            const int sh = min(4 + 6 * lvl, 31);
            if (c < (rs >> sh) || c > (re_last >> sh)) return false;
            return !beyond_gate(box_min_dist2(bx, q), tau2);
          },
          [&](int32_t b, bool has_b) {
            LbvhPoint p = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
            if (has_b) p = a.bvh.points[(int64_t)b * LBVH_BLOCK + tl];
            point_tests += has_b ? 1u : 0u;
            const int32_t at = b * LBVH_BLOCK + tl;  // my slot
            const float d2 = knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z);
            const bool near = has_b && at >= rs && at <= re_last && d2 <= tau2 && p.id != s.skip;  // (a NaN on either side: not a neighbour)
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
// The same predicate, the same gate (a node whose near corner lies beyond it, or whose slots miss the batch's range, is stepped over
// through its rope), a sorted list of (distance, index) keys in registers: K >= k entries, of which the first k are the row.
template <int K>
__global__ void __launch_bounds__(kBknnLaneBlock) batch_lane_kernel(BatchKnnArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kBknnLaneBlock + threadIdx.x;
  const bool has_q = t < (int64_t)a.ws[kRknnWsRedo];
  const int32_t item = has_q ? a.redo[t] : 0;
  const BknnQuery s = bknn_query(a, item, has_q);
  const LbvhPoint &q = s.q;
  KList<K> list;
  list.clear();
  float gate = s.gate_r;
  unsigned long long node_tests = 0, point_tests = 0;
  if (s.valid)
    lane_walk<LaneRope::kWithNode>(a.bvh,
        [&](int32_t ref, const LbvhNode &nd, int32_t) {
          node_tests++;
          if (lbvh_last(ref, nd.other) < s.s || lbvh_first(ref, nd.other) >= s.e) return lane_rope();
          if (!lane_box_hit(nd, q, s.r_wide)) return lane_rope();
          float far2, near2;
          lane_box_dist2(nd, q, far2, near2);
          return near2 * 0.999995f > gate ? lane_rope() : lane_descend();
        },
        [&](int32_t slot, const LbvhPoint &p) {
          point_tests++;
          const float d = knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z));
          if (slot >= s.s && slot < s.e && d <= s.r && p.id != s.skip) {
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

using BknnEntry = void (*)(BatchKnnArgs);
const BknnEntry kBknnSeeds[4] = {batch_seed_kernel<1>, batch_seed_kernel<2>, batch_seed_kernel<3>, batch_seed_kernel<4>};
const BknnEntry kBknnWalks[4] = {batch_walk_kernel<1>, batch_walk_kernel<2>, batch_walk_kernel<3>, batch_walk_kernel<4>};

}  // namespace

void Engine::build_batched(const float *d_xyz, const int32_t *d_ids, const int32_t *d_batch, int32_t num_batches, int64_t n, tknnBuildInfo *info,
                           hipStream_t s) {
  int bits = 0;  // the smallest multiple of 3 with 2^bits >= num_batches: the key loses whole levels of cells
  while ((1 << bits) < num_batches) bits += 3;
  unsigned long long *d_bad = (unsigned long long *)workspace(256);
  OWLMI_HIP(hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), s));
  const int blocks = (int)std::min<int64_t>((n + kBknnLaneBlock - 1) / kBknnLaneBlock, (int64_t)cu_count_ * 8);
  hipLaunchKernelGGL(batch_label_check_kernel, dim3(blocks), dim3(kBknnLaneBlock), 0, s, d_batch, n, num_batches, d_bad);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipMemcpyAsync(h_counters_, d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (h_counters_[0]) {
    bvh_.clear();
    num_batches_ = 0;
    throw ArgError{TKNN_E_ARG, "tknnBuildBatched: " + std::to_string(h_counters_[0]) + " of the " + std::to_string(n) + " labels in d_batch lie outside [0, num_batches = " +
                                   std::to_string(num_batches) + ")"};
  }
  if ((int64_t)num_batches + 1 > batch_starts_cap_) {
    if (batch_starts_) (void)hipFree(batch_starts_);
    batch_starts_ = nullptr;
    batch_starts_cap_ = 0;
    bvh_.clear();  // (if the allocation fails: no tree rather than a batched one without its starts)
    OWLMI_HIP(hipMalloc((void **)&batch_starts_, ((size_t)num_batches + 1) * sizeof(int32_t)));
    batch_starts_cap_ = (int64_t)num_batches + 1;
  }
  build(d_xyz, d_ids, n, info, s, d_batch, bits);
  hipLaunchKernelGGL(batch_starts_kernel, dim3((unsigned)((num_batches + 1 + kBknnLaneBlock - 1) / kBknnLaneBlock)), dim3(kBknnLaneBlock), 0, s,
                     bvh_.keys_device(), (int32_t)n, num_batches, bits, batch_starts_);
  try {
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipStreamSynchronize(s));
  } catch (...) {
    bvh_.clear();
    throw;
  }
  num_batches_ = num_batches;
  batch_bits_ = bits;
}

void Engine::batch_layout(int32_t *num_batches, int32_t *key_bits, int32_t *d_starts, hipStream_t s) {
  if (num_batches) *num_batches = num_batches_;
  if (key_bits) *key_bits = batch_bits_;
  if (d_starts) {
    OWLMI_HIP(hipMemcpyAsync(d_starts, batch_starts_, ((size_t)num_batches_ + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    OWLMI_HIP(hipStreamSynchronize(s));
  }
}

void Engine::batch_knn(const tknnBatchKnnOptions &o, tknnBatchKnnInfo *info, hipStream_t s) {
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

  BatchKnnArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.wide = bvh_.wide_view();
  a.keys = bvh_.keys_device();
  a.starts = batch_starts_;
  a.num_batches = num_batches_;
  a.key_bits = batch_bits_;
  a.queries = o.d_queries;
  a.query_batch = o.d_query_batch;
  a.order = self ? nullptr : order;
  a.slots = self ? nullptr : slots;
  a.m = (int32_t)m;
  a.k = o.k;
  a.radius = o.radius;
  a.radii = o.d_radii;
  a.bounds = seeded ? bounds : nullptr;
  a.skip_ids = o.d_skip_ids;
  if (const char *e = getenv("TKNN_BATCH_KNN_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.out_idx = o.d_idx;
  a.out_dist = o.d_dist;
  a.out_counts = o.d_counts;
  a.redo = redo;
  a.ws = d_words;

  const unsigned lane_grid = (unsigned)((m + kBknnLaneBlock - 1) / kBknnLaneBlock);
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(d_words, 0, kRknnWsWords * sizeof(unsigned long long), s));
  if (!self) {  // query_order (query_order.h) with the label above the code: one sort of the same width
    hipLaunchKernelGGL(batch_query_code_kernel, dim3(lane_grid), dim3(kBknnLaneBlock), 0, s, o.d_queries, o.d_query_batch, (int32_t)m, bvh_.scene_device(),
                       bvh_.curve(), num_batches_, batch_bits_, codes, order_in);
    OWLMI_HIP(hipGetLastError());
    size_t bytes = sort_bytes;
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp, bytes, codes, codes_alt, order_in, order, (int)m, 0, kCodeBits + 1, s));
  }
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  if (seeded) {
    if (!self) {
      hipLaunchKernelGGL(batch_slot_kernel, dim3(lane_grid), dim3(kBknnLaneBlock), 0, s, o.d_queries, o.d_query_batch, (const uint32_t *)order, (int32_t)m,
                         bvh_.scene_device(), bvh_.curve(), a.keys, a.starts, num_batches_, batch_bits_, slots);
      OWLMI_HIP(hipGetLastError());
    }
    const int blocks = (int)std::min<int64_t>((m + 3) / 4, (int64_t)cu_count_ * kBknnSeedBlocksPerCu);
    void *kargs[] = {(void *)&a};
    OWLMI_HIP(hipLaunchKernel((const void *)kBknnSeeds[query_nreg(o.k) - 1], dim3(blocks), dim3(kBknnBlock), kargs, 0, s));
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  // the walk, then the lane kernel for what the walk left
  unsigned long long *h_words = h_counters_;
  {
    const int blocks = (int)std::min<int64_t>((m + 3) / 4, (int64_t)cu_count_ * kBknnBlocksPerCu);
    void *kargs[] = {(void *)&a};
    OWLMI_HIP(hipLaunchKernel((const void *)kBknnWalks[query_nreg(o.k) - 1], dim3(blocks), dim3(kBknnBlock), kargs, 0, s));
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipMemcpyAsync(h_words, d_words, kRknnWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));  // the call's one host sync before its last: the redo list's length
  const unsigned long long n_redo = h_words[kRknnWsRedo];
  if (n_redo) {
    const unsigned lane_blocks = (unsigned)((n_redo + kBknnLaneBlock - 1) / kBknnLaneBlock);
    ListCapacities::dispatch(list_capacity_for(o.k), [&](auto cap) {
      hipLaunchKernelGGL(batch_lane_kernel<decltype(cap)::value>, dim3(lane_blocks), dim3(kBknnLaneBlock), 0, s, a);
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
