// radius_walk.h -- the one walk and the one lane kernel of the calls that visit EVERY point within a radius of each query:
// tknnRadiusQuery's count and fill passes (radius_query.hip), tknnRadiusReduce (radius_reduce.hip) and tknnLocalPca
// (local_pca.hip), and the launch pair they share.  (The calls that keep at most k of those points: radius_knn_walk.h.)  A call
// differs from the next in its RULE, a struct of static device functions next to its argument block Args, whose common fields
// (bvh, wide, queries, order, m, force_redo, redo, ws) the code here reads directly:
//   Query, query(a, pos, has_q)       the query at sorted position pos: point q, output row, the literal bound r, the query box's
//                                     half-width r_wide, the inside bound in2, the slot `self` treated apart (-1: none), and the
//                                     call's own fields
//   Lane, start(st, lds)              my lane's share of a row beyond its count `part`; lds: my team's kTeamLds words (walk only)
//   member(a, s, slot, p, d)          the literal predicate on the fp32 distance d (a NaN on either side fails it)
//   take(a, s, st, part, hit, ...)    the walk, every lane of the wave, `hit` my point's member(): counts it, takes its share
//   kArith                            an inside box is counted arithmetically at every level and nothing of it is read; else a
//                                     box above the leaf level goes to the team's range list and is streamed after the walk
//   kRolled                           walk_tree's ROLLED: the visitor is too large to have four times
//   kTeamLds                          64-bit words of LDS per team beyond the stack, the levels and the range list
//   row_end(a, s, st, part, team, tl) the walk, every lane: the team reductions (and what still waits); the row's length
//   row_write(a, s, st, cnt)          one lane, walk and lane kernel: the finished row to memory; 1 if the row counts into the
//                                     call's own counter word (kRadOwn)
//   lane_arith(a)                     the lane kernel counts a node inside the sphere instead of walking it
//   lane_take(a, s, st, cnt, ...)     the lane kernel, for a point that passed member(): its share; cnt: the row's length so far
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lane_walk.h"
#include "team_lanes.h"
#include "team_walk.h"
#include "trueknn_engine.h"

namespace owlmi {

// words of a call's own counters (in the workspace, zeroed per pass)
enum {
  kRadCursor = 0,
  kRadRedo = 1,
  kRadTotal = 2,
  kRadMaxRow = 3,
  kRadLaneRows = 4,  // rows the lane kernel wrote
  kRadNodeTests = 5,
  kRadPointTests = 6,
  kRadOwn = 7,  // the call's own: rows that do not fit their segment (fill pass), degenerate rows (PCA)
  kRadWords = 8
};

constexpr int kRadBlock = 64;        // one wave per workgroup, four teams
constexpr int kRadBlocksPerCu = 16;  // 6.3 KB of LDS each, 7.5 with the fill pass's stage
constexpr int kRadLaneBlock = 256;
constexpr int kRadRanges = 16;  // inside boxes above the leaf level a team notes for streaming; a 17th is walked

// The box rule.  A child box lies wholly INSIDE the sphere if the squared distance far2 from q to its far corner is at most
// radius_in2.  The margin's direction: radius_in2 = r^2 * 0.999995 rounded DOWN, so the rule can only call fewer boxes inside
// than the exact one would -- a box is called inside only if every point of it certainly passes the literal test.  (For a point p
// of the box, lo <= p <= hi, and fp32 subtraction, multiplication and addition are monotone, so p's own dist2 as knn_dist2 rounds
// it is <= far2 <= r^2, and the correctly rounded root of a value <= r^2 is <= r.  The margin is the one the other counting rules
// keep, on top of that.)  Its slots must end before clean_end: NaN points sort last and are nobody's neighbour, and the padding of
// the last block is no point at all.
//   kArith:     the box's slot count is added arithmetically (less the query's own slot where that is left out and lies in it),
//               nothing below it is read;
//   otherwise:  the points have to be read, for their id and distance or for their share of a sum.  A leaf block is kept and
//               tested like any other; a box above the leaf level is noted in the team's range list and streamed after the walk,
//               the lanes striding its slots (its child boxes are never read).  A full list: the box is walked.
// radius_in2: that product in double, rounded DOWN to fp32 (a rounded-up f is positive: its bits less one are the float below it)
__host__ __device__ inline float radius_inside2(float r) {
  const double want = (double)r * (double)r * 0.999995;
  float f = (float)want;
  if ((double)f > want) f = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) - 1u);
  return f;
}

namespace {

// The point worked on at sorted position pos and the row its results go to: external queries along `order`; the set's own points
// (queries null) in sorted-slot order, position i is slot i -- that slot is returned, -1 for an external query.  q.id: the
// point's name (-1: external).
template <class Args>
__device__ __forceinline__ int32_t rad_point(const Args &a, int32_t pos, bool has_q, LbvhPoint &q, int32_t &row) {
  if (a.queries) {
    row = has_q ? (int32_t)a.order[pos] : 0;
    q = LbvhPoint{a.queries[3 * (int64_t)row], a.queries[3 * (int64_t)row + 1], a.queries[3 * (int64_t)row + 2], -1};
    return -1;
  }
  const int32_t slot = has_q ? pos : 0;
  q = a.bvh.points[slot];
  row = a.bvh.prim_id[slot];
  return slot;
}

__device__ __forceinline__ void rad_add_stats(unsigned long long *ws, int lane, unsigned long long total, unsigned int max_row, unsigned long long lane_rows,
                                              unsigned long long own, unsigned long long node_tests, unsigned long long point_tests) {
  const unsigned long long tsum = t_wave_sum(total), lr = t_wave_sum(lane_rows), osum = t_wave_sum(own), nt = t_wave_sum(node_tests),
                           pt = t_wave_sum(point_tests);
  unsigned int mx = max_row;  // (t_wave_max is a float's: a row length has 31 bits)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, off));
  if (lane == 0) {
    if (tsum) atomicAdd(&ws[kRadTotal], tsum);
    if (mx) atomicMax(&ws[kRadMaxRow], (unsigned long long)mx);
    if (lr) atomicAdd(&ws[kRadLaneRows], lr);
    if (osum) atomicAdd(&ws[kRadOwn], osum);
    if (nt) atomicAdd(&ws[kRadNodeTests], nt);
    if (pt) atomicAdd(&ws[kRadPointTests], pt);
  }
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
// Persistent, one 16-lane team per query, four teams per wave; a cursor hands out groups of four sorted positions.  walk_tree
// (team_walk.h) with the query's box of half-width r_wide = r (1 + 1e-6): the box prefilter must not cut what the rounded sphere
// test accepts.  Lane tl tests point tl of a leaf block with the rule's literal predicate and takes its share into its OWN
// registers; one team reduction per row at the end.  A query whose team stack overflowed (and every query under the call's
// TKNN_*_FORCE_FALLBACK=1) goes to the redo list, whose length lives on the device.  Teams of a wave loop in lock step: no
// __syncthreads, only t_wave_sync.
template <class Rule>
__global__ void __launch_bounds__(kRadBlock) __attribute__((amdgpu_waves_per_eu(4))) rad_walk_kernel(typename Rule::Args a) {
  constexpr bool kRanges = !Rule::kArith;
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[LBVH_WIDE_LEVELS];
  __shared__ unsigned long long team_mem[Rule::kTeamLds > 0 ? 4 * Rule::kTeamLds : 1];
  __shared__ int32_t range_mem[kRanges ? 4 * kRadRanges : 1];
  __shared__ uint32_t range_n_mem[4];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  int32_t *range = range_mem + (kRanges ? team * kRadRanges : 0);
  uint32_t *range_n = range_n_mem + team;
  walk_fill_levels<1>(levels, &a.wide, lane);
  if (tl == 0) *range_n = 0u;
  t_wave_sync();
  const LbvhWideView &wv = a.wide;
  const int32_t clean_end = lane_clean_end(a.bvh);
  unsigned long long node_tests = 0, point_tests = 0, total = 0, own = 0;
  unsigned int max_row = 0;
  for (;;) {
    int got = 0;
    if (lane == 0) got = (int)atomicAdd(&a.ws[kRadCursor], 4ull);
    const int base = __builtin_amdgcn_readfirstlane(got);
    if (base >= a.m) break;
    const int32_t pos = base + team;
    const bool has_q = pos < a.m;
    const typename Rule::Query s = Rule::query(a, pos, has_q);
    const LbvhPoint &q = s.q;
    const bool active = has_q && !a.force_redo;
    const WalkBox qb(q, s.r_wide);
    uint32_t part = 0;  // my lane's share of the row length
    typename Rule::Lane st;
    Rule::start(st, team_mem + (Rule::kTeamLds > 0 ? team * Rule::kTeamLds : 0));
    // lane tl takes point tl of the sixteen slots from `slot0` (the sorted arrays are padded with NaN sentinels to whole blocks)
    auto test_points = [&](int64_t slot0, bool has_b) __attribute__((always_inline)) {
      const int64_t slot = slot0 + tl;
      LbvhPoint p = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
      if (has_b) p = a.bvh.points[slot];
      const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
      const float d2 = t_dist2(dx, dy, dz);
      const float d = knn_sqrt(d2);
      const bool hit = has_b && Rule::member(a, s, (int32_t)slot, p, d);
      point_tests += has_b ? 1u : 0u;
      Rule::take(a, s, st, part, hit, slot, p, dx, dy, dz, d2, d, team, tl);
    };
    bool overflow = wv.levels <= 0;
    if (wv.levels > 0)
      walk_tree<Rule::kRolled>(
          levels, wv, stack, kWalkStack, active, q, qb, team, tl, node_tests,
          [&](const LbvhBox &bx, int32_t c, int lvl) {
            if (kRanges && lvl == 0) return true;
            const float ax = fmaxf(fabsf(q.x - bx.lo[0]), fabsf(q.x - bx.hi[0])), ay = fmaxf(fabsf(q.y - bx.lo[1]), fabsf(q.y - bx.hi[1])),
                        az = fmaxf(fabsf(q.z - bx.lo[2]), fabsf(q.z - bx.hi[2]));
            const float far2 = t_dist2(ax, ay, az);
            const int64_t span = (int64_t)LBVH_BLOCK << (6 * lvl);  // points under one child of this level
            if (!(far2 <= s.in2 && ((int64_t)c + 1) * span <= (int64_t)clean_end)) return true;
            if constexpr (!kRanges) {
              const bool mine = (int64_t)s.self >= (int64_t)c * span && (int64_t)s.self < ((int64_t)c + 1) * span;  // (self = -1: never)
              part += (uint32_t)span - (mine ? 1u : 0u);
              return false;
            } else {
              const uint32_t at = atomicAdd(range_n, 1u);
              if (at >= (uint32_t)kRadRanges) return true;
              range[at] = (lvl << 26) | c;
              return false;
            }
          },
          [&](int32_t b, bool has_b) { test_points((int64_t)b * LBVH_BLOCK, has_b); }, [] {}, overflow);
    if constexpr (kRanges) {
      // the noted inside boxes, sixteen slots a step (every point but a query's own passes; the literal test costs one compare and decides)
      t_wave_sync();
      const uint32_t nr = min(*range_n, (uint32_t)kRadRanges);
      for (uint32_t i = 0; __ballot(i < nr) != 0ull; i++) {
        const bool has_r = i < nr;
        const int32_t e = has_r ? range[i] : 0;
        const int64_t span = has_r ? (int64_t)LBVH_BLOCK << (6 * (e >> 26)) : 0;
        const int64_t first = (int64_t)(e & 0x3ffffff) * span;
#pragma unroll 1
        for (int64_t t = 0; __ballot(t < span) != 0ull; t += LBVH_BLOCK) test_points(first + t, t < span);
      }
      t_wave_sync();
      if (tl == 0) *range_n = 0u;
      t_wave_sync();
    }
    const uint32_t cnt = Rule::row_end(a, s, st, part, team, tl);
    if (has_q && tl == 0) {
      if (overflow || a.force_redo) {
        // left to the lane kernel, which starts the row again: nothing of it is counted here
        a.redo[atomicAdd(&a.ws[kRadRedo], 1ull)] = pos;
      } else {
        own += Rule::row_write(a, s, st, cnt);
        total += cnt;
        max_row = max(max_row, cnt);
      }
    }
  }
  rad_add_stats(a.ws, lane, total, max_row, 0ull, own, node_tests, point_tests);
}

// ---- one query per lane: the positions of the redo list ----------------------------------------------------------------------------
// The rope walk (lane_walk.h) with the same predicate, for the queries whose team stack overflowed and for trees too small for a
// pyramid -- the result is complete on any tree.  Where the rule counts arithmetically, a node inside the sphere is counted, not
// walked (db_count_from; the margin: in2).
template <class Rule>
__global__ void __launch_bounds__(kRadLaneBlock) rad_lane_kernel(typename Rule::Args a) {
  const int64_t t = (int64_t)blockIdx.x * kRadLaneBlock + threadIdx.x;
  const bool has_q = t < (int64_t)a.ws[kRadRedo];
  const int32_t pos = has_q ? a.redo[t] : 0;
  const int32_t clean_end = lane_clean_end(a.bvh);
  const typename Rule::Query s = Rule::query(a, pos, has_q);
  const LbvhPoint &q = s.q;
  uint32_t cnt = 0;
  typename Rule::Lane st;
  Rule::start(st, nullptr);
  unsigned long long node_tests = 0, point_tests = 0;
  if (has_q)
    lane_walk<LaneRope::kWithNode>(a.bvh,
        [&](int32_t ref, const LbvhNode &nd, int32_t) {
          node_tests++;
          if (!lane_box_hit(nd, q, s.r_wide)) return lane_rope();
          if (Rule::lane_arith(a)) {
            float far2, near2;
            lane_box_dist2(nd, q, far2, near2);
            const int32_t first = lbvh_first(ref, nd.other), last = lbvh_last(ref, nd.other);
            if (far2 <= s.in2 && last < clean_end) {
              cnt += (uint32_t)(last - first + 1) - (s.self >= first && s.self <= last ? 1u : 0u);
              return lane_rope();
            }
          }
          return lane_descend();
        },
        [&](int32_t slot, const LbvhPoint &p) {
          point_tests++;
          const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
          const float d2 = t_dist2(dx, dy, dz);
          const float d = knn_sqrt(d2);
          if (Rule::member(a, s, slot, p, d)) {
            Rule::lane_take(a, s, st, cnt, slot, p, dx, dy, dz, d2, d);
            cnt++;
          }
          return lane_rope();
        });
  const unsigned long long own = has_q ? Rule::row_write(a, s, st, cnt) : 0ull;
  // (all lanes of the wave are here)
  rad_add_stats(a.ws, threadIdx.x & 63, has_q ? cnt : 0u, has_q ? cnt : 0u, has_q ? 1u : 0u, own, node_tests, point_tests);
}

// ---- the launches ------------------------------------------------------------------------------------------------------------------
// The walk over the m positions of `a`, then the lane kernel (LaneRule's, where its template arguments are fewer than the walk's)
// over what the walk left; one host sync before the caller's last -- the redo list's length, which is returned.  h_words:
// kRadWords words of pinned host memory, the counters as they stand once the stream has been synchronised again.
template <class Rule, class LaneRule = Rule>
unsigned long long rad_walks(const typename Rule::Args &a, int cu_count, unsigned long long *h_words, hipStream_t s) {
  const int blocks = (int)std::min<int64_t>(((int64_t)a.m + 3) / 4, (int64_t)cu_count * kRadBlocksPerCu);
  hipLaunchKernelGGL(rad_walk_kernel<Rule>, dim3(blocks), dim3(kRadBlock), 0, s, a);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kRadWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));  // the call's one host sync before its last: the redo list's length
  const unsigned long long n_redo = h_words[kRadRedo];
  if (n_redo) {
    const unsigned lane_blocks = (unsigned)((n_redo + kRadLaneBlock - 1) / kRadLaneBlock);
    hipLaunchKernelGGL(rad_lane_kernel<LaneRule>, dim3(lane_blocks), dim3(kRadLaneBlock), 0, s, a);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kRadWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  }
  return n_redo;
}

}  // namespace

}  // namespace owlmi
