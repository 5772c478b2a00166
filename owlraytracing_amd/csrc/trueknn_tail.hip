// trueknn_tail.hip -- what follows the packet kernel (trueknn_team.hip) in a team solve, k <= 64: the hand-over walk
// (team_walk_kernel: the queries whose candidate lists outgrew the packet kernel's LDS lists, one query per team) and the tie
// pass (tie_fix_kernel: flagged rows redone in the reference's order of exact-distance ties), with their launches, the slot
// compaction in front of both, and the host code every team launch shares: the argument block (TeamArgs, team_args.h), the
// start-of-solve state and the statistics' stripes.
#include "knn_thresholds.h"  // knn_gate_from_worst
#include "team_args.h"
#include "team_lanes.h"
#include "team_walk.h"
#include "trueknn_engine.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

#ifndef TKNN_WALK_WAVES
// waves per SIMD the walks' register allocation aims at (0: the compiler's choice, 3 with 131 .. 147 registers).  Round 4: 4 --
// a few words of scratch outside the loops; 10 M points: the hand-over walk 12 .. 18 % faster (taxi-like set at k = 10: 4.4 -> 3.9 ms,
// uniform at k = 48: 5.3 -> 4.4 ms), the k > 64 walk 17 % (k = 65: 209 -> 174 ms); 5 and 6 spill inside the loops and lose
#define TKNN_WALK_WAVES 4
#endif
#if TKNN_WALK_WAVES
#define TKNN_WALK_ATTR __attribute__((amdgpu_waves_per_eu(TKNN_WALK_WAVES)))
#else
#define TKNN_WALK_ATTR
#endif
constexpr int kWalkBlocksPerCu = 4 * (TKNN_WALK_WAVES > 4 ? TKNN_WALK_WAVES : 4);  // one-wave workgroups of the walks' launches

// ---- team walk: the stragglers, one query per team, no packet lists --------------------------------
// Queries the packet kernel hands over (outliers whose boxes have grown over whole clusters, dense
// duplicates) have candidate sets far beyond its LDS lists.  Here a team walks the pyramid for ONE
// query: its 16 lanes test 16 child boxes of a wide node at a time and push the survivors on the
// team's LDS stack; a leaf block is 16 points = 16 lanes, tested, counted and selected exactly like
// in the packet kernel's passes.  A child box that lies inside the part of the query's box where the
// candidate test is certain, and beyond the list's gate, is COUNTED (its points are consecutive
// sorted slots: the count is arithmetic) instead of walked -- a box over a cluster of 100 000 points
// costs a few hundred steps.  Levels loop inside the kernel (hostCode.cpp:285-340 per query).
// The walk itself, its box and block tests and the counting rule are team_walk.h's.

struct NotDone {
  __host__ __device__ bool operator()(uint8_t d) const { return d == 0; }
};

template <bool HALO, int NREG>
__global__ void __launch_bounds__(kTeamBlock) TKNN_WALK_ATTR team_walk_kernel(TeamArgs a, const int32_t *slots, int32_t nslots) {
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[2][LBVH_WIDE_LEVELS];
  __shared__ unsigned long long cand_mem[4 * kCandCapacity];  // per team: candidates waiting to be merged into its list (t_merge_rows)
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  walk_fill_levels<2>(levels[0], a.wide, lane);
  t_wave_sync();
  unsigned long long isect_sum = 0, levels_sum = 0, node_tests = 0, point_tests = 0;
  unsigned int unfinished = 0, failed = 0;
  int max_level = 0;
  int turn_next = 0, turn_left = 0;  // (t_next_slots)
  for (;;) {
    const int base = t_next_slots(&a.counters[0], a.grab, lane, turn_next, turn_left);
    if (base >= nslots) break;
    const bool has_q = base + team < nslots;
    const int32_t slot = has_q ? (slots ? slots[base + team] : base + team) : 0;
    const LbvhPoint q = a.bvh.points[slot];
    const int32_t row = a.bvh.prim_id[slot];
    int level = has_q ? a.next_level[slot] : 0;
    int64_t isect = has_q ? a.isect_sorted[slot] : 0;
    const float q_r0 = a.start_radii ? a.start_radii[row] : a.start_radius;  // per-query schedule, if asked for
    float r = q_r0;
    for (int i = 0; i < level; i++) r = r * 2.0f;
    bool active = has_q;
    while (__ballot(active) != 0ull) {  // one radius level for every team that is still at work
      const WalkBox qb(q, r);
      uint32_t part = 0;  // my lane's share of the candidate count of this level
      uint32_t bd[NREG], bi[NREG];  // register j of lane t holds list entry 16 j + t (indices are compile-time: stays in VGPRs)
#pragma unroll
      for (int j = 0; j < NREG; j++) {
        bd[j] = 0x7f7fffffu;  // KNN_EMPTY_KEY = {FLT_MAX, 0}
        bi[j] = 0u;
      }
      float tau2 = INFINITY;
      bool overflow = false;
      const bool full = a.k == 16 * NREG;  // see team_pass
      uint32_t left_out = 0xffffffffu;
      // candidates wait in the team's buffer and are merged sixteen at a time, as in the passes (one insert per lock-step
      // round was most of this kernel's time at k = 64: some 200 inserts per query)
      unsigned long long *my_cand = cand_mem + team * kCandCapacity;
      uint32_t fill_n = 0;
      auto merge_buffer = [&]() __attribute__((always_inline)) {
        t_wave_sync();
        t_merge_rows<NREG>(bd, bi, left_out, full, my_cand, fill_n, tl);
        t_wave_sync();
        fill_n = 0;
        tau2 = knn_gate_from_worst(t_kth_dist<NREG>(bd, a.k, team));
      };
      for (int tree = 0; tree < (HALO ? 2 : 1); tree++) {
        const LbvhWideView &wv = a.wide[tree];
        const LbvhView &tv = tree == 0 ? a.bvh : a.halo;
        if (tv.n <= 0 || wv.levels <= 0) continue;
        const int32_t clean_end = tv.n - (tv.nan_count ? *tv.nan_count : 0);  // NaN points sort last
        walk_tree<false>(
            levels[tree], wv, stack, kWalkStack, active, q, qb, team, tl, node_tests,
            [&](const LbvhBox &bx, int32_t c, int lvl) { return !walk_count_box(bx, q, qb, tau2, c, lvl, clean_end, part); },
            [&](int32_t b, bool has_b) {
              LbvhPoint p;
              float d2;
              const unsigned long long in_m = walk_block_test(tv.points, b, has_b, tl, q, qb, p, d2);
              point_tests += has_b ? 1u : 0u;
              part = t_count(part, in_m);
              unsigned long long pm = in_m & __ballot(p.id != q.id) & __ballot(d2 <= tau2);
              if (TKNN_DIAG_BUILD && (a.diag & 1)) pm = 0;
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
      }
      if (__ballot(fill_n > 0u) != 0ull) merge_buffer();
      if (full) left_out = t_team_min_u32(left_out);  // the smallest key left out by any merge, where the tie test below looks for it: lane 15
      // ---- the level's outcome, per team ----
      const uint32_t cnt = t_team_sum(part);
      const uint32_t others = cnt ? cnt - 1u : 0u;  // a query lies in its own box
      const bool fin = active && !overflow && others >= (uint32_t)a.k;
      if (active && overflow) {  // stack exhausted: leave the query to the lane rounds, state untouched
        failed += tl == 0 ? 1u : 0u;
        active = false;
      } else if (active) {
        isect += cnt;
        levels_sum += tl == 0 ? 1ull : 0ull;
        if (fin) {
#pragma unroll
          for (int reg = 0; reg < NREG; reg++) {
            const int j = tl + 16 * reg;
            if (j >= a.k) continue;
            t_write_entry(a.out_idx, a.out_dist, a.out_fb, (int64_t)row * a.k + j, knn_key_prim(((uint64_t)bd[reg] << 32) | bi[reg]),
                          __uint_as_float(bd[reg]), j, a.k, isect);
          }
          bool tie, edge;
          t_row_ties<NREG>(bd, left_out, full, a.k, tl, q, q_r0, r, a.tie_span, true, tie, edge);
          const bool tied = t_team_any(tie, team), tied_edge = t_team_any(edge, team);
          if (tl == 0) {
            if (a.out_isect) a.out_isect[row] = isect;
            if (a.out_level) a.out_level[row] = level;
            if (tied) knn_flag_tie(a.tie, a.tie_list, a.counters, slot, level, tied_edge ? 1 : 0);
            a.done[slot] = 1;
            isect_sum += (unsigned long long)isect;
          }
          max_level = max(max_level, level + 1);
          active = false;
        } else {
          level++;
          r = r * 2.0f;  // hostCode.cpp:321
          if (level >= a.max_rounds) {
            // out of rounds: the caller decides (allow_unfinished); the state says where it stopped
            if (tl == 0) {
              a.isect_sorted[slot] = isect;
              a.next_level[slot] = level;
              unfinished++;
            }
            max_level = max(max_level, level);
            active = false;
          }
        }
      }
    }
  }
  unsigned long long *st = a.counters + kStatBase + (blockIdx.x & (kStatStripes - 1)) * kStatStride;  // (my stripe: see kStatBase)
  t_add_stats(st, lane, max_level, node_tests, point_tests, isect_sum, levels_sum, unfinished);
  const unsigned long long fsum = t_wave_sum((unsigned long long)failed);
  if (lane == 0 && fsum) atomicAdd(&st[8], fsum);
}

// ---- exact-distance ties in the reference's order ---------------------------------------------------
// The reference's per-query lists persist over the rounds (deviceCode.cu:77-85 skips what is listed
// already, :116,:125 insert with a strict '<'): of two candidates at bit-identical fp32 distances the
// one that became a candidate in an EARLIER round stays ahead, whatever its index; inside one round
// the canonical order is by index (oracle/trueknn_oracle.c, decision 2).  The solve's kernels list by
// (dist, index) only -- the age would cost every insert a third key word -- and flag the rows where
// that can matter (a.tie).  Here a team redoes one flagged row with the full key (dist, first level,
// index): the first level of a candidate is the first radius of the doubling sequence whose box test
// it passes (the test is monotone in r).  Only neighbours within the row's k-th distance can be
// part of the answer, and that distance is already known (it does not depend on the order of ties):
// the walk prunes with it from the start, so a row costs a few wide nodes and leaf blocks.
// (The stack is the walk's: 6 KB of LDS per wave leaves room for 16 waves per CU; the ball pruning keeps stacks far below.)
struct HasTie {
  __host__ __device__ bool operator()(uint8_t t) const { return (t & 0x7f) != 0; }  // (bit 7 alone: team_pass's note, no flag)
};

template <bool HALO, int NREG>
__global__ void __launch_bounds__(kTeamBlock) tie_fix_kernel(TeamArgs a, const int32_t *slots, int32_t nslots) {
  // nslots < 0: `slots` is the kernels' own list (knn_flag_tie), as long as the device-side count says --
  // launched without the host knowing whether anything was flagged; nothing was: every wave leaves at once
  // nslots == -2: `slots` is a compacted list whose length hipCUB's select wrote to a.slot_count.  The host's
  // count of knn_flag_tie calls is only an upper bound of it (a wave-kernel solve that gives up on its
  // LDS stack is redone by the lane kernel, which flags the same rows a second time).
  if (nslots == -2)
    nslots = *a.slot_count;
  else if (nslots < 0)
    nslots = (int32_t)min(a.counters[kTieCounter], (unsigned long long)kTieListCap);
  if (nslots <= 0) return;
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[2][LBVH_WIDE_LEVELS];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  walk_fill_levels<2>(levels[0], a.wide, lane);
  t_wave_sync();
  unsigned int failed = 0, stood = 0;
  int turn_next = 0, turn_left = 0;  // (t_next_slots)
  for (;;) {
    const int base = t_next_slots(&a.counters[kTieCounter + 1], a.grab, lane, turn_next, turn_left);
    if (base >= nslots) break;
    bool active = base + team < nslots;
    const int32_t slot = active ? slots[base + team] : 0;
    const LbvhPoint q = a.bvh.points[slot];
    const int32_t row = a.bvh.prim_id[slot];
    const uint32_t tie_word = active ? (uint32_t)a.tie[slot] : 0u;
    active = active && (tie_word & 0x7fu) != 0u;  // a listed slot that is not flagged (any more) keeps its row
    const int level = active ? (int)(tie_word & 0x7fu) - 1 : 0;
    const float q_r0 = a.start_radii ? a.start_radii[row] : a.start_radius;
    float r = q_r0;
    for (int i = 0; i < level; i++) r = r * 2.0f;
    const WalkBox qb(q, r);
    uint32_t bd[NREG], bl[NREG], bi[NREG];
#pragma unroll
    for (int j = 0; j < NREG; j++) {
      bd[j] = 0x7f7fffffu;  // KNN_EMPTY_KEY = {FLT_MAX, 0}
      bl[j] = 0u;
      bi[j] = 0u;
    }
    // the row's k-th distance, if the caller asked for distances (else the gate closes as the list fills)
    float tau2 = INFINITY;
    if (active) {
      const int64_t last = (int64_t)row * a.k + (a.k - 1);
      if (a.out_dist)
        tau2 = knn_gate_from_worst(a.out_dist[last]);
      else if (a.out_fb)
        tau2 = knn_gate_from_worst(a.out_fb[last].dist);
    }
    // Every tie of the row between two WRITTEN entries (no `edge`): the row is in (distance, index) order already, which is the
    // full key's order unless two tied neighbours became candidates at different levels.  Look that up from the row -- two
    // points per tied pair -- before walking for it: the duplicates of a data set (taxi pick-ups at one street corner) tie in
    // every row that holds both, always at one level, and are most of what is flagged on such sets (10 M taxi-like points with
    // 5 % duplicates, k = 10: 0.78 M rows flagged, 2.5 of the solve's 13.1 ms in this pass before this check).
    if (!HALO && a.row_slot && __ballot(active && !(tie_word & 0x80u)) != 0ull) {
      bool differs = false;
      const bool look = active && !(tie_word & 0x80u);
      uint32_t rd[NREG], ri[NREG];
#pragma unroll
      for (int reg = 0; reg < NREG; reg++) {
        const int j = tl + 16 * reg;
        rd[reg] = 0xffffffffu;  // (no entry: never equal to a distance)
        ri[reg] = 0u;
        if (look && j < a.k) {
          const int64_t o = (int64_t)row * a.k + j;
          if (a.out_dist && a.out_idx) {
            rd[reg] = __float_as_uint(a.out_dist[o]);
            ri[reg] = (uint32_t)a.out_idx[o];
          } else if (a.out_fb) {
            rd[reg] = __float_as_uint(a.out_fb[o].dist);
            ri[reg] = (uint32_t)a.out_fb[o].ind;
          } else {
            differs = true;  // (indices without distances: nothing to compare)
          }
        }
      }
#pragma unroll
      for (int reg = 0; reg < NREG; reg++) {
        uint32_t pd = t_team_shr1(rd[reg]), pi = t_team_shr1(ri[reg]);
        if (reg > 0) {
          const uint32_t lane0 = tl == 0 ? 0xffffffffu : 0u;
          pd = (pd & ~lane0) | (t_dpp<0x121>(rd[reg - 1]) & lane0);
          pi = (pi & ~lane0) | (t_dpp<0x121>(ri[reg - 1]) & lane0);
        }
        const int j = tl + 16 * reg;
        if (look && j >= 1 && j < a.k && rd[reg] == pd) {
          if (ri[reg] >= (uint32_t)a.bvh.n || pi >= (uint32_t)a.bvh.n) {
            differs = true;
          } else {
            const LbvhPoint pa = a.bvh.points[a.row_slot[ri[reg]]], pb = a.bvh.points[a.row_slot[pi]];
            differs |= first_level(pa, q, q_r0, level) != first_level(pb, q, q_r0, level);
          }
        }
      }
      if (look && !t_team_any(differs, team)) {  // the row stands
        active = false;
        stood += tl == 0 ? 1u : 0u;
      }
    }
    bool overflow = false;
    unsigned long long node_tests = 0;  // (this pass reports no statistics)
    for (int tree = 0; tree < (HALO ? 2 : 1); tree++) {
      const LbvhWideView &wv = a.wide[tree];
      const LbvhView &tv = tree == 0 ? a.bvh : a.halo;
      if (tv.n <= 0 || wv.levels <= 0) continue;
      walk_tree<false>(
          levels[tree], wv, stack, kWalkStack, active, q, qb, team, tl, node_tests,
          // every box beyond the gate goes: nothing is counted here
          [&](const LbvhBox &bx, int32_t, int) { return !beyond_gate(box_min_dist2(bx, q), tau2); },
          [&](int32_t b, bool has_b) {
            LbvhPoint p;
            float d2;
            const unsigned long long in_m = walk_block_test(tv.points, b, has_b, tl, q, qb, p, d2);
            unsigned long long pm = in_m & __ballot(p.id != q.id) & __ballot(d2 <= tau2);
            if (pm) {
              const uint32_t key_d = __float_as_uint(knn_sqrt(d2));
              const uint32_t key_l = ((pm >> lane) & 1ull) ? first_level(p, q, q_r0, level) : 0u;
              const uint32_t key_i = (uint32_t)p.id;
              do {
                const uint32_t pending_mine = (uint32_t)(pm >> (team * 16)) & 0xffffu;
                const bool has = pending_mine != 0u;
                const int src = (team << 4) + (has ? __ffs((int)pending_mine) - 1 : 0);
                const uint32_t cd = t_lane_read(key_d, src), cl = t_lane_read(key_l, src), ci = t_lane_read(key_i, src);
                const uint64_t chi = ((uint64_t)cd << 32) | cl;
                const uint32_t lane0 = tl == 0 ? 0xffffffffu : 0u;
                uint32_t nd_[NREG], nl_[NREG], ni_[NREG];
#pragma unroll
                for (int j = 0; j < NREG; j++) {
                  uint32_t pd = t_team_shr1(bd[j]), pl = t_team_shr1(bl[j]), pi = t_team_shr1(bi[j]);
                  if (j > 0) {
                    pd |= t_dpp<0x121>(bd[j - 1]) & lane0;
                    pl |= t_dpp<0x121>(bl[j - 1]) & lane0;
                    pi |= t_dpp<0x121>(bi[j - 1]) & lane0;
                  }
                  const uint64_t cur_hi = ((uint64_t)bd[j] << 32) | bl[j], prev_hi = ((uint64_t)pd << 32) | pl;
                  const bool below_cur = (chi < cur_hi) | ((chi == cur_hi) & (ci < bi[j]));
                  const bool below_prev = (chi < prev_hi) | ((chi == prev_hi) & (ci < pi));
                  const bool take_prev = has & ((j > 0) | (tl != 0)) & below_prev;  // entry 0 has no entry before it
                  const bool take_c = has & below_cur;
                  nd_[j] = take_prev ? pd : (take_c ? cd : bd[j]);
                  nl_[j] = take_prev ? pl : (take_c ? cl : bl[j]);
                  ni_[j] = take_prev ? pi : (take_c ? ci : bi[j]);
                }
#pragma unroll
                for (int j = 0; j < NREG; j++) {
                  bd[j] = nd_[j];
                  bl[j] = nl_[j];
                  bi[j] = ni_[j];
                }
                pm &= ~__ballot(lane == src);
              } while (pm);
              tau2 = fminf(tau2, knn_gate_from_worst(t_kth_dist<NREG>(bd, a.k, team)));
            }
          },
          [] {}, overflow);
    }
    if (active && overflow) {
      failed += tl == 0 ? 1u : 0u;  // the row keeps its (dist, index) order; reported in tknnSolveInfo.tie_rows_left
    } else if (active) {
#pragma unroll
      for (int reg = 0; reg < NREG; reg++) {
        const int j = tl + 16 * reg;
        if (j >= a.k) continue;
        const int64_t o = (int64_t)row * a.k + j;
        const int32_t prim = knn_key_prim(((uint64_t)bd[reg] << 32) | bi[reg]);
        const float d = __uint_as_float(bd[reg]);
        if (a.out_idx) a.out_idx[o] = prim;
        if (a.out_dist) a.out_dist[o] = d;
        if (a.out_fb) {
          a.out_fb[o].ind = prim;
          a.out_fb[o].dist = d;
        }
      }
    }
  }
  const unsigned long long fsum = t_wave_sum((unsigned long long)failed);
  if (lane == 0 && fsum) atomicAdd(&a.counters[kTieCounter + 2], fsum);
  const unsigned long long ssum = t_wave_sum((unsigned long long)stood);
  if (lane == 0 && ssum) atomicAdd(&a.counters[kTieCounter + 3], ssum);
}

}  // namespace

// The team kernels' end-of-wave statistics live in stripes (kStatBase): zeroed before a launch of a walk (the packet kernel's
// prep launch does it itself), copied behind h_counters_[16] after it and folded once the stream is idle
void Engine::reset_stat_stripes(hipStream_t s) {
  OWLMI_HIP(hipMemsetAsync(counters_ + kStatBase, 0, kStatStripes * kStatStride * sizeof(unsigned long long), s));
}
void Engine::fetch_stat_stripes(hipStream_t s) {
  OWLMI_HIP(hipMemcpyAsync(h_counters_ + kHostStripes, counters_ + kStatBase, kStatStripes * kStatStride * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
}
KernelStats Engine::fold_stat_stripes(bool with_min) const {
  KernelStats sum;
  if (with_min) sum.first_handover_level = ~0ull;
  for (int j = 0; j < kStatStripes; j++) {
    const KernelStats st = KernelStats::from_words(h_counters_ + kHostStripes + j * kStatStride);
    sum.rounds = std::max(sum.rounds, st.rounds);
    sum.node_tests += st.node_tests;
    sum.point_tests += st.point_tests;
    sum.intersections += st.intersections;
    sum.flags |= st.flags;
    sum.active_rounds += st.active_rounds;
    sum.unfinished += st.unfinished;
    sum.handed_over += st.handed_over;
    if (with_min) sum.first_handover_level = std::min(sum.first_handover_level, st.first_handover_level);
  }
  return sum;
}

void Engine::reset_solve_state(int32_t *levels, hipStream_t s) {
  const int64_t n = bvh_.size();
  OWLMI_HIP(hipMemsetAsync(tie_, 0, (size_t)n, s));
  OWLMI_HIP(hipMemsetAsync(counters_, 0, kCounters * sizeof(unsigned long long), s));
  OWLMI_HIP(hipMemsetAsync(done_, 0, (size_t)n, s));
  OWLMI_HIP(hipMemsetAsync(isect_sorted_, 0, (size_t)n * sizeof(int64_t), s));
  OWLMI_HIP(hipMemsetAsync(next_level_, 0, (size_t)n * sizeof(int32_t), s));
  if (levels) OWLMI_HIP(hipMemsetAsync(levels, 0xff, (size_t)n * sizeof(int32_t), s));
}

TeamArgs Engine::team_args(const SolveArgs &sa) const {
  TeamArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.halo = halo_view();
  a.wide[0] = bvh_.wide_view();
  if (halo_count() > 0) a.wide[1] = halo_.wide_view();
  a.start_radius = sa.start_radius;
  a.start_radii = sa.d_start_radii;
  a.k = sa.k;
  a.out_idx = sa.d_idx;
  a.out_dist = sa.d_dist;
  a.out_fb = sa.d_fb;
  a.tie = tie_;
  a.tie_list = tie_list_;
  a.counters = counters_;
  return a;
}

void Engine::set_solve_args(TeamArgs &a, const SolveArgs &sa) const {
  a.max_rounds = sa.max_rounds;
  a.allow_unfinished = sa.allow_unfinished ? 1 : 0;
  a.out_isect = sa.d_isect;
  a.out_level = sa.d_levels;
  a.done = done_;
  a.skip = sa.phase ? boundary_ : nullptr;
  a.skip_is = sa.phase == 1 ? 1 : 0;
  a.isect_sorted = isect_sorted_;
  a.next_level = next_level_;
}

int32_t *Engine::compact_slots(bool ties, hipStream_t s) {
  const int64_t n = bvh_.size();
  int32_t *slots = slot_list(n), *d_count = slots + n;
  hipcub::CountingInputIterator<int32_t> iota(0);
  auto select = [&](const uint8_t *bytes, auto flag) {
    hipcub::TransformInputIterator<bool, decltype(flag), const uint8_t *> flags(bytes, flag);
    size_t tmp_bytes = 0;
    OWLMI_HIP(hipcub::DeviceSelect::Flagged(nullptr, tmp_bytes, iota, flags, slots, d_count, (int)n, s));
    OWLMI_HIP(hipcub::DeviceSelect::Flagged(workspace(tmp_bytes), tmp_bytes, iota, flags, slots, d_count, (int)n, s));
  };
  if (ties)
    select(tie_, HasTie{});
  else
    select(done_, NotDone{});
  return d_count;
}


void Engine::launch_tie_fix(const SolveArgs &sa, const int32_t *slots, int32_t nslots, int blocks, hipStream_t s, const int32_t *d_slot_count,
                            int64_t expected_rows) {
  TeamArgs a = team_args(sa);
  a.slot_count = d_slot_count;
  // (10 M taxi-like points, k = 10 / 24, 0.78 / 2.3 M rows, 24 workgroups per CU: turns of 4 / 8 / 12 / 24 / 32 slots 2.55 / 1.42 / 1.08 /
  // 0.89 / 0.94 ms and 7.2 / 3.8 / 2.6 / 1.81 / 1.85 ms; 64 and more slots a turn: the waves' own chains of loads show, 2.8 ms and up)
  a.grab = grab_for(expected_rows, blocks, 6, 6);
  const bool look = !ids_given_ && !(getenv("TKNN_TIE_LOOK") && !strcmp(getenv("TKNN_TIE_LOOK"), "0"));  // (TKNN_TIE_LOOK=0: A/B switch)
  a.row_slot = look ? bvh_.row_slot_device() : nullptr;
  using FixEntry = void (*)(TeamArgs, const int32_t *, int32_t);
  static const FixEntry entries[2][4] = {{tie_fix_kernel<false, 1>, tie_fix_kernel<false, 2>, tie_fix_kernel<false, 3>, tie_fix_kernel<false, 4>},
                                         {tie_fix_kernel<true, 1>, tie_fix_kernel<true, 2>, tie_fix_kernel<true, 3>, tie_fix_kernel<true, 4>}};
  const FixEntry entry = entries[halo_count() > 0 ? 1 : 0][nreg_for(sa.k) - 1];
  void *kargs[] = {(void *)&a, (void *)&slots, (void *)&nslots};
  OWLMI_HIP(hipLaunchKernel((const void *)entry, dim3(blocks), dim3(kTeamBlock), kargs, 0, s));
}

void Engine::fix_ties(const SolveArgs &sa, tknnSolveInfo *info, hipStream_t s) {
  if (ties_early_) {  // solve_team's own launch has seen them all
    if (early_tie_rows_ && getenv("TKNN_VERBOSE"))
      fprintf(stderr, "[ties] %lld rows redone in the reference's tie order: %.3f ms, %lld left\n", (long long)early_tie_rows_, early_tie_ms_, (long long)early_tie_left_);
    if (info) {
      info->tie_rows = early_tie_rows_;
      info->tie_rows_left = early_tie_left_;
      info->tie_ms = early_tie_ms_;
      info->solve_ms += early_tie_ms_;
    }
    return;
  }
  const int64_t n = bvh_.size();
  OWLMI_HIP(hipMemsetAsync(counters_ + kTieCounter + 1, 0, 3 * sizeof(unsigned long long), s));  // work cursor, rows left
  // First go: the kernels' own list, count read on the device -- no host round trip before the launch;
  // the usual handful of rows (or none) costs one small launch behind the solve.
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  launch_tie_fix(sa, tie_list_, -1, std::min(cu_count_ * 4, kTieListCap / 4), s);  // a team per listed row
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  OWLMI_HIP(hipMemcpyAsync(h_counters_, counters_ + kTieCounter, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  float ms = 0;
  OWLMI_HIP(hipEventElapsedTime(&ms, ev_a_, ev_b_));
  const int64_t flagged = (int64_t)h_counters_[0];
  if (flagged > kTieListCap) {
    // more than the list holds (quantised coordinates, lattices): all flagged slots, compacted from tie_
    // (rows redone twice come out the same: the gate is the row's k-th distance, which no order changes)
    const int32_t *d_count = compact_slots(/*ties=*/true, s);
    OWLMI_HIP(hipMemsetAsync(counters_ + kTieCounter + 1, 0, 3 * sizeof(unsigned long long), s));
    OWLMI_HIP(hipEventRecord(ev_a_, s));
    // the list's length is read on the device (d_count): `flagged` counts flag calls, an upper bound
    const int64_t rows = std::min<int64_t>(flagged, n);
    launch_tie_fix(sa, slot_list_, -2, (int)std::min<int64_t>((rows + 3) / 4, (int64_t)cu_count_ * 24), s, d_count, rows);
    OWLMI_HIP(hipEventRecord(ev_b_, s));
    OWLMI_HIP(hipMemcpyAsync(h_counters_, counters_ + kTieCounter, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
    float again = 0;
    OWLMI_HIP(hipEventElapsedTime(&again, ev_a_, ev_b_));
    ms += again;
  }
  if (flagged && getenv("TKNN_VERBOSE"))
    fprintf(stderr, "[ties] %lld rows redone in the reference's tie order: %.3f ms, %llu left (%llu stood after a look at the written row)\n", (long long)flagged, ms,
            h_counters_[2], h_counters_[3]);
  if (info) {
    info->tie_rows = flagged;
    info->tie_rows_left = (int64_t)h_counters_[2];
    info->tie_ms = ms;
    info->solve_ms += ms;
  }
}

// One query per team, each from the level its solve state holds: what exhausts its stack keeps that state untouched and goes
// on to lane rounds from lane_level
tknnSolveInfo Engine::walk(const SolveArgs &sa, TeamArgs a, int nreg, const int32_t *slots, int32_t nslots, int lane_level,
                           bool count_lane_launches, hipStream_t s) {
  using WalkEntry = void (*)(TeamArgs, const int32_t *, int32_t);
  static const WalkEntry walks[2][4] = {{team_walk_kernel<false, 1>, team_walk_kernel<false, 2>, team_walk_kernel<false, 3>, team_walk_kernel<false, 4>},
                                        {team_walk_kernel<true, 1>, team_walk_kernel<true, 2>, team_walk_kernel<true, 3>, team_walk_kernel<true, 4>}};
  OWLMI_HIP(hipMemsetAsync(counters_, 0, 16 * sizeof(unsigned long long), s));
  reset_stat_stripes(s);
  const int blocks = (int)std::min<int64_t>(((int64_t)nslots + 3) / 4, (int64_t)cu_count_ * kWalkBlocksPerCu);
  a.grab = 1;  // (queries differ too much for longer turns: measured, see TeamArgs::grab)
  void *kargs[] = {(void *)&a, (void *)&slots, (void *)&nslots};
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipLaunchKernel((const void *)walks[halo_count() > 0 ? 1 : 0][nreg - 1], dim3(blocks), dim3(kTeamBlock), kargs, 0, s));
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  fetch_stat_stripes(s);
  OWLMI_HIP(hipStreamSynchronize(s));
  const KernelStats st = fold_stat_stripes(false);
  float ms = 0;
  OWLMI_HIP(hipEventElapsedTime(&ms, ev_a_, ev_b_));
  tknnSolveInfo info = solve_info(st, sa.start_radius, TKNN_KERNEL_TEAM, 16 * nreg, ms);
  if (info.unfinished && !sa.allow_unfinished) throw RoundsExceeded{};
  if (st.handed_over) {
    if (sa.d_start_radii)
      throw ArgError{TKNN_E_UNSUPPORTED, "per-query start radii: a query's candidate walk outgrew the team walk's stack (the lane rounds that take over otherwise use one radius per launch)"};
    tknnSolveInfo rest;
    std::memset(&rest, 0, sizeof rest);
    continue_lane(sa, lane_level, &rest, s);
    merge_tail(info, rest, sa.start_radius, count_lane_launches);
  }
  return info;
}

}  // namespace owlmi
