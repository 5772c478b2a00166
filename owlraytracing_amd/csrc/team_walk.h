// team_walk.h -- one 16-lane team's walk of the 64-ary box pyramid for ONE query, and the pieces around it, shared by the
// kernels that walk it: team_walk_kernel and tie_fix_kernel (trueknn_tail.hip), bigk_walk_kernel (trueknn_bigk.hip) and
// query_walk_kernel (trueknn_query.hip).  Four teams of a wave walk in lock step, so there is no __syncthreads, only t_wave_sync.  What a kernel
// does differently comes in as callables (the box rule, the block visitor, the end-of-chunk hook) or as template parameters;
// every function is inlined into its caller.  The box test, its margins and the counting rule below are what make rows equal
// the reference's bit for bit: they are written here once.
#pragma once
#include "knn_thresholds.h"  // knn_gate_from_worst
#include "owlknn.h"  // tknnNeigh
#include "team_lanes.h"

namespace owlmi {

namespace {

constexpr int kWalkStack = 384;  // stack entries per team: up to 63 siblings wait on each of <= 6 levels (6 KB of LDS per wave)
#ifndef TKNN_MERGE_AT
#define TKNN_MERGE_AT 12  // buffered candidates of some team at the end of a group of four blocks that trigger a merge
#endif

// ---- the level table -----------------------------------------------------------------------------------------------------
struct WalkLevel {  // per tree and pyramid level, in LDS: lanes of different teams are at different levels
  const LbvhBox *boxes;
  int32_t count;
  int32_t pad_;
};
// levels[t * LBVH_WIDE_LEVELS + l] of trees t < TREES, by the first lanes of the wave; the caller's t_wave_sync follows
template <int TREES>
__device__ __forceinline__ void walk_fill_levels(WalkLevel *levels, const LbvhWideView *wide, int lane) {
  if (lane < TREES * LBVH_WIDE_LEVELS) {
    const int t = lane / LBVH_WIDE_LEVELS, l = lane % LBVH_WIDE_LEVELS;
    levels[lane].boxes = wide[t].level[l];
    levels[lane].count = wide[t].count[l];
  }
}

// ---- the query box of one radius level ---------------------------------------------------------------------------------
struct WalkBox {
  float r;
  float mg;                // the rounding margin M of the box test
  float in_below, in_upto;  // Chebyshev distance <= in_below: certainly a candidate; > in_upto: certainly none
  // boxes that can hold a candidate meet [q - r - 2M, q + r + 2M]; every point of a box inside
  // [q - r + 2M, q + r - 2M] certainly is one
  float rl, rs;
  __device__ __forceinline__ WalkBox(const LbvhPoint &q, float r_) : r(r_) {
    mg = (fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fabsf(q.z)) + 2.0f * r) * 4.76837158203125e-07f;  // 2^-21
    in_below = r - mg, in_upto = r + mg;
    rl = r + 2.0f * mg, rs = r - 2.0f * mg;
  }
};
__device__ __forceinline__ float box_min_dist2(const LbvhBox &bx, const LbvhPoint &q) {
  const float gx = fmaxf(fmaxf(bx.lo[0] - q.x, q.x - bx.hi[0]), 0.f), gy = fmaxf(fmaxf(bx.lo[1] - q.y, q.y - bx.hi[1]), 0.f),
              gz = fmaxf(fmaxf(bx.lo[2] - q.z, q.z - bx.hi[2]), 0.f);
  return (gx * gx + gy * gy) + gz * gz;  // <= every point's squared distance, up to rounding
}
// beyond the gate: nothing in the box can be listed (0.999995: roundings of m2 and of the points' distance arithmetic)
__device__ __forceinline__ bool beyond_gate(float m2, float tau2) { return m2 * 0.999995f > tau2; }

// The box rule of the kernels that count candidates: a child box inside the part of the query's box where the candidate test
// is certain, and beyond the list's gate, is COUNTED (its points are consecutive sorted slots: the count is arithmetic, into
// `part`) instead of walked.  `c`: the child's index at level `lvl`; clean_end: the tree's slots before its NaN points.
__device__ __forceinline__ bool walk_count_box(const LbvhBox &bx, const LbvhPoint &q, const WalkBox &qb, float tau2, int32_t c, int lvl,
                                               int32_t clean_end, uint32_t &part) {
  const bool inside = (bx.lo[0] >= q.x - qb.rs) & (bx.hi[0] <= q.x + qb.rs) & (bx.lo[1] >= q.y - qb.rs) & (bx.hi[1] <= q.y + qb.rs) &
                      (bx.lo[2] >= q.z - qb.rs) & (bx.hi[2] <= q.z + qb.rs);
  if (inside) {
    const float m2 = box_min_dist2(bx, q);
    const int64_t span = (int64_t)LBVH_BLOCK << (6 * lvl);  // points under one child of this level
    const int64_t first = (int64_t)c * span;
    if (beyond_gate(m2, tau2) && first + span <= (int64_t)clean_end) {
      part += (uint32_t)span;
      return true;
    }
  }
  return false;
}

// ---- the descent of one tree -------------------------------------------------------------------------------------------
// The team's 16 lanes test 16 child boxes of a wide node at a time, the four chunks of a node loaded at once, and push the
// children that overlap the query's box and that keep_box(bx, c, lvl) keeps on the team's LDS stack (`capacity` entries of
// (lvl << 26) | child); a kept child of level 0 is a leaf block: visit_block(b, has_b) runs for one of them at a time with the
// lanes as the block's 16 points (has_b: my team has a block in this step), and after_chunk() once the blocks of a chunk are
// through.  ROLLED: the chunk loop is not unrolled and picks its box by selects, not by an index (for a visitor too large to
// have four times).  `overflow` is set if the stack overflowed for my team: its walk then is incomplete.  (A reference, not the
// return value: one flag over both trees of a halo walk instead of two that are or-ed saves these kernels, which sit at the
// 128-register cap, up to 48 bytes of scratch per lane.)
// stop() is asked after every node; a team for which it holds (the same in its 16 lanes) drops what is left on its stack and is
// through -- the early exit of a walk that looks for one witness (nms.hip).  The default never stops.
struct WalkNoStop {
  __device__ __forceinline__ bool operator()() const { return false; }
};
template <bool ROLLED, class BoxRule, class BlockVisitor, class ChunkEnd, class Stop = WalkNoStop>
__device__ __forceinline__ void walk_tree(const WalkLevel *levels, const LbvhWideView &wv, int32_t *stack, int capacity, bool active,
                                          const LbvhPoint &q, const WalkBox &qb, int team, int tl, unsigned long long &node_tests,
                                          BoxRule keep_box, BlockVisitor visit_block, ChunkEnd after_chunk, bool &overflow, Stop stop = Stop{}) {
  const int top = wv.levels;
  int sp = 0;
  if (active) {
    if (tl == 0) stack[0] = (top << 26) | 0;  // virtual root above the top level
    sp = 1;
  }
  t_wave_sync();
  while (__ballot(sp > 0) != 0ull) {
    const bool work = sp > 0;
    const int32_t e = work ? stack[sp - 1] : (1 << 26);
    if (work) sp--;
    const int lvl = (e >> 26) - 1;  // level of the children
    const int32_t first_child = (e & 0x3ffffff) * 64;
    const WalkLevel wl = levels[lvl];
    // the virtual root has the top level's few boxes as its children
    const int32_t nchild = lvl == top - 1 ? (first_child == 0 ? wl.count : 0) : wl.count;
    LbvhBox bx4[4];  // the node's 64 child boxes, all four loads in flight at once
#pragma unroll
    for (int chunk = 0; chunk < 4; chunk++) {
      const int32_t c = first_child + 16 * chunk + tl;
      bx4[chunk] = LbvhBox{{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
      if (work && c < nchild) bx4[chunk] = wl.boxes[c];
    }
    auto one_chunk = [&](int chunk, const LbvhBox &bx) __attribute__((always_inline)) {
      const int32_t c = first_child + 16 * chunk + tl;
      const bool valid = work && c < nchild;
      const bool ov = valid & (bx.lo[0] <= q.x + qb.rl) & (bx.hi[0] >= q.x - qb.rl) & (bx.lo[1] <= q.y + qb.rl) &
                      (bx.hi[1] >= q.y - qb.rl) & (bx.lo[2] <= q.z + qb.rl) & (bx.hi[2] >= q.z - qb.rl);
      node_tests += valid ? 1u : 0u;
      const bool keep = ov && keep_box(bx, c, lvl);
      const uint32_t keep_mine = (uint32_t)(__ballot(keep) >> (team * 16)) & 0xffffu;
      if (lvl > 0) {
        if (sp + __popc(keep_mine) > capacity) {
          overflow = true;
        } else {
          if (keep) stack[sp + __popc(keep_mine & ((1u << tl) - 1u))] = (lvl << 26) | c;
          sp += __popc(keep_mine);
        }
      } else {
        // children are leaf blocks: lanes become the 16 points of one block at a time
        uint32_t todo = keep_mine;
        while (__ballot(todo != 0u) != 0ull) {
          const bool has_b = todo != 0u;
          const int32_t b = first_child + 16 * chunk + (has_b ? __ffs((int)todo) - 1 : 0);
          todo &= todo - 1u;
          visit_block(b, has_b);
        }
        after_chunk();
      }
    };
    if constexpr (ROLLED) {
#pragma unroll 1
      for (int chunk = 0; chunk < 4; chunk++) {
        LbvhBox bx = bx4[0];
#pragma unroll
        for (int u = 1; u < 4; u++)
          if (chunk == u) bx = bx4[u];
        one_chunk(chunk, bx);
      }
    } else {
#pragma unroll
      for (int chunk = 0; chunk < 4; chunk++) one_chunk(chunk, bx4[chunk]);
    }
    if (stop()) sp = 0;
    t_wave_sync();
  }
}

// ---- the block test ----------------------------------------------------------------------------------------------------
// Lane tl takes point tl of block `b` (the sorted arrays are padded with NaN sentinels to whole blocks: lbvh.hip; no block:
// the sentinel) and tests it against the query's box at this level: a Chebyshev distance up to in_below certainly passes, one
// beyond in_upto certainly does not, knn_in_box -- the literal test -- decides the few in between.  Returns the wave's mask of
// candidates; p and d2: my point and its squared distance.
__device__ __forceinline__ unsigned long long walk_block_test(const LbvhPoint *points, int32_t b, bool has_b, int tl, const LbvhPoint &q,
                                                               const WalkBox &qb, LbvhPoint &p, float &d2) {
  p = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
  if (has_b) p = points[(int64_t)b * LBVH_BLOCK + tl];
  const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
  const float t = has_b ? fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz)) : __uint_as_float(0x7fc00000u);
  unsigned long long in_m = __ballot(t <= qb.in_below);
  const unsigned long long maybe_m = __ballot(t <= qb.in_upto) & ~in_m;
  if (maybe_m) in_m |= maybe_m & __ballot(knn_in_box(p.x, p.y, p.z, qb.r, q.x, q.y, q.z));
  d2 = t_dist2(dx, dy, dz);
  return in_m;
}

// ---- the smaller pieces ------------------------------------------------------------------------------------------------
// distance of entry k - 1 of my team's list (register j of lane t holds entry 16 j + t), in every lane
template <int NREG>
__device__ __forceinline__ float t_kth_dist(const uint32_t (&bd)[NREG], int k, int team) {
  uint32_t reg = bd[0];
#pragma unroll
  for (int j = 1; j < NREG; j++) reg = ((k - 1) >> 4) == j ? bd[j] : reg;
  return __uint_as_float(t_lane_read(reg, (team << 4) + ((k - 1) & 15)));
}
// registers per lane of a team's list of k <= 64 entries (host side: which instantiation of a walk kernel serves k)
inline int query_nreg(int k) { return k <= 16 ? 1 : (k <= 32 ? 2 : (k <= 48 ? 3 : 4)); }
// min over the 16 lanes of my team, result in every lane of the team
__device__ __forceinline__ uint32_t t_team_min_u32(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x128 /*row_ror:8*/, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x124 /*row_ror:4*/, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x122 /*row_ror:2*/, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x121 /*row_ror:1*/, 0xf, 0xf, false));
  return v;
}
// key word between distance and index: the level at which the candidate was first one -- the first radius of the doubling
// sequence from q_r0 whose box test it passes (the test is monotone in r), `level` at the latest
__device__ __forceinline__ uint32_t first_level(const LbvhPoint &p, const LbvhPoint &q, float q_r0, int level) {
  float rr = q_r0;
  for (int l = 0; l < level; l++) {
    if (knn_in_box(p.x, p.y, p.z, rr, q.x, q.y, q.z)) return (uint32_t)l;
    rr = rr * 2.0f;
  }
  return (uint32_t)level;
}
// Does a finished row depend on how bit-identical distances are ordered?  The list holds (dist, index) order; the reference's
// is (dist, first level, index): they differ only where two tied candidates can have become candidates at different levels
// (tie_may_straddle; r0, r: the query's first and last radius).  Per lane and for the entries where `look` holds: `tie` -- my
// entry ties with the one before it, or (lane 15 of a full list) with left_out, the smallest key any merge left out, team
// minimum taken; `edge` -- that tie is with a candidate that is not written: entry k, or the one left out (knn_flag_tie).
template <int NREG>
__device__ __forceinline__ void t_row_ties(const uint32_t (&bd)[NREG], uint32_t left_out, bool full, int k, int tl, const LbvhPoint &q, float r0,
                                           float r, float span, bool look, bool &tie, bool &edge) {
  tie = false, edge = false;
  const float qmax = fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fabsf(q.z));
#pragma unroll
  for (int reg = 0; reg < NREG; reg++) {
    uint32_t before = t_team_shr1(bd[reg]);
    if (reg > 0) before |= t_dpp<0x121>(bd[reg - 1]) & (tl == 0 ? 0xffffffffu : 0u);
    bool t = ((reg > 0) | (tl >= 1)) & (16 * reg + tl <= k) & (bd[reg] == before);
    const bool out_t = reg == NREG - 1 && full && tl == 15 && left_out == bd[reg];
    t |= out_t;
    t = t && look && tie_may_straddle(__uint_as_float(bd[reg]), r0, r, qmax, span);
    tie |= t;
    edge |= t && (16 * reg + tl == k || out_t);
  }
}
// whether any lane of my team has `v`
__device__ __forceinline__ bool t_team_any(bool v, int team) { return ((uint32_t)(__ballot(v) >> (team * 16)) & 0xffffu) != 0u; }

// entry j of a finished row of k, at o = row * k + j, into the arrays the caller asked for; the tknnNeigh record is the
// reference's frame buffer: the row's count and intersections sit in its entry 0
__device__ __forceinline__ void t_write_entry(int32_t *out_idx, float *out_dist, tknnNeigh *out_fb, int64_t o, int32_t prim, float d, int j,
                                              int k, int64_t isect) {
  if (out_idx) out_idx[o] = prim;
  if (out_dist) out_dist[o] = d;
  if (out_fb) {
    tknnNeigh ev;
    ev.ind = prim;
    ev.dist = d;
    ev.numNeighbors = j == 0 ? 0 : k;
    ev.pad_ = 0;
    ev.intersections = j == 0 ? isect : 0;
    out_fb[o] = ev;
  }
}

// The next four slots of my wave at a work cursor: a wave takes 4 * grab slots per turn at the cursor (one atomic; see
// TeamArgs::grab) and hands them out four at a time.  turn_next, turn_left: wave-uniform, zero at the start.
__device__ __forceinline__ int t_next_slots(unsigned long long *cursor, int grab, int lane, int &turn_next, int &turn_left) {
  if (turn_left == 0) {
    int got = 0;
    if (lane == 0) got = (int)atomicAdd(cursor, 4ull * (unsigned long long)max(grab, 1));
    turn_next = __builtin_amdgcn_readfirstlane(got);
    turn_left = max(grab, 1);
  }
  const int base = turn_next;
  turn_next += 4;
  turn_left--;
  return base;
}

// a wave's counters, summed over its lanes (point_tests: per lane and block step), into the statistics stripe `st` of its
// workgroup (kStatBase, knn_device.h)
__device__ __forceinline__ void t_add_stats(unsigned long long *st, int lane, int max_level, unsigned long long node_tests,
                                            unsigned long long point_tests, unsigned long long isect_sum, unsigned long long levels_sum,
                                            unsigned int unfinished) {
  const unsigned long long isum = t_wave_sum(isect_sum), lsum = t_wave_sum(levels_sum), nt = t_wave_sum(node_tests),
                           pt = t_wave_sum(point_tests) * LBVH_BLOCK / 16, usum = t_wave_sum((unsigned long long)unfinished);
  const int ml = (int)t_wave_max((float)max_level);
  if (lane == 0) {
    atomicMax(&st[1], (unsigned long long)ml);
    atomicAdd(&st[2], nt);
    atomicAdd(&st[3], pt);
    atomicAdd(&st[4], isum);
    atomicAdd(&st[6], lsum);
    if (usum) atomicAdd(&st[7], usum);
  }
}

}  // namespace

}  // namespace owlmi
