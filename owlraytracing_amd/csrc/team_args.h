// team_args.h -- TeamArgs, the argument block of the team kernels, and the few constants more than one of their files needs:
// the packet kernel (trueknn_team.hip), the hand-over walk and the tie pass (trueknn_tail.hip), the k > 64 walk (trueknn_bigk.hip).
// Engine's members take and return a TeamArgs across those files (trueknn_engine.h), so it is not in an anonymous namespace.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "lbvh.h"
#include "owlknn.h"  // tknnNeigh

// Diagnostic build only (make DIAG=1 -> libowl_mi355x_diag.so, never the shipped library): lets
// scripts/diag_team.py price the phases by switching them off; results are wrong when any bit is set.
#ifndef TKNN_DIAG_BUILD
#define TKNN_DIAG_BUILD 0
#endif

namespace owlmi {

constexpr int kTeamBlock = 64;      // one wave per workgroup: LDS, not the block shape, limits residency
// slots (in fours) a wave takes per turn at the tie pass's work cursor (TeamArgs::grab): so many that a wave comes `turns` times in
// all, at most `cap`; TKNN_GRAB overrides (measurements)
inline int grab_for(int64_t count, int blocks, int turns, int cap) {
  if (const char *g = getenv("TKNN_GRAB")) return std::max(1, atoi(g));
  return (int)std::max<int64_t>(1, std::min<int64_t>(cap, count / ((int64_t)std::max(1, blocks) * 4 * turns)));
}
// list registers per lane for k: 16 entries each.  Three (k = 33 .. 48; round 4) spare those k the four-register
// instantiation's fourth merge step and its 13 granules of LDS (10 M uniform points: 22.2 -> 15.0 ms at k = 33, 14.2 -> 12.7 at k = 32)
#ifndef TKNN_NREG3
#define TKNN_NREG3 1
#endif
inline int nreg_for(int k) { return k <= 16 ? 1 : (k <= 32 ? 2 : (k <= 48 && TKNN_NREG3 ? 3 : 4)); }

// what every team kernel is launched with (Engine::team_args, Engine::set_solve_args)
struct TeamArgs {
  LbvhView bvh, halo;
  LbvhWideView wide[2];
  float start_radius;
  // per-query radius schedule (tknnSolveOptions.d_start_radii): per ROW the radius query `row` starts
  // with, or null -- then every query starts with start_radius, as in the reference (hostCode.cpp:185,325)
  const float *start_radii;
  int k;
  int max_rounds;
  int allow_unfinished;
  int first_step;  // levels the first gather of every packet serves (density estimate, 1..kMaxStep)
  int first_ext;   // ... and whether that gather also lists the blocks of the level after them (see the level loop)
  int merge_ext;   // ... and whether the step's SELECT pass serves that level, too (1; 0: in a turn of its own -- TKNN_TEAM_MERGE=0, measurements)
  int count_flat_max;  // a COUNT round whose longest list is at most this long (<= 12 blocks) has all its block loads in flight at once (team_pass)
  int lite;        // SELECT rounds whose queries all finish inside the step with <= 16 others take the pass's light path (1; 0: TKNN_TEAM_LITE=0, measurements and tests)
  float tie_span;  // sqrt(number of axes along which the points differ), rounded up: d <= tie_span * Chebyshev distance
  int diag;        // TKNN_DIAG_BUILD only: 1 skip inserts, 2 skip SELECT passes, 4 skip COUNT passes, 8 skip per-block query tests,
                   // 16 / 32 step and gather statistics (atomics: slow), 64 every block visit of a query reads its first listed block
  int32_t ngroups;
  int32_t *out_idx;
  float *out_dist;
  int64_t *out_isect;
  tknnNeigh *out_fb;
  int32_t *out_level;
  // continuation state for queries whose candidate lists outgrow the LDS lists (finished by the
  // lane kernel): per sorted slot, preset by the host to done=1
  uint8_t *done;
  int64_t *isect_sorted;
  int32_t *next_level;
  // per sorted slot: 1 + level (| 0x80: knn_flag_tie's `edge`) for rows that finished with bit-identical distances among entries
  // 0..k of the list (entry k: the best candidate left out); tie_fix_kernel redoes them in the reference's tie order
  uint8_t *tie;
  int32_t *tie_list;
  const uint8_t *skip;  // per sorted slot, or null: queries with skip[slot] == skip_is sit this solve out (tknnSolveOptions.phase)
  int32_t skip_is;
  const int32_t *slot_count;  // tie_fix_kernel, nslots == -2: length of `slots` as hipCUB's select wrote it (device side)
  // a wave takes 4 * grab consecutive slots per turn at the work cursor (>= 1).  One address, device scope: a turn costs some
  // 12 ns whoever asks -- at four rows a turn that was ALL of the tie pass on duplicate-heavy sets (10 M taxi-like points, k = 10 / 24:
  // 0.78 / 2.3 M rows in 2.5 / 7.2 ms; with longer turns 1.1 / 2.8 ms).  The walks keep 1: their queries differ too much in cost
  // (turns of up to 64 slots: the hand-over walk 4.0 -> 4.5 ms on that set, the k = 65 walk 173 -> 189 ms on 10 M uniform points).
  int grab;
  // tie_fix_kernel: the sorted slot of row i (Lbvh::row_slot_device), or null: no look at the written row first.  The look
  // turns a written neighbour into its point through this table, which is indexed by input ROW: right only where a point's
  // id is its row.  An engine built with ids (tknnBuildIds) names neighbours by the caller's id, so it gets null and every
  // flagged row is walked (an id below n would otherwise fetch some other point and let a wrongly ordered row stand).
  const int32_t *row_slot;
  // [0] (unused here) [kXcdCounter + 32 x] per-XCD packet counters [1] max levels [2] node tests [3] point tests [4] sum isect
  // [5] error flags (1 max_rounds) [6] sum levels [7] unfinished [8] handed over [9] min hand-over level
  unsigned long long *counters;
};

// The packet kernel's argument block for a PLAIN solve (team_kernel<..., PLAIN = true>, trueknn_team.hip): one own tree, k <= 16,
// rows into idx, dist and intersections, and nothing else -- no frame buffer, no per-query start radii, no levels, no phase, no
// halo tree, no measurement knob.  What such a solve never has is a constant of the type, under the name TeamArgs gives it: the
// kernel's text reads `a.out_fb`, `a.skip`, `a.lite` for both blocks, and for this one the compiler folds the test away with
// everything behind it.  What is left are the values the kernel reads, some 200 bytes against TeamArgs' 480: few enough that the
// pass loops need not fetch any of them from the argument segment again.
struct PlainTeamArgs {
  struct {
    const LbvhPoint *points;
    const int32_t *prim_id;
    int32_t n;
  } bvh;
  struct NoTree {
    static constexpr const LbvhPoint *points = nullptr;
    static constexpr int32_t n = 0;
  };
  static constexpr NoTree halo = {};
  LbvhWideView wide[1];  // (the pyramid's table is read whole, by level: the gather)
  float start_radius;
  static constexpr const float *start_radii = nullptr;
  int k;
  int max_rounds;
  int allow_unfinished;
  int first_step;
  int first_ext;
  static constexpr int merge_ext = 1;
  static constexpr int count_flat_max = 12;  // 4 * kCountFlatGroups (trueknn_team.hip asserts it)
  static constexpr int lite = 1;
  float tie_span;
  static constexpr int diag = 0;
  int32_t ngroups;
  int32_t *out_idx;  // the three of them: never null
  float *out_dist;
  int64_t *out_isect;
  static constexpr tknnNeigh *out_fb = nullptr;
  static constexpr int32_t *out_level = nullptr;
  uint8_t *done;
  int64_t *isect_sorted;
  int32_t *next_level;
  uint8_t *tie;
  int32_t *tie_list;
  static constexpr const uint8_t *skip = nullptr;
  static constexpr int32_t skip_is = 0;
  unsigned long long *counters;
};

// whether a solve with this (complete) block is a plain one as far as the block says: the caller adds what the block does not
// show -- that no measurement knob is set, and that k takes one list register
inline bool plain_team_solve(const TeamArgs &a) {
  return a.out_idx && a.out_dist && a.out_isect && !a.out_fb && !a.out_level && !a.start_radii && !a.skip && a.halo.n <= 0 && !a.halo.points &&
         a.merge_ext == PlainTeamArgs::merge_ext && a.lite == PlainTeamArgs::lite && a.count_flat_max == PlainTeamArgs::count_flat_max &&
         a.diag == PlainTeamArgs::diag;
}
// ... and the plain block of that solve: every field from the generic one, so the two cannot differ
inline PlainTeamArgs plain_team_args(const TeamArgs &a) {
  PlainTeamArgs p;
  p.bvh.points = a.bvh.points;
  p.bvh.prim_id = a.bvh.prim_id;
  p.bvh.n = a.bvh.n;
  p.wide[0] = a.wide[0];
  p.start_radius = a.start_radius;
  p.k = a.k;
  p.max_rounds = a.max_rounds;
  p.allow_unfinished = a.allow_unfinished;
  p.first_step = a.first_step;
  p.first_ext = a.first_ext;
  p.tie_span = a.tie_span;
  p.ngroups = a.ngroups;
  p.out_idx = a.out_idx;
  p.out_dist = a.out_dist;
  p.out_isect = a.out_isect;
  p.done = a.done;
  p.isect_sorted = a.isect_sorted;
  p.next_level = a.next_level;
  p.tie = a.tie;
  p.tie_list = a.tie_list;
  p.counters = a.counters;
  return p;
}
template <bool PLAIN>
using TeamArgsOf = std::conditional_t<PLAIN, PlainTeamArgs, TeamArgs>;

}  // namespace owlmi
