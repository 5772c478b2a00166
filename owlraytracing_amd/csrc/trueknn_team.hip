// trueknn_team.hip -- the team TrueKNN kernel (TKNN_KERNEL_TEAM), k <= 64 (k > 16: two list registers per lane, k > 32: four).
//
// The wave-packet kernel (trueknn_wave.hip) broadcasts every candidate of a 64-query packet to all
// 64 lanes; on MI355X it is VALU-issue-bound with ~2.5 % useful lanes (profiles/r01_wave_v2_*),
// because the packet's candidate union is ~40x one query's own box content.  This kernel turns
// the work around: a wave is FOUR TEAMS OF 16 LANES; a team handles one query at a time and its
// lanes are the 16 CANDIDATES of one leaf block (LBVH_BLOCK consecutive curve-sorted points,
// one coalesced 256-byte read) of that query's OWN block list.
//
// Per packet of 64 curve-consecutive queries and per radius level (hostCode.cpp:285-340 rounds):
//   1. lanes = queries: LDS query records and conservative query boxes for the gather.
//   2. lanes = child boxes: the wave walks the 64-ary block pyramid (LbvhWideView) depth-first
//      with an LDS stack, one wide node per step, against the union box of the packet.
//   3. every surviving leaf block is tested against the 64 individual query boxes
//      (lanes = queries again, block box broadcast by v_readlane); blocks some query needs are
//      appended to the packet's block list and to the per-query lists of byte slots (no atomics).
//   4. COUNT pass, teams over the compacted list of active queries: count candidates in the
//      query's box (deviceCode.cu:74) and those other than the query itself (:103).
//   5. queries with >= k others are finished at this level (deviceCode.cu:118): SELECT pass,
//      teams over the compacted list of finishing queries: distances, gate, and a team-parallel
//      sorted insert -- lane j of the team holds the j-th best (dist,index) key; a new key is
//      broadcast to the team and every lane decides locally whether it keeps, takes the key, or
//      takes its left neighbour's entry (DPP row shift).  Rows are written straight from the
//      team: lane j stores neighbour j (coalesced 4*k bytes per array).
// Results are bit-identical to the other kernels: the candidate test is the literal one wherever a
// cheap bound cannot decide it (see the record layout below), same distance arithmetic, keys ordered
// by (dist, index).
#include "knn_thresholds.h"  // knn_gate_from_worst
#include "team_args.h"
#include "team_lanes.h"
#include "team_walk.h"
#include "trueknn_engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace owlmi {

namespace {

// leaf blocks one packet may need per level.  A per-query list names them by byte slots: 256 -- except with four list
// registers per lane (k > 48), where the lists of the last level outgrow that (10 M uniform points at k = 64: 36 % of the queries
// were handed to the team walk, two thirds of the solve): 512, the ninth bit of a slot in a word of its own
// (four words per query)
#ifndef TKNN_MAX_BLOCKS_3
#define TKNN_MAX_BLOCKS_3 256
#endif
#ifndef TKNN_MAX_BLOCKS_4
#define TKNN_MAX_BLOCKS_4 512
#endif
constexpr int max_blocks(int nreg) { return nreg == 4 ? TKNN_MAX_BLOCKS_4 : (nreg == 3 ? TKNN_MAX_BLOCKS_3 : 256); }
#ifndef TKNN_MAX_PER_QUERY
#define TKNN_MAX_PER_QUERY 72  // (k <= 16)
#endif
// leaf blocks one query may need per level, by the number of list registers per lane (k <= 16 / 32 / 48 / 64).  LDS is
// allocated in granules of 1 280 bytes, 128 of them per CU (lds_workgroups_per_cu below), so the sizes are chosen by the granule:
//   1: 72 slots (lists of the benchmark run to 60)             10 192 bytes = 8 granules, 16 waves per CU (the register limit)
//   2, 3: 88 slots                                             11 472 bytes = 9 granules, 14 waves
//         (round 4; 96 slots = 10 granules = 12 waves cost 10 % at k = 17 .. 44 on uniform, mixture and taxi-like sets of
//         10 M points; 72 would hand over a third of the queries of the uniform set at k = 32, 88 none)
//   4: 124 slots and 512 blocks per packet                     16 400 bytes = 13 granules, 9 waves
//         (round 4: with 256 blocks and 96 slots 36 % of the queries of 10 M uniform points were handed over at k = 64;
//         116 slots and 384 blocks = 12 granules = 10 waves: the packet kernel 8 % faster, the hand-overs eat it)
#ifndef TKNN_MAX_PER_QUERY_2
#define TKNN_MAX_PER_QUERY_2 88
#endif
#ifndef TKNN_MAX_PER_QUERY_3
#define TKNN_MAX_PER_QUERY_3 88
#endif
#ifndef TKNN_MAX_PER_QUERY_4
#define TKNN_MAX_PER_QUERY_4 124
#endif
constexpr int max_per_query(int nreg) {
  return nreg == 1 ? TKNN_MAX_PER_QUERY : (nreg == 4 ? TKNN_MAX_PER_QUERY_4 : (nreg == 3 ? TKNN_MAX_PER_QUERY_3 : TKNN_MAX_PER_QUERY_2));
}
// One-wave workgroups of `lds` bytes a CU holds at once: LDS is allocated in granules of 1 280 bytes (measured:
// scripts/microbench/lds_granule.hip, profiles/r04_lds_granule.txt -- the residency of a launch steps at every multiple of 1 280
// bytes, hipOccupancyMaxActiveBlocksPerMultiprocessor divides by the byte and says 13 where 12 fit)
inline int lds_workgroups_per_cu(size_t lds) {
  const size_t granule = 1280, total = 160 * 1024;  // gfx950
  return lds ? (int)((total / granule) / ((lds + granule - 1) / granule)) : 1 << 20;
}
#ifndef TKNN_SORT_FIRST
#define TKNN_SORT_FIRST 1  // k <= 16: 1 = sort the query's own block on the spot instead of buffering its candidates
#endif
#ifndef TKNN_TEAM_WAVES
#define TKNN_TEAM_WAVES 4  // waves per SIMD the packet kernel's register allocation aims at
#endif
// the per-XCD packet counters: 256 bytes apart, behind the kCounters words (the words RT-DBSCAN stripes its statistics over: not in
// use during a solve).  Side by side in one cache line (round 3: counters[16 + x]) their atomics -- one per packet, 156 000 per launch
// of the benchmark -- queued at one place (see TeamArgs::grab for what a turn at one address costs)
constexpr int kXcdCounter = kDbStats, kXcdCounterStride = 32;
// ... and the packet kernel's end-of-wave statistics: five atomics per wave on one cache line, 20 000 at the end of a launch of the
// benchmark, cost it 0.10 of 6.6 ms (measured by leaving them out).  Striped over the workgroups, a cache line per stripe (the layout
// is kStatBase .. in knn_device.h: behind RT-DBSCAN's words), folded by the host (Engine::fold_stat_stripes)
// (kStatStripes, kStatStride, kStatBase: knn_device.h)
constexpr int kTeamStack = 192;     // wide-pyramid stack entries per wave
constexpr int kQrecStride = 6;      // floats per LDS query record (layout below)
constexpr int kScanBudget = 16384;  // leaf blocks one packet-level may test against its queries before it is handed over
constexpr int kMaxStep = 2;          // radius levels one gather may serve (the count slots and the inner-box test assume <= 2)
constexpr int kCountFlatGroups = 3;  // groups of four blocks a COUNT round may have in flight at once (team_pass's flat path)
// LDS per wave: query records | block list | per-query block lists | counts, query list / stack.
// The pyramid stack is live only during the gather, the counts and the query list only during the
// passes, so they share one region.  Every KB counts: LDS, not registers, limits residency.
constexpr int kLdsQrec = 64 * kQrecStride * 4;
constexpr int kLdsCnt = 64 * 2 * 4;  // per query: candidates at the inner level, at the outer level | self << 31
constexpr int kLdsList = 64 * 4 + 16;  // + the bucket-presence word of the list builder
constexpr int kLdsStack = kTeamStack * 4;
constexpr int kLdsShared = (kLdsCnt + kLdsList) > kLdsStack ? (kLdsCnt + kLdsList) : kLdsStack;
constexpr int kLdsSharedPadded = (kLdsShared + 15) & ~15;  // the entry lists are read 16 bytes at a time
constexpr int kCandCap = kCandCapacity;
// LDS per wave, by the number of list registers per lane: query records | block list | per-query block lists |
// counts, query list / pyramid stack | per-team entry lists | per-team candidate buffers
template <int NREG>
struct TeamLayout {
  static constexpr int kMaxPerQuery = max_per_query(NREG);
  static constexpr int kMaxBlocks = max_blocks(NREG);
  static constexpr int kLdsBlk = kMaxBlocks * 4;
  static constexpr int kLdsMask = 64 * kMaxPerQuery;  // per-query lists of block slots (bytes)
  static constexpr int kHiWords = kMaxBlocks > 256 ? (kMaxPerQuery + 31) / 32 : 0;  // per query: the slots' ninth bits
  static constexpr int kLdsHi = 64 * kHiWords * 4;
  // per team: the block entries of the query it serves, resolved and in visit order (+ 4: a pass
  // prefetches one group of four past the end of a list rounded up to whole groups)
  static constexpr int kEntStride = kMaxPerQuery + 4;
  static constexpr int kLdsEnt = 4 * kEntStride * 4;
  static constexpr int kLdsCand = 4 * kCandCap * 8;
  static constexpr int kOffMask = kLdsQrec + kLdsBlk;
  static constexpr int kOffHi = kOffMask + kLdsMask;
  static constexpr int kOffShared = kOffHi + kLdsHi;
  static constexpr int kOffEnt = kOffShared + kLdsSharedPadded;
  static constexpr int kOffCand = kOffEnt + kLdsEnt;
  static constexpr int kTeamLds = kOffCand + kLdsCand;
  static_assert(kEntStride % 4 == 0 && kOffEnt % 16 == 0, "entry lists must be 16-byte aligned");
  static_assert(kLdsMask % 4 == 0, "the ninth bits are words");
  static_assert(kMaxPerQuery <= 124 && kMaxPerQuery / 4 < 32, "list-length buckets of the pass lists are one bit each of a 32-bit word");
};

// LDS query record: [0..2] q, [3] id, [4] radius of the box the pass works in (outermost level of
// the step for COUNT, the finishing level for SELECT), [5] packed: #blocks | position of the query's
// own block in its list << 8.  (The margin of the fast box test and the query's row are recomputed /
// re-read by the passes: 512 bytes of LDS decide between 15 and 16 waves per CU.)
//
// The candidate test (deviceCode.cu:38-56: fl(c-r) <= q <= fl(c+r) per axis) is done in two tiers.
// With t = max |fl(c_a - q_a)| over the axes (the differences the distance needs anyway) and the
// margin M = 2^-21 (max_a |q_a| + 2r):  t <= r - M proves the literal test true, t > r + M (or t
// NaN) proves it false -- the rounding of fl(c-r), fl(c+r) and fl(c-q) is below 2^-23 (|q| + 2r),
// an eighth of M -- and only candidates inside that 2M band (about 1e-4 of them) run the literal
// test.  Three instructions instead of stored per-axis thresholds, and 2.5 KB less LDS per wave.
struct TeamLds {
  float *qrec;        // [64][kQrecStride]
  int32_t *blk;       // [kMaxBlocks] block entries of the packet (bit 31: halo tree)
  uint8_t *qblk;      // [64][kMaxPerQuery] per-query slots into blk[]
  uint32_t *qhi;      // [64][kHiWords] (k > 32) bit p of a query's words: the ninth bit of the slot at position p of its list
  uint32_t *qcnt;     // [64][2] out: candidates in the inner box, in the outer box | self << 31
  int32_t *qlist;     // compact list of the queries this pass serves
  int32_t *ent;       // [4][kEntStride] per team: resolved block entries of its query, in visit order
  unsigned long long *cand;  // [4][kCandCap] per team: keys waiting to be merged into its list
};

// a value the compiler takes as it is from here on (it cannot make it again from where it came from)
// (through a vector register and back: the compiler takes what an asm statement leaves in a scalar register for a per-lane value)
__device__ __forceinline__ uint32_t t_hold_word(uint32_t w) {
  asm volatile("" : "+v"(w));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)w);
}
template <class T>
__device__ __forceinline__ void t_hold(T &v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "a word or a pointer");
  uint32_t w[sizeof(T) / 4];
  memcpy(w, &v, sizeof(T));
  for (size_t i = 0; i < sizeof(T) / 4; i++) w[i] = t_hold_word(w[i]);
  memcpy(&v, w, sizeof(T));
}

// my lane, as a value the compiler cannot tell from a new one: what is made from it is made where it is used, not carried there
__device__ __forceinline__ int t_lane_again(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

// what the plain kernel holds for its passes (team_kernel); the generic kernel: nothing, its passes read the argument block
template <bool PLAIN>
struct TeamHeld {};
template <>
struct TeamHeld<true> {
  int32_t *out_idx;
  float *out_dist;
  int64_t *out_isect;
  uint8_t *tie;  // (and the start radius: read where a row has ties that may span two levels -- rare, but inside the SELECT rounds)
  float start_radius;
  int k;
};

template <bool PLAIN>
__device__ __forceinline__ int team_k(const TeamArgsOf<PLAIN> &a, const TeamHeld<PLAIN> &held) {
  if constexpr (PLAIN)
    return held.k;
  else
    return a.k;
}

// One pass of the four teams over a compact list of queries.  SELECT = false: count candidates
// (deviceCode.cu:74,103).  SELECT = true: also keep the k best (dist,index) keys, lane j of the
// team holding the j-th, and write the row if the query turns out finished (>= k others).
// NREG: list registers per lane -- the team's sorted list holds 16 * NREG keys (k <= 16: 1, k <= 32: 2, k <= 64: 4)
// TWO: a COUNT pass that also counts the inner box of a two-level step (a template flag: as a run-time value the
// compiler kept "m > 1" as a lane mask and re-derived a branch from it for every block)
// PLAIN: the argument block is PlainTeamArgs (team_args.h) -- what a plain solve never has is a constant of that type, and its
// three result arrays are there
template <bool SELECT, bool HALO, int NREG, bool FULL, bool TWO, bool PLAIN = false>
__device__ __forceinline__ void team_pass(const TeamArgsOf<PLAIN> &a, const TeamHeld<PLAIN> &held, const TeamLds &L, int n_list, int32_t first_slot,
                                          const LbvhPoint *own_pts, const LbvhPoint *halo_pts, int lane) {
  const int team = lane >> 4, tl = lane & 15;
  constexpr int kMaxPerQuery = TeamLayout<NREG>::kMaxPerQuery, kEntStride = TeamLayout<NREG>::kEntStride;
  static_assert(!(SELECT && TWO), "only a COUNT pass serves two levels");
#define TEAM_K team_k<PLAIN>(a, held)  // (and the row's arrays below: held by the plain kernel, arguments of the generic one)
  n_list = __builtin_amdgcn_readfirstlane(n_list);  // wave-uniform by construction; says so to the compiler (scalar branches on it)
  [[maybe_unused]] unsigned long long tp[4] = {0, 0, 0, 0};  // TKNN_DIAG_BUILD, flag 128: setup | first group | other groups | epilogue
  for (int r0 = 0; r0 < n_list; r0 += 4) {
    [[maybe_unused]] unsigned long long tp_mark = 0;
    if (TKNN_DIAG_BUILD && (a.diag & 128)) tp_mark = __builtin_amdgcn_s_memtime();
#define TP_LAP(i)                                                     \
  do {                                                                \
    if (TKNN_DIAG_BUILD && (a.diag & 128)) {                          \
      const unsigned long long now_ = __builtin_amdgcn_s_memtime();   \
      tp[i] += now_ - tp_mark;                                        \
      tp_mark = now_;                                                 \
    }                                                                 \
  } while (0)
    const bool on = r0 + team < n_list;
    int qi = 0;
    if (on) qi = L.qlist[r0 + team];
    // (SELECT, k <= 16) bit 8 of the entry: a light query -- it finishes inside the step with at most sixteen others in its
    // box (exact from COUNT), on a front list of at most a.count_flat_max blocks; see the light round below
    bool lite_q = false;
    if (SELECT && NREG == 1) {
      lite_q = (qi >> 8) != 0;
      qi &= 0xff;
    }
    if (TKNN_DIAG_BUILD && SELECT && (a.diag & 128)) {  // SELECT rounds, their queries, the light ones among them
      const unsigned long long q_m = __ballot(on && tl == 0), l_m = __ballot(on && tl == 0 && lite_q);
      if (lane == 0) {
        atomicAdd(&a.counters[18], 1ull);
        atomicAdd(&a.counters[19], (unsigned long long)__popcll(q_m));
        atomicAdd(&a.counters[20], (unsigned long long)__popcll(l_m));
      }
    }
    const float *rec = L.qrec + qi * kQrecStride;
    const float t_qx = rec[0], t_qy = rec[1], t_qz = rec[2];
    const int32_t t_qid = __float_as_int(rec[3]);
    const float t_r = rec[4];
    const float t_mg = (fmaxf(fmaxf(fabsf(t_qx), fabsf(t_qy)), fabsf(t_qz)) + 2.0f * t_r) * 4.76837158203125e-07f;  // 2^-21, see above
    const float in_below = t_r - t_mg, in_upto = t_r + t_mg;          // certainly / possibly a candidate
    // the inner level of a two-level COUNT step: half my outer radius (exact: radii double in fp32).  Not a pass
    // argument: with a per-query schedule every query has radii of its own.
    const float r_inner = t_r * 0.5f;
    const float i0_below = r_inner - t_mg, i0_upto = r_inner + t_mg;
    uint32_t cnt_i0 = 0;  // inner level of a two-level COUNT step (m = levels served by this gather, wave-uniform)
    const int packed = __float_as_int(rec[5]);
    // the query's output row, read at set-up: a load in flight over the whole round instead of a round trip to memory
    // between the last block and the row's stores (-1.4 % on the benchmark)
    [[maybe_unused]] int32_t out_row = 0;
    if (SELECT) out_row = a.bvh.prim_id[first_slot + qi];
    const int my_n = on ? (packed & 0xff) : 0;  // leaf blocks of my team's query
    // wave-uniform trip count: longest list of the 4 teams -- from v_readlane values only, so that the
    // compiler keeps it (and the loop tests below) in scalar registers
    const int steps = max(max((int)__builtin_amdgcn_readlane(my_n, 0), (int)__builtin_amdgcn_readlane(my_n, 16)),
                          max((int)__builtin_amdgcn_readlane(my_n, 32), (int)__builtin_amdgcn_readlane(my_n, 48)));
    if (TKNN_DIAG_BUILD && (a.diag & 16) && lane == 0) atomicAdd(&a.counters[15], (unsigned long long)steps);
    // my query's block entries, spread over the team's lanes: lane tl holds entries tl, tl+16, ...
    // (clamped to the last one; teams without a query read block 0 of the own tree and ignore it)
    const uint8_t *mine = L.qblk + qi * kMaxPerQuery;
    const int last = my_n - 1;
    // positions past the end of my list (and teams without a query) name the all-NaN block after
    // the own tree's last block: its points fail every test, so the loop needs no "am I still in
    // my list" check
    const int32_t nan_block = a.wide[0].count[0];
    // SELECT visits blocks outward from the query's own block, alternating sides of its curve-ordered
    // list: near blocks first tightens the k-th-distance gate early (about 30 % fewer inserts than
    // list order on uniform data) and changes nothing else -- the result does not depend on order.
    // COUNT takes the list as it is.
    // A list that serves the level AFTER the step it was gathered for (see team_kernel) is "the step's blocks in curve
    // order, then the rest": outward order inside the first part (bits 16..23 of the record; 0: the whole list), the
    // rest as listed -- farther than every block of the first part anyway.
    const int own_pos = (packed >> 8) & 0xff;
    const int n_near = (packed >> 16) & 0xff;
    const int last_near = n_near ? n_near - 1 : last;
    const int both = min(own_pos, last_near - own_pos);
    const bool right_longer = last_near - own_pos > own_pos;
    auto list_pos = [&](int it) -> int {
      if (!SELECT) return it;
      const int half = (it + 1) >> 1;
      const int alt = (it & 1) ? half : -half;  // it = 0: own block
      const int far = it - both;
      const int off = it <= 2 * both ? alt : (right_longer ? far : -far);
      return it > last_near ? it : own_pos + off;
    };
    auto list_entry = [&](int pos) -> int32_t {
      int lp = list_pos(pos);
      if (n_near && lp >= n_near) lp = kMaxPerQuery - 1 - (lp - n_near);  // the back part, filled downwards
      const int at = min(max(lp, 0), kMaxPerQuery - 1);
      int slot_at = mine[at];
      if (TeamLayout<NREG>::kHiWords) slot_at |= (int)((L.qhi[qi * TeamLayout<NREG>::kHiWords + (at >> 5)] >> (at & 31)) & 1u) << 8;
      int32_t e = L.blk[slot_at];
      if (TKNN_DIAG_BUILD && (a.diag & 64)) e = L.blk[mine[0]];  // every visit reads one and the same block: what do cache misses cost?
      return resolve_entry<HALO>(pos <= last ? e : nan_block);
    };
    // The team's entries go to LDS once, resolved (byte offsets) and in visit order, lane tl writing
    // positions tl, tl + 16, ...; the loop below then fetches four of them with ONE 16-byte LDS read per
    // team (same address in the team's 16 lanes) -- no cross-lane read, no select, no address
    // arithmetic per block.  Positions up to the longest list rounded up to whole groups of four, plus
    // one group of prefetch, name the all-NaN block.
    const int steps4 = (steps + 3) & ~3;
    int32_t *my_ent = L.ent + team * kEntStride;
    // A LIGHT round: every team with a query serves a light one (the pass list has them first: build_qlist) and the longest
    // list has at most a.count_flat_max (<= 12) blocks.  Wave-uniform.  Its entries are the list as it is, as COUNT's: a light
    // query has no back part, nothing is gated, so the order of the visits buys nothing.  One store per lane: sixteen entries
    // are the at most twelve blocks and the group of prefetch behind them (the all-NaN block).
    const bool lite_round = SELECT && NREG == 1 && steps <= a.count_flat_max && __ballot(on && !lite_q) == 0ull;
    if (lite_round) {
      static_assert(4 * kCountFlatGroups + 4 <= 16, "one entry per lane of the team, the group of prefetch included");
      int32_t e = L.blk[mine[tl]];
      if (TKNN_DIAG_BUILD && (a.diag & 64)) e = L.blk[mine[0]];
      my_ent[tl] = resolve_entry<HALO>(tl <= last ? e : nan_block);
    } else {
      for (int base = 0; base < steps4 + 4; base += 16)
        if (base + tl < kEntStride) my_ent[base + tl] = list_entry(base + tl);
    }
    t_wave_sync();
    uint32_t cnt = 0;
    uint32_t bd[NREG], bi[NREG];  // register j of lane t holds list entry 16 j + t (indices are compile-time: stays in VGPRs)
#pragma unroll
    for (int j = 0; j < NREG; j++) {
      bd[j] = 0x7f7fffffu;  // KNN_EMPTY_KEY = {FLT_MAX, 0}
      bi[j] = 0u;
    }
    // k == list size: the smallest distance (bits) among the keys that found no room, tracked in the lane
    // of the last entry -- equal to the k-th distance iff a candidate tied with the row's last stayed out
    // (FULL is a template parameter: as a run-time flag the three instructions it adds to an insert
    // were if-converted into every k's loop, +4 % on the benchmark)
    constexpr bool full = FULL;
    uint32_t left_out = 0xffffffffu;
    // the k-th best of my team, whose distance gates further candidates
    auto kth_dist = [&]() -> float {
      uint32_t reg = bd[0];
#pragma unroll
      for (int j = 1; j < NREG; j++) reg = ((TEAM_K - 1) >> 4) == j ? bd[j] : reg;
      return __uint_as_float(t_lane_read(reg, (team << 4) + ((TEAM_K - 1) & 15)));
    };
    float tau2 = INFINITY;
    // Candidates that pass the gate wait in the team's LDS buffer and are merged into the sorted list sixteen at a time
    // (t_merge_rows).  Between merges the gate is the last merge's k-th distance: looser than it could be, never wrong.
    bool dirty = false;  // wave-uniform: some team has buffered candidates
    // how many wait in my team's buffer (the same in its sixteen lanes).  In a register, advanced by population counts of the
    // candidate mask: the slot of a candidate used to come from an LDS atomic -- a round trip through the LDS pipe in the
    // middle of every block step that had a candidate, in a kernel that is bound by the latency of such chains
    uint32_t fill_n = 0;
    auto merge_buffer = [&]() {
      t_wave_sync();
      t_merge_rows<NREG>(bd, bi, left_out, full, L.cand + team * kCandCap, fill_n, tl);
      t_wave_sync();  // (the rows are read: the next candidates may overwrite them)
      fill_n = 0;
      dirty = false;
      tau2 = knn_gate_from_worst(kth_dist());
    };
    // one block's test.  The candidate test in two tiers (see the record layout above): outside the
    // band |t - r| <= M the comparison t <= r IS the literal test; inside it (about 1e-6 of the points,
    // every point of a face-aligned lattice) the literal test runs.  The band check is one subtraction,
    // one compare and a branch that is almost never taken -- lane predicates cost a compare (twice a
    // plain VALU instruction on gfx950) and every wave-mask operation a slot of the CU's one scalar
    // pipe, which this kernel fills as much as the vector pipes (scripts/microbench/issue_rate.hip).
    auto in_box = [&](const LbvhPoint &p, float t, float radius, float below, float upto) -> unsigned long long {
      // certainly in | possibly in: two compares against the band's edges (no subtraction); they differ for a point in a
      // thousand blocks, and only then does the literal test run
      unsigned long long in_m = __ballot(t <= below);
      const unsigned long long maybe = __ballot(t <= upto);
      if (__builtin_expect(maybe != in_m, 0)) in_m |= maybe & __ballot(knn_in_box(p.x, p.y, p.z, radius, t_qx, t_qy, t_qz));
      return in_m;
    };
    auto process = [&](const LbvhPoint &p, bool own_block = false) {
      const float dx = p.x - t_qx, dy = p.y - t_qy, dz = p.z - t_qz;
      // NaN only if all three are (sentinels; lbvh.hip turns a point with any NaN coordinate into one)
      const float t = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
      const unsigned long long in_m = in_box(p, t, t_r, in_below, in_upto);
      cnt = t_count_keep(cnt, in_m, p.id);
      if (TWO) cnt_i0 = t_count(cnt_i0, in_box(p, t, r_inner, i0_below, i0_upto));
      if (SELECT) {
        const float d2 = t_dist2(dx, dy, dz);
        // candidates that pass the gate.  The query itself sits in its own block, which SELECT visits
        // first and settles in the sorted first step, so no block seen here can hold it (ids are unique).
        unsigned long long pm = in_m & __ballot(d2 <= tau2);
        if (own_block) pm &= __ballot(p.id != t_qid);  // deviceCode.cu:103: a query is no neighbour of itself (ids are unique: only its own block holds it)
        if (TKNN_DIAG_BUILD && (a.diag & 1)) pm = 0;
        if (pm) {
          if (TKNN_DIAG_BUILD && (a.diag & 16) && lane == 0) atomicAdd(&a.counters[26], (unsigned long long)__popcll(pm));
          // my candidate into the team's buffer; a full row of sixteen is merged at once (a block
          // adds at most sixteen to at most fifteen: the buffer holds 32)
          const uint32_t mine16 = (uint32_t)(pm >> (team << 4)) & 0xffffu;  // my team's lanes with a candidate
          if ((mine16 >> tl) & 1u) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)p.id;  // (the root: merge_buffer)
            L.cand[team * kCandCap + fill_n + __popc(mine16 & ((1u << tl) - 1u))] = key;
          }
          fill_n += __popc(mine16);
          dirty = true;
          if (__ballot(fill_n >= 16u) != 0ull) {
            if (TKNN_DIAG_BUILD && (a.diag & 16) && lane == 0) atomicAdd(&a.counters[27], 1ull);
            merge_buffer();
          }
        }
      }
    };
    // A ring of four block buffers: while one block is tested the next three are in flight, and the
    // NEXT group's four entries are read from LDS a whole group ahead.  Loads are unconditional and
    // consumed in strict rotation (the compiler's s_waitcnt vmcnt(N) then counts exactly); whole groups
    // only: positions past a list's end are the all-NaN block, whose points fail every test.
    const LbvhPoint *own_base = a.bvh.points;  // wave-uniform
    const uint32_t lane_bytes = (uint32_t)tl * (uint32_t)sizeof(LbvhPoint);
    typedef int32_t t_int4 __attribute__((ext_vector_type(4)));
    const t_int4 *my_groups = (const t_int4 *)my_ent;
    // A block in flight is ONE 128-bit value (x, y, z, id bits): carried through the loop as a vector, it stays
    // in the register tuple the load writes.  As four scalars the compiler narrows the COUNT pass's loads
    // to three words and copies them into other registers at the loop's back edge -- which waits for
    // every load in flight.
    auto fetch = [&](int32_t entry) -> t_point4 {
      const LbvhPoint p = load_block_point<HALO>(own_pts, halo_pts, entry, own_base, lane_bytes);
      return t_point4{p.x, p.y, p.z, __int_as_float(p.id)};
    };
    auto unpack = [](const t_point4 &v) -> LbvhPoint { return LbvhPoint{v.x, v.y, v.z, __float_as_int(v.w)}; };
    auto sort_first = [&](const LbvhPoint &p) {
      // The first block (the query's own) meets an empty list: every candidate in it would be inserted,
      // one lock-step round each.  Instead the team SORTS its 16 keys (non-candidates = the empty key)
      // with a bitonic network written so that every exchange keeps the smaller key in the lower lane:
      // mirror within 2, 4, 8, 16 lanes followed by xor 4 / 2 / 1 steps -- ten exchanges of two
      // cross-lane moves (DPP quad permutes and mirrors, one ds_swizzle) and a 64-bit compare each.
      const float dx = p.x - t_qx, dy = p.y - t_qy, dz = p.z - t_qz;
      const float t = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
      bool in = t <= t_r;
      if (__ballot(fabsf(t - t_r) <= t_mg) != 0ull) in = (t <= in_below) || ((t <= in_upto) && knn_in_box(p.x, p.y, p.z, t_r, t_qx, t_qy, t_qz));
      cnt = t_count(cnt, __ballot(in));
      bool cand = in && (p.id != t_qid);
      if (TKNN_DIAG_BUILD && (a.diag & 1)) cand = false;
      // (the squares go through the team's candidate buffer, empty at this point, so that the sorted lanes can fetch them)
      const uint32_t d2_bits = __float_as_uint(t_dist2(dx, dy, dz));
      unsigned long long *my_buf = L.cand + team * kCandCap;
      my_buf[tl] = ((unsigned long long)d2_bits << 32) | (uint32_t)p.id;
      t_wave_sync();
      t_sorted_row(d2_bits, (uint32_t)p.id, cand, tl, [&](int from) { return my_buf[from]; }, bd[0], bi[0]);
      t_wave_sync();  // (read: the first candidates may overwrite them)
      tau2 = knn_gate_from_worst(kth_dist());  // k > 16: the second register is still empty, the gate stays open
    };
    TP_LAP(0);
    // A COUNT round of at most a.count_flat_max blocks (its longest list; 73 % of the benchmark's rounds have at most 8, 99 % at
    // most 12) is no loop at all: the loads of ALL its whole groups are issued, then the blocks are tested in order.  A group's
    // test is 60 to 90 instructions, far less than one trip to the L2, and the ring below keeps one group in flight ahead: a round
    // of two or three groups waits two or three memory latencies one after the other where this path waits one.  Straight-line
    // code per number of groups -- no back edge to carry buffers over, every s_waitcnt counts exactly, no group past the list's
    // end is loaded -- and the pass has the registers: no list, no keys, no merge.  Whole 16-byte points as in the ring: loads
    // of the three words the count reads measured the same mean and three times the spread (profiles/count_flat_ab.json).
    if (lite_round) {
      // SELECT for queries whose boxes hold at most sixteen others, all of them on a short list: every point in the box
      // but the query itself is a neighbour, so nothing can be pruned -- no gate, no own block first, no merge while the
      // round runs.  Every candidate goes to the team's buffer (at most sixteen arrive: COUNT has counted them with this
      // very test on these very blocks), and ONE sort makes the list.  The query is told from its neighbours by its id on
      // every block: in list order its own block is anywhere.
      auto lite_test = [&](const LbvhPoint &p) {
        const float dx = p.x - t_qx, dy = p.y - t_qy, dz = p.z - t_qz;
        const float t = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
        const unsigned long long in_m = in_box(p, t, t_r, in_below, in_upto);
        cnt = t_count_keep(cnt, in_m, p.id);
        const float d2 = t_dist2(dx, dy, dz);
        unsigned long long pm = in_m & __ballot(p.id != t_qid);  // deviceCode.cu:103
        if (TKNN_DIAG_BUILD && (a.diag & 1)) pm = 0;
        if (pm) {
          const uint32_t mine16 = (uint32_t)(pm >> (team << 4)) & 0xffffu;
          if ((mine16 >> tl) & 1u) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)p.id;
            // (masked: whatever the counts say, a slot lies inside the team's buffer)
            L.cand[team * kCandCap + ((fill_n + __popc(mine16 & ((1u << tl) - 1u))) & (uint32_t)(kCandCap - 1))] = key;
          }
          fill_n += __popc(mine16);
        }
      };
      // Loads as the ring below has them, four blocks in flight and the next group's entries read a group ahead (positions past
      // the list's end name the all-NaN block): the registers of the ring, which is what SELECT has to spare -- eight or twelve
      // blocks in flight, as in COUNT's flat path, spilled the level loop's registers around both passes and cost the ordinary
      // rounds 4 % (profiles/HISTORY.md).
      {
        t_point4 b0, b1, b2, b3;
        {
          const t_int4 g = my_groups[0];
          b0 = fetch(g.x);
          b1 = fetch(g.y);
          b2 = fetch(g.z);
          b3 = fetch(g.w);
        }
        for (int it = 0; it < steps; it += 4) {
          const t_int4 g = my_groups[(it >> 2) + 1];  // entries it+4 .. it+7
          lite_test(unpack(b0));
          b0 = fetch(g.x);
          lite_test(unpack(b1));
          b1 = fetch(g.y);
          lite_test(unpack(b2));
          b2 = fetch(g.z);
          lite_test(unpack(b3));
          b3 = fetch(g.w);
          TP_LAP(it == 0 ? 1 : 2);
        }
      }
      // the list: the buffered keys, sorted (t_merge_rows' first half: there is no list to merge them into), empty keys
      // in the lanes past the last.  The buffer is next written after the following round's set-up has synchronised.
      t_wave_sync();
      const unsigned long long *my_buf = L.cand + team * kCandCap;
      const bool have = (uint32_t)tl < fill_n;
      const unsigned long long key = have ? my_buf[tl] : 0ull;
      t_sorted_row((uint32_t)(key >> 32), (uint32_t)key, have, tl, [&](int from) { return my_buf[from]; }, bd[0], bi[0]);
      if (TKNN_DIAG_BUILD && (a.diag & 128)) {
        const unsigned long long served = __ballot(on && tl == 0);
        if (lane == 0) {
          atomicAdd(&a.counters[16], 1ull);                                    // light rounds
          atomicAdd(&a.counters[17], (unsigned long long)__popcll(served));  // ... and the queries they served
        }
      }
      TP_LAP(2);
    } else if (!SELECT && steps <= a.count_flat_max) {
      auto flat = [&](auto groups_c) {
        constexpr int kBlocks = 4 * decltype(groups_c)::value;
        LbvhPoint c[kBlocks];  // (indices are compile-time: registers)
#pragma unroll
        for (int j = 0; j < kBlocks; j += 4) {
          const t_int4 g = my_groups[j >> 2];
          c[j + 0] = load_block_point<HALO>(own_pts, halo_pts, g.x, own_base, lane_bytes);
          c[j + 1] = load_block_point<HALO>(own_pts, halo_pts, g.y, own_base, lane_bytes);
          c[j + 2] = load_block_point<HALO>(own_pts, halo_pts, g.z, own_base, lane_bytes);
          c[j + 3] = load_block_point<HALO>(own_pts, halo_pts, g.w, own_base, lane_bytes);
        }
        __builtin_amdgcn_sched_barrier(0);  // (every load before the first test)
#pragma unroll
        for (int j = 0; j < kBlocks; j++) {
          process(c[j]);
          if (j == 3) TP_LAP(1);
        }
        if (kBlocks > 4) TP_LAP(2);
      };
      if (steps > 8)
        flat(std::integral_constant<int, 3>{});
      else if (steps > 4)
        flat(std::integral_constant<int, 2>{});
      else if (steps > 0)
        flat(std::integral_constant<int, 1>{});
    } else {
      t_point4 b0, b1, b2, b3;
      {
        // issued in ring order (the scheduler would reorder four independent loads, and the loop's
        // s_waitcnt vmcnt(N) is the minimum over the orders it can be entered with)
        const t_int4 g = my_groups[0];
        b0 = fetch(g.x);
        __builtin_amdgcn_sched_barrier(0);
        b1 = fetch(g.y);
        __builtin_amdgcn_sched_barrier(0);
        b2 = fetch(g.z);
        __builtin_amdgcn_sched_barrier(0);
        b3 = fetch(g.w);
        __builtin_amdgcn_sched_barrier(0);
      }
      for (int it = 0; it < steps; it += 4) {
        const t_int4 g = my_groups[(it >> 2) + 1];  // entries it+4 .. it+7
        if (SELECT && it == 0) {
          // the query's own block meets an empty list.  k <= 16: its candidates simply are the first into the team's
          // buffer, sorted by the first merge; larger k: sorted on the spot (sort_first), the other blocks insert one by one
          if (NREG == 1 && TKNN_SORT_FIRST == 0)
            process(unpack(b0), true);
          else
            sort_first(unpack(b0));
        } else {
          process(unpack(b0));
        }
        b0 = fetch(g.x);
        process(unpack(b1));
        b1 = fetch(g.y);
        process(unpack(b2));
        b2 = fetch(g.z);
        process(unpack(b3));
        b3 = fetch(g.w);
        // a tighter gate for the next group as soon as a handful of candidates wait (the first groups, whose
        // blocks lie next to the query, bring most of them)
        if (SELECT && dirty && __ballot(fill_n >= (uint32_t)TKNN_MERGE_AT) != 0ull) {
          if (TKNN_DIAG_BUILD && (a.diag & 16) && lane == 0) atomicAdd(&a.counters[27], 1ull);
          merge_buffer();
        }
        TP_LAP(it == 0 ? 1 : 2);
      }
    }  // the ring
    if (SELECT && dirty) {
      if (TKNN_DIAG_BUILD && (a.diag & 16) && lane == 0) atomicAdd(&a.counters[27], 1ull);
      merge_buffer();
    }
    if (SELECT && full) {
      // the smallest key left out by any merge, where the tie test below looks for it: lane 15
      uint32_t v = left_out;
      v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x128 /*row_ror:8*/, 0xf, 0xf, false));
      v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x124 /*row_ror:4*/, 0xf, 0xf, false));
      v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x122 /*row_ror:2*/, 0xf, 0xf, false));
      v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x121 /*row_ror:1*/, 0xf, 0xf, false));
      left_out = v;
    }
    cnt = t_team_sum(cnt);
    const uint32_t self = cnt ? 1u : 0u;  // a query lies in its own box, and ids are unique
    const uint32_t others = cnt - self;
    if (TWO) cnt_i0 = t_team_sum(cnt_i0);
    uint32_t tied = 0u;
    if (SELECT) {
      // entry j against entry j - 1, for j = 1..k (KList::has_ties is the per-lane form of this)
      bool tie[NREG];
      bool any = false;
#pragma unroll
      for (int j = 0; j < NREG; j++) {
        uint32_t before = t_team_shr1(bd[j]);
        if (j > 0) before |= t_dpp<0x121>(bd[j - 1]) & (tl == 0 ? 0xffffffffu : 0u);
        tie[j] = ((j > 0) | (tl >= 1)) & (16 * j + tl <= TEAM_K) & (bd[j] == before);
        if (full && j == NREG - 1) tie[j] |= (tl == 15) & (left_out == bd[j]);
        any |= tie[j];
      }
      if (__ballot(any) != 0ull) {  // rare: does any of them span two rounds?
        const float qmax = fmaxf(fmaxf(fabsf(t_qx), fabsf(t_qy)), fabsf(t_qz));
        any = false;
        bool edge = false;
        float q_r0;
        if constexpr (PLAIN)
          q_r0 = held.start_radius;
        else
          q_r0 = a.start_radii ? a.start_radii[a.bvh.prim_id[first_slot + qi]] : a.start_radius;
#pragma unroll
        for (int j = 0; j < NREG; j++) {
          const bool t = tie[j] && tie_may_straddle(__uint_as_float(bd[j]), q_r0, t_r, qmax, a.tie_span);
          any |= t;
          // ... with a candidate that is not written: entry k of a list with room to spare, the best one left out of a full list
          edge |= t && (16 * j + tl == TEAM_K || (full && j == NREG - 1 && tl == 15 && left_out == bd[j]));
        }
        // (said to knn_flag_tie through the flag byte itself, here in the rare branch: a second bit through the passes' count
        // words and the level loop moved the packet kernel's register allocation -- 0.6 % of the benchmark)
        if (on && edge) {
          if constexpr (PLAIN)
            knn_note_tie_edge(held.tie, first_slot + qi);
          else
            knn_note_tie_edge(a.tie, first_slot + qi);
        }
      }
      tied = ((uint32_t)(__ballot(any) >> (team * 16)) & 0xffffu) ? 1u : 0u;
    }
    if (on && tl == 0) {
      // counts innermost level first; a one-level pass fills slot 0
      uint32_t *out = L.qcnt + qi * 2;
      if (!TWO) {
        out[0] = cnt;
        out[1] = (self << 31) | (tied << 30);
      } else {
        out[0] = cnt_i0;
        out[1] = cnt | (self << 31);
      }
    }
    if (SELECT) {
      // finished at this level (deviceCode.cu:118: k insertions happened): lane j < k stores neighbour j.
      // The query's own lane adds the intersection count and the level afterwards (team_kernel).
      if (on && others >= (uint32_t)TEAM_K) {
#pragma unroll
        for (int reg = 0; reg < NREG; reg++) {
          const int j = tl + 16 * reg;  // my entry of this register
          if (j >= TEAM_K) continue;
          const int64_t o = (int64_t)out_row * TEAM_K + j;
          const int32_t prim = knn_key_prim(((uint64_t)bd[reg] << 32) | bi[reg]);
          const float d = __uint_as_float(bd[reg]);
          if constexpr (PLAIN) {
            held.out_idx[o] = prim;
            held.out_dist[o] = d;
          } else {
            if (a.out_idx) a.out_idx[o] = prim;
            if (a.out_dist) a.out_dist[o] = d;
          }
          if (a.out_fb) {
            // slot 0 of the row: everything but `intersections`, which only the query's lane writes
            int2 *rec8 = (int2 *)(a.out_fb + o);
            rec8[0] = make_int2(prim, __float_as_int(d));
            rec8[1] = make_int2(j == 0 ? 0 : TEAM_K, 0);
            if (j != 0) {
              // (a zero made here: as a constant the compiler keeps the pair in registers over the whole kernel, spills it,
              // and reloads it from scratch at this point of the pass loop)
              int zero;
              asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
              rec8[2] = make_int2(zero, zero);
            }
          }
        }
      }
    }
    TP_LAP(3);
  }
#undef TP_LAP
  if (TKNN_DIAG_BUILD && (a.diag & 128) && lane == 0)
    for (int i = 0; i < 4; i++) atomicAdd(&a.counters[(SELECT ? 36 : 28) + i], tp[i]);  // (32..34: the tie pass)
}

template <bool HALO, int NREG, bool FULL, bool PLAIN = false>
__global__ void __launch_bounds__(kTeamBlock) __attribute__((amdgpu_waves_per_eu(TKNN_TEAM_WAVES))) team_kernel(TeamArgsOf<PLAIN> a) {
  static_assert(!PLAIN || (!HALO && NREG == 1), "the plain kernel: one own tree, k <= 16");
  static_assert(PlainTeamArgs::count_flat_max == 4 * kCountFlatGroups, "a plain solve's flat COUNT rounds are the generic solve's");
  // The plain kernel reads what its pass loops need from the argument segment ONCE and holds it: an argument is a value the
  // compiler may fetch again wherever it runs short of scalar registers, and it did -- the row's two pointers before every row's
  // stores, a scalar load and its wait at the end of every SELECT round.  (The generic kernel reads its block as ever.)
  TeamHeld<PLAIN> held;
  if constexpr (PLAIN) {
    held.out_idx = a.out_idx, held.out_dist = a.out_dist, held.out_isect = a.out_isect, held.tie = a.tie;
    held.start_radius = a.start_radius, held.k = a.k;
    t_hold(held.out_idx);
    t_hold(held.out_dist);
    t_hold(held.out_isect);
    t_hold(held.tie);
    t_hold(held.start_radius);
    t_hold(held.k);
  }
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;  // 0 with one wave per workgroup
  const int tl = lane & 15;
  using Lay = TeamLayout<NREG>;
  constexpr int kMaxPerQuery = Lay::kMaxPerQuery;
  unsigned char *base = smem + wid * Lay::kTeamLds;
  float *qrec = (float *)base;
  int32_t *blk = (int32_t *)(base + kLdsQrec);
  uint8_t *qblk = (uint8_t *)(base + Lay::kOffMask);  // [query][kMaxPerQuery] slots into blk[]
  uint32_t *qhi = (uint32_t *)(base + Lay::kOffHi);    // [query][kHiWords] their ninth bits (k > 32)
  constexpr int kMaxBlocks = Lay::kMaxBlocks;
  uint32_t *qcnt = (uint32_t *)(base + Lay::kOffShared);
  int32_t *qlist = (int32_t *)(base + Lay::kOffShared + kLdsCnt);
  int32_t *stack = (int32_t *)(base + Lay::kOffShared);  // shares the counts / query list region
  int32_t *ent = (int32_t *)(base + Lay::kOffEnt);
  unsigned long long *cand = (unsigned long long *)(base + Lay::kOffCand);

  const LbvhPoint *own_pts = a.bvh.points + tl, *halo_pts = a.halo.points ? a.halo.points + tl : a.bvh.points + tl;
  unsigned long long my_isect_sum = 0, wave_node_tests = 0, wave_point_tests = 0;
  uint32_t my_levels = 0, my_unfinished = 0;  // (per lane, a few dozen packets each: 32 bits, a register less apiece -- the kernel sits at its 128)
  int wave_levels = 0, wave_err = 0;
  uint32_t my_handed = 0;
  [[maybe_unused]] unsigned long long diag_scanned = 0, diag_listed = 0;  // TKNN_DIAG_BUILD only
  int wave_min_handover = 0x7fffffff;
#if TKNN_DIAG_BUILD
  unsigned long long ph[5] = {0, 0, 0, 0, 0}, t_mark = __builtin_amdgcn_s_memtime();
#define PHASE_END(i)                                         \
  do {                                                       \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    ph[i] += now_ - t_mark;                                  \
    t_mark = now_;                                           \
  } while (0)
#else
#define PHASE_END(i) \
  do {               \
  } while (0)
#endif

  // Packets are curve-consecutive, so neighbouring packets read the same leaf blocks.  Each XCD has
  // its own L2: packets are dealt to the XCDs in chunks of up to 1024 consecutive packets, a wave
  // pulls from the chunks of the XCD it runs on (HW_REG_XCC_ID) and steals from the others when
  // those are used up.  Placement changes speed only.  (Measured at C2: 15.0 ms with one global
  // counter, 14.4 ms with chunks of 1024-4096; whole eighths of the range are slower, 21.9 ms.)
  const int xcc = (int)__builtin_amdgcn_s_getreg(6164 /* hwreg(HW_REG_XCC_ID, 0, 4) */) & 7;
  const int chunk = max(1, min(1024, a.ngroups / 128));
  uint32_t seg_empty = 0;  // XCDs whose chunks are used up (wave-uniform)
  for (;;) {
    int g = -1;
    for (int t = 0; t < 8 && g < 0; t++) {
      const int x = (xcc + t) & 7;
      if (seg_empty & (1u << x)) continue;
      int v = 0;
      if (lane == 0) v = (int)atomicAdd(&a.counters[kXcdCounter + kXcdCounterStride * x], 1ull);
      v = __builtin_amdgcn_readfirstlane(v);
      const int cand = ((v / chunk) * 8 + x) * chunk + (v % chunk);  // v-th packet of XCD x
      if (cand < a.ngroups)
        g = cand;
      else
        seg_empty |= 1u << x;
    }
    if (g < 0 || wave_err) break;

    const int32_t slot = g * 64 + lane;
    bool active = slot < a.bvh.n;
    if (a.skip) {
      if (active && (int32_t)a.skip[slot] == a.skip_is) active = false;
      if (__ballot(active) == 0ull) continue;  // a packet without a query of this phase
    }
    LbvhPoint q = {0.f, 0.f, 0.f, -1};
    if (active) q = a.bvh.points[slot];
    const int32_t row = active ? a.bvh.prim_id[slot] : 0;
    float r = a.start_radius;
    if (a.start_radii && active) r = a.start_radii[row];  // a radius schedule of my own (levels stay common: level t = r0_q * 2^t)
    int level = 0;
    int64_t isect = 0;
    uint32_t prev_others = 0;  // others in my box at the previous level
    int step = a.first_step;   // levels the next gather serves
    TeamLds L;
    L.qrec = qrec;
    L.blk = blk;
    L.qblk = qblk;
    L.qhi = qhi;
    L.qcnt = qcnt;
    L.qlist = qlist;
    L.ent = ent;
    L.cand = cand;

    // One gather may serve MORE than the step it is made for: when the queries are unlikely all to finish inside the step
    // (levels level .. level+m-1), the walk is made at the radius of the level after it ("extension"), and every block a
    // query needs is listed either at the front of its list (needed inside the step) or at its back (needed at the
    // extension level only).  The step's COUNT pass works on the front parts; its SELECT pass serves the queries that finish
    // inside the step on their front parts and, on their whole lists, those that go on to the extension level with enough
    // others to finish there almost surely (see the passes) -- at BASELINE config 2 (levels 0 and 1 share a step, 59 % of
    // the queries go on to level 2) one pyramid walk and one SELECT pass per packet instead of two of each.  Queries that pass
    // has not served find their lists in LDS in the next turn of the level loop (`reuse`), which runs its passes without a
    // walk of its own.  A packet whose extended lists do not fit walks again for the step alone.
    bool reuse = false;          // wave-uniform: this level's lists are in LDS already
    int ext_next = a.first_ext;  // wave-uniform: extend the next gather
    bool ext_ok = a.first_ext >= 0;  // ... no more for this packet once its extended lists did not fit (its boxes only grow); < 0: never
    bool served = false;         // per lane, for a `reuse` turn: the step's SELECT pass has served me at this level already
    for (;;) {  // radius levels
      PHASE_END(4);
      // ---- 1. query records, conservative query boxes ---------------------------------------
      // This step serves levels level .. level+m-1 with ONE gather at the outermost radius.
      // (level, step and r are the same in every lane; readfirstlane says so to the compiler, which then
      // keeps them and everything derived from them in scalar registers and branches on them without exec masks)
      level = __builtin_amdgcn_readfirstlane(level);
      step = __builtin_amdgcn_readfirstlane(step);
      if (!a.start_radii) r = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(r)));
      int m = step < 1 ? 1 : (step > kMaxStep ? kMaxStep : step);
      if (reuse) m = 1;  // the extension level of the previous gather
      if (level + m > a.max_rounds) m = a.max_rounds - level;
      const float r_in0 = r;                        // radius of the inner level of a two-level step
      float r_out = r;
      for (int j = 1; j < m; j++) r_out = r_out * 2.0f;
      {
        float *rec = qrec + lane * kQrecStride;
        rec[0] = q.x;
        rec[1] = q.y;
        rec[2] = q.z;
        rec[3] = __int_as_float(q.id);
        rec[4] = r_out;
      }
      int my_nblk = 0;  // lane = query: how many blocks of the packet's list this turn's passes visit for me
      int n_in = 0, n_out = 0;  // ... of my list: needed inside the step (its front part) / at the extension level only (its back)
      int my_own_pos = 0;       // ... and where my own block (the one holding me) sits in the front part
      bool too_big = false;  // this packet-level does not fit the LDS lists
      bool ext = !reuse && ext_next > 0 && level + m < a.max_rounds;
      ext = __builtin_amdgcn_readfirstlane((int)ext) != 0;
      if (reuse) {
        // front part + back part (team_pass maps positions past the front part to the back of the list); their lengths
        // wait in my record -- three more registers live across the passes would spill
        const int pk = __float_as_int(qrec[lane * kQrecStride + 5]);
        n_in = pk & 0xff;
        my_own_pos = (pk >> 8) & 0xff;
        n_out = (pk >> 24) & 0xff;
        my_nblk = n_in + n_out;
        reuse = false;
      } else
      for (;;) {  // the walk; a second time, for the step alone, if the extended lists do not fit
      const float r_walk = ext ? r_out * 2.0f : r_out;
      // conservative query boxes for the gather: every literal candidate of q at r_walk lies inside
      float lo_x = INFINITY, lo_y = INFINITY, lo_z = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY, hi_z = -INFINITY;
      // ... and, per query, how far a block's box may be from the query POINT (largest per-axis gap) to be needed at the
      // walk's radius / inside the step: radius plus the margin of the candidate test (-inf: a query that needs nothing)
      float reach_walk = -INFINITY, reach_step = -INFINITY;
      {
        const float qabs = fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fabsf(q.z));
        const float mg = (qabs + 2.0f * r_walk) * 4.76837158203125e-07f;  // 2^-21
        if (active && q.x == q.x) {  // (a NaN query -- lbvh.hip makes every coordinate NaN -- keeps the empty box: it needs no block)
          lo_x = (q.x - r_walk) - 2.0f * mg;
          lo_y = (q.y - r_walk) - 2.0f * mg;
          lo_z = (q.z - r_walk) - 2.0f * mg;
          hi_x = (q.x + r_walk) + 2.0f * mg;
          hi_y = (q.y + r_walk) + 2.0f * mg;
          hi_z = (q.z + r_walk) + 2.0f * mg;
          reach_walk = r_walk + 2.0f * mg;
          reach_step = ext ? r_out + 2.0f * ((qabs + 2.0f * r_out) * 4.76837158203125e-07f) : reach_walk;
        }
      }
      // The pyramid is culled against FOUR boxes, one per 16 curve-consecutive queries (= one leaf
      // block of queries), not against the packet's one union box: where the Z-curve jumps, or
      // among the outliers of a clustered set, the union covers space none of the queries needs.
      float s_lo_x[4], s_lo_y[4], s_lo_z[4], s_hi_x[4], s_hi_y[4], s_hi_z[4];
      {
        const float r_lo_x = t_team_min(lo_x), r_lo_y = t_team_min(lo_y), r_lo_z = t_team_min(lo_z);
        const float r_hi_x = t_team_max(hi_x), r_hi_y = t_team_max(hi_y), r_hi_z = t_team_max(hi_z);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          s_lo_x[j] = t_bcast(r_lo_x, 16 * j);
          s_lo_y[j] = t_bcast(r_lo_y, 16 * j);
          s_lo_z[j] = t_bcast(r_lo_z, 16 * j);
          s_hi_x[j] = t_bcast(r_hi_x, 16 * j);
          s_hi_y[j] = t_bcast(r_hi_y, 16 * j);
          s_hi_z[j] = t_bcast(r_hi_z, 16 * j);
        }
      }
      // Box against box as arithmetic, not as six compares and five mask operations: the largest separation along
      // any axis, max_a max(b.lo_a - hi_a, lo_a - b.hi_a), is <= 0 exactly when the closed boxes meet (block boxes
      // are never NaN, empty ones are (+inf, -inf): lbvh.hip).  Plain subtractions and maxima issue at twice the
      // rate of compares on gfx950 and leave the CU's scalar pipe alone (scripts/microbench/issue_rate.hip).
      auto separation = [](float b_lo_x, float b_lo_y, float b_lo_z, float b_hi_x, float b_hi_y, float b_hi_z, float q_lo_x, float q_lo_y,
                           float q_lo_z, float q_hi_x, float q_hi_y, float q_hi_z) -> float {
        const float sx = fmaxf(b_lo_x - q_hi_x, q_lo_x - b_hi_x), sy = fmaxf(b_lo_y - q_hi_y, q_lo_y - b_hi_y),
                    sz = fmaxf(b_lo_z - q_hi_z, q_lo_z - b_hi_z);
        return fmaxf(fmaxf(sx, sy), sz);
      };
      auto overlaps_packet = [&](const LbvhBox &bx) -> bool {
        float best = INFINITY;
#pragma unroll
        for (int j = 0; j < 4; j++)
          best = fminf(best, separation(bx.lo[0], bx.lo[1], bx.lo[2], bx.hi[0], bx.hi[1], bx.hi[2], s_lo_x[j], s_lo_y[j], s_lo_z[j], s_hi_x[j],
                                        s_hi_y[j], s_hi_z[j]));
        return best <= 0.f;
      };
      // The 64 child boxes of the wide node in hand, lane = child, go to LDS (the passes' entry lists are dead
      // during the gather) so that a surviving child's box reaches all 64 query lanes by three broadcast reads
      // instead of six v_readlane.
      float *node_boxes = (float *)ent;
      static_assert(64 * 6 * 4 <= Lay::kLdsEnt + Lay::kLdsCand, "the gather's child boxes borrow the entry lists' LDS");
      auto stash_boxes = [&](const LbvhBox &bx) {
        float2 *dst = (float2 *)(node_boxes + 6 * lane);
        dst[0] = make_float2(bx.lo[0], bx.lo[1]);
        dst[1] = make_float2(bx.lo[2], bx.hi[0]);
        dst[2] = make_float2(bx.hi[1], bx.hi[2]);
        t_wave_sync();
      };
      // the largest per-axis gap between the child box in lane `src` and MY query point (<= 0: I am inside): the child is
      // needed at radius R iff gap <= R (+ the margin: reach_*).  One distance serves the walk's radius and the step's.
      struct ChildBox {
        float2 w0, w1, w2;
      };
      auto child_box = [&](int src) -> ChildBox {
        // (src is wave-uniform: its byte offset is a scalar product -- left to itself the compiler folds the product and
        // the address add into one v_mad_u64_u32, a quarter-rate instruction, for every block tested)
        int boff;
        asm("s_mul_i32 %0, %1, 24" : "=s"(boff) : "s"(src));
        const float2 *b = (const float2 *)((const char *)node_boxes + boff);
        return ChildBox{b[0], b[1], b[2]};
      };
      auto gap_to_me = [&](const ChildBox &c) -> float {
        return separation(c.w0.x, c.w0.y, c.w1.x, c.w1.y, c.w2.x, c.w2.y, q.x, q.y, q.z, q.x, q.y, q.z);
      };
      // The children named by `mask`, from the highest lane down or from the lowest up, one after the other through
      // test(child, its box) -- false ends the walk -- with the NEXT child's box read from LDS before the child in hand is
      // tested: three broadcast reads, their wait, a dozen vector instructions, a ballot, a branch and the list stores are
      // one dependent chain per child, some seventy per packet, and the lists are bytes, so the compiler may not lift the
      // next child's reads over this child's stores by itself.  Two boxes take turns (no copy at the back edge: it would
      // wait for the read it copies); after the last child its own box is read once more -- a read that is not made
      // would zero the wait count of the one before it where the two ways meet.
      auto for_children_ahead = [&](unsigned long long mask, bool top_down, auto test) {
        auto take = [&](int last) -> int {
          if (!mask) return last;
          const int src = top_down ? 63 - __builtin_clzll(mask) : __ffsll((long long)mask) - 1;
          mask &= ~(1ull << src);
          return src;
        };
        if (!mask) return;
        int s0 = take(0), s1;
        ChildBox c0 = child_box(s0), c1;
        for (;;) {
          bool more = mask != 0ull;
          s1 = take(s0);
          c1 = child_box(s1);
          if (!test(s0, c0) || !more) break;
          more = mask != 0ull;
          s0 = take(s1);
          c0 = child_box(s0);
          if (!test(s1, c1) || !more) break;
        }
      };

      PHASE_END(0);
      // ---- 2+3. gather the packet's block list and the per-query masks ----------------------
      my_own_pos = 0;
      int cur = 0;  // lane = query: blocks in the front part of my list | blocks in its back part << 16
      uint8_t *my_list = qblk + lane * kMaxPerQuery;
      if (Lay::kHiWords) {
#pragma unroll
        for (int w = 0; w < Lay::kHiWords; w++) qhi[lane * Lay::kHiWords + w] = 0u;  // (my own words: no lane but mine writes them)
      }
      int nb = 0, scanned = 0;
      for (int tree = 0; tree < (PLAIN ? 1 : 2) && !too_big; tree++) {
        const LbvhWideView &wv = a.wide[tree];
        const int32_t tree_n = tree == 0 ? a.bvh.n : a.halo.n;
        if (tree_n <= 0 || wv.levels <= 0) continue;
        // Depth-first over the inner levels of the pyramid.  Wide nodes whose children are leaf blocks
        // are not expanded one by one but collected (the list grows down from the top of the stack
        // array) and drained together: in ascending curve order, the next node's child boxes in
        // flight while this node's blocks are tested against the 64 queries.
        int sp = 0, nleaf = 0;
        if (lane == 0) stack[wv.levels > 1 ? 0 : kTeamStack - 1] = (wv.levels << 26) | 0;  // virtual root above the top level
        if (wv.levels > 1)
          sp = 1;
        else
          nleaf = 1;
        t_wave_sync();
        const int32_t last_block = wv.count[0] - 1;
        while ((sp > 0 || nleaf > 0) && !too_big) {
          if (sp > 0 && sp + nleaf + 63 <= kTeamStack) {  // room for the 64 children of one more node
            const int32_t e = __builtin_amdgcn_readfirstlane(stack[sp - 1]);  // same address in every lane
            sp--;
            const int lvl = (e >> 26) - 1;    // level of the children (>= 1 here)
            const int32_t first_child = (e & 0x3ffffff) * 64;
            const int32_t c = first_child + lane;
            const bool valid = lvl == wv.levels - 1 ? (lane < wv.count[lvl] && first_child == 0) : (c < wv.count[lvl]);
            LbvhBox bx = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
            if (valid) bx = wv.level[lvl][c];
            wave_node_tests += 64;
            const bool ov = valid & overlaps_packet(bx);
            const unsigned long long om = __ballot(ov);
            const int cnt = __popcll(om);
            if (lvl > 1) {
              if (ov) stack[sp + t_rank(om)] = (lvl << 26) | c;
              sp += cnt;
            } else {
              // children of `c` are leaf blocks.  Keep a survivor only if some single QUERY box reaches
              // it (lanes = queries, the survivor's box by v_readlane): a dozen instructions that save
              // its 64 blocks from being tested one by one where only the group box, not a query,
              // overlapped.  Nodes are popped in descending curve order and taken here from the
              // highest lane down, so filling the list downwards keeps it ascending in memory.
              if (om) stash_boxes(bx);
              for_children_ahead(om, /*top_down=*/true, [&](int src, const ChildBox &box) -> bool {
                if (__ballot(gap_to_me(box) <= reach_walk) == 0ull) return true;
                if (lane == 0) stack[kTeamStack - 1 - nleaf] = (lvl << 26) | (first_child + src);
                nleaf++;
                return true;
              });
            }
            t_wave_sync();
            continue;
          }
          if (nleaf == 0) {  // inner nodes alone fill the stack
            too_big = true;
            break;
          }
          auto leaf_boxes = [&](int i) -> LbvhBox {  // i-th collected node; index and children clamped
            const int32_t e = __builtin_amdgcn_readfirstlane(stack[kTeamStack - nleaf + (i < nleaf ? i : nleaf - 1)]);
            return wv.level[0][min((e & 0x3ffffff) * 64 + lane, last_block)];
          };
          LbvhBox bx_next = leaf_boxes(0);
          for (int i = 0; i < nleaf && !too_big; i++) {
            const int32_t e = __builtin_amdgcn_readfirstlane(stack[kTeamStack - nleaf + i]);
            const int32_t first_child = (e & 0x3ffffff) * 64;
            const LbvhBox bx = bx_next;
            bx_next = leaf_boxes(i + 1);
            const bool valid = first_child + lane <= last_block;
            wave_node_tests += 64;
            const bool ov = valid & overlaps_packet(bx);
            unsigned long long om = __ballot(ov);
            // A packet of far-apart queries (outliers of a clustered set) has a union box that covers
            // whole clusters none of its queries needs: testing those blocks one by one would keep
            // this wave busy long after the others have finished.  The lane kernel walks per query.
            scanned += __popcll(om);
            if (TKNN_DIAG_BUILD && (a.diag & 32)) diag_scanned += __popcll(om);
            if (scanned > kScanBudget) {
              too_big = true;
              break;
            }
            // leaf blocks: which of my 64 queries need block c?  (lanes = queries, box from LDS)
            if (om) stash_boxes(bx);
            for_children_ahead(om, /*top_down=*/false, [&](int src, const ChildBox &box) -> bool {
              const float gap = gap_to_me(box);
              bool need = gap <= reach_walk;
              if (TKNN_DIAG_BUILD && (a.diag & 8)) need = false;
              if (__ballot(need) == 0ull) return true;
              if (nb >= kMaxBlocks) {
                too_big = true;  // more blocks than a byte slot can name
                return false;
              }
              const int32_t block = first_child + src;
              blk[nb] = (int32_t)((uint32_t)block | ((uint32_t)tree << 31));  // (every lane stores the same word: no exec mask to set up)
              // my own block is one of the packet's own four (a scalar test; its position: how many I have listed before it)
              if (tree == 0 && (uint32_t)(block - g * 4) < 4u && block == (slot >> 4)) my_own_pos = cur & 0xffff;
              if (need) {
                // inside the step: the front of my list, upwards; at the extension level only: its back, downwards.  A list
                // that outgrows its slots keeps writing inside them (clamped): the packet walks again or is handed over.
                const bool inner = gap <= reach_step;
                const int at = inner ? (cur & 0xffff) : kMaxPerQuery - 1 - (cur >> 16);
                const int at_c = min(max(at, 0), kMaxPerQuery - 1);  // (v_med3_i32)
                my_list[at_c] = (uint8_t)nb;
                if (Lay::kHiWords && nb >= 256) qhi[lane * Lay::kHiWords + (at_c >> 5)] |= 1u << (at_c & 31);
                cur += inner ? 1 : 0x10000;
              }
              nb++;
              return true;
            });
          }
          nleaf = 0;
          t_wave_sync();
        }
        t_wave_sync();  // the stack array is rewritten by the next tree / shared with the passes
      }
      if (TKNN_DIAG_BUILD && (a.diag & 32)) diag_listed += nb;
      n_in = cur & 0xffff, n_out = cur >> 16;
      if (ext) {
        // extended lists that do not fit (a list longer than its slots, more blocks than the packet's list names, the
        // scan budget): once more, for the step alone
        if (too_big || __ballot(n_in + n_out > kMaxPerQuery) != 0ull) {
          ext = false;
          ext_ok = false;
          too_big = false;
          t_wave_sync();
          continue;
        }
        reuse = __ballot(active) != 0ull;
      }
      my_nblk = n_in;
      if (!ext) n_out = 0;
      break;
      }  // the walk
      // The packet's block list or scan budget is exhausted, or a query needs more blocks than its own
      // list holds: the packet's unfinished queries are handed over (team walk / lane rounds / wave
      // kernel, see solve_team), from this level on.  With four list registers (k > 32: boxes of
      // hundreds of candidates at the last level) only the queries whose own lists overflow go and
      // the rest carry on -- 0.49 M instead of 2.3 M of 10 M uniform points at k = 50.  (For k <= 32
      // that finer hand-over changed little on the clustered sets and cost 1 % on the benchmark: the
      // loop no longer ends at this point, which moved the register allocation.)
      if (NREG < 3) {
        if (__ballot(my_nblk > kMaxPerQuery) != 0ull) too_big = true;
        if (too_big) {
          if (active) {
            // (plain: the three addresses made here -- made at the packet's start, for a store few packets ever make, they are
            // three register pairs across the passes, two of them in scratch)
            int32_t slot_now = slot;
            if constexpr (PLAIN) slot_now = g * 64 + t_lane_again(lane);
            a.done[slot_now] = 0;
            a.isect_sorted[slot_now] = isect;
            a.next_level[slot_now] = level;
            my_handed++;
          }
          wave_min_handover = min(wave_min_handover, level);
          active = false;
          break;
        }
      } else if (too_big || __ballot(my_nblk > kMaxPerQuery) != 0ull) {
        const bool hand_over = active && (too_big || my_nblk > kMaxPerQuery);
        if (hand_over) {
          a.done[slot] = 0;
          a.isect_sorted[slot] = isect;
          a.next_level[slot] = level;
          my_handed++;
          active = false;
        }
        wave_min_handover = min(wave_min_handover, level);
        if (__ballot(active) == 0ull) break;
      }
      // read back by the teams: list length | position of my own block | length of the front part if a back part follows
      // (bits 24..31, which the teams ignore: the back part's length while the step's passes run on the front part)
      const int my_packed = my_nblk | (my_own_pos << 8) | (my_nblk > n_in ? n_in << 16 : n_out << 24);
      qrec[lane * kQrecStride + 5] = __int_as_float(my_packed);

      PHASE_END(1);
      // ---- 4. passes ---------------------------------------------------------------------------
      // One-level step: the box grows 8x per level, so a query with a few others at the previous
      // level will almost surely reach k now and goes straight to the fused count+select pass; the
      // rest are counted first and selected only if they turn out finished.  Multi-level step:
      // count all m nested boxes in one pass, pick the first level with >= k others, select there.
      // A row is written only when its query really has >= k others in the chosen box, so neither
      // speculation nor level grouping can change a result.
      // A gather with an extension has the lists of the level after the step at hand, so an unfinished query that would
      // speculate at that level in the next turn does so NOW: it joins the step's SELECT pass with its whole list and the
      // extension level's radius (fin_at = m).  If that serves every query still active, the `reuse` turn is not run at all:
      // one round of the teams and one turn's bookkeeping less per packet.  If not (a query with hardly any others yet, a
      // speculation at the step's own level that failed) the turn runs for the queries left over, `served` keeping the
      // others out of its passes.  (`reuse` is set here exactly when this turn's gather has an extension.)
      const bool speculate = m == 1 && active && !served && level > 0 && prev_others * 8u >= (uint32_t)(TEAM_K + TEAM_K / 2);
      const bool count_first = active && !served && !speculate;
      served = false;  // (set only on the way into a `reuse` turn)
      // The four teams of a pass step through their lists in lockstep, so a group of four queries
      // costs the longest of its lists: the pass lists are ordered by list length (buckets of 4
      // blocks), which lifts the teams' occupancy from ~77 % to ~95 % on uniform data.
      // The SELECT pass's list has the light queries (`lite`, see below) first, in buckets of their own and marked by bit 8
      // of their entries: the pass takes a round of light queries alone down a shorter path, a mixed round -- at most one
      // per pass -- down the usual one.
      constexpr int kLiteBuckets = NREG == 1 ? kCountFlatGroups + 1 : 0;  // lists of 0 .. 4 * kCountFlatGroups blocks
      static_assert(kMaxPerQuery / 4 + kLiteBuckets < 32, "list-length buckets of the pass lists are one bit each of a 32-bit word");
      auto build_qlist = [&](bool sel, int nblk, bool lite) -> int {
        const int bucket = lite ? nblk >> 2 : (nblk >> 2) + kLiteBuckets;  // <= kMaxPerQuery / 4 + kLiteBuckets < 32
        if (lane == 0) qlist[64] = 0;
        t_wave_sync();
        if (sel) __hip_atomic_fetch_or((uint32_t *)&qlist[64], 1u << bucket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        t_wave_sync();
        uint32_t present = (uint32_t)__builtin_amdgcn_readfirstlane(qlist[64]);
        int base = 0, pos = 0;
        while (present) {
          const int b = __ffs((int)present) - 1;
          present &= present - 1u;
          const bool mine = sel && bucket == b;
          const unsigned long long bm = __ballot(mine);
          if (mine) pos = base + t_rank(bm);
          base += __popcll(bm);
        }
        if (sel) qlist[pos] = lite ? lane | 0x100 : lane;
        t_wave_sync();
        return base;
      };
      {
        const int n_count = build_qlist(count_first, my_nblk, false);
        if (!(TKNN_DIAG_BUILD && (a.diag & 4))) {
          if (m > 1)
            team_pass<false, HALO, NREG, false, true, PLAIN>(a, held, L, n_count, g * 64, own_pts, halo_pts, lane);
          else
            team_pass<false, HALO, NREG, false, false, PLAIN>(a, held, L, n_count, g * 64, own_pts, halo_pts, lane);
        }
        t_wave_sync();
      }
      PHASE_END(2);
      // first level of the step at which I have >= k others (deviceCode.cu:118), -1 if none; m: none, and the SELECT pass
      // serves me at the extension level
      uint32_t c0 = 0, c1 = 0, selfc = 0;
      int fin_at = -1;
      if (count_first) {
        c0 = qcnt[lane * 2 + 0];
        const uint32_t w1 = qcnt[lane * 2 + 1];
        c1 = m > 1 ? (w1 & 0x3fffffffu) : 0u;
        selfc = w1 >> 31;
        if (c0 - selfc >= (uint32_t)TEAM_K)
          fin_at = 0;
        else if (m > 1 && c1 - selfc >= (uint32_t)TEAM_K)
          fin_at = 1;
      }
      int sel_nblk = my_nblk;
      if (reuse && a.merge_ext && count_first && fin_at < 0 && ((m > 1 ? c1 : c0) - selfc) * 8u >= (uint32_t)(TEAM_K + TEAM_K / 2)) {  // the rule of `speculate`, a turn early
        // my whole list, as the `reuse` turn would have it: front + back | own position | front length << 16 (bits 24..31
        // keep the back part's length until the statistics below have read it), and that level's radius
        fin_at = m;
        const int pk = __float_as_int(qrec[lane * kQrecStride + 5]);
        sel_nblk = (pk & 0xff) + ((pk >> 24) & 0xff);
        qrec[lane * kQrecStride + 4] = qrec[lane * kQrecStride + 4] * 2.0f;
        qrec[lane * kQrecStride + 5] = __int_as_float(sel_nblk | (pk & 0xff00) | ((pk & 0xff) << 16) | (pk & (int)0xff000000u));
      }
      const bool select_now = speculate || fin_at >= 0;
      if (m > 1 && fin_at == 0) qrec[lane * kQrecStride + 4] = r_in0;  // finishing inside the step: SELECT works in the inner box
      // A LIGHT query finishes inside the step (counted, so neither speculating nor served at the extension level) with at
      // most sixteen others in its finishing box -- one row of keys, every one of them a neighbour -- on a list without a
      // back part that the flat loads of a round can hold (team_pass).  Read from the record: nothing more lives across the passes.
      bool lite = false;
      if (NREG == 1 && a.lite && fin_at >= 0 && fin_at < m) {
        const int pk = __float_as_int(qrec[lane * kQrecStride + 5]);
        lite = (fin_at == 0 ? c0 : c1) - selfc <= 16u && (pk & 0xff0000) == 0 && (pk & 0xff) <= a.count_flat_max;
      }
      {
        t_wave_sync();
        const int n_select = build_qlist(select_now, sel_nblk, lite);
        if (!(TKNN_DIAG_BUILD && (a.diag & 2))) team_pass<true, HALO, NREG, FULL, false, PLAIN>(a, held, L, n_select, g * 64, own_pts, halo_pts, lane);
        t_wave_sync();
      }
      PHASE_END(3);
      // (the SELECT pass counts a light query's box once more: the count its path relies on)
      if (TKNN_DIAG_BUILD && lite && qcnt[lane * 2 + 0] != (fin_at == 0 ? c0 : c1)) atomicAdd(&a.counters[21], 1ull);
      const bool ext_sel = fin_at == m;  // served at the extension level
      bool finished = fin_at >= 0 && !ext_sel;
      uint32_t last_others = prev_others;  // (a query served a turn ago keeps its count)
      if (speculate) {
        c0 = qcnt[lane * 2 + 0];
        selfc = qcnt[lane * 2 + 1] >> 31;
        finished = c0 - selfc >= (uint32_t)TEAM_K;
        fin_at = finished ? 0 : -1;
      }
      uint32_t c_ext = 0, n_back = 0;  // candidates in my box at the extension level; blocks of my list it alone needs
      if (ext_sel) {
        c_ext = qcnt[lane * 2 + 0];
        finished = c_ext - selfc >= (uint32_t)TEAM_K;
        // (should the `reuse` turn run for others, it reads a list without a back part for me)
        const int pk = __float_as_int(qrec[lane * kQrecStride + 5]);
        n_back = ((uint32_t)pk >> 24) & 0xffu;
        qrec[lane * kQrecStride + 5] = __int_as_float(pk & 0x00ffffff);
      }
      int levels_run = 0;
      if (count_first || speculate) {  // (every active query but those served a turn ago)
        levels_run = finished || ext_sel ? fin_at + 1 : m;
        isect += c0;
        if (levels_run > 1) isect += c1;  // (0 in a one-level step)
        isect += c_ext;
        my_levels += (uint32_t)levels_run;
        last_others = ext_sel ? c_ext - selfc : (m > 1 ? c1 : c0) - selfc;
        prev_others = last_others;
      }
      wave_levels = max(wave_levels, (int)t_wave_max((float)(active ? level + levels_run : 0)));
      {
        // exact box tests executed for my query: LBVH_BLOCK per listed block and pass
        const unsigned long long passes = (count_first ? 1ull : 0ull) + (select_now ? 1ull : 0ull);
        wave_point_tests += t_wave_sum(((unsigned long long)my_nblk * passes + n_back) * LBVH_BLOCK);
      }
      if (finished) {
        // the team wrote the row (SELECT pass); the counter and the level come from the query's lane
        my_isect_sum += (unsigned long long)isect;
        if constexpr (PLAIN) {
          // (the row's address made HERE: made where the row is read -- it is the same over a packet's levels -- it is a pair of
          // registers that lives across the passes, and did so in scratch: a load and its wait in front of this store)
          int32_t row_now = row;
          asm volatile("" : "+v"(row_now));
          held.out_isect[row_now] = isect;
        } else if (a.out_isect) {
          a.out_isect[row] = isect;
        }
        if (a.out_fb) a.out_fb[(int64_t)row * TEAM_K].intersections = isect;
        const int fin_level = level + (fin_at > 0 ? fin_at : 0);
        if (a.out_level) a.out_level[row] = fin_level;
        if ((qcnt[lane * 2 + 1] >> 30) & 1u) {  // SELECT saw exact-distance ties
          if constexpr (PLAIN) {
            const int32_t slot_now = g * 64 + t_lane_again(lane);  // (as the row above; my slot, made again from my lane)
            knn_flag_tie(held.tie, a.tie_list, a.counters, slot_now, fin_level, 2);
          } else {
            knn_flag_tie(a.tie, a.tie_list, a.counters, slot, fin_level, 2);
          }
        }
      }
      active = active && !finished;
      int m_done = m;  // levels behind the packet after this turn
      if (reuse && a.merge_ext) {
        if (__ballot(active && !ext_sel) == 0ull) {
          m_done = m + 1;  // the extension level is served: no turn of its own
          reuse = false;
        } else {
          served = ext_sel;
        }
      }
      level += m_done;
      t_wave_sync();
      if (__ballot(active) == 0ull) break;
      if (level >= a.max_rounds) {
        if (!a.allow_unfinished) wave_err |= 1;
        break;
      }
      for (int j = 0; j < m_done; j++) r = r * 2.0f;  // hostCode.cpp:321
      // how many levels the next gather should serve: the box grows 8x per level; group levels as
      // long as even the best-off unfinished query is unlikely to collect k others
      {
        const float pmax = t_wave_max(active ? (float)last_others : 0.f);
        float expect = pmax * 8.f;
        step = 1;
        while (step < kMaxStep && expect < 0.5f * (float)TEAM_K) {
          step++;
          expect *= 8.f;
        }
        // ... and list the blocks of the level after the step, too, unless even the best-off query will almost
        // surely finish inside it (a packet walks again as long as ONE of its 64 queries is unfinished)
        ext_next = ext_ok && expect < 2.5f * (float)TEAM_K ? 1 : 0;
      }
    }
    if (active) my_unfinished++;
  }

  const unsigned long long isum = t_wave_sum(my_isect_sum), lsum = t_wave_sum((unsigned long long)my_levels), usum = t_wave_sum((unsigned long long)my_unfinished),
                           hsum = t_wave_sum((unsigned long long)my_handed);
  if (lane == 0) {
    unsigned long long *st = a.counters + kStatBase + (blockIdx.x & (kStatStripes - 1)) * kStatStride;  // my stripe: [1] .. [9] as in counters
    atomicMax(&st[1], (unsigned long long)wave_levels);
    atomicAdd(&st[2], wave_node_tests);
    atomicAdd(&st[3], wave_point_tests);
    atomicAdd(&st[4], isum);
    atomicAdd(&st[6], lsum);
    if (usum) atomicAdd(&st[7], usum);
    if (hsum) {
      atomicAdd(&st[8], hsum);
      atomicMin(&st[9], (unsigned long long)wave_min_handover);
    }
    if (wave_err) atomicOr(&st[5], (unsigned long long)wave_err);
#if TKNN_DIAG_BUILD
    for (int i = 0; i < 5; i++) atomicAdd(&a.counters[10 + i], ph[i]);
    if (a.diag & 32) {
      atomicAdd(&a.counters[24], diag_scanned);
      atomicAdd(&a.counters[25], diag_listed);
    }
#endif
  }
}


#undef TEAM_K

// Start-of-solve state of the packet kernel in one launch: done[] = 1 (a query is "done" unless handed
// over), tie[] = 0, counters = 0 except [9] = ~0 (min hand-over level), levels[] = -1 if asked for.
__global__ void __launch_bounds__(256) team_prep_kernel(uint8_t *done, uint8_t *tie, int64_t n, unsigned long long *counters, int32_t *levels) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  if (tid < kCounters + 8 * kXcdCounterStride) counters[tid] = tid == 9 ? ~0ull : 0ull;  // (+ the per-XCD packet counters behind them)
  if (tid < kStatStripes * kStatStride) counters[kStatBase + tid] = (tid & (kStatStride - 1)) == 9 ? ~0ull : 0ull;  // the statistics' stripes
  // hipMalloc'd arrays are 256-byte aligned: whole 16-byte words, then the last few bytes
  const int64_t words = n / 16;
  uint4 *d16 = reinterpret_cast<uint4 *>(done), *t16 = reinterpret_cast<uint4 *>(tie);
  const uint4 ones = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u), zeros = make_uint4(0u, 0u, 0u, 0u);
  for (int64_t i = tid; i < words; i += nth) {
    d16[i] = ones;
    t16[i] = zeros;
  }
  for (int64_t i = words * 16 + tid; i < n; i += nth) {
    done[i] = 1;
    tie[i] = 0;
  }
  if (levels)
    for (int64_t i = tid; i < n; i += nth) levels[i] = -1;
}

}  // namespace

bool Engine::team_kernel_supports(int k) { return k >= 1 && k <= 64; }


// How many radius levels the first gather of every packet should serve: with the average density
// of the scene, the first level at which a box is expected to hold about k/2 other points.  Only
// a work estimate -- every level is still resolved exactly.
int Engine::first_step_estimate(const SolveArgs &sa) const {
  float radius = sa.start_radius;
  for (int m = 1; m < 3; m++) {
    if (expected_box_population(radius) >= 0.5 * sa.k) return m;
    radius *= 2.0f;
  }
  return 3;
}

bool Engine::solve_team(const SolveArgs &sa, tknnSolveInfo *info, hipStream_t s) {
  const int64_t n = bvh_.size();
  if (n >= (1ll << 28)) return false;  // leaf blocks are addressed by 32-bit byte offsets; the caller takes the wave kernel
  TeamArgs a = team_args(sa);
  set_solve_args(a, sa);
  a.first_step = sa.d_start_radii ? 1 : first_step_estimate(sa);  // (the estimate is from ONE start radius and the mean density)
  {
    // the first gather also lists the blocks of the level after its step unless the boxes of the step's last level are
    // expected to hold k others several times over (team_kernel: the same rule between later steps)
    float radius = sa.start_radius;
    for (int t = 1; t < std::min(a.first_step, kMaxStep); t++) radius *= 2.0f;
    a.first_ext = !sa.d_start_radii && expected_box_population(radius) < 2.5 * sa.k ? 1 : 0;
    if (const char *e = getenv("TKNN_TEAM_EXT")) a.first_ext = atoi(e) > 0 ? a.first_ext : -1;  // measurements: 0 = no extended gathers at all
    a.merge_ext = 1;
    if (const char *e = getenv("TKNN_TEAM_MERGE")) a.merge_ext = atoi(e) > 0 ? 1 : 0;  // measurements and tests: 0 = the extension level in a turn of its own
    // COUNT rounds of up to so many blocks take the pass's flat path; measurements and tests: 0 = the ring for every round
    a.count_flat_max = 4 * kCountFlatGroups;
    if (const char *e = getenv("TKNN_TEAM_COUNT_FLAT")) a.count_flat_max = std::max(0, std::min(atoi(e), 4 * kCountFlatGroups));
    // SELECT rounds of light queries take the pass's light path; measurements and tests: 0 = the usual path for every round
    a.lite = 1;
    if (const char *e = getenv("TKNN_TEAM_LITE")) a.lite = atoi(e) > 0 ? 1 : 0;
  }
  {
    // axes along which the built points differ at all (2-D inputs carry z = 0, hostCode.cpp:115-118);
    // a halo tree may hold anything
    int dims = 0;
    for (int ax = 0; ax < 3; ax++) dims += scene_[3 + ax] > scene_[ax] ? 1 : 0;
    if (halo_count() > 0) dims = 3;
    a.tie_span = dims >= 3 ? 1.73206f : (dims == 2 ? 1.41422f : 1.00001f);
  }
  if (TKNN_DIAG_BUILD)
    if (const char *d = getenv("TKNN_TEAM_DIAG")) a.diag = atoi(d);
  a.ngroups = (int32_t)((n + 63) / 64);

  const int nreg = nreg_for(sa.k);  // list registers per lane
  const char *walk_all = getenv("TKNN_TEAM_WALK_ALL");    // measurements only: k > 32 without the packet kernel
  if (sa.k > 32 && walk_all && atoi(walk_all)) {
    // (33 <= k <= 64 as it was before the packet kernel had four list registers per lane:) every
    // query goes through the team walk, four list registers per lane, from level 0
    reset_solve_state(sa.d_levels, s);
    const tknnSolveInfo all = walk(sa, a, 4, nullptr, (int32_t)n, 0, /*count_lane_launches=*/false, s);
    if (info) *info = all;
    return true;
  }
  int per_cu = 2;
  static_assert(kDbStripes * kDbStripeWords >= 8 * kXcdCounterStride, "the packet counters borrow the words of RT-DBSCAN's striped statistics");
  const size_t lds = (size_t)kTeamBlock / 64 * (size_t)(nreg == 1 ? TeamLayout<1>::kTeamLds : (nreg == 2 ? TeamLayout<2>::kTeamLds
                                                         : (nreg == 3 ? TeamLayout<3>::kTeamLds : TeamLayout<4>::kTeamLds)));
  const bool full_list = sa.k == 16 * nreg;  // no spare list entry to see a tie with the row's last in
  using TeamEntry = void (*)(TeamArgs);
  static const TeamEntry entries[2][4][2] = {
      {{team_kernel<false, 1, false>, team_kernel<false, 1, true>}, {team_kernel<false, 2, false>, team_kernel<false, 2, true>},
       {team_kernel<false, 3, false>, team_kernel<false, 3, true>}, {team_kernel<false, 4, false>, team_kernel<false, 4, true>}},
      {{team_kernel<true, 1, false>, team_kernel<true, 1, true>}, {team_kernel<true, 2, false>, team_kernel<true, 2, true>},
       {team_kernel<true, 3, false>, team_kernel<true, 3, true>}, {team_kernel<true, 4, false>, team_kernel<true, 4, true>}}};
  // A PLAIN solve -- rows into idx, dist and intersections and nothing else of what TeamArgs can ask for (plain_team_solve), one list
  // register, no measurement knob in the environment -- takes the instantiation that carries none of it, with an argument block of
  // what is left (PlainTeamArgs).  Every other solve takes the generic kernel; TKNN_TEAM_PLAIN=0 (measurements and tests): every solve.
  using PlainEntry = void (*)(PlainTeamArgs);
  static const PlainEntry plain_entries[2] = {team_kernel<false, 1, false, true>, team_kernel<false, 1, true, true>};
  bool plain = nreg == 1 && halo_count() == 0 && plain_team_solve(a);
  for (const char *knob : {"TKNN_TEAM_MERGE", "TKNN_TEAM_LITE", "TKNN_TEAM_COUNT_FLAT", "TKNN_TEAM_EXT", "TKNN_TEAM_DIAG"})
    if (getenv(knob)) plain = false;
  if (const char *e = getenv("TKNN_TEAM_PLAIN")) plain = plain && atoi(e) > 0;
  const PlainTeamArgs plain_a = plain_team_args(a);
  if (getenv("TKNN_VERBOSE")) fprintf(stderr, "[team] packet kernel: the %s instantiation\n", plain ? "plain" : "generic");
  const void *entry = plain ? (const void *)plain_entries[full_list ? 1 : 0] : (const void *)entries[halo_count() > 0 ? 1 : 0][nreg - 1][full_list ? 1 : 0];
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, entry, kTeamBlock, lds) != hipSuccess) per_cu = 2;
  // (the query divides the CU's LDS by the byte; the hardware hands it out in granules: scripts/microbench/lds_granule.hip --
  // a launch of more workgroups than fit would leave the surplus waiting for a slot and then for the last packets)
  per_cu = std::max(1, std::min(per_cu, lds_workgroups_per_cu(lds)));
  if (const char *cap = getenv("TKNN_TEAM_WAVES_PER_CU"))  // measurements only: how the packet kernel's time scales with the waves in flight
    per_cu = std::max(1, std::min(per_cu, atoi(cap)));
  const int64_t want = (a.ngroups + kTeamBlock / 64 - 1) / (kTeamBlock / 64);
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cu_count_ * per_cu));

  // one launch instead of six fills (each costs a few microseconds of its own on the stream): done = 1,
  // tie = 0, all counters 0 except [9] (min hand-over level) = ~0, levels = -1
  // (phases 2 and 3 complete the rows and levels an earlier call has begun: levels are preset once, by phase 0 or 1)
  hipLaunchKernelGGL(team_prep_kernel, dim3(cu_count_ * 4), dim3(256), 0, s, done_, tie_, n, counters_, sa.phase >= 2 ? nullptr : sa.d_levels);
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  {
    void *kargs[] = {plain ? (void *)&plain_a : (void *)&a};
    OWLMI_HIP(hipLaunchKernel(entry, dim3(blocks), dim3(kTeamBlock), kargs, lds, s));
  }
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  // the tie pass over the rows this kernel has flagged and listed, count read on the device: launched
  // before the host knows anything, so the usual handful costs no round trip of its own
  launch_tie_fix(sa, tie_list_, -1, std::min(cu_count_ * 4, kTieListCap / 4), s);
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  fetch_stat_stripes(s);
  OWLMI_HIP(hipMemcpyAsync(h_counters_ + 10, counters_ + kTieCounter, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  const KernelStats st = fold_stat_stripes(true);
  float ms = 0;
  OWLMI_HIP(hipEventElapsedTime(&ms, ev_a_, ev_b_));
  if (st.handed_over == 0 && h_counters_[10] <= (unsigned long long)kTieListCap) {  // nothing handed over, every flagged row listed
    ties_early_ = true;
    early_tie_rows_ = (int64_t)h_counters_[10];
    early_tie_left_ = (int64_t)h_counters_[12];
    OWLMI_HIP(hipEventElapsedTime(&early_tie_ms_, ev_b_, ev_c_));
  }
#if TKNN_DIAG_BUILD
  if (getenv("TKNN_TEAM_DIAG")) {
    unsigned long long t[5];
    OWLMI_HIP(hipMemcpy(t, counters_ + 10, sizeof t, hipMemcpyDeviceToHost));
    const double tot = (double)(t[0] + t[1] + t[2] + t[3] + t[4]);
    unsigned long long wave_steps = 0;
    OWLMI_HIP(hipMemcpy(&wave_steps, counters_ + 15, sizeof wave_steps, hipMemcpyDeviceToHost));
    fprintf(stderr, "[team diag] block steps: %.3g wave steps x 4 teams for %.3g listed blocks (lockstep efficiency %.1f%%)\n",
            (double)wave_steps, (double)st.point_tests / LBVH_BLOCK, 100.0 * ((double)st.point_tests / LBVH_BLOCK) / (4.0 * (double)wave_steps));
    if (a.diag & 16) {
      unsigned long long g[2];
      OWLMI_HIP(hipMemcpy(g, counters_ + 26, sizeof g, hipMemcpyDeviceToHost));
      fprintf(stderr, "[team diag] inserts: %.4g candidates passed the gate after the sorted first block (%.2f per query), in %.4g lock-step rounds of the wave (%.2f per query)\n",
              (double)g[0], (double)g[0] / (double)n, (double)g[1], (double)g[1] / (double)n);
    }
    if (a.diag & 128) {
      unsigned long long g[12];
      OWLMI_HIP(hipMemcpy(g, counters_ + 28, sizeof g, hipMemcpyDeviceToHost));
      for (int pass = 0; pass < 2; pass++) {
        const unsigned long long *t4 = g + 8 * pass;
        const double tt = (double)(t4[0] + t4[1] + t4[2] + t4[3]);
        fprintf(stderr, "[team diag] %s pass, wave time: %.3g cycles in all; set-up %.1f%%  first group %.1f%%  other groups %.1f%%  epilogue %.1f%%\n",
                pass ? "SELECT" : "COUNT", tt, 100 * t4[0] / tt, 100 * t4[1] / tt, 100 * t4[2] / tt, 100 * t4[3] / tt);
      }
      unsigned long long lt[6];  // light rounds, their queries | SELECT rounds, their queries, the light ones among them | count mismatches
      OWLMI_HIP(hipMemcpy(lt, counters_ + 16, sizeof lt, hipMemcpyDeviceToHost));
      fprintf(stderr, "[team diag] SELECT rounds: %.4g with %.4g queries, %.4g of them light; light rounds: %.4g (%.1f%% of the rounds) with %.4g queries; "
                      "light queries whose SELECT count differs from COUNT's: %llu\n",
              (double)lt[2], (double)lt[3], (double)lt[4], (double)lt[0], lt[2] ? 100.0 * (double)lt[0] / (double)lt[2] : 0.0, (double)lt[1], lt[5]);
    }
    if (a.diag & 32) {
      unsigned long long g[2];
      OWLMI_HIP(hipMemcpy(g, counters_ + 24, sizeof g, hipMemcpyDeviceToHost));
      fprintf(stderr, "[team diag] gather: %.3g leaf blocks tested against the 64 queries, %.3g of them listed (%.1f%%)\n", (double)g[0], (double)g[1], 100.0 * (double)g[1] / (double)g[0]);
    }
    fprintf(stderr, "[team diag] mean busy time per wave %.2f ms of %.2f ms kernel time (%d waves; s_memtime at 100 MHz)\n",
            tot / 1e8 * 1e3 / blocks, ms, blocks);
    fprintf(stderr, "[team diag] wave-time shares: records %.1f%%  gather %.1f%%  count %.1f%%  select %.1f%%  rest %.1f%%\n",
            100 * t[0] / tot, 100 * t[1] / tot, 100 * t[2] / tot, 100 * t[3] / tot, 100 * t[4] / tot);
  }
#endif
  if (st.flags & 1ull) throw RoundsExceeded{};
  if (info) *info = solve_info(st, sa.start_radius, TKNN_KERNEL_TEAM, 16 * nreg, ms);
  const unsigned long long handed = st.handed_over;
  if (handed) {
    // Stragglers whose candidate lists outgrew the LDS lists (outliers of a clustered set, whose boxes
    // grow over whole clusters; dense duplicates): team_walk_kernel, one query per team, from the level
    // at which each was handed over; what exhausts its stack goes on to per-round lane launches.  A
    // quarter or more of all queries (a start radius far too large for the density: hundreds of
    // candidates per query from level 0 on): the wave-packet kernel, which streams candidate sets of
    // any size, re-solves just those queries.
    tknnSolveInfo tail;
    std::memset(&tail, 0, sizeof tail);
    const char *force = getenv("TKNN_TEAM_TAIL");  // "walk" / "lane" / "wave": tests and measurements only
    // (k > 32: the team walk beats the wave kernel's 64-entry register lists on any share, 10 M uniform
    // points from level 0: 137 against 223 ms at k = 50)
    const bool by_wave = !sa.d_start_radii && wave_kernel_available() &&
                         (force ? !strcmp(force, "wave") : (handed * 4ull >= (unsigned long long)n && sa.k <= 32));
    const bool by_walk = !by_wave && !(force && !strcmp(force, "lane"));
    const int first_handover_level = (int)st.first_handover_level;
    if (by_wave) {
      solve_wave(sa, &tail, s, /*only_unfinished=*/true);
    } else if (by_walk) {
      // the stragglers' sorted slots as a compact ascending list
      compact_slots(/*ties=*/false, s);
      tail = walk(sa, a, nreg, slot_list_, (int32_t)handed, first_handover_level, /*count_lane_launches=*/true, s);
    } else {
      if (sa.d_start_radii) throw ArgError{TKNN_E_UNSUPPORTED, "per-query start radii are served by the team kernels only (TKNN_TEAM_TAIL=lane)"};
      continue_lane(sa, first_handover_level, &tail, s);
    }
    if (getenv("TKNN_VERBOSE"))
      fprintf(stderr, "[team] %llu of %lld queries handed over from level %d on: team kernel %.2f ms, %s %.2f ms (%d launches)\n",
              handed, (long long)n, first_handover_level, ms, by_wave ? "wave kernel" : (by_walk ? "team walk" : "lane rounds"), tail.solve_ms,
              tail.dominant_kernel_launches);
    if (info) merge_tail(*info, tail, sa.start_radius, /*count_launches=*/false);
  }
  return true;
}

}  // namespace owlmi
