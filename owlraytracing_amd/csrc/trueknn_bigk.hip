// trueknn_bigk.hip -- the team TrueKNN kernel for 64 < k <= TKNN_MAX_K (bigk_walk_kernel): one query per team, the lists in
// memory, and its launch (Engine::solve_bigk).  The argument block is the team kernels' (TeamArgs, team_args.h), the walk team_walk.h's.
#include "knn_thresholds.h"  // knn_gate_from_worst
#include "bigk_keys.h"
#include "team_args.h"
#include "team_lanes.h"
#include "team_walk.h"
#include "trueknn_engine.h"

#include <algorithm>

namespace owlmi {

namespace {

// waves per SIMD the kernel's register allocation aims at (measured with the hand-over walk's: TKNN_WALK_WAVES, trueknn_tail.hip)
#ifndef TKNN_BIGK_WAVES
#define TKNN_BIGK_WAVES 4
#endif
#if TKNN_BIGK_WAVES
#define TKNN_BIGK_ATTR __attribute__((amdgpu_waves_per_eu(TKNN_BIGK_WAVES)))
#else
#define TKNN_BIGK_ATTR
#endif

// ---- k > 64: the list in memory -----------------------------------------------------------------------------------------
// The reference keeps every query's k-list in global memory and takes any k from its command line (hostCode.cpp:111,
// deviceCode.cu:77-134).  The other team kernels hold up to 64 entries in registers.  Larger lists live in memory, sixteen keys
// to a CHUNK (lane j of the team reads and writes entry 16 c + j of chunk c: one coalesced 256-byte access, and always the
// lane's own words), per team that is resident on the device, not per query: a query's list is built anew at every radius
// level, as in team_walk_kernel, whose walk of the pyramid this kernel shares -- one query per team, its sixteen lanes the
// child boxes of a wide node or the points of a leaf block.  Candidates wait in the team's LDS buffer and are merged a sorted
// row of sixteen at a time (t_merge_rows with the registers in memory): the row goes to the first chunk whose largest distance
// is not below the row's smallest (the chunks' maxima sit in LDS), meets it mirrored -- the sixteen smallest of both stay, the
// sixteen largest travel on to the next chunk -- until what travels is empty.
// BigKey and its sorting network: bigk_keys.h.
constexpr int kBigMaxChunks = TKNN_MAX_K / 16;
static_assert(TKNN_MAX_K % 16 == 0 && kBigMaxChunks <= 64, "chunk maxima: 64 words of LDS per team");

template <bool HALO>
__global__ void __launch_bounds__(kTeamBlock) TKNN_BIGK_ATTR bigk_walk_kernel(TeamArgs a, BigKey *lists, int chunks) {
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[2][LBVH_WIDE_LEVELS];
  __shared__ BigKey cand_mem[4 * kCandCapacity];     // per team: candidates waiting to be merged, (squared distance, first level, index)
  __shared__ uint32_t cmax_mem[4 * kBigMaxChunks];   // per team and chunk of its list: the largest distance in it (bits)
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  BigKey *my_cand = cand_mem + team * kCandCapacity;
  uint32_t *my_cmax = cmax_mem + team * kBigMaxChunks;
  BigKey *my_list = lists + ((size_t)blockIdx.x * 4 + (size_t)team) * (size_t)chunks * 16;
  walk_fill_levels<2>(levels[0], a.wide, lane);
  t_wave_sync();
  const int32_t n = a.bvh.n;
  const int kc = (a.k - 1) >> 4;  // the chunk of the k-th entry
  unsigned long long isect_sum = 0, levels_sum = 0, node_tests = 0, point_tests = 0;
  unsigned int unfinished = 0, failed = 0;
  int max_level = 0;
  int turn_next = 0, turn_left = 0;  // (t_next_slots)
  for (;;) {
    const int base = t_next_slots(&a.counters[0], a.grab, lane, turn_next, turn_left);
    if (base >= n) break;
    const int32_t slot = min(base + team, n - 1);
    bool has_q = base + team < n;
    if (has_q && a.skip && (int32_t)a.skip[slot] == a.skip_is) has_q = false;  // (tknnSolveOptions.phase: not a query of this call)
    const LbvhPoint q = a.bvh.points[slot];
    const int32_t row = a.bvh.prim_id[slot];
    int level = 0;
    int64_t isect = 0;
    const float q_r0 = a.start_radii ? a.start_radii[row] : a.start_radius;
    float r = q_r0;
    bool active = has_q;
    // A level only COUNTS (deviceCode.cu:74) as long as the query is unlikely to finish at it -- its box grows eightfold per
    // level, so: fewer than k / 5 others at the level before, and in the first levels the scene's mean density (a.first_step)
    // -- and keeps no list; a level that counts k others after all is walked once more, with the list.  (Every level with its
    // list: 10 M uniform points at k = 65 took three times the k = 64 solve.)
    uint32_t prev_others = 0;
    bool again = false;  // this level has counted k others without a list
    while (__ballot(active) != 0ull) {  // one radius level for every team that is still at work
      const bool select_on = again || level >= a.first_step || prev_others * 5u >= (uint32_t)a.k;
      const unsigned long long select_m = __ballot(select_on);
      const WalkBox qb(q, r);
      uint32_t part = 0;       // my lane's share of the candidate count of this level
      uint32_t n_list = 0;     // keys in my team's list (the same in its lanes)
      uint32_t kth_bits = 0x7f7fffffu;  // distance of the list's k-th entry (FLT_MAX: not that many yet)
      // (a squared distance that has overflowed is no neighbour: the reference's strict `<` against its initial FLT_MAX,
      // hostCode.cpp:41, deviceCode.cu:116)
      float tau2 = 3.402823466e+38f;
      bool overflow = false;
      uint32_t fill_n = 0;
      auto merge_buffer = [&]() {
        t_wave_sync();
#pragma unroll 1
        for (int rw = 0; rw < kCandCapacity / 16; rw++) {
          if (rw > 0 && __ballot(fill_n > 16u * (uint32_t)rw) == 0ull) break;
          const uint32_t at = 16u * (uint32_t)rw + (uint32_t)tl;
          const bool have = at < fill_n;
          BigKey c = {0u, 0u, 0u, 0u};
          if (have) c = my_cand[at];
          const float dist = knn_sqrt(__uint_as_float(c.d));
          uint32_t kd = have ? __float_as_uint(dist) : 0x7f7fffffu, kl = have ? c.l : 0u, ki = have ? c.i : 0u;  // the empty key past the end
          t_sort16_3(kd, kl, ki, tl);
          const uint32_t in_row = fill_n > 16u * (uint32_t)rw ? min(fill_n - 16u * (uint32_t)rw, 16u) : 0u;
          const uint32_t row_min = t_lane_read(kd, team << 4);
          const int nch = (int)((n_list + 15u) >> 4);  // chunks that hold keys
          // the first chunk a key of the row can get into: the chunks whose largest distance is below the row's smallest stay
          uint32_t below = 0;
          for (int j = tl; j < nch; j += 16) below += my_cmax[j] < row_min ? 1u : 0u;
          const int j0 = (int)t_team_sum(below);
          const int jend = min(nch, chunks - 1);  // ... and the last: the first chunk without keys, if the list has room for one
          bool live = in_row > 0u;                // what travels still holds keys
          int j_first = live ? j0 : 0x7fffffff;
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) j_first = min(j_first, __shfl_xor(j_first, off));
          for (int j = j_first; __ballot(live && j <= jend) != 0ull; j++) {
            const bool on = live && j >= j0 && j <= jend;
            BigKey e = {0x7f7fffffu, 0u, 0u, 0u};
            if (on && j < nch) e = my_list[(size_t)j * 16 + tl];
            const uint32_t od = t_dpp<0x140>(kd), ol = t_dpp<0x140>(kl), oi = t_dpp<0x140>(ki);  // the row's key 15 - tl
            const bool take = t_less3(od, ol, oi, e.d, e.l, e.i);
            uint32_t hd = take ? e.d : od, hl = take ? e.l : ol, hi_i = take ? e.i : oi;  // the larger of the pair: travels on
            uint32_t ld = take ? od : e.d, ll = take ? ol : e.l, li = take ? oi : e.i;    // the smaller: stays in this chunk
            t_clean16_3(ld, ll, li, tl);
            t_clean16_3(hd, hl, hi_i, tl);
            const uint32_t kth_here = t_lane_read(ld, (team << 4) + ((a.k - 1) & 15));
            if (on) {
              my_list[(size_t)j * 16 + tl] = BigKey{ld, ll, li, 0u};
              if (tl == 15) my_cmax[j] = ld;
              if (j == kc) kth_bits = kth_here;
              kd = hd, kl = hl, ki = hi_i;
            }
            const bool more = ((uint32_t)(__ballot(kd != 0x7f7fffffu) >> (team * 16)) & 0xffffu) != 0u;
            if (on) live = more && j < nch;  // (a chunk that held no key takes all that travels)
          }
          n_list = min((uint32_t)chunks * 16u, n_list + in_row);
          t_wave_sync();  // (the chunk maxima are read by the next row's lanes)
        }
        fill_n = 0;
        tau2 = fminf(3.402823466e+38f, knn_gate_from_worst(__uint_as_float(kth_bits)));
      };
      for (int tree = 0; tree < (HALO ? 2 : 1); tree++) {
        const LbvhWideView &wv = a.wide[tree];
        const LbvhView &tv = tree == 0 ? a.bvh : a.halo;
        if (tv.n <= 0 || wv.levels <= 0) continue;
        const int32_t clean_end = tv.n - (tv.nan_count ? *tv.nan_count : 0);  // NaN points sort last
        // (the chunk loop of a node is not unrolled: the merge is large)
        walk_tree<true>(
            levels[tree], wv, stack, kWalkStack, active, q, qb, team, tl, node_tests,
            [&](const LbvhBox &bx, int32_t c, int lvl) { return !walk_count_box(bx, q, qb, tau2, c, lvl, clean_end, part); },
            [&](int32_t b, bool has_b) {
              LbvhPoint p;
              float d2;
              const unsigned long long in_m = walk_block_test(tv.points, b, has_b, tl, q, qb, p, d2);
              point_tests += has_b ? 1u : 0u;
              part = t_count(part, in_m);
              const unsigned long long pm = in_m & __ballot(p.id != q.id) & __ballot(d2 <= tau2) & select_m;
              if (pm) {
                const uint32_t mine16 = (uint32_t)(pm >> (team << 4)) & 0xffffu;  // my team's lanes with a candidate
                if ((mine16 >> tl) & 1u)
                  my_cand[fill_n + __popc(mine16 & ((1u << tl) - 1u))] = BigKey{__float_as_uint(d2), first_level(p, q, q_r0, level), (uint32_t)p.id, 0u};
                fill_n += __popc(mine16);
                if (__ballot(fill_n >= 16u) != 0ull) merge_buffer();
              }
            },
            [] {}, overflow);
      }
      if (__ballot(fill_n > 0u) != 0ull) merge_buffer();
      // ---- the level's outcome, per team ----
      const uint32_t cnt = t_team_sum(part);
      const uint32_t others = cnt ? cnt - 1u : 0u;  // a query lies in its own box
      const bool fin = active && !overflow && others >= (uint32_t)a.k;
      if (active && overflow) {  // (cannot happen: 63 siblings wait on each of at most six levels; reported, never wrong)
        failed += tl == 0 ? 1u : 0u;
        active = false;
      } else if (active && fin && !select_on) {
        again = true;  // the same level once more, with its list
      } else if (active) {
        again = false;
        prev_others = others;
        isect += cnt;
        levels_sum += tl == 0 ? 1ull : 0ull;
        if (fin) {
          for (int j = 0; j <= kc; j++) {
            const int en = 16 * j + tl;
            if (en >= a.k) continue;
            const BigKey ky = my_list[(size_t)j * 16 + tl];
            const int32_t prim = (ky.d == 0x7f7fffffu && ky.i == 0u) ? -1 : (int32_t)ky.i;
            t_write_entry(a.out_idx, a.out_dist, a.out_fb, (int64_t)row * a.k + en, prim, __uint_as_float(ky.d), en, a.k, isect);
          }
          if (tl == 0) {
            if (a.out_isect) a.out_isect[row] = isect;
            if (a.out_level) a.out_level[row] = level;
            a.done[slot] = 1;
            isect_sum += (unsigned long long)isect;
          }
          max_level = max(max_level, level + 1);
          active = false;
        } else {
          level++;
          r = r * 2.0f;  // hostCode.cpp:321
          if (level >= a.max_rounds) {
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

}  // namespace

bool Engine::bigk_supports(int k) { return k > 64 && k <= TKNN_MAX_K; }

// k > 64: every query through bigk_walk_kernel, one query per team, the k-lists in memory (one per resident team)
void Engine::solve_bigk(const SolveArgs &sa, tknnSolveInfo *info, hipStream_t s) {
  const int64_t n = bvh_.size();
  TeamArgs a = team_args(sa);
  set_solve_args(a, sa);
  // the first level that keeps a list whatever the level before has counted: where a box is expected to hold k / 2 others at the
  // scene's mean density (a work estimate only; a per-query radius schedule has none: every level keeps its list)
  a.first_step = sa.d_start_radii ? 0 : first_step_estimate(sa) - 1;
  a.grab = 1;
  int per_cu = 4;
  const void *entry = halo_count() > 0 ? (const void *)bigk_walk_kernel<true> : (const void *)bigk_walk_kernel<false>;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, entry, kTeamBlock, 0) != hipSuccess) per_cu = 4;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, (int64_t)cu_count_ * std::max(1, per_cu)));
  int chunks = (sa.k + 15) / 16;
  BigKey *lists = (BigKey *)workspace((size_t)blocks * 4 * (size_t)chunks * 16 * sizeof(BigKey));
  // (three-word keys: no row is left to the tie pass; phases 2, 3 complete an earlier call's rows and levels)
  reset_solve_state(sa.phase < 2 ? sa.d_levels : nullptr, s);
  reset_stat_stripes(s);
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  void *kargs[] = {(void *)&a, (void *)&lists, (void *)&chunks};
  OWLMI_HIP(hipLaunchKernel(entry, dim3(blocks), dim3(kTeamBlock), kargs, 0, s));
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  fetch_stat_stripes(s);
  OWLMI_HIP(hipStreamSynchronize(s));
  const KernelStats st = fold_stat_stripes(false);
  float ms = 0;
  OWLMI_HIP(hipEventElapsedTime(&ms, ev_a_, ev_b_));
  if (st.handed_over) throw ArgError{TKNN_E_UNSUPPORTED, "k > 64: a query's walk outgrew its stack (a pyramid of more than six levels?)"};
  const tknnSolveInfo mine = solve_info(st, sa.start_radius, TKNN_KERNEL_TEAM, chunks * 16, ms);
  if (mine.unfinished && !sa.allow_unfinished) throw RoundsExceeded{};
  ties_early_ = true;  // nothing flagged, nothing to redo
  early_tie_rows_ = early_tie_left_ = 0;
  early_tie_ms_ = 0.f;
  if (info) *info = mine;
}

}  // namespace owlmi
