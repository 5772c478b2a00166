// trueknn_query.hip -- TrueKNN for query points that are NOT in the tree (tknnQuery, include/owlknn.h).
//
// Row j is the row the reference's loop (samples/s01-trueknn/hostCode.cpp:285-340 around deviceCode.cu:62-153)
// gives to q_j in the set P + {q_j}: radius levels from start_radius, doubled in fp32; the candidates of a level
// are the points of P whose box holds q_j; the first level with >= k candidates finishes the query; its row is
// the k best in (distance, level at which first a candidate, index) order.  There is no self to skip.
//
// The self-solve's packet kernel lives on queries being tree slots (64 consecutive sorted slots share leaf
// blocks).  External queries have no slot, so:
//   1. query_code_kernel + a radix sort (query_order.h): the queries along the tree's own curve (curve_key.h) over the tree's own quantisation, so that
//      the four teams of a wave and the waves of a workgroup's neighbours walk neighbouring nodes;
//   2. query_walk_kernel: persistent, one 16-lane team per query, every radius level inside the kernel -- the
//      walk of team_walk_kernel (trueknn_tail.hip; both on team_walk.h) without anything that is per slot;
//   3. query_lane_kernel: one query per lane, rope traversal (lane_walk.h), keys that carry the level -- for the few queries
//      the walk leaves: stack exhausted, or a row whose order depends on how bit-identical distances are ordered;
//   4. exact = 1: both kernels once more with a fixed radius per row (the box of half-width d_k), (dist, index).
#include "knn_thresholds.h"  // knn_gate_from_worst
#include "lane_walk.h"
#include "query_order.h"
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

constexpr int kQueryBlock = 64;       // one wave per workgroup, four teams
constexpr int kQueryBlocksPerCu = 16;  // 7.3 KB of LDS each: far inside what a CU holds
constexpr int kLaneBlock = 256;

// words of the call's own counters (in the workspace, zeroed per pass)
enum { kWsCursor = 0, kWsRedo = 1, kWsTies = 2, kWsFailed = 3, kWsWords = 8 };

struct QueryKernelArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const float *queries;   // m packed triples, caller order
  const uint32_t *order;  // m: the query processed at sorted position i
  int32_t m;
  float start_radius;
  int k;
  int max_rounds;
  int exact;              // 1: one level of half-width d_k per finished row, (dist, index) order, no statistics
  int force_redo;         // TKNN_QUERY_FORCE_FALLBACK (tests): the walk leaves every query to the lane kernel
  int32_t *out_idx;       // m*k (may be null)
  float *out_dist;        // m*k (may be null; never with exact)
  int64_t *out_isect;     // m (may be null)
  int32_t *levels;        // m, preset to -1 (never null: the engine's own if the caller has none)
  int32_t *redo;          // m: queries left to the lane kernel
  unsigned long long *ws;     // kWsWords counters
  unsigned long long *stats;  // the engine's statistics stripes (kStatBase)
};

// ---- 1. the order: query_order.h (shared with tknnDbscanQuery) ----------------------------------------------------

// ---- 2. the walk -------------------------------------------------------------------------------------------
// A team walks the 64-ary pyramid for one query (walk_tree, team_walk.h): a child box inside the part of the
// query's box where the candidate test is certain, and beyond the list's gate, is counted instead of walked.
// Candidates wait in the team's LDS buffer and are merged into the sorted register list sixteen at a time
// (t_merge_rows).  Teams of a wave loop in lock step, so there is no __syncthreads, only t_wave_sync.
template <int NREG>
__global__ void __launch_bounds__(kQueryBlock) __attribute__((amdgpu_waves_per_eu(4))) query_walk_kernel(QueryKernelArgs a) {
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[LBVH_WIDE_LEVELS];
  __shared__ unsigned long long cand_mem[4 * kCandCapacity];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  walk_fill_levels<1>(levels, &a.wide, lane);
  t_wave_sync();
  const LbvhWideView &wv = a.wide;
  const int32_t clean_end = lane_clean_end(a.bvh);
  unsigned long long isect_sum = 0, levels_sum = 0, node_tests = 0, point_tests = 0;
  unsigned int unfinished = 0, failed = 0, tied_rows = 0;
  int max_level = 0;
  for (;;) {
    int got = 0;
    if (lane == 0) got = (int)atomicAdd(&a.ws[kWsCursor], 4ull);
    const int base = __builtin_amdgcn_readfirstlane(got);
    if (base >= a.m) break;
    const bool has_q = base + team < a.m;
    const int32_t qi = has_q ? (int32_t)a.order[base + team] : 0;
    LbvhPoint q;
    q.x = a.queries[3 * (int64_t)qi], q.y = a.queries[3 * (int64_t)qi + 1], q.z = a.queries[3 * (int64_t)qi + 2];
    q.id = -1;  // ids of the tree's points are non-negative: nothing is "self"
    int level = 0;
    int64_t isect = 0;
    float r = a.start_radius;
    bool active = has_q;
    if (a.exact) {
      // every neighbour at distance <= d_k lies in the box of half-width d_k (the bound: repair_kernel, trueknn.hip)
      active = has_q && a.levels[qi] >= 0;
      const float dk = active ? a.out_dist[(int64_t)qi * a.k + a.k - 1] : 0.f;
      active = active && dk <= FLT_MAX;
      r = dk * 1.000001f + 0x1p-74f;
    }
    while (__ballot(active) != 0ull) {  // one radius level for every team that is still at work
      const WalkBox qb(q, r);
      uint32_t part = 0;  // my lane's share of the candidate count of this level
      uint32_t bd[NREG], bi[NREG];  // register j of lane t holds list entry 16 j + t
#pragma unroll
      for (int j = 0; j < NREG; j++) {
        bd[j] = 0x7f7fffffu;  // KNN_EMPTY_KEY = {FLT_MAX, 0}
        bi[j] = 0u;
      }
      float tau2 = INFINITY;
      const bool full = a.k == 16 * NREG;  // no spare list entry to see a tie with the row's last in
      uint32_t left_out = 0xffffffffu;
      unsigned long long *my_cand = cand_mem + team * kCandCapacity;
      uint32_t fill_n = 0;
      auto merge_buffer = [&]() __attribute__((always_inline)) {
        t_wave_sync();
        t_merge_rows<NREG>(bd, bi, left_out, full, my_cand, fill_n, tl);
        t_wave_sync();
        fill_n = 0;
        tau2 = knn_gate_from_worst(t_kth_dist<NREG>(bd, a.k, team));
      };
      bool overflow = false;
      if (wv.levels > 0)
        walk_tree<false>(
            levels, wv, stack, kWalkStack, active, q, qb, team, tl, node_tests,
            [&](const LbvhBox &bx, int32_t c, int lvl) { return !walk_count_box(bx, q, qb, tau2, c, lvl, clean_end, part); },
            [&](int32_t b, bool has_b) {
              LbvhPoint p;
              float d2;
              const unsigned long long in_m = walk_block_test(a.bvh.points, b, has_b, tl, q, qb, p, d2);
              point_tests += has_b ? 1u : 0u;
              part = t_count(part, in_m);
              const unsigned long long pm = in_m & __ballot(d2 <= tau2);
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
      if (full) left_out = t_team_min_u32(left_out);  // where the tie test below looks for it: lane 15
      // ---- the level's outcome, per team ----
      const uint32_t cnt = t_team_sum(part);  // no self: every candidate is a neighbour
      const bool fin = active && !overflow && (a.exact || cnt >= (uint32_t)a.k);
      // Does the row depend on how bit-identical distances are ordered (t_row_ties)?  At level 0 the list's order and
      // the reference's are the same.
      bool tie = false, edge = false;
      if (!a.exact && level > 0) t_row_ties<NREG>(bd, left_out, full, a.k, tl, q, a.start_radius, r, 1.73206f, fin, tie, edge);
      const bool tied = t_team_any(tie, team);
      if (active && (overflow || a.force_redo || (fin && tied))) {
        // left to the lane kernel, which starts the query from level 0: nothing of it is written or counted here
        if (tl == 0) {
          a.redo[atomicAdd(&a.ws[kWsRedo], 1ull)] = qi;
          if (overflow || a.force_redo)
            failed++;
          else
            tied_rows++;
        }
        active = false;
      } else if (active) {
        isect += cnt;
        if (fin) {
#pragma unroll
          for (int reg = 0; reg < NREG; reg++) {
            const int j = tl + 16 * reg;
            if (j >= a.k) continue;
            const int64_t o = (int64_t)qi * a.k + j;
            if (a.out_idx) a.out_idx[o] = knn_key_prim(((uint64_t)bd[reg] << 32) | bi[reg]);
            if (a.out_dist) a.out_dist[o] = __uint_as_float(bd[reg]);
          }
          if (tl == 0 && !a.exact) {
            if (a.out_isect) a.out_isect[qi] = isect;
            a.levels[qi] = level;
            isect_sum += (unsigned long long)isect;
            levels_sum += (unsigned long long)(level + 1);
          }
          if (!a.exact) max_level = max(max_level, level + 1);
          active = false;
        } else {
          level++;
          r = r * 2.0f;  // hostCode.cpp:321
          if (level >= a.max_rounds) {  // out of rounds: the caller decides (allow_unfinished)
            if (tl == 0) {
              unfinished++;
              levels_sum += (unsigned long long)level;
            }
            max_level = max(max_level, level);
            active = false;
          }
        }
      }
    }
  }
  const unsigned long long fsum = t_wave_sum((unsigned long long)failed), tsum = t_wave_sum((unsigned long long)tied_rows);
  if (lane == 0) {
    if (fsum) atomicAdd(&a.ws[kWsFailed], fsum);
    if (tsum) atomicAdd(&a.ws[kWsTies], tsum);
  }
  if (!a.exact)
    t_add_stats(a.stats + (blockIdx.x & (kStatStripes - 1)) * kStatStride, lane, max_level, node_tests, point_tests, isect_sum, levels_sum, unfinished);
}

// ---- 3. one query per lane -----------------------------------------------------------------------------------
// A sorted list of (distance, level at which first a candidate, index) keys in registers: the reference's
// order (its lists persist over rounds, deviceCode.cu:77-85, so of two candidates at the same distance the one
// listed in an earlier round stays in front).
template <int K>
struct LevelList {
  uint32_t d[K];   // fp32 bits of the distance (non-negative: bits order like values)
  uint64_t li[K];  // level << 32 | index
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < K; j++) {
      d[j] = 0x7f7fffffu;  // KNN_EMPTY_KEY: a candidate at distance FLT_MAX never enters
      li[j] = 0ull;
    }
  }
  __device__ __forceinline__ bool less(uint32_t cd, uint64_t cli, int j) const { return cd < d[j] || (cd == d[j] && cli < li[j]); }
  __device__ __forceinline__ void insert(uint32_t cd, uint64_t cli) {
    if (!less(cd, cli, K - 1)) return;
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
      const bool shift = less(cd, cli, j - 1), here = less(cd, cli, j);
      d[j] = shift ? d[j - 1] : (here ? cd : d[j]);
      li[j] = shift ? li[j - 1] : (here ? cli : li[j]);
    }
    const bool first = less(cd, cli, 0);
    d[0] = first ? cd : d[0];
    li[0] = first ? cli : li[0];
  }
  __device__ __forceinline__ int32_t prim(int j) const { return d[j] == 0x7f7fffffu && li[j] == 0ull ? -1 : (int32_t)(uint32_t)li[j]; }
};

// The queries of a list (redo, its length on the device), each from level 0, all levels in the lane's own loop.
template <int K>
__global__ void __launch_bounds__(kLaneBlock) query_lane_kernel(QueryKernelArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kLaneBlock + threadIdx.x;
  const bool has_q = t < (int64_t)a.ws[kWsRedo];
  const int32_t qi = has_q ? a.redo[t] : 0;
  const LbvhView &tv = a.bvh;
  const int32_t clean_end = lane_clean_end(tv);
  const LbvhPoint q = {a.queries[3 * (int64_t)qi], a.queries[3 * (int64_t)qi + 1], a.queries[3 * (int64_t)qi + 2], -1};  // no self
  float r = a.start_radius;
  bool active = has_q;
  if (a.exact) {
    active = has_q && a.levels[qi] >= 0;
    const float dk = active ? a.out_dist[(int64_t)qi * a.k + a.k - 1] : 0.f;
    active = active && dk <= FLT_MAX;
    r = dk * 1.000001f + 0x1p-74f;
  }
  unsigned long long node_tests = 0, point_tests = 0, isect_sum = 0, levels_sum = 0, unfinished = 0;
  int max_level = 0, level = 0;
  int64_t isect = 0;
  LevelList<K> list;
  while (active) {
    list.clear();
    int32_t cnt = 0;
    lane_walk<LaneRope::kWhenTaken>(tv,
        [&](int32_t ref, const LbvhNode &nd, int32_t) {
          node_tests++;
          const bool hit = lane_box_hit(nd, q, r);
          int32_t c;  // a subtree of candidates that can neither enter the list nor tie with its last entry is counted
          if (hit && lane_counts_subtree(ref, nd, q, r, knn_gate_from_worst(__uint_as_float(list.d[K - 1])), clean_end, c)) {
            cnt += c;
            return lane_rope();
          }
          return hit ? lane_descend() : lane_rope();
        },
        [&](int32_t, const LbvhPoint &p) {
          point_tests++;
          if (knn_in_box(p.x, p.y, p.z, r, q.x, q.y, q.z)) {
            cnt++;
            // the first level whose box held the query (not beyond this one: its test has just passed)
            uint32_t first = 0;
            if (!a.exact)
              for (float rr = a.start_radius; (int)first < level && !knn_in_box(p.x, p.y, p.z, rr, q.x, q.y, q.z); rr = rr * 2.0f) first++;
            const float d = knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z));
            list.insert(__float_as_uint(d), ((uint64_t)first << 32) | (uint32_t)p.id);
          }
          return lane_rope();
        });
    isect += cnt;
    if (a.exact || cnt >= a.k) {
      const int64_t base = (int64_t)qi * a.k;
#pragma unroll
      for (int j = 0; j < K; j++)
        if (j < a.k) {
          if (a.out_idx) a.out_idx[base + j] = list.prim(j);
          if (a.out_dist) a.out_dist[base + j] = __uint_as_float(list.d[j]);
        }
      if (!a.exact) {
        if (a.out_isect) a.out_isect[qi] = isect;
        a.levels[qi] = level;
        isect_sum = (unsigned long long)isect;
        levels_sum = (unsigned long long)(level + 1);
        max_level = level + 1;
      }
      active = false;
    } else {
      level++;
      r = r * 2.0f;
      if (level >= a.max_rounds) {
        unfinished = 1;
        levels_sum = (unsigned long long)level;
        max_level = level;
        active = false;
      }
    }
  }
  if (a.exact) return;
  // (all lanes of the wave are here)
  const unsigned long long nt = t_wave_sum(node_tests), pt = t_wave_sum(point_tests), isum = t_wave_sum(isect_sum),
                           lsum = t_wave_sum(levels_sum), usum = t_wave_sum(unfinished);
  const int ml = (int)t_wave_max((float)max_level);
  if ((threadIdx.x & 63) == 0 && nt) {
    unsigned long long *st = a.stats + (blockIdx.x & (kStatStripes - 1)) * kStatStride;
    atomicMax(&st[1], (unsigned long long)ml);
    atomicAdd(&st[2], nt);
    atomicAdd(&st[3], pt);
    atomicAdd(&st[4], isum);
    atomicAdd(&st[6], lsum);
    if (usum) atomicAdd(&st[7], usum);
  }
}

using WalkEntry = void (*)(QueryKernelArgs);
const WalkEntry kWalks[4] = {query_walk_kernel<1>, query_walk_kernel<2>, query_walk_kernel<3>, query_walk_kernel<4>};

}  // namespace

// One pass of both kernels over the sorted queries: the walk, then the lane kernel for what the walk left.
// Returns {queries left to the lane kernel for their stack, ... for their ties}; the events bracket the two launches.
static void query_pass(QueryKernelArgs &a, int cu_count, unsigned long long *h_words, hipEvent_t after_walk, hipEvent_t after_lane,
                       unsigned long long &failed, unsigned long long &tied, hipStream_t s) {
  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kWsWords * sizeof(unsigned long long), s));
  const int blocks = (int)std::min<int64_t>(((int64_t)a.m + 3) / 4, (int64_t)cu_count * kQueryBlocksPerCu);
  void *kargs[] = {(void *)&a};
  OWLMI_HIP(hipLaunchKernel((const void *)kWalks[query_nreg(a.k) - 1], dim3(blocks), dim3(kQueryBlock), kargs, 0, s));
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(after_walk, s));
  OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  const unsigned long long redo = h_words[kWsRedo];
  failed = h_words[kWsFailed];
  tied = h_words[kWsTies];
  if (redo) {
    const unsigned lane_blocks = (unsigned)((redo + kLaneBlock - 1) / kLaneBlock);
    ListCapacities::dispatch(list_capacity_for(a.k), [&](auto cap) {
      hipLaunchKernelGGL(query_lane_kernel<decltype(cap)::value>, dim3(lane_blocks), dim3(kLaneBlock), 0, s, a);
    });
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipEventRecord(after_lane, s));
}

void Engine::query(const tknnQueryOptions &o, tknnSolveInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const int k = o.k;
  // the call's workspace: counters | codes, order (+ the sort's second halves) | lane list | levels | distances | sort space
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t sort_bytes = query_order_sort_bytes(m, s);
  const bool own_levels = o.d_levels == nullptr, own_dist = o.exact != 0 && o.d_dist == nullptr;
  const size_t words_b = align(kWsWords * sizeof(unsigned long long)), col_b = align((size_t)m * sizeof(uint32_t)),
               dist_b = own_dist ? align((size_t)m * k * sizeof(float)) : 0;
  char *ws = (char *)workspace(words_b + 6 * col_b + dist_b + align(sort_bytes));
  unsigned long long *d_words = (unsigned long long *)ws;
  uint32_t *codes = (uint32_t *)(ws + words_b), *codes_alt = (uint32_t *)(ws + words_b + col_b), *order_in = (uint32_t *)(ws + words_b + 2 * col_b),
           *order = (uint32_t *)(ws + words_b + 3 * col_b);
  int32_t *redo = (int32_t *)(ws + words_b + 4 * col_b);
  int32_t *levels = own_levels ? (int32_t *)(ws + words_b + 5 * col_b) : o.d_levels;
  float *dist = own_dist ? (float *)(ws + words_b + 6 * col_b) : o.d_dist;
  void *sort_tmp = ws + words_b + 6 * col_b + dist_b;

  QueryKernelArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.wide = bvh_.wide_view();
  a.queries = o.d_queries;
  a.order = order;
  a.m = (int32_t)m;
  a.start_radius = o.start_radius;
  a.k = k;
  a.max_rounds = resolve_max_rounds(o.max_rounds);
  if (const char *e = getenv("TKNN_QUERY_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.out_idx = o.d_idx;
  a.out_dist = dist;
  a.out_isect = o.d_intersections;
  a.levels = levels;
  a.redo = redo;
  a.ws = d_words;
  a.stats = counters_ + kStatBase;

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(levels, 0xff, (size_t)m * sizeof(int32_t), s));
  reset_stat_stripes(s);
  query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, sort_tmp, sort_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  unsigned long long failed = 0, tied = 0, failed_exact = 0, tied_exact = 0;
  query_pass(a, cu_count_, h_counters_, ev_c_, ev_d_, failed, tied, s);
  fetch_stat_stripes(s);
  OWLMI_HIP(hipStreamSynchronize(s));
  KernelStats st = fold_stat_stripes(false);
  st.handed_over = failed;
  if (o.exact != 0 && !(st.unfinished && o.allow_unfinished == 0)) {
    a.exact = 1;
    query_pass(a, cu_count_, h_counters_, ev_e_, ev_f_, failed_exact, tied_exact, s);
    OWLMI_HIP(hipStreamSynchronize(s));
    st.handed_over += failed_exact;
  } else {
    OWLMI_HIP(hipEventRecord(ev_f_, s));
    OWLMI_HIP(hipStreamSynchronize(s));
  }
  float total_ms = 0, walk_ms = 0, lane_ms = 0;
  OWLMI_HIP(hipEventElapsedTime(&total_ms, ev_a_, ev_f_));
  OWLMI_HIP(hipEventElapsedTime(&walk_ms, ev_b_, ev_c_));
  OWLMI_HIP(hipEventElapsedTime(&lane_ms, ev_c_, ev_d_));
  if (info) {
    *info = solve_info(st, o.start_radius, TKNN_KERNEL_QUERY, 16 * query_nreg(k), total_ms);
    info->dominant_kernel_ms = walk_ms;  // the walk over the sorted queries; solve_ms also holds the order, the lane pass and the exact pass
    info->tie_rows = (int64_t)tied;
    info->tie_ms = lane_ms;
  }
  if (st.unfinished && o.allow_unfinished == 0) throw RoundsExceeded{};
}

}  // namespace owlmi
