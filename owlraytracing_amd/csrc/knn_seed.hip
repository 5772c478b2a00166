// knn_seed.hip -- the k nearest points, exactly, with no radius from the caller (tknnKnn, include/owlknn_knn.h), for query points
// that are not in the tree or for the tree's own points.
//
// Row j is the row tknnRadiusKnn gives q_j at radius FLT_MAX.  The radius the walk really starts with is found here: the tree's
// points are sorted along a space-filling curve, so the blocks of 16 around a query's place in that order are real points close to
// it.  If k of them are eligible for the row (finite distance, not the skipped point), the k-th smallest of their distances is
// an upper bound r_j of the row's k-th distance, whatever the data are: the row's k entries are the k smallest distances of ALL
// eligible points, of which the seeds are a subset.  Every entry of the row then lies within r_j, and the walk of radius_knn.hip
// at radius r_j returns the row of radius FLT_MAX: both are the first k of the same ascending sequence.  With fewer than k
// eligible seeds r_j is FLT_MAX itself.  Nothing here depends on the place being a good one; a bad one only costs a wider walk.
//   1. external queries: query_order (query_order.h), then knn_slot_kernel: a query's full 21-level curve key, searched in the
//      tree's sorted keys (Lbvh::keys_device()), one query per lane.  The tree's own points are their slots: no such pass.
//   2. knn_seed_kernel<NREG, SELF>: one 16-lane team per query, four teams per wave; the team reads the ceil(k / 16) + 1 blocks
//      around the slot (clipped to the blocks that hold points without a NaN), a 16-byte load per lane and block, and keeps the k
//      smallest in its register list (t_merge_rows, team_lanes.h); r_j goes to a workspace column.  SELF: the teams work in slot
//      order, and the query, its id as the skipped point and r_j go to workspace columns by slot.
//   3. radius_knn_walks (radius_knn_walk.h): radius_knn.hip's walk and lane kernels with those columns as the rows' radii
//      (zero_radius_ok: k duplicates of a query give r_j = 0); SELF: rows written through prim_id, the caller's row of a slot.
#include "curve_key.h"
#include "query_order.h"
#include "radius_knn_walk.h"
#include "team_lanes.h"
#include "team_walk.h"  // query_nreg
#include "trueknn_engine.h"

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kSeedBlock = 64;        // one wave per workgroup, four teams
constexpr int kSeedBlocksPerCu = 32;  // 1 KB of LDS each
constexpr int kSlotBlock = 256;

struct KnnSeedArgs {
  const LbvhPoint *points;   // the tree's sorted points, padded with sentinels to whole blocks
  const int32_t *nan_count;  // device: how many of the last sorted points have a NaN coordinate
  int32_t n;
  const float *queries;      // external: m packed triples, caller order
  const uint32_t *order;     // external: the query worked on at sorted position i
  const int32_t *slots;      // external: its place in the tree's order, by sorted position (0 .. n)
  const int32_t *skip_ids;   // external: m, by the caller's j (may be null)
  int32_t m;
  int k;
  float *radii;              // out: r_j, by the caller's j (SELF: by slot)
  float *self_queries;       // SELF, out: the slot's point as a query, packed triples by slot
  int32_t *self_skip;        // SELF, out: the slot's id, by slot
  unsigned long long *ws;    // kRknnWsWords counters
};

// ---- 1. a query's place in the tree's order ------------------------------------------------------------------------------------
// The first slot whose key is not below the query's: the tree's quantisation at all 21 levels (morton_kernel, lbvh.hip), queries
// outside the scene box clamped to its faces as query_code_kernel clamps them; a query with a NaN coordinate lands behind the last
// finite point.
__global__ void __launch_bounds__(kSlotBlock) knn_slot_kernel(const float *__restrict__ queries, const uint32_t *__restrict__ order, int32_t m,
                                                             const float *__restrict__ scene, int curve, const uint64_t *__restrict__ keys, int32_t n,
                                                             int32_t *__restrict__ slots) {
  const int32_t i = blockIdx.x * kSlotBlock + threadIdx.x;
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

// ---- 2. the seed bound -------------------------------------------------------------------------------------------------------
// Lane tl takes point tl of a block of the window: d2 = knn_dist2; a seed is a point the row could list -- d2 finite (a NaN point,
// a sentinel or a NaN query make it NaN) and not the skipped point.  Seeds wait in the team's LDS buffer as (d2, id) and are merged
// sixteen at a time into the sorted register list, as the walk's candidates are.  The window is the same number of blocks for every
// query of a launch, so the teams of a wave loop in lock step: no __syncthreads, only t_wave_sync.
template <int NREG, bool SELF>
__global__ void __launch_bounds__(kSeedBlock) knn_seed_kernel(KnnSeedArgs a) {
  __shared__ unsigned long long cand_mem[4 * kCandCapacity];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  unsigned long long *my_cand = cand_mem + team * kCandCapacity;
  const int32_t clean_blocks = __builtin_amdgcn_readfirstlane((a.n - *a.nan_count + LBVH_BLOCK - 1) / LBVH_BLOCK);  // blocks with a point that has no NaN
  const int32_t window = min((a.k + LBVH_BLOCK - 1) / LBVH_BLOCK + 1, clean_blocks);
  unsigned long long seed_tests = 0;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < (int64_t)a.m; base += (int64_t)gridDim.x * 4) {
    const int64_t pos = base + team;
    const bool has_q = pos < (int64_t)a.m;
    LbvhPoint q = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
    int32_t skip = -1, slot = 0;
    int64_t qi = 0;
    if (has_q) {
      if (SELF) {
        slot = (int32_t)pos;
        q = a.points[pos];
        skip = q.id;
      } else {
        qi = a.order[pos];
        q.x = a.queries[3 * qi], q.y = a.queries[3 * qi + 1], q.z = a.queries[3 * qi + 2];
        skip = a.skip_ids ? a.skip_ids[qi] : -1;
        slot = a.slots[pos];
      }
    }
    // the window's first block: the slot's block in the middle, clipped at both ends of the order
    const int32_t first = max(0, min((min(slot, a.n - 1) >> 4) - (window - 1) / 2, clean_blocks - window));
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
      if (has_q) p = a.points[(int64_t)(first + w) * LBVH_BLOCK + tl];
      seed_tests += has_q ? 1u : 0u;
      const float d2 = knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z);
      const bool seed = has_q && d2 <= FLT_MAX && p.id != skip;  // (NaN: not a seed)
      const uint32_t mine16 = (uint32_t)(__ballot(seed) >> (team << 4)) & 0xffffu;
      if (seed) my_cand[fill_n + __popc(mine16 & ((1u << tl) - 1u))] = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)p.id;
      fill_n += __popc(mine16);
      if (__ballot(fill_n >= 16u) != 0ull) merge_buffer();
    }
    if (__ballot(fill_n > 0u) != 0ull) merge_buffer();
    // the list holds rounded roots (t_sorted_row); an empty entry k - 1 is FLT_MAX: fewer than k seeds
    const float bound = fminf(rknn_kth_dist<NREG>(bd, a.k, team), FLT_MAX);
    if (has_q && tl == 0) {
      a.radii[SELF ? pos : qi] = bound;
      if (SELF) {
        a.self_queries[3 * pos] = q.x, a.self_queries[3 * pos + 1] = q.y, a.self_queries[3 * pos + 2] = q.z;
        a.self_skip[pos] = skip;
      }
    }
  }
  const unsigned long long st = t_wave_sum(seed_tests);
  if (lane == 0 && st) atomicAdd(&a.ws[kRknnWsSeedTests], st);
}

using KnnSeedEntry = void (*)(KnnSeedArgs);
const KnnSeedEntry kKnnSeeds[2][4] = {{knn_seed_kernel<1, false>, knn_seed_kernel<2, false>, knn_seed_kernel<3, false>, knn_seed_kernel<4, false>},
                                      {knn_seed_kernel<1, true>, knn_seed_kernel<2, true>, knn_seed_kernel<3, true>, knn_seed_kernel<4, true>}};

}  // namespace

void Engine::knn(const tknnKnnOptions &o, tknnKnnInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const bool self = o.d_queries == nullptr;
  // the call's workspace: counters | lane list, radii | external: codes, order (+ the sort's second halves), slots, sort space
  //                                                   | self: skipped ids, queries (three columns)
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t sort_bytes = self ? 0 : query_order_sort_bytes(m, s);
  const size_t words_b = align(kRknnWsWords * sizeof(unsigned long long)), col_b = align((size_t)m * sizeof(uint32_t));
  char *ws = (char *)workspace(words_b + 6 * col_b + align(sort_bytes));
  unsigned long long *d_words = (unsigned long long *)ws;
  auto column = [&](int c) { return ws + words_b + (size_t)c * col_b; };
  int32_t *redo = (int32_t *)column(0);
  float *radii = (float *)column(1);
  uint32_t *codes = (uint32_t *)column(2), *codes_alt = (uint32_t *)column(3), *order_in = (uint32_t *)column(4), *order = (uint32_t *)column(5);
  int32_t *slots = (int32_t *)column(2);  // (over the codes: the sort is through when the slots are written)
  void *sort_tmp = column(6);
  int32_t *self_skip = (int32_t *)column(2);
  float *self_queries = (float *)column(3);

  const LbvhView tv = bvh_.view();
  KnnSeedArgs sa;
  std::memset(&sa, 0, sizeof sa);
  sa.points = tv.points;
  sa.nan_count = tv.nan_count;
  sa.n = tv.n;
  sa.queries = o.d_queries;
  sa.order = self ? nullptr : order;
  sa.slots = self ? nullptr : slots;
  sa.skip_ids = o.d_skip_ids;
  sa.m = (int32_t)m;
  sa.k = o.k;
  sa.radii = radii;
  sa.self_queries = self ? self_queries : nullptr;
  sa.self_skip = self ? self_skip : nullptr;
  sa.ws = d_words;

  RadiusKnnKernelArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = tv;
  a.wide = bvh_.wide_view();
  a.queries = self ? self_queries : o.d_queries;
  a.order = self ? nullptr : order;
  a.m = (int32_t)m;
  a.k = o.k;
  a.radii = radii;
  a.skip_ids = self ? self_skip : o.d_skip_ids;
  a.out_row = self ? tv.prim_id : nullptr;
  if (const char *e = getenv("TKNN_KNN_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.zero_radius_ok = 1;
  a.out_idx = o.d_idx;
  a.out_dist = o.d_dist;
  a.out_counts = o.d_counts;
  a.redo = redo;
  a.ws = d_words;

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(d_words, 0, kRknnWsWords * sizeof(unsigned long long), s));
  if (!self) query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, sort_tmp, sort_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  if (!self) {
    hipLaunchKernelGGL(knn_slot_kernel, dim3((unsigned)((m + kSlotBlock - 1) / kSlotBlock)), dim3(kSlotBlock), 0, s, o.d_queries, (const uint32_t *)order,
                       (int32_t)m, bvh_.scene_device(), bvh_.curve(), bvh_.keys_device(), tv.n, slots);
    OWLMI_HIP(hipGetLastError());
  }
  const int blocks = (int)std::min<int64_t>((m + 3) / 4, (int64_t)cu_count_ * kSeedBlocksPerCu);
  void *kargs[] = {(void *)&sa};
  OWLMI_HIP(hipLaunchKernel((const void *)kKnnSeeds[self ? 1 : 0][query_nreg(o.k) - 1], dim3(blocks), dim3(kSeedBlock), kargs, 0, s));
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  unsigned long long *h_words = h_counters_;
  const unsigned long long n_redo = radius_knn_walks(a, cu_count_, h_words, s);
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
