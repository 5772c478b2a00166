// nms.hip -- greedy suppression within a radius inside each cloud of a built point tree (tknnRadiusNms, include/owlknn_nms.h).
//
// The kept set K is defined down the key order: p is kept iff no KEPT point of its cloud within r beats its key.  A point's fate
// so depends only on points with greater keys, and the call decides the points in rounds: a walk of the tree around p looks for
// a dominator within r; a KEPT one drops p at once (and ends the walk: the early exit that makes a round cheaper than a count
// pass), an UNDECIDED one leaves p for the next round, and a walk that meets neither keeps p.  A state only ever moves from
// UNDECIDED to a final value, and a final value is right by the induction, so a walk may use states written earlier in the same
// launch (relaxed atomic loads and stores): that changes how many rounds a call takes, never what it gives.  The undecided point
// with the greatest key of a cloud meets no undecided dominator, so every round decides something.  No kernel waits for another
// workgroup: rounds are launches, and the host reads ONE word per round, the length of the next list.
//   1. nms_init_kernel: per sorted slot the key (strength << 32 | ~(name's order): the larger uint64 dominates) and the state --
//      UNDECIDED, or INELIGIBLE for a NaN coordinate or a NaN score --, and the first work list: the slots [0, n - nan) in sorted
//      order (a round passes over an item whose state is final already, which is how a slot with a NaN score leaves it).
//   2. nms_walk_kernel<false>: persistent, one wave per workgroup, four 16-lane teams, one item per team, walk_tree with
//      its stop hook (team_walk.h) and the item's box of half-width r (1 + 1e-6); keep_box is the overlap test plus batch_knn.hip's slot-range
//      rule for the item's cloud.  At a leaf block the lanes take their slot if it lies in the cloud's range, is not the item's
//      own, is within r by the literal predicate and its key beats the item's; then they read its state.
//   3. nms_lane_kernel<false>: one item per lane on the rope walk (lane_walk.h), nodes pruned by their slot range, the same early
//      exit, for the items whose team stack ran out (the redo list; TKNN_NMS_FORCE_FALLBACK=1: every item).
//   4. the next list: the walks write a flag per list position, rocprim::select compacts the list by them, so it stays in sorted-slot
//      order and the four teams of a wave keep walking neighbouring items.
//   5. nms_scatter_kernel: d_keep and, for the points that need no walk, d_cover, by the caller's row; d_counts is a segmented
//      reduction of the states over the clouds' ranges.
//   6. nms_walk_kernel<true>, nms_lane_kernel<true>: the cover pass, one launch over the slots [0, n - nan): the same walk without
//      the dominance test for the DROPPED ones; the visitor keeps the team's minimum of (distance bits << 32 | name's order) over the
//      KEPT slots within r.
// The call's workspace (Engine::workspace, one layout):
//      counters (kNmsWsWords) | the two lists' lengths, the plain tree's range | keys, 8 n | states, 4 n | list A, list B, 4 n each |
//      redo list, 4 n | flags, n | rocPRIM's temporary (select, segmented reduce)
#include "owlknn_nms.h"
#include "lane_walk.h"
#include "team_lanes.h"
#include "team_walk.h"
#include "trueknn_engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

namespace owlmi {

namespace {

constexpr int kNmsBlock = 64;        // one wave per workgroup, four teams
constexpr int kNmsBlocksPerCu = 16;  // 6 KB of LDS each
constexpr int kNmsLaneBlock = 256;
constexpr int kNmsLaneBlocksPerCu = 4;
constexpr int kNmsFlatBlock = 256;

enum : uint32_t { kNmsUndecided = 0, kNmsKept = 1, kNmsDropped = 2, kNmsIneligible = 3 };
enum { kNmsByHash = 0, kNmsByScore = 1, kNmsByName = 2 };
// words of the call's counters; the first two are zeroed before every walk launch
enum { kNmsWsCursor, kNmsWsRedo, kNmsWsEligible, kNmsWsBadScores, kNmsWsKept, kNmsWsFallback, kNmsWsNodeTests, kNmsWsPointTests, kNmsWsWords };

struct NmsArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const uint64_t *tree_keys;  // batched: the cloud of a slot is tree_keys[slot] >> (63 - key_bits)
  const int32_t *starts;      // num_batches + 1 (null: a plain tree, one cloud [0, n - nan))
  int32_t num_batches;
  int key_bits;
  int32_t n;
  float radius;
  float radius_wide;          // radius * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts
  int mode;                   // kNmsByHash, kNmsByScore, kNmsByName
  int force_redo;             // TKNN_NMS_FORCE_FALLBACK (tests): the walk leaves every item to the lane kernel
  const float *scores;        // n, by the caller's row (kNmsByScore)
  unsigned long long *keys;   // n, by sorted slot
  uint32_t *state;            // n, by sorted slot
  int32_t *list;              // the work list (cover pass: null, the item at position i is slot i)
  const uint32_t *len;        // its length
  uint8_t *flags;             // by list position: 1 = the item is still undecided
  int32_t *redo;              // list positions left to the lane kernel
  uint32_t *lens;             // [0], [1]: the lengths of list A and B; [2], [3]: 0 and n - nan, the plain tree's range
  uint8_t *out_keep;          // n
  int32_t *out_cover;         // n (may be null)
  unsigned long long *ws;     // kNmsWsWords counters
};

__device__ __forceinline__ uint32_t nms_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
// a name's place in the signed order, as a uint32 that ascends with it
__device__ __forceinline__ uint32_t nms_name_order(int32_t name) { return (uint32_t)name ^ 0x80000000u; }
__device__ __forceinline__ int32_t nms_order_name(uint32_t order) { return (int32_t)(order ^ 0x80000000u); }
__device__ __forceinline__ unsigned long long nms_key(const NmsArgs &a, int32_t name, int32_t row) {
  uint32_t strength = 0u;
  if (a.mode == kNmsByScore) {
    const uint32_t u = __float_as_uint(a.scores[row]);
    strength = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  } else if (a.mode == kNmsByHash) {
    strength = nms_fmix32((uint32_t)name);
  }
  return ((unsigned long long)strength << 32) | (unsigned long long)(~nms_name_order(name));
}
// does the key kq of slot sq beat the key kp of slot sp (equal keys -- repeated ids --: the earlier slot)
__device__ __forceinline__ bool nms_beats(unsigned long long kq, int32_t sq, unsigned long long kp, int32_t sp) {
  return kq > kp || (kq == kp && sq < sp);
}
__device__ __forceinline__ uint32_t nms_state_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void nms_state_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the sorted slots [s, e) of the cloud of `slot`, a slot without a NaN
__device__ __forceinline__ void nms_range(const NmsArgs &a, int32_t slot, int32_t clean_end, int32_t &s, int32_t &e) {
  s = 0, e = clean_end;
  if (a.starts) {
    const uint32_t label = (uint32_t)(a.tree_keys[slot] >> (63 - a.key_bits));
    s = 0, e = 0;
    if (label < (uint32_t)a.num_batches) s = a.starts[label], e = a.starts[label + 1];
  }
}
// min of 64-bit words over the 16 lanes of my team: the smallest high word, then the smallest low word among the lanes that hold it
__device__ __forceinline__ unsigned long long nms_team_min(unsigned long long v) {
  const uint32_t hi = (uint32_t)(v >> 32), top = t_team_min_u32(hi);
  return ((unsigned long long)top << 32) | t_team_min_u32(hi == top ? (uint32_t)v : 0xffffffffu);
}
__device__ __forceinline__ void nms_add_stats(unsigned long long *ws, int lane, unsigned long long node_tests, unsigned long long point_tests,
                                              unsigned long long fallback) {
  const unsigned long long nt = t_wave_sum(node_tests), pt = t_wave_sum(point_tests), fb = t_wave_sum(fallback);
  if (lane == 0) {
    if (nt) atomicAdd(&ws[kNmsWsNodeTests], nt);
    if (pt) atomicAdd(&ws[kNmsWsPointTests], pt);
    if (fb) atomicAdd(&ws[kNmsWsFallback], fb);
  }
}

// ---- 1. keys, states, the first list ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kNmsFlatBlock) nms_init_kernel(NmsArgs a) {
  const int32_t t = blockIdx.x * kNmsFlatBlock + threadIdx.x;
  const int32_t clean_end = lane_clean_end(a.bvh);
  unsigned long long eligible = 0, bad = 0;
  if (t < a.n) {
    const int32_t name = a.bvh.points[t].id, row = a.bvh.prim_id[t];
    const bool bad_score = a.mode == kNmsByScore && a.scores[row] != a.scores[row];
    const bool ok = t < clean_end && !bad_score;
    a.keys[t] = nms_key(a, name, row);
    a.state[t] = ok ? kNmsUndecided : kNmsIneligible;
    a.list[t] = t;
    a.flags[t] = 0;
    eligible = ok ? 1u : 0u, bad = bad_score ? 1u : 0u;
  }
  if (t == 0) a.lens[0] = (uint32_t)clean_end, a.lens[1] = 0u, a.lens[2] = 0u, a.lens[3] = (uint32_t)clean_end;
  eligible = t_wave_sum(eligible), bad = t_wave_sum(bad);
  if ((threadIdx.x & 63) == 0) {
    if (eligible) atomicAdd(&a.ws[kNmsWsEligible], eligible);
    if (bad) atomicAdd(&a.ws[kNmsWsBadScores], bad);
  }
}

// ---- 2. a round (COVER: the cover pass) ------------------------------------------------------------------------------------------
// Teams of a wave loop in lock step: no __syncthreads, only t_wave_sync.  `dropped`, `blocked` and `best` are the same in the 16
// lanes of a team.
template <bool COVER>
__global__ void __launch_bounds__(kNmsBlock) __attribute__((amdgpu_waves_per_eu(4))) nms_walk_kernel(NmsArgs a) {
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[LBVH_WIDE_LEVELS];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  walk_fill_levels<1>(levels, &a.wide, lane);
  t_wave_sync();
  const LbvhWideView &wv = a.wide;
  const int32_t clean_end = lane_clean_end(a.bvh);
  const int32_t len = (int32_t)*a.len;
  unsigned long long node_tests = 0, point_tests = 0;
  for (;;) {
    int got = 0;
    if (lane == 0) got = (int)atomicAdd(&a.ws[kNmsWsCursor], 4ull);
    const int base = __builtin_amdgcn_readfirstlane(got);
    if (base >= len) break;
    const int32_t pos = base + team;
    const bool has_i = pos < len;
    const int32_t item = has_i ? (COVER ? pos : a.list[pos]) : 0;
    // (only the item's own walk writes its state, and no later list holds a decided item: a plain load)
    const bool todo = has_i && a.state[item] == (COVER ? kNmsDropped : kNmsUndecided);
    const LbvhPoint q = a.bvh.points[item];
    const unsigned long long key_i = a.keys[item];
    int32_t s, e;
    nms_range(a, item, clean_end, s, e);
    const bool active = todo && !a.force_redo;
    const WalkBox qb(q, a.radius_wide);
    bool dropped = false, blocked = false;
    unsigned long long best = ~0ull;
    bool overflow = wv.levels <= 0;
    if (wv.levels > 0)
      walk_tree<false>(
          levels, wv, stack, kWalkStack, active, q, qb, team, tl, node_tests,
          [&](const LbvhBox &, int32_t c, int lvl) {  // the range rule (batch_knn.hip)
            const int sh = min(4 + 6 * lvl, 31);
            return !dropped && c >= (s >> sh) && c <= ((e - 1) >> sh);
          },
          [&](int32_t b, bool has_b) {
            const int32_t slot = b * LBVH_BLOCK + tl;
            const bool in = has_b && !dropped && slot >= s && slot < e && slot != item;
            LbvhPoint p = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
            if (in) p = a.bvh.points[slot];
            const float d = knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z));
            const bool near = in && d <= a.radius;  // (a NaN: not within r)
            point_tests += has_b ? 1u : 0u;
            if constexpr (COVER) {
              if (near && a.state[slot] == kNmsKept)
                best = min(best, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)nms_name_order(p.id));
            } else {
              const bool dom = near && nms_beats(a.keys[slot], slot, key_i, item);
              const uint32_t st = dom ? nms_state_load(&a.state[slot]) : (uint32_t)kNmsDropped;
              if ((uint32_t)(__ballot(dom && st == kNmsKept) >> (team << 4)) & 0xffffu) dropped = true;
              if ((uint32_t)(__ballot(dom && st == kNmsUndecided) >> (team << 4)) & 0xffffu) blocked = true;
            }
          },
          [] {}, overflow, [&] { return !COVER && dropped; });
    if constexpr (COVER) best = nms_team_min(best);
    if (has_i && tl == 0) {
      const bool redo = todo && (overflow || a.force_redo);
      if (redo) a.redo[atomicAdd(&a.ws[kNmsWsRedo], 1ull)] = pos;  // left to the lane kernel, which starts the walk again
      if constexpr (COVER) {
        if (todo && !redo) a.out_cover[a.bvh.prim_id[item]] = best == ~0ull ? -1 : nms_order_name((uint32_t)best);
      } else {
        if (todo && !redo && (dropped || !blocked)) nms_state_store(&a.state[item], dropped ? kNmsDropped : kNmsKept);
        a.flags[pos] = todo && !redo && !dropped && blocked ? 1 : 0;
      }
    }
  }
  nms_add_stats(a.ws, lane, node_tests, point_tests, 0ull);
}

// ---- 3. one item per lane: the items of the redo list -------------------------------------------------------------------------------
template <bool COVER>
__global__ void __launch_bounds__(kNmsLaneBlock) nms_lane_kernel(NmsArgs a) {
  const int64_t n_redo = (int64_t)a.ws[kNmsWsRedo];
  const int32_t clean_end = lane_clean_end(a.bvh);
  unsigned long long node_tests = 0, point_tests = 0, decided = 0;
  for (int64_t t = (int64_t)blockIdx.x * kNmsLaneBlock + threadIdx.x; t < n_redo; t += (int64_t)gridDim.x * kNmsLaneBlock) {
    const int32_t pos = a.redo[t];
    const int32_t item = COVER ? pos : a.list[pos];
    const LbvhPoint q = a.bvh.points[item];
    const unsigned long long key_i = a.keys[item];
    int32_t s, e;
    nms_range(a, item, clean_end, s, e);
    bool dropped = false, blocked = false;
    unsigned long long best = ~0ull;
    lane_walk<LaneRope::kWithNode>(
        a.bvh,
        [&](int32_t ref, const LbvhNode &nd, int32_t) {
          node_tests++;
          if (lbvh_last(ref, nd.other) < s || lbvh_first(ref, nd.other) >= e) return lane_rope();
          return lane_box_hit(nd, q, a.radius_wide) ? lane_descend() : lane_rope();
        },
        [&](int32_t slot, const LbvhPoint &p) {
          point_tests++;
          if (slot < s || slot >= e || slot == item) return lane_rope();
          const float d = knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z));
          if (!(d <= a.radius)) return lane_rope();
          if constexpr (COVER) {
            if (a.state[slot] == kNmsKept) best = min(best, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)nms_name_order(p.id));
          } else {
            if (!nms_beats(a.keys[slot], slot, key_i, item)) return lane_rope();
            const uint32_t st = nms_state_load(&a.state[slot]);
            if (st == kNmsKept) {
              dropped = true;
              return lane_stop();
            }
            if (st == kNmsUndecided) blocked = true;
          }
          return lane_rope();
        });
    if constexpr (COVER) {
      a.out_cover[a.bvh.prim_id[item]] = best == ~0ull ? -1 : nms_order_name((uint32_t)best);
    } else {
      if (dropped || !blocked) {
        nms_state_store(&a.state[item], dropped ? kNmsDropped : kNmsKept);
        decided++;
      }
      a.flags[pos] = !dropped && blocked ? 1 : 0;
    }
  }
  // (all lanes of the wave are here)
  nms_add_stats(a.ws, threadIdx.x & 63, node_tests, point_tests, decided);
}

// ---- 5. the outputs by row ---------------------------------------------------------------------------------------------------------
// d_keep for every point; d_cover for the points that need no walk: a kept point's own name, -1 for one that is not eligible
__global__ void __launch_bounds__(kNmsFlatBlock) nms_scatter_kernel(NmsArgs a) {
  const int32_t t = blockIdx.x * kNmsFlatBlock + threadIdx.x;
  unsigned long long kept = 0;
  if (t < a.n) {
    const uint32_t st = a.state[t];
    const int32_t row = a.bvh.prim_id[t];
    a.out_keep[row] = st == kNmsKept ? 1 : 0;
    if (a.out_cover && st != kNmsDropped) a.out_cover[row] = st == kNmsKept ? a.bvh.points[t].id : -1;
    kept = st == kNmsKept ? 1u : 0u;
  }
  kept = t_wave_sum(kept);
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&a.ws[kNmsWsKept], kept);
}
struct NmsIsKept {
  __host__ __device__ int32_t operator()(uint32_t st) const { return st == kNmsKept ? 1 : 0; }
};

}  // namespace

void Engine::radius_nms(const tknnRadiusNmsOptions &o, tknnRadiusNmsInfo *info, hipStream_t s) {
  const int64_t n = bvh_.size();
  const int32_t clouds = num_clouds();
  // the call's workspace (the layout: the file head)
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t select_bytes = 0, reduce_bytes = 0;
  {
    int32_t *null_i32 = nullptr;
    uint8_t *null_u8 = nullptr;
    uint32_t *null_u32 = nullptr;
    OWLMI_HIP(rocprim::select(nullptr, select_bytes, null_i32, null_u8, null_i32, null_u32, (size_t)n, s));
    if (o.d_counts)
      OWLMI_HIP(rocprim::segmented_reduce(nullptr, reduce_bytes, rocprim::make_transform_iterator(null_u32, NmsIsKept{}), null_i32, (unsigned int)clouds,
                                          null_i32, null_i32, rocprim::plus<int32_t>(), (int32_t)0, s));
  }
  const size_t words_b = align(kNmsWsWords * sizeof(unsigned long long)), lens_b = align(4 * sizeof(uint32_t)),
               keys_b = align((size_t)n * sizeof(unsigned long long)), col_b = align((size_t)n * sizeof(int32_t)), flags_b = align((size_t)n),
               tmp_b = align(std::max(select_bytes, reduce_bytes));
  char *ws = (char *)workspace(words_b + lens_b + keys_b + 4 * col_b + flags_b + tmp_b);
  int32_t *lists[2] = {(int32_t *)(ws + words_b + lens_b + keys_b + col_b), (int32_t *)(ws + words_b + lens_b + keys_b + 2 * col_b)};
  void *tmp = ws + words_b + lens_b + keys_b + 4 * col_b + flags_b;

  NmsArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.wide = bvh_.wide_view();
  a.tree_keys = bvh_.keys_device();
  a.starts = batched() ? batch_starts_ : nullptr;
  a.num_batches = num_batches_;
  a.key_bits = batch_bits_;
  a.n = (int32_t)n;
  a.radius = o.radius;
  a.radius_wide = o.radius * 1.000001f;
  a.mode = o.d_scores ? kNmsByScore : (o.flags & TKNN_NMS_BY_NAME) ? kNmsByName : kNmsByHash;
  if (const char *e = getenv("TKNN_NMS_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.scores = o.d_scores;
  a.ws = (unsigned long long *)ws;
  a.lens = (uint32_t *)(ws + words_b);
  a.keys = (unsigned long long *)(ws + words_b + lens_b);
  a.state = (uint32_t *)(ws + words_b + lens_b + keys_b);
  a.redo = (int32_t *)(ws + words_b + lens_b + keys_b + 3 * col_b);
  a.flags = (uint8_t *)(ws + words_b + lens_b + keys_b + 4 * col_b);
  a.out_keep = o.d_keep;
  a.out_cover = o.d_cover;

  const unsigned flat_blocks = (unsigned)((n + kNmsFlatBlock - 1) / kNmsFlatBlock);
  auto walks = [&](bool cover, int64_t items) {  // one walk launch over `items` list positions at most, and its lane kernel
    OWLMI_HIP(hipMemsetAsync(a.ws, 0, 2 * sizeof(unsigned long long), s));  // kNmsWsCursor, kNmsWsRedo
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 3) / 4, (int64_t)cu_count_ * kNmsBlocksPerCu));
    const unsigned lane_blocks =
        (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kNmsLaneBlock - 1) / kNmsLaneBlock, (int64_t)cu_count_ * kNmsLaneBlocksPerCu));
    if (cover) {
      hipLaunchKernelGGL(nms_walk_kernel<true>, dim3(blocks), dim3(kNmsBlock), 0, s, a);
      hipLaunchKernelGGL(nms_lane_kernel<true>, dim3(lane_blocks), dim3(kNmsLaneBlock), 0, s, a);
    } else {
      hipLaunchKernelGGL(nms_walk_kernel<false>, dim3(blocks), dim3(kNmsBlock), 0, s, a);
      hipLaunchKernelGGL(nms_lane_kernel<false>, dim3(lane_blocks), dim3(kNmsLaneBlock), 0, s, a);
    }
    OWLMI_HIP(hipGetLastError());
  };

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kNmsWsWords * sizeof(unsigned long long), s));
  a.list = lists[0];
  hipLaunchKernelGGL(nms_init_kernel, dim3(flat_blocks), dim3(kNmsFlatBlock), 0, s, a);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  // The rounds.  `have`: the current list's length as the host knows it -- for the first list its bound n (the flags behind
  // n - nan are 0), afterwards the word read back.  A round that leaves as many items as it had decided nothing (with the
  // bound, the first round's stall shows one round later).
  uint32_t *h_len = (uint32_t *)(h_counters_ + kNmsWsWords);
  int64_t have = n, rounds = 0;
  int cur = 0;
  bool stalled = false, out_of_rounds = false;
  for (;;) {
    a.list = lists[cur];
    a.len = a.lens + cur;
    walks(false, have);
    size_t bytes = select_bytes;
    OWLMI_HIP(rocprim::select(tmp, bytes, lists[cur], a.flags, lists[cur ^ 1], a.lens + (cur ^ 1), (size_t)have, s));
    OWLMI_HIP(hipMemcpyAsync(h_len, a.lens + (cur ^ 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
    rounds++;
    const int64_t left = (int64_t)*h_len;
    if (left == 0) break;
    if (left >= have) {
      stalled = true;
      break;
    }
    if (o.max_rounds > 0 && rounds >= o.max_rounds) {
      out_of_rounds = true;
      break;
    }
    have = left;
    cur ^= 1;
  }
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  unsigned long long *h_words = h_counters_;
  auto fill_info = [&](hipEvent_t last) {
    if (!info) return;
    info->kept = (int64_t)h_words[kNmsWsKept];
    info->eligible = (int64_t)h_words[kNmsWsEligible];
    info->bad_scores = (int64_t)h_words[kNmsWsBadScores];
    info->rounds = rounds;
    info->fallback_items = (int64_t)h_words[kNmsWsFallback];
    info->point_tests = (int64_t)h_words[kNmsWsPointTests];
    info->node_tests = (int64_t)h_words[kNmsWsNodeTests];
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, last));
    OWLMI_HIP(hipEventElapsedTime(&info->init_ms, ev_a_, ev_b_));
    OWLMI_HIP(hipEventElapsedTime(&info->rounds_ms, ev_b_, ev_c_));
  };
  if (stalled || out_of_rounds) {
    OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kNmsWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
    fill_info(ev_c_);
    if (info) info->undecided = (int64_t)*h_len;
    throw ArgError{TKNN_E_STATE, stalled ? "tknnRadiusNms: round " + std::to_string(rounds) + " decided no point (a bug: the strongest undecided point of a cloud can be decided)"
                                         : "tknnRadiusNms: max_rounds = " + std::to_string(o.max_rounds) + " rounds left points undecided; nothing was written"};
  }
  // the outputs
  hipLaunchKernelGGL(nms_scatter_kernel, dim3(flat_blocks), dim3(kNmsFlatBlock), 0, s, a);
  OWLMI_HIP(hipGetLastError());
  if (o.d_counts) {
    const int32_t *offsets = a.starts ? a.starts : (const int32_t *)(a.lens + 2);
    size_t bytes = reduce_bytes;
    OWLMI_HIP(rocprim::segmented_reduce(tmp, bytes, rocprim::make_transform_iterator(a.state, NmsIsKept{}), o.d_counts, (unsigned int)clouds, offsets, offsets + 1,
                                        rocprim::plus<int32_t>(), (int32_t)0, s));
  }
  if (o.d_cover) {
    a.list = nullptr;
    a.len = a.lens + 3;
    walks(true, n);
  }
  OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kNmsWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  fill_info(ev_d_);
  if (info) OWLMI_HIP(hipEventElapsedTime(&info->cover_ms, ev_c_, ev_d_));
}

}  // namespace owlmi
