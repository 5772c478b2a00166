// fps.hip -- farthest point sampling inside each cloud of a built point tree (tknnFps, include/owlknn_fps.h), pruned by the tree's
// 64-ary box pyramid.
//
// A cloud is one range [s, e) of sorted slots (a plain tree: [0, n - nan); a batched one: batch_knn.hip's starts).  ONE workgroup
// of one wave owns a cloud for all of its w_b samples: the iterations of a cloud are a chain, clouds are independent, and nothing
// in here waits for another workgroup -- the only barriers are the workgroup's own, every loop has a step count (w_b samples, the
// pyramid's levels, a cloud's boxes).
//   state. D, 4 bytes per slot: the running squared distance of an unchosen eligible slot, -1 once the slot is chosen.  Per level
//      l of the pyramid and per box c that touches the cloud, M = the largest key ((D bits << 32) | ~name) over the box's unchosen
//      slots of the cloud (0: none) and the slot that holds it.  A box may straddle a cloud boundary, so M is kept per (box,
//      cloud): cloud b's copy of box c of a level is entry c + b of that level's arrays -- ((e - 1) >> sh) + b < (e >> sh) + b + 1,
//      so the entries of consecutive clouds never meet, and a level takes count[l] + B entries.  All of it lives in the engine's
//      grow-only workspace.
//   1. fps_init_kernel: D = +inf, the keys of the cloud's blocks and of the boxes above them up to the cloud's top level, and the
//      slot of d_start_rows[b] (-1: the default).
//   2. fps_walk_kernel: per sample a depth-first walk from the cloud's top level (the lowest one at which it touches <= 64 boxes).
//      Lanes are the 64 children of a box on the way down and the 16 slots of four blocks at the leaves; an LDS stack holds the
//      entered children and, under them, their parent's "recompute" entry, so M is rebuilt bottom-up on the way back.  A child is
//      tested against the M it had before this sample touched it: only its own subtree's way back writes it.  The maximum over
//      the top boxes, which the last entry of the walk computes, is the next sample.
// The rule that decides which blocks are visited and why it drops nothing: include/owlknn_fps.h.
#include "owlknn_fps.h"
#include "team_lanes.h"
#include "team_walk.h"  // box_min_dist2
#include "trueknn_engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kFpsBlock = 64;                        // one wave per workgroup, one workgroup per cloud
constexpr int kFpsStack = 65 * LBVH_WIDE_LEVELS + 2;  // per level at most 64 entered children and their parent's recompute entry
enum { kFpsWsSamples, kFpsWsPointTests, kFpsWsNodeTests, kFpsWsBadStarts, kFpsWsWords };

struct FpsArgs {
  const LbvhPoint *points;    // sorted, padded with NaN sentinels to whole blocks
  const int32_t *row_slot;    // n: the sorted slot of a row of the caller's buffer
  const int32_t *nan_count;   // device: the points with a NaN (the last sorted slots)
  LbvhWideView wide;
  const int32_t *starts;      // num_clouds + 1 (null: a plain tree, one cloud [0, n - nan))
  int32_t n;
  int32_t num_clouds;
  int32_t S;                  // num_samples: the row stride
  int no_prune;
  const int32_t *num;         // num_clouds (may be null)
  const int32_t *start_rows;  // num_clouds (may be null)
  float *D;                   // whole blocks of slots
  unsigned long long *key[LBVH_WIDE_LEVELS];  // per level: count[l] + num_clouds keys, cloud b's box c at c + b
  int32_t *arg[LBVH_WIDE_LEVELS];             // ... and the slot that holds the key (-1: none)
  int32_t *first_slot;        // num_clouds: the slot of the cloud's start row, -1: the default
  int32_t *out_idx;           // num_clouds * S
  float *out_dist;            // num_clouds * S (may be null)
  int32_t *out_counts;        // num_clouds (may be null)
  unsigned long long *ws;     // kFpsWsWords counters
};

struct FpsLevel {  // a level's arrays, in LDS: the walk picks its level at run time
  unsigned long long *key;
  int32_t *arg;
  const LbvhBox *boxes;
};
__device__ __forceinline__ void fps_fill_levels(FpsLevel *lv, const FpsArgs &a, int lane) {
#pragma unroll
  for (int l = 0; l < LBVH_WIDE_LEVELS; l++)
    if (lane == l) lv[l] = FpsLevel{a.key[l], a.arg[l], a.wide.level[l]};
}

__device__ __forceinline__ void fps_range(const FpsArgs &a, int b, int32_t &s, int32_t &e) {
  if (a.starts)
    s = a.starts[b], e = a.starts[b + 1];
  else
    s = 0, e = a.n - *a.nan_count;
}
// a slot's key: larger D first, among equal D bits the smaller name (no name is negative, so no key of a slot is 0)
__device__ __forceinline__ unsigned long long fps_key(float d, int32_t name) {
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)name);
}
__device__ __forceinline__ float fps_key_d(unsigned long long k) { return __uint_as_float((uint32_t)(k >> 32)); }
// child c of level l covers the slots [c << sh, (c + 1) << sh) (every slot is below 2^31: a shift by 31 gives the same zeros)
__device__ __forceinline__ int fps_shift(int lvl) { return min(4 + 6 * lvl, 31); }
// the lowest level at which [s, e) touches at most 64 boxes (the tree's top level has at most 64)
__device__ __forceinline__ int fps_top_level(const FpsArgs &a, int32_t s, int32_t e) {
  int l = 0;
  while (l < a.wide.levels - 1 && ((e - 1) >> fps_shift(l)) - (s >> fps_shift(l)) + 1 > 64) l++;
  return l;
}
// max over the 16 lanes of my team, result in every lane of the team: DPP row rotations, no LDS crossbar
__device__ __forceinline__ uint32_t fps_team_max_u32(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128 /*row_ror:8*/, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124 /*row_ror:4*/, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122 /*row_ror:2*/, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121 /*row_ror:1*/, 0xf, 0xf, false));
  return v;
}
// ... of 64-bit keys: the largest high word, then the largest low word among the lanes that hold it
__device__ __forceinline__ unsigned long long fps_team_max(unsigned long long v) {
  const uint32_t hi = (uint32_t)(v >> 32), top = fps_team_max_u32(hi);
  return ((unsigned long long)top << 32) | fps_team_max_u32(hi == top ? (uint32_t)v : 0u);
}
// the largest key over the wave's lanes and the slot its lane holds (0, -1: no lane has a key): the four teams' maxima meet in
// scalar registers
__device__ __forceinline__ void fps_wave_best(unsigned long long k, int32_t ar, unsigned long long &best, int32_t &best_arg) {
  const unsigned long long tk = fps_team_max(k);
  best = 0ull;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const unsigned long long other = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(tk >> 32), 16 * t) << 32) |
                                     (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)tk, 16 * t);
    best = max(best, other);
  }
  const unsigned long long win = __ballot(k == best && k != 0ull);
  best_arg = win ? __builtin_amdgcn_readlane(ar, __ffsll((long long)win) - 1) : -1;
}

// Lanes as the 16 slots of block `blk` (has: my team has a block in this step).  INIT: D = +inf for the slots of [s, e);
// otherwise D = min(D, d2 to the sample sp) for the unchosen ones, and the sample's own slot `cur` leaves the running.  tk, targ:
// the block's key and its slot over the unchosen slots of [s, e), in every lane of the team.
template <bool INIT>
__device__ __forceinline__ void fps_block(const FpsArgs &a, int32_t s, int32_t e, int32_t blk, bool has, int team, int tl, const LbvhPoint &sp, int32_t cur,
                                          unsigned long long &tk, int32_t &targ) {
  const int32_t slot = blk * LBVH_BLOCK + tl;
  const bool in = has && slot >= s && slot < e;
  LbvhPoint p = LbvhPoint{0.f, 0.f, 0.f, -1};
  float d = -1.f;
  if (in) {
    p = a.points[slot];
    d = INIT ? INFINITY : a.D[slot];
  }
  if (!INIT && in && d >= 0.f) {
    d = fminf(d, knn_dist2(p.x, p.y, p.z, sp.x, sp.y, sp.z));
    if (slot == cur) d = -1.f;
  }
  if (in && (INIT || d != -1.f || slot == cur)) a.D[slot] = d;
  const unsigned long long k = in && d >= 0.f ? fps_key(d, p.id) : 0ull;
  tk = fps_team_max(k);
  const uint32_t win = (uint32_t)(__ballot(k == tk && k != 0ull) >> (team << 4)) & 0xffffu;
  targ = win ? blk * LBVH_BLOCK + (__ffs((int)win) - 1) : -1;
}

// ---- 1. the state of a cloud before its first sample --------------------------------------------------------------------------------
__global__ void __launch_bounds__(kFpsBlock) fps_init_kernel(FpsArgs a) {
  __shared__ FpsLevel lv[LBVH_WIDE_LEVELS];
  const int b = blockIdx.x, lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  fps_fill_levels(lv, a, lane);
  int32_t s, e;
  fps_range(a, b, s, e);
  if (lane == 0) {  // the start row: a row of the caller's buffer whose slot lies in the cloud (a NaN point's lies behind every cloud)
    int32_t first = -1;
    const int32_t r = a.start_rows ? a.start_rows[b] : -1;
    if (r >= 0) {
      if (r < a.n) {
        const int32_t at = a.row_slot[r];
        if (at >= s && at < e) first = at;
      }
      if (first < 0) atomicAdd(&a.ws[kFpsWsBadStarts], 1ull);
    }
    a.first_slot[b] = first;
  }
  if (e <= s) return;
  __syncthreads();
  const int top = fps_top_level(a, s, e);
  const LbvhPoint none = LbvhPoint{0.f, 0.f, 0.f, -1};
  const int32_t b0 = s >> 4, b1 = (e - 1) >> 4;
  for (int32_t base = b0; base <= b1; base += 4) {
    const int32_t blk = base + team;
    const bool has = blk <= b1;
    unsigned long long tk;
    int32_t targ;
    fps_block<true>(a, s, e, blk, has, team, tl, none, -1, tk, targ);
    if (has && tl == 0) lv[0].key[(int64_t)blk + b] = tk, lv[0].arg[(int64_t)blk + b] = targ;
  }
  for (int l = 1; l <= top; l++) {
    __syncthreads();  // the level below is written
    const int32_t c0 = s >> fps_shift(l), c1 = (e - 1) >> fps_shift(l), k0 = s >> fps_shift(l - 1), k1 = (e - 1) >> fps_shift(l - 1);
    for (int32_t c = c0; c <= c1; c++) {
      const int64_t child = (int64_t)c * 64 + lane;
      const bool valid = child >= k0 && child <= k1;
      const unsigned long long k = valid ? lv[l - 1].key[child + b] : 0ull;
      const int32_t ar = valid ? lv[l - 1].arg[child + b] : -1;
      unsigned long long best;
      int32_t best_arg;
      fps_wave_best(k, ar, best, best_arg);
      if (lane == 0) lv[l].key[(int64_t)c + b] = best, lv[l].arg[(int64_t)c + b] = best_arg;
    }
  }
}

// ---- 2. the samples of a cloud -------------------------------------------------------------------------------------------------------
// A stack entry: bit 30 -- recompute the parent's key from its children's --, bits 26 .. 28 the children's level, the low bits the
// parent's index at the level above (the cloud's top level has no parent: its children are the boxes c0 .. c1 <= c0 + 63).
__global__ void __launch_bounds__(kFpsBlock) fps_walk_kernel(FpsArgs a) {
  __shared__ FpsLevel lv[LBVH_WIDE_LEVELS];
  __shared__ uint32_t stack[kFpsStack];
  __shared__ unsigned long long child_key[64];
  __shared__ int32_t child_arg[64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  fps_fill_levels(lv, a, lane);
  int32_t s, e;
  fps_range(a, b, s, e);
  int32_t w = min(a.S, max(e - s, 0));
  if (a.num) w = min(w, max(a.num[b], 0));
  const int64_t row = (int64_t)b * a.S;
  for (int32_t j = w + lane; j < a.S; j += kFpsBlock) {
    a.out_idx[row + j] = -1;
    if (a.out_dist) a.out_dist[row + j] = INFINITY;
  }
  if (lane == 0 && a.out_counts) a.out_counts[b] = w;
  if (w == 0) return;
  __syncthreads();
  const int top = fps_top_level(a, s, e);
  unsigned long long node_tests = 0, point_tests = 0;
  int32_t cur = a.first_slot[b];
  float cur_d = INFINITY;
  if (cur < 0) {  // the default: every D is +inf, so the largest key is the smallest name
    const int64_t c = (int64_t)(s >> fps_shift(top)) + lane;
    const bool valid = c <= ((e - 1) >> fps_shift(top));
    unsigned long long best;
    fps_wave_best(valid ? lv[top].key[c + b] : 0ull, valid ? lv[top].arg[c + b] : -1, best, cur);
  }
  for (int32_t it = 0; it < w && cur >= 0; it++) {
    const LbvhPoint sp = a.points[cur];
    if (lane == 0) {
      a.out_idx[row + it] = sp.id;
      if (a.out_dist) a.out_dist[row + it] = knn_sqrt(cur_d);
    }
    unsigned long long next_key = 0ull;
    int32_t next_arg = -1;
    int sp_n = 1;
    if (lane == 0) stack[0] = (uint32_t)top << 26;
    while (sp_n > 0) {
      __syncthreads();  // the stack, and the keys written on the way back
      const uint32_t en = stack[--sp_n];
      const bool recompute = (en >> 30) & 1u;
      const int lvl = (int)((en >> 26) & 7u);
      const int32_t parent = (int32_t)(en & 0x3ffffffu);
      const int sh = fps_shift(lvl);
      const int32_t c0 = s >> sh, c1 = (e - 1) >> sh;
      const int64_t base = lvl == top ? (int64_t)c0 : (int64_t)parent * 64;
      const int64_t c = base + lane;
      const bool valid = c >= c0 && c <= c1;
      unsigned long long k = valid ? lv[lvl].key[c + b] : 0ull;
      int32_t ar = valid ? lv[lvl].arg[c + b] : -1;
      if (!recompute) {
        LbvhBox bx = LbvhBox{{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
        if (valid) bx = lv[lvl].boxes[c];
        node_tests += valid ? 1u : 0u;
        const bool own = valid && (int64_t)(cur >> sh) == c;
        const bool enter = valid && (a.no_prune || own || box_min_dist2(bx, sp) < fps_key_d(k));
        unsigned long long mask = __ballot(enter);
        if (lvl > 0) {  // the children's way back under the children
          if (lane == 0) stack[sp_n] = en | (1u << 30);
          if (enter) stack[sp_n + 1 + t_rank(mask)] = ((uint32_t)(lvl - 1) << 26) | (uint32_t)c;
          sp_n += 1 + __popcll(mask);
          continue;
        }
        // the children are blocks: four at a time, their new keys beside the others' in LDS
        child_key[lane] = k;
        child_arg[lane] = ar;
        t_wave_sync();
        while (mask) {
          int j = -1;
#pragma unroll
          for (int t = 0; t < 4; t++) {
            const int pos = mask ? __ffsll((long long)mask) - 1 : -1;
            j = t == team ? pos : j;
            mask &= mask - 1ull;
          }
          const bool has = j >= 0;
          const int32_t blk = (int32_t)base + max(j, 0);
          unsigned long long tk;
          int32_t targ;
          fps_block<false>(a, s, e, blk, has, team, tl, sp, cur, tk, targ);
          if (has && tl == 0) {
            child_key[j] = tk, child_arg[j] = targ;
            lv[0].key[(int64_t)blk + b] = tk, lv[0].arg[(int64_t)blk + b] = targ;
            point_tests += LBVH_BLOCK;
          }
        }
        t_wave_sync();
        k = child_key[lane];
        ar = child_arg[lane];
      }
      unsigned long long best;
      int32_t best_arg;
      fps_wave_best(k, ar, best, best_arg);
      if (lvl == top)
        next_key = best, next_arg = best_arg;
      else if (lane == 0)
        lv[lvl + 1].key[(int64_t)parent + b] = best, lv[lvl + 1].arg[(int64_t)parent + b] = best_arg;
    }
    cur = next_arg;
    cur_d = fps_key_d(next_key);
  }
  const unsigned long long nt = t_wave_sum(node_tests), pt = t_wave_sum(point_tests);
  if (lane == 0) {
    atomicAdd(&a.ws[kFpsWsSamples], (unsigned long long)w);
    atomicAdd(&a.ws[kFpsWsPointTests], pt);
    atomicAdd(&a.ws[kFpsWsNodeTests], nt);
  }
}

}  // namespace

void Engine::fps(const tknnFpsOptions &o, tknnFpsInfo *info, hipStream_t s) {
  const int32_t clouds = num_clouds();
  const LbvhWideView wv = bvh_.wide_view();
  // the call's workspace: counters | D | start slots | per level: keys, slots
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t words_b = align(kFpsWsWords * sizeof(unsigned long long));
  const size_t d_b = align((size_t)wv.count[0] * LBVH_BLOCK * sizeof(float)), first_b = align((size_t)clouds * sizeof(int32_t));
  size_t total = words_b + d_b + first_b;
  for (int l = 0; l < wv.levels; l++) total += align(((size_t)wv.count[l] + clouds) * sizeof(unsigned long long)) + align(((size_t)wv.count[l] + clouds) * sizeof(int32_t));
  char *ws = (char *)workspace(total);

  FpsArgs a;
  std::memset(&a, 0, sizeof a);
  const LbvhView bv = bvh_.view();
  a.points = bv.points;
  a.row_slot = bvh_.row_slot_device();
  a.nan_count = bv.nan_count;
  a.wide = wv;
  a.starts = batched() ? batch_starts_ : nullptr;
  a.n = (int32_t)bvh_.size();
  a.num_clouds = clouds;
  a.S = o.num_samples;
  a.no_prune = (o.flags & TKNN_FPS_NO_PRUNE) != 0;
  a.num = o.d_num;
  a.start_rows = o.d_start_rows;
  a.out_idx = o.d_idx;
  a.out_dist = o.d_dist;
  a.out_counts = o.d_counts;
  a.ws = (unsigned long long *)ws;
  char *at = ws + words_b;
  a.D = (float *)at, at += d_b;
  a.first_slot = (int32_t *)at, at += first_b;
  for (int l = 0; l < wv.levels; l++) {
    a.key[l] = (unsigned long long *)at, at += align(((size_t)wv.count[l] + clouds) * sizeof(unsigned long long));
    a.arg[l] = (int32_t *)at, at += align(((size_t)wv.count[l] + clouds) * sizeof(int32_t));
  }

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kFpsWsWords * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(fps_init_kernel, dim3((unsigned)clouds), dim3(kFpsBlock), 0, s, a);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  hipLaunchKernelGGL(fps_walk_kernel, dim3((unsigned)clouds), dim3(kFpsBlock), 0, s, a);
  OWLMI_HIP(hipGetLastError());
  unsigned long long *h_words = h_counters_;
  OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kFpsWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->samples = (int64_t)h_words[kFpsWsSamples];
    info->point_tests = (int64_t)h_words[kFpsWsPointTests];
    info->node_tests = (int64_t)h_words[kFpsWsNodeTests];
    info->bad_starts = (int64_t)h_words[kFpsWsBadStarts];
    info->lds_clouds = 0;
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_c_));
    OWLMI_HIP(hipEventElapsedTime(&info->init_ms, ev_a_, ev_b_));
    OWLMI_HIP(hipEventElapsedTime(&info->walk_ms, ev_b_, ev_c_));
  }
}

}  // namespace owlmi
