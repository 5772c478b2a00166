// radius_query.hip -- fixed-radius neighbour lists for query points that are NOT in the tree (tknnRadiusQuery, include/owlknn.h).
//
// Row j holds the points p of the built set with sqrt((dx*dx + dy*dy) + dz*dz) <= radius, every operation fp32 and uncontracted:
// knn_sqrt(knn_dist2(..)) <= r, the predicate of RT-DBSCAN (db_device.h), so a row's length is the count tknnDbscanQuery gives.  Rows are
// CSR: a COUNT pass writes the exclusive scan of the row lengths into d_offsets, a FILL pass writes row j into its segment
// d_offsets[j] .. d_offsets[j + 1] and never outside it (the two passes of tknnHaloSelect).
//   1. query_order (query_order.h): the queries along the tree's own curve, as tknnQuery orders them;
//   2. radius_walk_kernel<FILL>: persistent, one 16-lane team per query, four teams per wave, walk_tree (team_walk.h) with the
//      query's box of half-width r; the lanes of a team test the 16 points of a leaf block with the sphere predicate.  A child
//      box wholly inside the sphere is not walked: the count pass adds its slots arithmetically, the fill pass streams them;
//   3. radius_lane_kernel<FILL>: one query per lane on the rope walk (lane_walk.h), for the queries whose team stack overflowed
//      (a redo list whose length lives on the device, as query_lane_kernel's) -- the result is complete on any tree;
//   4. count pass: a device exclusive scan of the uint32 row lengths into the caller's int64 offsets;
//      fill pass with sort = 1: the walk wrote 64-bit keys (distance bits << 32 | index; distances are non-negative, so their
//      bits order like their values), a segmented radix sort over the offsets orders every row, a split kernel writes the
//      caller's arrays.
#include "lane_walk.h"
#include "query_order.h"
#include "team_lanes.h"
#include "team_walk.h"
#include "trueknn_engine.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

namespace owlmi {

namespace {

constexpr int kRadiusBlock = 64;        // one wave per workgroup, four teams
constexpr int kRadiusBlocksPerCu = 16;  // 7.5 KB of LDS each
constexpr int kRadiusLaneBlock = 256;
constexpr int kSplitBlock = 256;
constexpr int kStageCapacity = 32;  // keys a team holds back until sixteen can be written at once (at most 15 wait when a block adds 16)
constexpr int kRangeCapacity = 16;  // inside boxes above the leaf level a team's fill walk notes for streaming; a 17th is walked

// words of the call's own counters (in the workspace, zeroed per pass)
enum { kWsCursor = 0, kWsRedo = 1, kWsTotal = 2, kWsMaxRow = 3, kWsMismatched = 4, kWsNodeTests = 5, kWsPointTests = 6, kWsWords = 8 };

struct RadiusKernelArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const float *queries;   // m packed triples, caller order
  const uint32_t *order;  // m: the query worked on at sorted position i
  int32_t m;
  float radius;
  float radius_wide;  // radius * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts
  float radius_in2;   // radius^2 * 0.999995, rounded down: a box whose far corner is within it lies inside the sphere
  int force_redo;     // TKNN_RADIUS_FORCE_FALLBACK (tests): the walk leaves every query to the lane kernel
  uint32_t *counts;   // count pass: m row lengths, by the caller's j
  const int64_t *offsets;    // fill pass: m + 1, the caller's
  int64_t total;             // fill pass: offsets[m] as the host read it
  unsigned long long *keys;  // fill pass, sort = 1: `total` keys in the workspace (then out_idx / out_dist are the split kernel's)
  int32_t *out_idx;          // fill pass, sort = 0
  float *out_dist;           // fill pass, sort = 0 (may be null)
  int32_t *redo;             // m: queries left to the lane kernel
  unsigned long long *ws;    // kWsWords counters
};

// ---- a row's segment ---------------------------------------------------------------------------------------------------------
struct RadiusRow {
  int64_t base;
  uint32_t len;
  bool valid;
};
// The segment the caller's offsets give query qi; offsets that do not describe a segment inside [0, total) give an empty one, so
// nothing is written for the row, and it is counted as mismatched whatever its length (the row sort never sees such offsets).
__device__ __forceinline__ RadiusRow radius_row(const RadiusKernelArgs &a, int32_t qi, bool has_q) {
  RadiusRow row = {0, 0u, !has_q};
  if (has_q) {
    const int64_t b = a.offsets[qi], e = a.offsets[(int64_t)qi + 1];
    if (0 <= b && b <= e && e <= a.total) row.base = b, row.len = (uint32_t)(e - b), row.valid = true;
  }
  return row;
}
__device__ __forceinline__ void radius_store(const RadiusKernelArgs &a, int64_t at, unsigned long long key) {
  if (a.keys) {
    a.keys[at] = key;
  } else {
    a.out_idx[at] = (int32_t)(uint32_t)key;
    if (a.out_dist) a.out_dist[at] = __uint_as_float((uint32_t)(key >> 32));
  }
}
__device__ __forceinline__ void radius_add_stats(unsigned long long *ws, int lane, unsigned long long total, unsigned int max_row,
                                                 unsigned long long mismatched, unsigned long long node_tests, unsigned long long point_tests) {
  const unsigned long long tsum = t_wave_sum(total), msum = t_wave_sum(mismatched), nt = t_wave_sum(node_tests), pt = t_wave_sum(point_tests);
  unsigned int mx = max_row;  // (t_wave_max is a float's: a row length has 31 bits)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, off));
  if (lane == 0) {
    if (tsum) atomicAdd(&ws[kWsTotal], tsum);
    if (mx) atomicMax(&ws[kWsMaxRow], (unsigned long long)mx);
    if (msum) atomicAdd(&ws[kWsMismatched], msum);
    if (nt) atomicAdd(&ws[kWsNodeTests], nt);
    if (pt) atomicAdd(&ws[kWsPointTests], pt);
  }
}

// ---- 2. the walk -------------------------------------------------------------------------------------------------------------
// The box rule.  A child box lies wholly INSIDE the sphere if the squared distance far2 from q to its far corner is at most
// radius_in2.  The margin's direction: radius_in2 = r^2 * 0.999995 rounded DOWN, so the rule can only call fewer boxes inside
// than the exact one would -- a box is called inside only if every point of it certainly passes the literal test.  (For a point p
// of the box, lo <= p <= hi, and fp32 subtraction, multiplication and addition are monotone, so p's own dist2 as knn_dist2 rounds
// it is <= far2 <= r^2, and the correctly rounded root of a value <= r^2 is <= r.  The margin is the one the other counting rules
// keep, on top of that.)  Its slots must end before clean_end: NaN points sort last and are nobody's neighbour, and the padding of
// the last block is no point at all.
//   count pass: the box's slot count is added arithmetically, nothing below it is read;
//   fill pass:  the points have to be read for their id and distance.  A leaf block is kept and tested like any other; a box above
//               the leaf level is noted in the team's range list and streamed after the walk, the lanes striding its slots (its
//               child boxes are never read).  A full list: the box is walked.
// Hits of the fill pass wait in the team's LDS stage as keys, ballot-compacted, and are written sixteen at a time at the row's
// cursor, so the writes of a row are contiguous 128-byte pieces.  Teams of a wave loop in lock step: no __syncthreads, only
// t_wave_sync.
template <bool FILL>
__global__ void __launch_bounds__(kRadiusBlock) __attribute__((amdgpu_waves_per_eu(4))) radius_walk_kernel(RadiusKernelArgs a) {
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[LBVH_WIDE_LEVELS];
  __shared__ unsigned long long stage_mem[FILL ? 4 * kStageCapacity : 1];
  __shared__ int32_t range_mem[FILL ? 4 * kRangeCapacity : 1];
  __shared__ uint32_t range_n_mem[4];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  unsigned long long *stage = stage_mem + (FILL ? team * kStageCapacity : 0);
  int32_t *range = range_mem + (FILL ? team * kRangeCapacity : 0);
  uint32_t *range_n = range_n_mem + team;
  walk_fill_levels<1>(levels, &a.wide, lane);
  if (tl == 0) *range_n = 0u;
  t_wave_sync();
  const LbvhWideView &wv = a.wide;
  const int32_t clean_end = lane_clean_end(a.bvh);
  unsigned long long node_tests = 0, point_tests = 0, total = 0, mismatched = 0;
  unsigned int max_row = 0;
  for (;;) {
    int got = 0;
    if (lane == 0) got = (int)atomicAdd(&a.ws[kWsCursor], 4ull);
    const int base = __builtin_amdgcn_readfirstlane(got);
    if (base >= a.m) break;
    const bool has_q = base + team < a.m;
    const int32_t qi = has_q ? (int32_t)a.order[base + team] : 0;
    LbvhPoint q;
    q.x = a.queries[3 * (int64_t)qi], q.y = a.queries[3 * (int64_t)qi + 1], q.z = a.queries[3 * (int64_t)qi + 2];
    q.id = -1;  // nothing is "self"
    const bool active = has_q && !a.force_redo;
    const WalkBox qb(q, a.radius_wide);
    const RadiusRow row = FILL ? radius_row(a, qi, has_q) : RadiusRow{0, 0u, true};
    uint32_t part = 0;               // count pass: my lane's share of the row length
    uint32_t wpos = 0, fill_n = 0;   // fill pass: entries of the row handed to memory, keys waiting in the stage (the same in a team's lanes)
    // the stage's first sixteen keys (`last`: whatever waits) to the row's cursor, the rest moved to the front
    auto flush = [&](bool last) __attribute__((always_inline)) {
      t_wave_sync();
      const bool go = last ? fill_n > 0u : fill_n >= 16u;
      const uint32_t nw = min(fill_n, 16u);
      const unsigned long long k0 = stage[tl], k1 = stage[16 + tl];
      if (go && (uint32_t)tl < nw && wpos + (uint32_t)tl < row.len) radius_store(a, row.base + wpos + tl, k0);
      t_wave_sync();
      if (go) {
        if (16u + (uint32_t)tl < fill_n) stage[tl] = k1;
        wpos += nw;
        fill_n -= nw;
      }
      t_wave_sync();
    };
    auto emit = [&](bool hit, int32_t id, float d) __attribute__((always_inline)) {
      const uint32_t mine16 = (uint32_t)(__ballot(hit) >> (team << 4)) & 0xffffu;  // my team's lanes with a hit
      if (hit) stage[fill_n + __popc(mine16 & ((1u << tl) - 1u))] = knn_key(d, id);
      fill_n += __popc(mine16);
      if (__ballot(fill_n >= 16u) != 0ull) flush(false);
    };
    // lane tl takes point tl of the sixteen slots from `slot0` (the sorted arrays are padded with NaN sentinels to whole blocks)
    auto test_points = [&](int64_t slot0, bool has_b) __attribute__((always_inline)) {
      LbvhPoint p = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
      if (has_b) p = a.bvh.points[slot0 + tl];
      const float d = knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z));
      const bool hit = has_b && d <= a.radius;  // (a NaN on either side: not a neighbour)
      point_tests += has_b ? 1u : 0u;
      if constexpr (FILL)
        emit(hit, p.id, d);
      else
        part = t_count(part, __ballot(hit));
    };
    bool overflow = wv.levels <= 0;
    if (wv.levels > 0)
      walk_tree<false>(
          levels, wv, stack, kWalkStack, active, q, qb, team, tl, node_tests,
          [&](const LbvhBox &bx, int32_t c, int lvl) {
            const float ax = fmaxf(fabsf(q.x - bx.lo[0]), fabsf(q.x - bx.hi[0])), ay = fmaxf(fabsf(q.y - bx.lo[1]), fabsf(q.y - bx.hi[1])),
                        az = fmaxf(fabsf(q.z - bx.lo[2]), fabsf(q.z - bx.hi[2]));
            const float far2 = t_dist2(ax, ay, az);
            const int64_t span = (int64_t)LBVH_BLOCK << (6 * lvl);  // points under one child of this level
            if (!(far2 <= a.radius_in2 && ((int64_t)c + 1) * span <= (int64_t)clean_end)) return true;
            if constexpr (!FILL) {
              part += (uint32_t)span;
              return false;
            } else {
              if (lvl == 0) return true;
              const uint32_t at = atomicAdd(range_n, 1u);
              if (at >= (uint32_t)kRangeCapacity) return true;
              range[at] = (lvl << 26) | c;
              return false;
            }
          },
          [&](int32_t b, bool has_b) { test_points((int64_t)b * LBVH_BLOCK, has_b); }, [] {}, overflow);
    if constexpr (FILL) {
      // the noted inside boxes, sixteen slots a step (every point passes; the literal test costs one compare and decides)
      t_wave_sync();
      const uint32_t nr = min(*range_n, (uint32_t)kRangeCapacity);
      for (uint32_t i = 0; __ballot(i < nr) != 0ull; i++) {
        const bool has_r = i < nr;
        const int32_t e = has_r ? range[i] : 0;
        const int64_t span = has_r ? (int64_t)LBVH_BLOCK << (6 * (e >> 26)) : 0;
        const int64_t first = (int64_t)(e & 0x3ffffff) * span;
        for (int64_t s = 0; __ballot(s < span) != 0ull; s += LBVH_BLOCK) test_points(first + s, s < span);
      }
      t_wave_sync();
      if (tl == 0) *range_n = 0u;
      if (__ballot(fill_n > 0u) != 0ull) flush(true);
      t_wave_sync();
    }
    const uint32_t cnt = FILL ? wpos : t_team_sum(part);
    if (has_q && tl == 0) {
      if (overflow || a.force_redo) {
        // left to the lane kernel, which starts the row again: nothing of it is counted here
        a.redo[atomicAdd(&a.ws[kWsRedo], 1ull)] = qi;
      } else {
        if constexpr (!FILL) a.counts[qi] = cnt;
        total += cnt;
        max_row = max(max_row, cnt);
        if (FILL && (cnt != row.len || !row.valid)) mismatched++;
      }
    }
  }
  radius_add_stats(a.ws, lane, total, max_row, mismatched, node_tests, point_tests);
}

// ---- 3. one query per lane: the queries of the redo list ---------------------------------------------------------------------------
template <bool FILL>
__global__ void __launch_bounds__(kRadiusLaneBlock) radius_lane_kernel(RadiusKernelArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kRadiusLaneBlock + threadIdx.x;
  const bool has_q = t < (int64_t)a.ws[kWsRedo];
  const int32_t qi = has_q ? a.redo[t] : 0;
  const int32_t clean_end = lane_clean_end(a.bvh);
  const LbvhPoint q = {a.queries[3 * (int64_t)qi], a.queries[3 * (int64_t)qi + 1], a.queries[3 * (int64_t)qi + 2], -1};  // no self
  const RadiusRow row = FILL ? radius_row(a, qi, has_q) : RadiusRow{0, 0u, true};
  uint32_t cnt = 0;
  unsigned long long node_tests = 0, point_tests = 0;
  if (has_q)
    lane_walk<LaneRope::kWithNode>(a.bvh,
        [&](int32_t ref, const LbvhNode &nd, int32_t) {
          node_tests++;
          if (!lane_box_hit(nd, q, a.radius_wide)) return lane_rope();
          if constexpr (!FILL) {  // a node inside the sphere is counted, not walked (db_count_from; the margin: radius_in2)
            float far2, near2;
            lane_box_dist2(nd, q, far2, near2);
            const int32_t first = lbvh_first(ref, nd.other), last = lbvh_last(ref, nd.other);
            if (far2 <= a.radius_in2 && last < clean_end) {
              cnt += (uint32_t)(last - first + 1);
              return lane_rope();
            }
          }
          return lane_descend();
        },
        [&](int32_t, const LbvhPoint &p) {
          point_tests++;
          const float d = knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z));
          if (d <= a.radius) {
            if constexpr (FILL)
              if (cnt < row.len) radius_store(a, row.base + cnt, knn_key(d, p.id));
            cnt++;
          }
          return lane_rope();
        });
  if constexpr (!FILL)
    if (has_q) a.counts[qi] = cnt;
  // (all lanes of the wave are here)
  radius_add_stats(a.ws, threadIdx.x & 63, has_q ? cnt : 0u, has_q ? cnt : 0u, FILL && has_q && (cnt != row.len || !row.valid) ? 1u : 0u, node_tests, point_tests);
}

// ---- 4. sorted keys into the caller's arrays -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSplitBlock) radius_split_kernel(const unsigned long long *__restrict__ keys, int64_t total, int32_t *__restrict__ out_idx,
                                                                  float *__restrict__ out_dist) {
  const int64_t i = (int64_t)blockIdx.x * kSplitBlock + threadIdx.x;
  if (i >= total) return;
  const unsigned long long key = keys[i];
  out_idx[i] = (int32_t)(uint32_t)key;
  if (out_dist) out_dist[i] = __uint_as_float((uint32_t)(key >> 32));
}

// r^2 * 0.999995 in double, rounded DOWN to fp32 (see the box rule)
inline float radius_inside2(float r) {
  const double want = (double)r * (double)r * 0.999995;
  float f = (float)want;
  if ((double)f > want) f = std::nextafterf(f, 0.f);
  return f;
}

}  // namespace

void Engine::radius_query(const tknnRadiusOptions &o, tknnRadiusInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const bool fill = o.d_idx != nullptr, sorted = fill && o.sort != 0;
  int64_t total = 0;
  if (fill) {
    // the one look at the caller's offsets: the fill pass's size
    int64_t *h_total = (int64_t *)(h_counters_ + kWsWords);
    OWLMI_HIP(hipMemcpyAsync(h_total, o.d_offsets + m, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
    total = *h_total;
    if (total < 0 || total > o.capacity)
      throw ArgError{TKNN_E_ARG, "tknnRadiusQuery: d_offsets[m] = " + std::to_string(total) + " neighbours do not fit the capacity of " + std::to_string(o.capacity)};
    if (total >= 0x80000000LL) throw ArgError{TKNN_E_UNSUPPORTED, "tknnRadiusQuery: 2^31 or more neighbours in one call: split the queries"};
  }
  // the call's workspace: counters | codes, order (+ the sort's second halves) | lane list | row lengths | keys, sorted keys | scan / sort space
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t order_bytes = query_order_sort_bytes(m, s);
  size_t scan_bytes = 0, seg_bytes = 0;
  uint32_t *null_u32 = nullptr;
  int64_t *null_i64 = nullptr;
  unsigned long long *null_key = nullptr;
  if (!fill) OWLMI_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, null_u32, null_i64, (int64_t)0, (size_t)m + 1, rocprim::plus<int64_t>(), s));
  const bool sorting = sorted && total > 0;
  if (sorting)
    OWLMI_HIP(rocprim::segmented_radix_sort_keys(nullptr, seg_bytes, null_key, null_key, (unsigned int)total, (unsigned int)m, o.d_offsets, o.d_offsets + 1, 0, 64, s));
  const size_t words_b = align(kWsWords * sizeof(unsigned long long)), col_b = align(((size_t)m + 1) * sizeof(uint32_t)),
               keys_b = sorting ? align((size_t)total * sizeof(unsigned long long)) : 0, tmp_b = align(std::max(order_bytes, std::max(scan_bytes, seg_bytes)));
  char *ws = (char *)workspace(words_b + 6 * col_b + 2 * keys_b + tmp_b);
  unsigned long long *d_words = (unsigned long long *)ws;
  uint32_t *codes = (uint32_t *)(ws + words_b), *codes_alt = (uint32_t *)(ws + words_b + col_b), *order_in = (uint32_t *)(ws + words_b + 2 * col_b),
           *order = (uint32_t *)(ws + words_b + 3 * col_b);
  int32_t *redo = (int32_t *)(ws + words_b + 4 * col_b);
  uint32_t *counts = (uint32_t *)(ws + words_b + 5 * col_b);
  unsigned long long *keys = (unsigned long long *)(ws + words_b + 6 * col_b), *keys_sorted = (unsigned long long *)(ws + words_b + 6 * col_b + keys_b);
  void *tmp = ws + words_b + 6 * col_b + 2 * keys_b;

  RadiusKernelArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.wide = bvh_.wide_view();
  a.queries = o.d_queries;
  a.order = order;
  a.m = (int32_t)m;
  a.radius = o.radius;
  a.radius_wide = o.radius * 1.000001f;
  a.radius_in2 = radius_inside2(o.radius);
  if (const char *e = getenv("TKNN_RADIUS_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.counts = counts;
  a.offsets = o.d_offsets;
  a.total = total;
  a.keys = sorting ? keys : nullptr;
  a.out_idx = o.d_idx;
  a.out_dist = o.d_dist;
  a.redo = redo;
  a.ws = d_words;

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(d_words, 0, kWsWords * sizeof(unsigned long long), s));
  if (!fill) OWLMI_HIP(hipMemsetAsync(counts + m, 0, sizeof(uint32_t), s));  // the scan runs over m + 1 lengths: offsets[m] is the total
  query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, tmp, order_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  // the walk, then the lane kernel for what the walk left
  const int blocks = (int)std::min<int64_t>((m + 3) / 4, (int64_t)cu_count_ * kRadiusBlocksPerCu);
  if (fill)
    hipLaunchKernelGGL(radius_walk_kernel<true>, dim3(blocks), dim3(kRadiusBlock), 0, s, a);
  else
    hipLaunchKernelGGL(radius_walk_kernel<false>, dim3(blocks), dim3(kRadiusBlock), 0, s, a);
  OWLMI_HIP(hipGetLastError());
  unsigned long long *h_words = h_counters_;
  OWLMI_HIP(hipMemcpyAsync(h_words, d_words, kWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (const unsigned long long n_redo = h_words[kWsRedo]) {
    const unsigned lane_blocks = (unsigned)((n_redo + kRadiusLaneBlock - 1) / kRadiusLaneBlock);
    if (fill)
      hipLaunchKernelGGL(radius_lane_kernel<true>, dim3(lane_blocks), dim3(kRadiusLaneBlock), 0, s, a);
    else
      hipLaunchKernelGGL(radius_lane_kernel<false>, dim3(lane_blocks), dim3(kRadiusLaneBlock), 0, s, a);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipMemcpyAsync(h_words, d_words, kWsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  }
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  const bool mismatch = fill && h_words[kWsMismatched] != 0;
  if (!fill) {
    OWLMI_HIP(rocprim::exclusive_scan(tmp, scan_bytes, counts, o.d_offsets, (int64_t)0, (size_t)m + 1, rocprim::plus<int64_t>(), s));
  } else if (sorting && !mismatch) {
    OWLMI_HIP(rocprim::segmented_radix_sort_keys(tmp, seg_bytes, keys, keys_sorted, (unsigned int)total, (unsigned int)m, o.d_offsets, o.d_offsets + 1, 0, 64, s));
    hipLaunchKernelGGL(radius_split_kernel, dim3((unsigned)((total + kSplitBlock - 1) / kSplitBlock)), dim3(kSplitBlock), 0, s, keys_sorted, total, o.d_idx,
                       o.d_dist);
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->total = (int64_t)h_words[kWsTotal];
    info->max_row = (int64_t)h_words[kWsMaxRow];
    info->mismatched = (int64_t)h_words[kWsMismatched];
    info->node_tests = (int64_t)h_words[kWsNodeTests];
    info->point_tests = (int64_t)h_words[kWsPointTests];
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_d_));
    OWLMI_HIP(hipEventElapsedTime(&info->order_ms, ev_a_, ev_b_));
    OWLMI_HIP(hipEventElapsedTime(&info->walk_ms, ev_b_, ev_c_));
    if (sorting && !mismatch) OWLMI_HIP(hipEventElapsedTime(&info->sort_ms, ev_c_, ev_d_));
  }
  if (mismatch)
    throw ArgError{TKNN_E_STATE, "tknnRadiusQuery: " + std::to_string(h_words[kWsMismatched]) +
                                     " rows differ in length from their segment in d_offsets (stale offsets, or another radius): run the count pass again"};
  if (!fill && h_words[kWsTotal] >= 0x80000000ull)
    throw ArgError{TKNN_E_UNSUPPORTED, "tknnRadiusQuery: 2^31 or more neighbours in one call: split the queries"};
}

}  // namespace owlmi
