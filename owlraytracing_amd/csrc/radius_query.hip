// radius_query.hip -- fixed-radius neighbour lists for query points that are NOT in the tree (tknnRadiusQuery, include/owlknn.h).
//
// Row j holds the points p of the built set with sqrt((dx*dx + dy*dy) + dz*dz) <= radius, every operation fp32 and uncontracted:
// knn_sqrt(knn_dist2(..)) <= r, the predicate of RT-DBSCAN (db_device.h), so a row's length is the count tknnDbscanQuery gives.  Rows are
// CSR: a COUNT pass writes the exclusive scan of the row lengths into d_offsets, a FILL pass writes row j into its segment
// d_offsets[j] .. d_offsets[j + 1] and never outside it (the two passes of tknnHaloSelect).
//   1. query_order (query_order.h): the queries along the tree's own curve, as tknnQuery orders them;
//   2. rad_walks (radius_walk.h: the walk, the box rule, the lane kernel for what the walk left) with one of two rules:
//      RadiusRule<false>, the count pass: a hit is counted, a box inside the sphere is a number of slots, the row is its length;
//      RadiusRule<true>, the fill pass: a hit is a 64-bit key in the team's LDS stage, written sixteen at a time into the row's
//      segment; the slots of an inside box are streamed.  A row that does not fit its segment is counted as mismatched;
//   3. count pass: a device exclusive scan of the uint32 row lengths into the caller's int64 offsets;
//      fill pass with sort = 1: the walk wrote 64-bit keys (distance bits << 32 | index; distances are non-negative, so their
//      bits order like their values), a segmented radix sort over the offsets orders every row, a split kernel writes the
//      caller's arrays.
#include "query_order.h"
#include "radius_walk.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

namespace owlmi {

namespace {

constexpr int kSplitBlock = 256;
constexpr int kStageCapacity = 32;  // keys a team holds back until sixteen can be written at once (at most 15 wait when a block adds 16)

struct RadiusKernelArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const float *queries;   // m packed triples, caller order
  const uint32_t *order;  // m: the query worked on at sorted position i
  int32_t m;
  float radius;
  float radius_wide;  // radius * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts
  float radius_in2;   // radius_inside2(radius): a box whose far corner is within it lies inside the sphere
  int force_redo;     // TKNN_RADIUS_FORCE_FALLBACK (tests): the walk leaves every query to the lane kernel
  uint32_t *counts;   // count pass: m row lengths, by the caller's j
  const int64_t *offsets;    // fill pass: m + 1, the caller's
  int64_t total;             // fill pass: offsets[m] as the host read it
  unsigned long long *keys;  // fill pass, sort = 1: `total` keys in the workspace (then out_idx / out_dist are the split kernel's)
  int32_t *out_idx;          // fill pass, sort = 0
  float *out_dist;           // fill pass, sort = 0 (may be null)
  int32_t *redo;             // m: positions left to the lane kernel
  unsigned long long *ws;    // kRadWords counters
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

// ---- 2. the rules of the two passes ------------------------------------------------------------------------------------------
// Hits of the fill pass wait in the team's LDS stage as keys, ballot-compacted, and are written sixteen at a time at the row's
// cursor, so the writes of a row are contiguous 128-byte pieces.
template <bool FILL>
struct RadiusRule {
  using Args = RadiusKernelArgs;
  static constexpr bool kArith = !FILL, kRolled = false;
  static constexpr int kTeamLds = FILL ? kStageCapacity : 0;
  struct Query {
    LbvhPoint q;
    int32_t row, self;  // (nothing is "self")
    float r, r_wide, in2;
    RadiusRow seg;
  };
  struct Lane {
    uint32_t wpos, fill_n;  // entries of the row handed to memory, keys waiting in the stage (the same in a team's lanes)
    unsigned long long *stage;
  };
  static __device__ __forceinline__ Query query(const Args &a, int32_t pos, bool has_q) {
    Query s;
    rad_point(a, pos, has_q, s.q, s.row);
    s.self = -1, s.r = a.radius, s.r_wide = a.radius_wide, s.in2 = a.radius_in2;
    s.seg = FILL ? radius_row(a, s.row, has_q) : RadiusRow{0, 0u, true};
    return s;
  }
  static __device__ __forceinline__ void start(Lane &st, unsigned long long *lds) { st.wpos = 0u, st.fill_n = 0u, st.stage = lds; }
  static __device__ __forceinline__ bool member(const Args &, const Query &s, int32_t, const LbvhPoint &, float d) { return d <= s.r; }
  // the stage's first sixteen keys (`last`: whatever waits) to the row's cursor, the rest moved to the front
  static __device__ __forceinline__ void flush(const Args &a, const Query &s, Lane &st, bool last, int tl) {
    t_wave_sync();
    const bool go = last ? st.fill_n > 0u : st.fill_n >= 16u;
    const uint32_t nw = min(st.fill_n, 16u);
    const unsigned long long k0 = st.stage[tl], k1 = st.stage[16 + tl];
    if (go && (uint32_t)tl < nw && st.wpos + (uint32_t)tl < s.seg.len) radius_store(a, s.seg.base + st.wpos + tl, k0);
    t_wave_sync();
    if (go) {
      if (16u + (uint32_t)tl < st.fill_n) st.stage[tl] = k1;
      st.wpos += nw;
      st.fill_n -= nw;
    }
    t_wave_sync();
  }
  static __device__ __forceinline__ void take(const Args &a, const Query &s, Lane &st, uint32_t &part, bool hit, int64_t, const LbvhPoint &p, float, float, float,
                                              float, float d, int team, int tl) {
    if constexpr (!FILL) {
      part = t_count(part, __ballot(hit));
    } else {
      const uint32_t mine16 = (uint32_t)(__ballot(hit) >> (team << 4)) & 0xffffu;  // my team's lanes with a hit
      if (hit) st.stage[st.fill_n + __popc(mine16 & ((1u << tl) - 1u))] = knn_key(d, p.id);
      st.fill_n += __popc(mine16);
      if (__ballot(st.fill_n >= 16u) != 0ull) flush(a, s, st, false, tl);
    }
  }
  static __device__ __forceinline__ uint32_t row_end(const Args &a, const Query &s, Lane &st, uint32_t part, int, int tl) {
    if constexpr (!FILL) {
      return t_team_sum(part);
    } else {
      if (__ballot(st.fill_n > 0u) != 0ull) flush(a, s, st, true, tl);
      return st.wpos;
    }
  }
  static __device__ __forceinline__ unsigned long long row_write(const Args &a, const Query &s, const Lane &, uint32_t cnt) {
    if constexpr (!FILL) a.counts[s.row] = cnt;
    return FILL && (cnt != s.seg.len || !s.seg.valid) ? 1u : 0u;
  }
  static __device__ __forceinline__ bool lane_arith(const Args &) { return !FILL; }
  static __device__ __forceinline__ void lane_take(const Args &a, const Query &s, Lane &, uint32_t cnt, int32_t, const LbvhPoint &p, float, float, float, float,
                                                   float d) {
    if constexpr (FILL)
      if (cnt < s.seg.len) radius_store(a, s.seg.base + cnt, knn_key(d, p.id));
  }
};

// ---- 3. sorted keys into the caller's arrays -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSplitBlock) radius_split_kernel(const unsigned long long *__restrict__ keys, int64_t total, int32_t *__restrict__ out_idx,
                                                                  float *__restrict__ out_dist) {
  const int64_t i = (int64_t)blockIdx.x * kSplitBlock + threadIdx.x;
  if (i >= total) return;
  const unsigned long long key = keys[i];
  out_idx[i] = (int32_t)(uint32_t)key;
  if (out_dist) out_dist[i] = __uint_as_float((uint32_t)(key >> 32));
}

}  // namespace

void Engine::radius_query(const tknnRadiusOptions &o, tknnRadiusInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const bool fill = o.d_idx != nullptr, sorted = fill && o.sort != 0;
  int64_t total = 0;
  if (fill) {
    // the one look at the caller's offsets: the fill pass's size
    int64_t *h_total = (int64_t *)(h_counters_ + kRadWords);
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
  const size_t words_b = align(kRadWords * sizeof(unsigned long long)), col_b = align(((size_t)m + 1) * sizeof(uint32_t)),
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
  OWLMI_HIP(hipMemsetAsync(d_words, 0, kRadWords * sizeof(unsigned long long), s));
  if (!fill) OWLMI_HIP(hipMemsetAsync(counts + m, 0, sizeof(uint32_t), s));  // the scan runs over m + 1 lengths: offsets[m] is the total
  query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, tmp, order_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  // the walk, then the lane kernel for what the walk left
  unsigned long long *h_words = h_counters_;
  if (fill)
    rad_walks<RadiusRule<true>>(a, cu_count_, h_words, s);
  else
    rad_walks<RadiusRule<false>>(a, cu_count_, h_words, s);
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  const bool mismatch = fill && h_words[kRadOwn] != 0;
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
    info->total = (int64_t)h_words[kRadTotal];
    info->max_row = (int64_t)h_words[kRadMaxRow];
    info->mismatched = (int64_t)h_words[kRadOwn];
    info->node_tests = (int64_t)h_words[kRadNodeTests];
    info->point_tests = (int64_t)h_words[kRadPointTests];
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_d_));
    OWLMI_HIP(hipEventElapsedTime(&info->order_ms, ev_a_, ev_b_));
    OWLMI_HIP(hipEventElapsedTime(&info->walk_ms, ev_b_, ev_c_));
    if (sorting && !mismatch) OWLMI_HIP(hipEventElapsedTime(&info->sort_ms, ev_c_, ev_d_));
  }
  if (mismatch)
    throw ArgError{TKNN_E_STATE, "tknnRadiusQuery: " + std::to_string(h_words[kRadOwn]) +
                                     " rows differ in length from their segment in d_offsets (stale offsets, or another radius): run the count pass again"};
  if (!fill && h_words[kRadTotal] >= 0x80000000ull)
    throw ArgError{TKNN_E_UNSUPPORTED, "tknnRadiusQuery: 2^31 or more neighbours in one call: split the queries"};
}

}  // namespace owlmi
