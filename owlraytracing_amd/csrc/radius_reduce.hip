// radius_reduce.hip -- weighted sums over the points within a radius of each query, without the lists (tknnRadiusReduce,
// include/owlknn_reduce.h).
//
// Row j is a count, a sum of weights w and C sums of w * v_c over the points p of the built set with sqrt((dx*dx + dy*dy) + dz*dz)
// <= radius: knn_sqrt(knn_dist2(..)) <= r, radius_query.hip's predicate, so the count is that call's row length.  No (query,
// neighbour) pair leaves the chip.
//   1. query_order (query_order.h): external queries along the tree's own curve.  The set's own points (d_queries NULL) are taken
//      in sorted-slot order: position i is slot i, its row prim_id[i]; nothing is ordered.
//   2. reduce_stage_kernel: d_values, n x C by the caller's row, gathered through prim_id into sorted-slot order in the workspace:
//      NC floats per slot, NC the channel tier (4, 8, 16: a lane fetches its point's channels as NC / 4 128-bit loads), the slots
//      padded to whole leaf blocks; padding channels and padding slots are 0.  C = 0: no stage.
//   3. rad_walks (radius_walk.h: the walk, the box rule, the lane kernel for what the walk left) with ReduceRule<WEIGHT, NC>: a
//      lane adds w and w * v_c into its OWN registers, under the predicate: a lane that has no hit loads no value and multiplies
//      nothing, so what the values of other points hold (NaN, inf) cannot reach a sum.  One team reduction (DPP row rotations)
//      per query at the end.  With TKNN_W_ONE and C = 0 an inside box is a number of slots; otherwise its slots are streamed.
//      The lane kernel has the weight as a run-time switch: ReduceRule<kAnyWeight, NC>.
// The call's workspace (Engine::workspace, one layout):
//      counters (kRadWords) | codes, sorted codes, order in, order (m + 1 each; external queries only) | redo list, m |
//      staged values, padded n x NC | the sort's temporary
#include "owlknn_reduce.h"
#include "query_order.h"
#include "radius_walk.h"
#include "radius_weights.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace owlmi {

namespace {

constexpr int kReduceFlatBlock = 256;
constexpr int kAnyWeight = -1;  // ReduceRule's WEIGHT where the weight is Args::weight (the lane kernel)

struct ReduceArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const float *queries;   // m packed triples, caller order; null: the set's own points, position i = sorted slot i
  const uint32_t *order;  // external queries: the query worked on at sorted position i
  int32_t m;
  float radius;
  float radius_wide;  // radius * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts
  float radius_in2;   // radius_inside2(radius): a box whose far corner is within it lies inside the sphere
  float coef;         // GAUSS: -1 / (2 h^2); EPANECHNIKOV: 1 / r^2; CUBIC_SPLINE: 2 / r
  int weight;         // TKNN_W_* (the lane kernel's switch)
  int channels;       // C
  int skip_self;      // own points: the query's slot is left out
  int normalize;
  int force_redo;     // TKNN_REDUCE_FORCE_FALLBACK (tests): the walk leaves every query to the lane kernel
  const float *user_values;  // n x C by the caller's row (the stage's input)
  float *values;             // staged: NC floats per sorted slot
  int64_t padded;            // slots of the staged copy: n rounded up to whole leaf blocks
  int32_t *counts;           // m, may be null
  float *wsum;               // m, may be null
  float *out;                // m x C, null with C = 0
  int32_t *redo;             // m: positions left to the lane kernel
  unsigned long long *ws;    // kRadWords counters
};

// A neighbour's share: w into wacc, w * v_c into acc.  Only called for a point that passed the predicate.
template <int NC, bool ONE>
__device__ __forceinline__ void rd_add(const float *values, int64_t slot, float w, float &wacc, float (&acc)[NC > 0 ? NC : 1]) {
  if constexpr (!ONE) wacc += w;
  if constexpr (NC > 0) {
    const float4 *vp = (const float4 *)(values + slot * NC);
#pragma unroll
    for (int g = 0; g < NC / 4; g++) {
      const float4 v = vp[g];
      acc[4 * g + 0] += ONE ? v.x : w * v.x;
      acc[4 * g + 1] += ONE ? v.y : w * v.y;
      acc[4 * g + 2] += ONE ? v.z : w * v.z;
      acc[4 * g + 3] += ONE ? v.w : w * v.w;
    }
  }
}

// one finished row, by the one lane that holds its sums
template <int NC>
__device__ __forceinline__ void rd_write(const ReduceArgs &a, int32_t row, uint32_t cnt, float wsum, const float (&acc)[NC > 0 ? NC : 1]) {
  if (a.counts) a.counts[row] = (int32_t)cnt;
  if (a.wsum) a.wsum[row] = wsum;
  if constexpr (NC > 0) {
    float *o = a.out + (int64_t)row * a.channels;
#pragma unroll
    for (int c = 0; c < NC; c++) {
      float v = acc[c];
      if (a.normalize) v = wsum == 0.f ? 0.f : v / wsum;
      if (c < a.channels) o[c] = v;
    }
  }
}

// ---- 2. the stage ----------------------------------------------------------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(kReduceFlatBlock) reduce_stage_kernel(ReduceArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kReduceFlatBlock + threadIdx.x;
  if (t >= a.padded * NC) return;
  const int64_t slot = t / NC;
  const int c = (int)(t % NC);
  float v = 0.f;
  if (slot < (int64_t)a.bvh.n && c < a.channels) v = a.user_values[(int64_t)a.bvh.prim_id[slot] * a.channels + c];
  a.values[t] = v;
}

// ---- 3. the rule -----------------------------------------------------------------------------------------------------------------------
// WEIGHT: a TKNN_W_* the walk is compiled for, or kAnyWeight: Args::weight decides (then ONE's sums are 1 * v, which is v).
template <int WEIGHT, int NC>
struct ReduceRule {
  using Args = ReduceArgs;
  static constexpr bool kOne = WEIGHT == TKNN_W_ONE;
  static constexpr bool kArith = kOne && NC == 0, kRolled = NC >= 8;
  static constexpr int kTeamLds = 0;
  struct Query {
    LbvhPoint q;
    int32_t row, self;  // self: the query's own slot where it is left out
    float r, r_wide, in2;
  };
  struct Lane {
    float wacc;                  // my lane's share of the sum of weights
    float acc[NC > 0 ? NC : 1];  // ... of the sums of w * v_c
  };
  static __device__ __forceinline__ Query query(const Args &a, int32_t pos, bool has_q) {
    Query s;
    const int32_t slot = rad_point(a, pos, has_q, s.q, s.row);
    s.q.id = -1;
    s.self = a.skip_self && has_q ? slot : -1;
    s.r = a.radius, s.r_wide = a.radius_wide, s.in2 = a.radius_in2;
    return s;
  }
  static __device__ __forceinline__ void start(Lane &st, unsigned long long *) {
    st.wacc = 0.f;
#pragma unroll
    for (int c = 0; c < (NC > 0 ? NC : 1); c++) st.acc[c] = 0.f;
  }
  static __device__ __forceinline__ bool one(const Args &a) { return WEIGHT == kAnyWeight ? a.weight == TKNN_W_ONE : kOne; }
  static __device__ __forceinline__ bool member(const Args &, const Query &s, int32_t slot, const LbvhPoint &, float d) { return d <= s.r && slot != s.self; }
  static __device__ __forceinline__ void lane_take(const Args &a, const Query &, Lane &st, uint32_t, int64_t slot, const LbvhPoint &, float, float, float, float d2,
                                                   float d) {
    const float w = WEIGHT == kAnyWeight ? rd_weight_of(a.weight, d2, d, a.coef) : rd_weight<WEIGHT>(d2, d, a.coef);
    rd_add<NC, kOne>(a.values, slot, w, st.wacc, st.acc);
  }
  static __device__ __forceinline__ void take(const Args &a, const Query &s, Lane &st, uint32_t &part, bool hit, int64_t slot, const LbvhPoint &p, float dx,
                                              float dy, float dz, float d2, float d, int, int) {
    part = t_count(part, __ballot(hit));
    if constexpr (!kArith)
      if (hit) lane_take(a, s, st, 0u, slot, p, dx, dy, dz, d2, d);
  }
  static __device__ __forceinline__ uint32_t row_end(const Args &, const Query &, Lane &st, uint32_t part, int, int) {
    if constexpr (!kOne) st.wacc = t_team_sum(st.wacc);
    if constexpr (NC > 0) {
#pragma unroll
      for (int c = 0; c < NC; c++) st.acc[c] = t_team_sum(st.acc[c]);
    }
    return t_team_sum(part);
  }
  static __device__ __forceinline__ unsigned long long row_write(const Args &a, const Query &s, const Lane &st, uint32_t cnt) {
    rd_write<NC>(a, s.row, cnt, one(a) ? (float)cnt : st.wacc, st.acc);
    return 0ull;
  }
  static __device__ __forceinline__ bool lane_arith(const Args &a) { return one(a) && NC == 0; }
};

// f(std::integral_constant<int, NC>{}) for the channel tier that serves C channels
template <class F>
void reduce_tier(int channels, F &&f) {
  if (channels == 0)
    f(std::integral_constant<int, 0>{});
  else if (channels <= 4)
    f(std::integral_constant<int, 4>{});
  else if (channels <= 8)
    f(std::integral_constant<int, 8>{});
  else
    f(std::integral_constant<int, 16>{});
}
template <class F>
void reduce_weight_case(int weight, F &&f) {
  switch (weight) {
    case TKNN_W_GAUSS: f(std::integral_constant<int, TKNN_W_GAUSS>{}); break;
    case TKNN_W_EPANECHNIKOV: f(std::integral_constant<int, TKNN_W_EPANECHNIKOV>{}); break;
    case TKNN_W_CUBIC_SPLINE: f(std::integral_constant<int, TKNN_W_CUBIC_SPLINE>{}); break;
    default: f(std::integral_constant<int, TKNN_W_ONE>{}); break;
  }
}

}  // namespace

void Engine::radius_reduce(const tknnRadiusReduceOptions &o, tknnRadiusReduceInfo *info, hipStream_t s) {
  const int64_t m = o.m, n = bvh_.size();
  const bool own = o.d_queries == nullptr;
  const int C = o.channels;
  int nc = 0;
  reduce_tier(C, [&](auto tier) { nc = decltype(tier)::value; });
  const int64_t padded = (n + LBVH_BLOCK - 1) / LBVH_BLOCK * LBVH_BLOCK;
  // the call's workspace (the layout: the file head)
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t order_bytes = own ? 0 : query_order_sort_bytes(m, s);
  const size_t words_b = align(kRadWords * sizeof(unsigned long long)), col_b = align(((size_t)m + 1) * sizeof(uint32_t)), order_cols = own ? 0 : 4 * col_b,
               stage_b = align((size_t)padded * (size_t)nc * sizeof(float)), tmp_b = align(order_bytes);
  char *ws = (char *)workspace(words_b + order_cols + col_b + stage_b + tmp_b);
  uint32_t *codes = (uint32_t *)(ws + words_b), *codes_alt = (uint32_t *)(ws + words_b + col_b), *order_in = (uint32_t *)(ws + words_b + 2 * col_b),
           *order = (uint32_t *)(ws + words_b + 3 * col_b);
  void *tmp = ws + words_b + order_cols + col_b + stage_b;

  ReduceArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.wide = bvh_.wide_view();
  a.queries = o.d_queries;
  a.order = own ? nullptr : order;
  a.m = (int32_t)m;
  a.radius = o.radius;
  a.radius_wide = o.radius * 1.000001f;
  a.radius_in2 = radius_inside2(o.radius);
  a.weight = o.weight;
  if (o.weight == TKNN_W_GAUSS) a.coef = (float)(-0.5 / ((double)o.bandwidth * (double)o.bandwidth));
  if (o.weight == TKNN_W_EPANECHNIKOV) a.coef = (float)(1.0 / ((double)o.radius * (double)o.radius));
  if (o.weight == TKNN_W_CUBIC_SPLINE) a.coef = (float)(2.0 / (double)o.radius);
  a.channels = C;
  a.skip_self = (o.flags & TKNN_REDUCE_SKIP_SELF) != 0;
  a.normalize = (o.flags & TKNN_REDUCE_NORMALIZE) != 0;
  if (const char *e = getenv("TKNN_REDUCE_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.user_values = o.d_values;
  a.values = (float *)(ws + words_b + order_cols + col_b);
  a.padded = padded;
  a.counts = o.d_counts;
  a.wsum = o.d_wsum;
  a.out = C > 0 ? o.d_out : nullptr;
  a.redo = (int32_t *)(ws + words_b + order_cols);
  a.ws = (unsigned long long *)ws;

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kRadWords * sizeof(unsigned long long), s));
  if (!own) query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, tmp, order_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  if (nc > 0) {
    const unsigned stage_blocks = (unsigned)((padded * nc + kReduceFlatBlock - 1) / kReduceFlatBlock);
    reduce_tier(C, [&](auto tier) {
      constexpr int NC = decltype(tier)::value;
      if constexpr (NC > 0) hipLaunchKernelGGL(reduce_stage_kernel<NC>, dim3(stage_blocks), dim3(kReduceFlatBlock), 0, s, a);
    });
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  // the walk, then the lane kernel for what the walk left
  unsigned long long *h_words = h_counters_;
  reduce_weight_case(o.weight, [&](auto weight) {
    reduce_tier(C, [&](auto tier) {
      constexpr int NC = decltype(tier)::value;
      rad_walks<ReduceRule<decltype(weight)::value, NC>, ReduceRule<kAnyWeight, NC>>(a, cu_count_, h_words, s);
    });
  });
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->total = (int64_t)h_words[kRadTotal];
    info->max_row = (int64_t)h_words[kRadMaxRow];
    info->fallback_items = (int64_t)h_words[kRadLaneRows];
    info->node_tests = (int64_t)h_words[kRadNodeTests];
    info->point_tests = (int64_t)h_words[kRadPointTests];
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_d_));
    if (!own) OWLMI_HIP(hipEventElapsedTime(&info->order_ms, ev_a_, ev_b_));
    if (nc > 0) OWLMI_HIP(hipEventElapsedTime(&info->stage_ms, ev_b_, ev_c_));
    OWLMI_HIP(hipEventElapsedTime(&info->walk_ms, ev_c_, ev_d_));
  }
}

}  // namespace owlmi
