// radius_reduce.hip -- weighted sums over the points within a radius of each query, without the lists (tknnRadiusReduce,
// include/owlknn_reduce.h).
//
// Row j is a count, a sum of weights w and C sums of w * v_c over the points p of the built set with sqrt((dx*dx + dy*dy) + dz*dz)
// <= radius: knn_sqrt(knn_dist2(..)) <= r, radius_query.hip's predicate, so the count is that call's row length.  The walk is the
// count pass of radius_query.hip with accumulators: no (query, neighbour) pair leaves the chip.
//   1. query_order (query_order.h): external queries along the tree's own curve.  The set's own points (d_queries NULL) are taken
//      in sorted-slot order: position i is slot i, its row prim_id[i]; nothing is ordered.
//   2. reduce_stage_kernel: d_values, n x C by the caller's row, gathered through prim_id into sorted-slot order in the workspace:
//      NC floats per slot, NC the channel tier (4, 8, 16: a lane fetches its point's channels as NC / 4 128-bit loads), the slots
//      padded to whole leaf blocks; padding channels and padding slots are 0.  C = 0: no stage.
//   3. reduce_walk_kernel<WEIGHT, NC>: persistent, one 16-lane team per query, four teams per wave, walk_tree (team_walk.h) with the
//      query's box of half-width r (1 + 1e-6).  Lane tl tests point tl of a leaf block with the literal predicate and adds w and
//      w * v_c into its OWN registers, under the predicate: a lane that has no hit loads no value and multiplies nothing, so what
//      the values of other points hold (NaN, inf) cannot reach a sum.  One team reduction (DPP row rotations) per query at the
//      end.  A child box wholly inside the sphere (radius_query.hip's box rule: radius_in2, clean_end): with TKNN_W_ONE and C = 0
//      its slots are added arithmetically; otherwise a box above the leaf level is noted in the team's range list and its slots
//      are streamed after the walk without further box tests, a leaf block is tested in place, and a full list means the box is
//      walked.
//   4. reduce_lane_kernel<NC>: one query per lane on the rope walk (lane_walk.h), the weight a run-time switch, for the queries
//      whose team stack overflowed (a redo list whose length lives on the device) -- the result is complete on any tree.
// The call's workspace (Engine::workspace, one layout):
//      counters (kRdWords) | codes, sorted codes, order in, order (m + 1 each; external queries only) | redo list, m |
//      staged values, padded n x NC | the sort's temporary
#include "owlknn_reduce.h"
#include "lane_walk.h"
#include "query_order.h"
#include "team_lanes.h"
#include "team_walk.h"
#include "trueknn_engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace owlmi {

namespace {

constexpr int kReduceBlock = 64;        // one wave per workgroup, four teams
constexpr int kReduceBlocksPerCu = 16;  // 6.3 KB of LDS each
constexpr int kReduceLaneBlock = 256;
constexpr int kReduceFlatBlock = 256;
constexpr int kReduceRanges = 16;  // inside boxes above the leaf level a team notes for streaming; a 17th is walked

// words of the call's own counters (in the workspace, zeroed per call)
enum { kRdCursor = 0, kRdRedo = 1, kRdTotal = 2, kRdMaxRow = 3, kRdFallback = 4, kRdNodeTests = 5, kRdPointTests = 6, kRdWords = 8 };

struct ReduceArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const float *queries;   // m packed triples, caller order; null: the set's own points, position i = sorted slot i
  const uint32_t *order;  // external queries: the query worked on at sorted position i
  int32_t m;
  float radius;
  float radius_wide;  // radius * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts
  float radius_in2;   // radius^2 * 0.999995, rounded down: a box whose far corner is within it lies inside the sphere
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
  unsigned long long *ws;    // kRdWords counters
};

__device__ __forceinline__ float rd_nan() { return __uint_as_float(0x7fc00000u); }

// ---- the weights ---------------------------------------------------------------------------------------------------------------------
// of a point that passed the predicate: d2 = knn_dist2, d = knn_sqrt(d2), every operation rounded on its own
template <int WEIGHT>
__device__ __forceinline__ float rd_weight(float d2, float d, float coef) {
#pragma clang fp contract(off)
  if constexpr (WEIGHT == TKNN_W_GAUSS) {
    return expf(d2 * coef);
  } else if constexpr (WEIGHT == TKNN_W_EPANECHNIKOV) {
    return fmaxf(0.f, 1.f - d2 * coef);
  } else if constexpr (WEIGHT == TKNN_W_CUBIC_SPLINE) {
    const float s = d * coef, s2 = s * s, t = 2.f - s;
    const float inner = (1.f - 1.5f * s2) + 0.75f * (s2 * s), outer = fmaxf(0.f, 0.25f * ((t * t) * t));
    return s <= 1.f ? inner : outer;
  } else {
    return 1.f;
  }
}
__device__ __forceinline__ float rd_weight_of(int weight, float d2, float d, float coef) {
  switch (weight) {
    case TKNN_W_GAUSS: return rd_weight<TKNN_W_GAUSS>(d2, d, coef);
    case TKNN_W_EPANECHNIKOV: return rd_weight<TKNN_W_EPANECHNIKOV>(d2, d, coef);
    case TKNN_W_CUBIC_SPLINE: return rd_weight<TKNN_W_CUBIC_SPLINE>(d2, d, coef);
    default: return 1.f;
  }
}

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

// sum over the 16 lanes of my team (lane 0 of the team reads it; the order of the additions differs by lane)
__device__ __forceinline__ float rd_team_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128 /*row_ror:8*/, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124 /*row_ror:4*/, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122 /*row_ror:2*/, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121 /*row_ror:1*/, 0xf, 0xf, false));
  return v;
}

// the query at position `pos`: its coordinates, the row its results go to, and the slot to leave out (-1: none)
__device__ __forceinline__ void rd_query(const ReduceArgs &a, int32_t pos, bool has_q, LbvhPoint &q, int32_t &row, int32_t &self) {
  self = -1;
  if (a.queries) {
    row = has_q ? (int32_t)a.order[pos] : 0;
    q.x = a.queries[3 * (int64_t)row], q.y = a.queries[3 * (int64_t)row + 1], q.z = a.queries[3 * (int64_t)row + 2];
  } else {
    const int32_t slot = has_q ? pos : 0;
    q = a.bvh.points[slot];
    row = a.bvh.prim_id[slot];
    if (a.skip_self && has_q) self = slot;
  }
  q.id = -1;
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

__device__ __forceinline__ void rd_add_stats(unsigned long long *ws, int lane, unsigned long long total, unsigned int max_row, unsigned long long fallback,
                                             unsigned long long node_tests, unsigned long long point_tests) {
  const unsigned long long tsum = t_wave_sum(total), fb = t_wave_sum(fallback), nt = t_wave_sum(node_tests), pt = t_wave_sum(point_tests);
  unsigned int mx = max_row;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, off));
  if (lane == 0) {
    if (tsum) atomicAdd(&ws[kRdTotal], tsum);
    if (mx) atomicMax(&ws[kRdMaxRow], (unsigned long long)mx);
    if (fb) atomicAdd(&ws[kRdFallback], fb);
    if (nt) atomicAdd(&ws[kRdNodeTests], nt);
    if (pt) atomicAdd(&ws[kRdPointTests], pt);
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

// ---- 3. the walk -----------------------------------------------------------------------------------------------------------------------
// The box rule is radius_query.hip's: a child box whose far corner is within radius_in2 and whose slots end before clean_end holds
// only points that pass the literal test.  Teams of a wave loop in lock step: no __syncthreads, only t_wave_sync.
template <int WEIGHT, int NC>
__global__ void __launch_bounds__(kReduceBlock) __attribute__((amdgpu_waves_per_eu(4))) reduce_walk_kernel(ReduceArgs a) {
  constexpr bool kOne = WEIGHT == TKNN_W_ONE;
  constexpr bool kArith = kOne && NC == 0;  // an inside box is a number of slots, nothing of it is read
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[LBVH_WIDE_LEVELS];
  __shared__ int32_t range_mem[kArith ? 1 : 4 * kReduceRanges];
  __shared__ uint32_t range_n_mem[4];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  int32_t *range = range_mem + (kArith ? 0 : team * kReduceRanges);
  uint32_t *range_n = range_n_mem + team;
  walk_fill_levels<1>(levels, &a.wide, lane);
  if (tl == 0) *range_n = 0u;
  t_wave_sync();
  const LbvhWideView &wv = a.wide;
  const int32_t clean_end = lane_clean_end(a.bvh);
  unsigned long long node_tests = 0, point_tests = 0, total = 0;
  unsigned int max_row = 0;
  for (;;) {
    int got = 0;
    if (lane == 0) got = (int)atomicAdd(&a.ws[kRdCursor], 4ull);
    const int base = __builtin_amdgcn_readfirstlane(got);
    if (base >= a.m) break;
    const int32_t pos = base + team;
    const bool has_q = pos < a.m;
    LbvhPoint q;
    int32_t row, self;
    rd_query(a, pos, has_q, q, row, self);
    const bool active = has_q && !a.force_redo;
    const WalkBox qb(q, a.radius_wide);
    uint32_t part = 0;  // my lane's share of the count
    float wacc = 0.f;   // ... of the sum of weights
    float acc[NC > 0 ? NC : 1];  // ... of the sums of w * v_c
#pragma unroll
    for (int c = 0; c < (NC > 0 ? NC : 1); c++) acc[c] = 0.f;
    // lane tl takes point tl of the sixteen slots from `slot0` (the sorted arrays are padded with NaN sentinels to whole blocks)
    auto test_points = [&](int64_t slot0, bool has_b) __attribute__((always_inline)) {
      const int64_t slot = slot0 + tl;
      LbvhPoint p = LbvhPoint{rd_nan(), 0.f, 0.f, -1};
      if (has_b) p = a.bvh.points[slot];
      const float d2 = knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z);
      const float d = knn_sqrt(d2);
      const bool hit = has_b && d <= a.radius && slot != (int64_t)self;  // (a NaN on either side: not a neighbour)
      point_tests += has_b ? 1u : 0u;
      part = t_count(part, __ballot(hit));
      if constexpr (!kArith) {
        if (hit) rd_add<NC, kOne>(a.values, slot, rd_weight<WEIGHT>(d2, d, a.coef), wacc, acc);
      }
    };
    bool overflow = wv.levels <= 0;
    if (wv.levels > 0)
      walk_tree<(NC >= 8)>(
          levels, wv, stack, kWalkStack, active, q, qb, team, tl, node_tests,
          [&](const LbvhBox &bx, int32_t c, int lvl) {
            const float ax = fmaxf(fabsf(q.x - bx.lo[0]), fabsf(q.x - bx.hi[0])), ay = fmaxf(fabsf(q.y - bx.lo[1]), fabsf(q.y - bx.hi[1])),
                        az = fmaxf(fabsf(q.z - bx.lo[2]), fabsf(q.z - bx.hi[2]));
            const float far2 = t_dist2(ax, ay, az);
            const int64_t span = (int64_t)LBVH_BLOCK << (6 * lvl);  // points under one child of this level
            if (!(far2 <= a.radius_in2 && ((int64_t)c + 1) * span <= (int64_t)clean_end)) return true;
            if constexpr (kArith) {
              const bool mine = (int64_t)self >= (int64_t)c * span && (int64_t)self < ((int64_t)c + 1) * span;  // (self = -1: never)
              part += (uint32_t)span - (mine ? 1u : 0u);
              return false;
            } else {
              if (lvl == 0) return true;
              const uint32_t at = atomicAdd(range_n, 1u);
              if (at >= (uint32_t)kReduceRanges) return true;
              range[at] = (lvl << 26) | c;
              return false;
            }
          },
          [&](int32_t b, bool has_b) { test_points((int64_t)b * LBVH_BLOCK, has_b); }, [] {}, overflow);
    if constexpr (!kArith) {
      // the noted inside boxes, sixteen slots a step (every point passes; the literal test costs one compare and decides)
      t_wave_sync();
      const uint32_t nr = min(*range_n, (uint32_t)kReduceRanges);
      for (uint32_t i = 0; __ballot(i < nr) != 0ull; i++) {
        const bool has_r = i < nr;
        const int32_t e = has_r ? range[i] : 0;
        const int64_t span = has_r ? (int64_t)LBVH_BLOCK << (6 * (e >> 26)) : 0;
        const int64_t first = (int64_t)(e & 0x3ffffff) * span;
#pragma unroll 1
        for (int64_t s = 0; __ballot(s < span) != 0ull; s += LBVH_BLOCK) test_points(first + s, s < span);
      }
      t_wave_sync();
      if (tl == 0) *range_n = 0u;
      t_wave_sync();
    }
    // the one reduction of the row
    const uint32_t cnt = t_team_sum(part);
    const float wsum = kOne ? (float)cnt : rd_team_sum(wacc);
    if constexpr (NC > 0) {
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] = rd_team_sum(acc[c]);
    }
    if (has_q && tl == 0) {
      if (overflow || a.force_redo) {
        // left to the lane kernel, which starts the row again: nothing of it is counted here
        a.redo[atomicAdd(&a.ws[kRdRedo], 1ull)] = pos;
      } else {
        rd_write<NC>(a, row, cnt, wsum, acc);
        total += cnt;
        max_row = max(max_row, cnt);
      }
    }
  }
  rd_add_stats(a.ws, lane, total, max_row, 0ull, node_tests, point_tests);
}

// ---- 4. one query per lane: the queries of the redo list -----------------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(kReduceLaneBlock) reduce_lane_kernel(ReduceArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kReduceLaneBlock + threadIdx.x;
  const bool has_q = t < (int64_t)a.ws[kRdRedo];
  const int32_t pos = has_q ? a.redo[t] : 0;
  const int32_t clean_end = lane_clean_end(a.bvh);
  const bool arith = a.weight == TKNN_W_ONE && NC == 0;
  LbvhPoint q;
  int32_t row, self;
  rd_query(a, pos, has_q, q, row, self);
  uint32_t cnt = 0;
  float wacc = 0.f;
  float acc[NC > 0 ? NC : 1];
#pragma unroll
  for (int c = 0; c < (NC > 0 ? NC : 1); c++) acc[c] = 0.f;
  unsigned long long node_tests = 0, point_tests = 0;
  if (has_q)
    lane_walk<LaneRope::kWithNode>(a.bvh,
        [&](int32_t ref, const LbvhNode &nd, int32_t) {
          node_tests++;
          if (!lane_box_hit(nd, q, a.radius_wide)) return lane_rope();
          if (arith) {  // a node inside the sphere is counted, not walked (radius_lane_kernel; the margin: radius_in2)
            float far2, near2;
            lane_box_dist2(nd, q, far2, near2);
            const int32_t first = lbvh_first(ref, nd.other), last = lbvh_last(ref, nd.other);
            if (far2 <= a.radius_in2 && last < clean_end) {
              cnt += (uint32_t)(last - first + 1) - (self >= first && self <= last ? 1u : 0u);
              return lane_rope();
            }
          }
          return lane_descend();
        },
        [&](int32_t slot, const LbvhPoint &p) {
          point_tests++;
          const float d2 = knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z);
          const float d = knn_sqrt(d2);
          if (d <= a.radius && slot != self) {
            cnt++;
            if (!arith) rd_add<NC, false>(a.values, slot, rd_weight_of(a.weight, d2, d, a.coef), wacc, acc);  // (ONE: 1 * v is v)
          }
          return lane_rope();
        });
  if (has_q) rd_write<NC>(a, row, cnt, a.weight == TKNN_W_ONE ? (float)cnt : wacc, acc);
  // (all lanes of the wave are here)
  rd_add_stats(a.ws, threadIdx.x & 63, has_q ? cnt : 0u, has_q ? cnt : 0u, has_q ? 1u : 0u, node_tests, point_tests);
}

// r^2 * 0.999995 in double, rounded DOWN to fp32 (radius_query.hip's box rule)
inline float reduce_inside2(float r) {
  const double want = (double)r * (double)r * 0.999995;
  float f = (float)want;
  if ((double)f > want) f = std::nextafterf(f, 0.f);
  return f;
}

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
  const size_t words_b = align(kRdWords * sizeof(unsigned long long)), col_b = align(((size_t)m + 1) * sizeof(uint32_t)), order_cols = own ? 0 : 4 * col_b,
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
  a.radius_in2 = reduce_inside2(o.radius);
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
  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kRdWords * sizeof(unsigned long long), s));
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
  const int blocks = (int)std::min<int64_t>((m + 3) / 4, (int64_t)cu_count_ * kReduceBlocksPerCu);
  reduce_weight_case(o.weight, [&](auto weight) {
    reduce_tier(C, [&](auto tier) {
      hipLaunchKernelGGL((reduce_walk_kernel<decltype(weight)::value, decltype(tier)::value>), dim3(blocks), dim3(kReduceBlock), 0, s, a);
    });
  });
  OWLMI_HIP(hipGetLastError());
  unsigned long long *h_words = h_counters_;
  OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kRdWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (const unsigned long long n_redo = h_words[kRdRedo]) {
    const unsigned lane_blocks = (unsigned)((n_redo + kReduceLaneBlock - 1) / kReduceLaneBlock);
    reduce_tier(C, [&](auto tier) { hipLaunchKernelGGL(reduce_lane_kernel<decltype(tier)::value>, dim3(lane_blocks), dim3(kReduceLaneBlock), 0, s, a); });
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kRdWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  }
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->total = (int64_t)h_words[kRdTotal];
    info->max_row = (int64_t)h_words[kRdMaxRow];
    info->fallback_items = (int64_t)h_words[kRdFallback];
    info->node_tests = (int64_t)h_words[kRdNodeTests];
    info->point_tests = (int64_t)h_words[kRdPointTests];
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_d_));
    if (!own) OWLMI_HIP(hipEventElapsedTime(&info->order_ms, ev_a_, ev_b_));
    if (nc > 0) OWLMI_HIP(hipEventElapsedTime(&info->stage_ms, ev_b_, ev_c_));
    OWLMI_HIP(hipEventElapsedTime(&info->walk_ms, ev_c_, ev_d_));
  }
}

}  // namespace owlmi
