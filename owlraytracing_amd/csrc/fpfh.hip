// fpfh.hip -- the 33-bin Fast Point Feature Histogram of each of the built set's own points, without the lists (tknnFpfh,
// include/owlknn_fpfh.h).
//
// Point i's neighbourhood N_i is its tknnRadiusQuery row less its own slot.  Two walks over the same pairs, flat kernels around them:
//   1. fpfh_stage_kernel: d_normals, n x 3 by the caller's row, gathered through prim_id into sorted-slot order, one float4 per slot,
//      the slots padded to whole leaf blocks (padding: zeros): the layout of reduce_stage_kernel's values.  No kernel here reads a
//      padding slot -- a normal and a staged row are loaded for a hit only, and a hit is a point --; the staged histograms'
//      padding is never written.
//   2. rad_walks (radius_walk.h) with SpfhRule: a lane fetches its hit's normal, computes the pair's three bins (fpfh_pair.h) and
//      adds 1 to three of its TEAM's 33 counters, which live in LDS (kTeamLds; ds_add, no global atomic per pair; 33 dynamically
//      indexed counters per lane would be scratch).  At the row's end the sixteen lanes read the counters back and write the staged
//      row in sorted-slot order, 36 words per slot: the 33 counts as they are, the factor 100 / valid as a float, two zeros.  An
//      SPFH value is (float)count * factor wherever it is needed.  Not kArith: an inside box is streamed.  The lane kernel
//      (SpfhRule<true>) keeps its 33 counters in LDS as well, one column of the workgroup's 33 x 256 words per lane (33 KB per
//      workgroup: the price of no scratch on the rare path), and one lane writes the whole row.
//   3. fpfh_rows_kernel, only with d_spfh or d_spfh_counts: the staged rows to the caller's rows.  (The walk carries no pointer
//      it does not need per pair: its scalar registers are the tight resource)
//   4. rad_walks with FpfhRule: the team holds the row's 33 sums A_i by column, three per lane.  The hits of a block step are
//      taken one at a time per team: slot and weight 1 / d2 come from the hit's lane over the crossbar and the sixteen lanes load
//      its staged row, 144 contiguous bytes, as three words each; a team without a hit loads nothing.  (33 sums per lane, fetched as
//      nine 128-bit loads per hit, do not fit next to the walk's four chunk boxes: 128 registers and 44 to 64 bytes of scratch per
//      lane)  At the row's end three masked team sums give S per feature, and the lanes normalise, add the self term from the staged row and
//      write the row of d_fpfh: the finish is the rule's row_end, there is no kernel for it.  The lane kernel (FpfhLaneRule) has
//      33 registers of sums per lane and writes its rows alone.  Skipped when d_fpfh is NULL.
// The call's workspace (Engine::workspace, one layout):
//      counters of pass 1, of pass 2 (kRadWords each) | redo list, n | staged normals, padded x float4 |
//      staged histograms, padded x 36 words
#include "owlknn_fpfh.h"
#include "fpfh_pair.h"
#include "radius_walk.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kFpfhFlatBlock = 256;
constexpr int kFpfhStageCols = 36;  // words of a staged row: 33 counts, the factor, two zeros
constexpr int kFpfhFactorCol = 33;
constexpr int kFpfhHistWords = 36;  // 32-bit words of a team's histogram in LDS: 33 counters, the rest zeroed with them

struct FpfhArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const float *queries;   // null: the set's own points, position i = sorted slot i (radius_walk.h reads it)
  const uint32_t *order;  // null
  int32_t m;              // n
  float radius;
  float radius_wide;  // radius * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts
  float radius_in2;   // radius_inside2(radius)
  int force_redo;     // TKNN_FPFH_FORCE_FALLBACK (tests): the walk leaves every row to the lane kernel
  int self_term;
  const float *user_normals;  // n x 3 by the caller's row (the stage's input)
  float4 *normals;            // staged: one per sorted slot
  int64_t padded;             // slots of the staged copies: n rounded up to whole leaf blocks
  uint32_t *stage;            // staged histograms: kFpfhStageCols words per sorted slot
  int32_t *counts;            // the caller's outputs, any may be null
  int32_t *spfh_counts;
  float *out_spfh, *out_fpfh;
  int32_t *redo;           // n: positions left to the lane kernel
  unsigned long long *ws;  // kRadWords counters (the pass's own)
};

struct FpfhQuery {
  LbvhPoint q;
  int32_t row, self;  // self: the point's own slot, left out
  float r, r_wide, in2;
  float nx, ny, nz;  // the point's normal (pass 1)
  bool has;          // the team has a row (the walk's row_end writes)
};
template <bool NORMAL>
__device__ __forceinline__ FpfhQuery fpfh_query(const FpfhArgs &a, int32_t pos, bool has_q) {
  FpfhQuery s;
  const int32_t slot = rad_point(a, pos, has_q, s.q, s.row);
  s.q.id = -1;
  s.self = slot;  // (a team without a row has an inactive walk)
  s.r = a.radius, s.r_wide = a.radius_wide, s.in2 = a.radius_in2;
  s.nx = s.ny = s.nz = 0.f;
  if constexpr (NORMAL) {
    const float4 nn = a.normals[slot];
    s.nx = nn.x, s.ny = nn.y, s.nz = nn.z;
  }
  s.has = has_q;
  return s;
}

// the factor of a row with `valid` pairs, and a value of its SPFH
__device__ __forceinline__ float spfh_factor(uint32_t valid) { return valid ? 100.f / (float)valid : 0.f; }
__device__ __forceinline__ float spfh_value(uint32_t count, float factor) { return (float)count * factor; }

// ---- 1. the stage ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kFpfhFlatBlock) fpfh_stage_kernel(FpfhArgs a) {
  const int64_t slot = (int64_t)blockIdx.x * kFpfhFlatBlock + threadIdx.x;
  if (slot >= a.padded) return;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (slot < (int64_t)a.bvh.n) {
    const float *src = a.user_normals + 3 * (int64_t)a.bvh.prim_id[slot];
    v.x = src[0], v.y = src[1], v.z = src[2];
  }
  a.normals[slot] = v;
}

// ---- 2. pass 1 -------------------------------------------------------------------------------------------------------------------------
// LANE: the lane kernel's (a column of the workgroup's LDS per lane, one lane writes the row); else the walk's
template <bool LANE>
struct SpfhRule {
  using Args = FpfhArgs;
  using Query = FpfhQuery;
  static constexpr bool kArith = false, kRolled = true;
  static constexpr int kTeamLds = LANE ? 0 : kFpfhHistWords / 2;
  static constexpr int kStride = LANE ? kRadLaneBlock : 1;  // words between two of my counters
  struct Lane {
    uint32_t *hist;    // my team's counters (the walk), my own column (the lane kernel)
    uint32_t skipped;  // my share of the row's degenerate pairs
  };
  static __device__ __forceinline__ Query query(const Args &a, int32_t pos, bool has_q) { return fpfh_query<true>(a, pos, has_q); }
  static __device__ __forceinline__ void start(Lane &st, unsigned long long *lds) {
    st.skipped = 0u;
    if constexpr (LANE) {
      __shared__ uint32_t columns[kFpfhBins * kRadLaneBlock];
      st.hist = columns + threadIdx.x;
#pragma unroll
      for (int b = 0; b < kFpfhBins; b++) st.hist[b * kStride] = 0u;
    } else {
      const int tl = threadIdx.x & 15;
      st.hist = (uint32_t *)lds;
      st.hist[tl] = 0u, st.hist[16 + tl] = 0u;
      if (tl < kFpfhHistWords - 32) st.hist[32 + tl] = 0u;
      t_wave_sync();
    }
  }
  static __device__ __forceinline__ bool member(const Args &, const Query &s, int32_t slot, const LbvhPoint &, float d) { return d <= s.r && slot != s.self; }
  // a point that passed member(): its pair's three bins into the counters, or one more degenerate pair
  static __device__ __forceinline__ void lane_take(const Args &a, const Query &s, Lane &st, uint32_t, int64_t slot, const LbvhPoint &, float dx, float dy, float dz,
                                                   float d2, float d) {
    const float4 nj = a.normals[slot];
    FpfhFeatures f;
    if (fpfh_pair(s.nx, s.ny, s.nz, nj.x, nj.y, nj.z, dx, dy, dz, d2, d, f)) {
      if constexpr (LANE) {
        st.hist[f.b1 * kStride] += 1u, st.hist[(11 + f.b2) * kStride] += 1u, st.hist[(22 + f.b3) * kStride] += 1u;
      } else {
        atomicAdd(&st.hist[f.b1], 1u), atomicAdd(&st.hist[11 + f.b2], 1u), atomicAdd(&st.hist[22 + f.b3], 1u);
      }
    } else {
      st.skipped++;
    }
  }
  static __device__ __forceinline__ void take(const Args &a, const Query &s, Lane &st, uint32_t &part, bool hit, int64_t slot, const LbvhPoint &p, float dx,
                                              float dy, float dz, float d2, float d, int, int) {
    part = t_count(part, __ballot(hit));
    if (hit) lane_take(a, s, st, 0u, slot, p, dx, dy, dz, d2, d);
  }
  // The walk: the sixteen lanes write the staged row, lane tl the words tl, 16 + tl and (the first four) 32 + tl.  A row whose
  // stack overflowed is written as far as it came and written again, whole, by the lane kernel after this kernel.
  static __device__ __forceinline__ uint32_t row_end(const Args &a, const Query &s, Lane &st, uint32_t part, int, int tl) {
    t_wave_sync();
    const uint32_t c0 = st.hist[tl], c1 = st.hist[16 + tl], c2 = st.hist[32];
    const float factor = spfh_factor(t_team_sum(tl < kFpfhBinsPerFeature ? c0 : 0u));
    st.skipped = t_team_sum(st.skipped);
    if (s.has) {
      uint32_t *stage = a.stage + (int64_t)s.self * kFpfhStageCols;
      stage[tl] = c0, stage[16 + tl] = c1;
      if (tl < kFpfhStageCols - 32) stage[32 + tl] = tl == 0 ? c2 : tl == kFpfhFactorCol - 32 ? __float_as_uint(factor) : 0u;
    }
    return t_team_sum(part);
  }
  static __device__ __forceinline__ unsigned long long row_write(const Args &a, const Query &s, const Lane &st, uint32_t cnt) {
    if (a.counts) a.counts[s.row] = (int32_t)cnt;
    if constexpr (LANE) {
      uint32_t valid = 0u;
#pragma unroll
      for (int b = 0; b < kFpfhBinsPerFeature; b++) valid += st.hist[b * kStride];
      uint32_t *stage = a.stage + (int64_t)s.self * kFpfhStageCols;
#pragma unroll
      for (int b = 0; b < kFpfhStageCols; b++)
        stage[b] = b < kFpfhBins ? st.hist[b * kStride] : b == kFpfhFactorCol ? __float_as_uint(spfh_factor(valid)) : 0u;
    }
    return st.skipped;
  }
  static __device__ __forceinline__ bool lane_arith(const Args &) { return false; }
};

// ---- 3. the first pass's outputs -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kFpfhFlatBlock) fpfh_rows_kernel(FpfhArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kFpfhFlatBlock + threadIdx.x;
  if (t >= (int64_t)a.m * kFpfhBins) return;
  const int64_t slot = t / kFpfhBins;
  const int b = (int)(t % kFpfhBins);
  const uint32_t *stage = a.stage + slot * kFpfhStageCols;
  const int64_t at = (int64_t)a.bvh.prim_id[slot] * kFpfhBins + b;
  if (a.spfh_counts) a.spfh_counts[at] = (int32_t)stage[b];
  if (a.out_spfh) a.out_spfh[at] = spfh_value(stage[b], __uint_as_float(stage[kFpfhFactorCol]));
}

// ---- 4. pass 2 -------------------------------------------------------------------------------------------------------------------------
// one value of a finished FPFH row: the blended sum normalised over its feature, plus the point's own SPFH
__device__ __forceinline__ float fpfh_value(const FpfhArgs &a, float A, float S, float own) {
  const float blend = S > 0.f ? A * (100.f / S) : 0.f;
  return a.self_term ? blend + own : blend;
}

// The walk's.  The team's sixteen lanes hold the row's sums A_i by COLUMN: lane tl the columns tl, 16 + tl and (lane 0) 32.  The
// hits of a block step are taken one at a time per team: the hit's slot and weight come from its lane over the crossbar, and the
// sixteen lanes load its staged row as coalesced words.
struct FpfhRule {
  using Args = FpfhArgs;
  using Query = FpfhQuery;
  static constexpr bool kArith = false, kRolled = true;
  static constexpr int kTeamLds = 0;
  struct Lane {
    float a0, a1, a2;  // A_i[tl], A_i[16 + tl], A_i[32] (lane 0)
  };
  static __device__ __forceinline__ Query query(const Args &a, int32_t pos, bool has_q) { return fpfh_query<false>(a, pos, has_q); }
  static __device__ __forceinline__ void start(Lane &st, unsigned long long *) { st.a0 = st.a1 = st.a2 = 0.f; }
  static __device__ __forceinline__ bool member(const Args &, const Query &s, int32_t slot, const LbvhPoint &, float d) { return d <= s.r && slot != s.self; }
  static __device__ __forceinline__ void take(const Args &a, const Query &, Lane &st, uint32_t &part, bool hit, int64_t slot, const LbvhPoint &, float, float, float,
                                              float d2, float, int team, int tl) {
    part = t_count(part, __ballot(hit));
    const float w = 1.f / d2;
    const bool enters = hit && d2 > 0.f && fpfh_finite(w);
    uint32_t todo = (uint32_t)(__ballot(enters) >> (team * 16)) & 0xffffu;
    while (__ballot(todo != 0u) != 0ull) {
      const bool has = todo != 0u;
      const int from = team * 16 + (has ? __ffs((int)todo) - 1 : 0);
      todo &= todo - 1u;
      const float wj = __uint_as_float(t_lane_read(__float_as_uint(w), from));
      const uint32_t sj = t_lane_read((uint32_t)slot, from);
      if (has) {  // (a team without a hit loads nothing)
        const uint32_t *row = a.stage + (int64_t)sj * kFpfhStageCols;
        const float factor = __uint_as_float(row[kFpfhFactorCol]);
        st.a0 += spfh_value(row[tl], factor) * wj, st.a1 += spfh_value(row[16 + tl], factor) * wj;
        if (tl == 0) st.a2 += spfh_value(row[32], factor) * wj;
      }
    }
  }
  // Every lane: the three sums S over a feature's 11 columns (masked team sums, the team's lane 0 has the word for all), the
  // normalisation, the self term, the row.  A row whose stack overflowed: as in pass 1.
  static __device__ __forceinline__ uint32_t row_end(const Args &a, const Query &s, Lane &st, uint32_t part, int team, int tl) {
    const float p0 = t_team_sum(tl < 11 ? st.a0 : 0.f), p1 = t_team_sum((tl >= 11 ? st.a0 : 0.f) + (tl < 6 ? st.a1 : 0.f)),
                p2 = t_team_sum((tl >= 6 ? st.a1 : 0.f) + (tl == 0 ? st.a2 : 0.f));
    const float S0 = __uint_as_float(t_lane_read(__float_as_uint(p0), team * 16)), S1 = __uint_as_float(t_lane_read(__float_as_uint(p1), team * 16)),
                S2 = __uint_as_float(t_lane_read(__float_as_uint(p2), team * 16));
    if (s.has) {
      const uint32_t *own = a.stage + (int64_t)s.self * kFpfhStageCols;
      const float factor = __uint_as_float(own[kFpfhFactorCol]);
      float *o = a.out_fpfh + (int64_t)s.row * kFpfhBins;
      o[tl] = fpfh_value(a, st.a0, tl < 11 ? S0 : S1, spfh_value(own[tl], factor));
      o[16 + tl] = fpfh_value(a, st.a1, tl < 6 ? S1 : S2, spfh_value(own[16 + tl], factor));
      if (tl == 0) o[32] = fpfh_value(a, st.a2, S2, spfh_value(own[32], factor));
    }
    return t_team_sum(part);
  }
  static __device__ __forceinline__ unsigned long long row_write(const Args &, const Query &, const Lane &, uint32_t) { return 0ull; }
};

// The lane kernel's: 33 sums of its own per lane (84 registers, no scratch), the whole row by that lane.
struct FpfhLaneRule {
  using Args = FpfhArgs;
  using Query = FpfhQuery;
  struct Lane {
    float acc[kFpfhBins];
  };
  static __device__ __forceinline__ Query query(const Args &a, int32_t pos, bool has_q) { return fpfh_query<false>(a, pos, has_q); }
  static __device__ __forceinline__ void start(Lane &st, unsigned long long *) {
#pragma unroll
    for (int b = 0; b < kFpfhBins; b++) st.acc[b] = 0.f;
  }
  static __device__ __forceinline__ bool member(const Args &, const Query &s, int32_t slot, const LbvhPoint &, float d) { return d <= s.r && slot != s.self; }
  static __device__ __forceinline__ void lane_take(const Args &a, const Query &, Lane &st, uint32_t, int64_t slot, const LbvhPoint &, float, float, float, float d2,
                                                   float) {
    const float w = 1.f / d2;
    if (!(d2 > 0.f && fpfh_finite(w))) return;
    const uint4 *vp = (const uint4 *)(a.stage + slot * kFpfhStageCols);
    const float factor = __uint_as_float(a.stage[slot * kFpfhStageCols + kFpfhFactorCol]);
#pragma unroll
    for (int g = 0; g < kFpfhStageCols / 4; g++) {
      const uint4 v = vp[g];
      st.acc[4 * g] += spfh_value(v.x, factor) * w;
      if (4 * g + 1 < kFpfhBins)
        st.acc[4 * g + 1] += spfh_value(v.y, factor) * w, st.acc[4 * g + 2] += spfh_value(v.z, factor) * w, st.acc[4 * g + 3] += spfh_value(v.w, factor) * w;
    }
  }
  static __device__ __forceinline__ unsigned long long row_write(const Args &a, const Query &s, const Lane &st, uint32_t) {
    const uint32_t *own = a.stage + (int64_t)s.self * kFpfhStageCols;
    const float factor = __uint_as_float(own[kFpfhFactorCol]);
    float *o = a.out_fpfh + (int64_t)s.row * kFpfhBins;
#pragma unroll
    for (int f = 0; f < 3; f++) {
      float S = 0.f;
#pragma unroll
      for (int k = 0; k < kFpfhBinsPerFeature; k++) S += st.acc[f * kFpfhBinsPerFeature + k];
#pragma unroll
      for (int k = 0; k < kFpfhBinsPerFeature; k++) {
        const int b = f * kFpfhBinsPerFeature + k;
        o[b] = fpfh_value(a, st.acc[b], S, spfh_value(own[b], factor));
      }
    }
    return 0ull;
  }
  static __device__ __forceinline__ bool lane_arith(const Args &) { return false; }
};

}  // namespace

void Engine::fpfh(const tknnFpfhOptions &o, tknnFpfhInfo *info, hipStream_t s) {
  const int64_t n = bvh_.size();
  const int64_t padded = (n + LBVH_BLOCK - 1) / LBVH_BLOCK * LBVH_BLOCK;
  const bool second = o.d_fpfh != nullptr;
  // the call's workspace (the layout: the file head)
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t words_b = align(2 * kRadWords * sizeof(unsigned long long)), redo_b = align(((size_t)n + 1) * sizeof(int32_t)),
               normals_b = align((size_t)padded * sizeof(float4)), stage_b = align((size_t)padded * kFpfhStageCols * sizeof(uint32_t));
  char *ws = (char *)workspace(words_b + redo_b + normals_b + stage_b);

  FpfhArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.wide = bvh_.wide_view();
  a.m = (int32_t)n;
  a.radius = o.radius;
  a.radius_wide = o.radius * 1.000001f;
  a.radius_in2 = radius_inside2(o.radius);
  if (const char *e = getenv("TKNN_FPFH_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.self_term = (o.flags & TKNN_FPFH_NO_SELF_TERM) == 0;
  a.user_normals = o.d_normals;
  a.normals = (float4 *)(ws + words_b + redo_b);
  a.padded = padded;
  a.stage = (uint32_t *)(ws + words_b + redo_b + normals_b);
  a.counts = o.d_counts, a.spfh_counts = o.d_spfh_counts, a.out_spfh = o.d_spfh, a.out_fpfh = o.d_fpfh;
  a.redo = (int32_t *)(ws + words_b);
  a.ws = (unsigned long long *)ws;

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(ws, 0, 2 * kRadWords * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(fpfh_stage_kernel, dim3((unsigned)((padded + kFpfhFlatBlock - 1) / kFpfhFlatBlock)), dim3(kFpfhFlatBlock), 0, s, a);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  // pass 1: the walk, then the lane kernel for what the walk left; its outputs
  unsigned long long *h_one = h_counters_, *h_two = h_counters_ + kRadWords;
  std::memset(h_two, 0, kRadWords * sizeof(unsigned long long));
  rad_walks<SpfhRule<false>, SpfhRule<true>>(a, cu_count_, h_one, s);
  if (o.d_spfh || o.d_spfh_counts) {
    hipLaunchKernelGGL(fpfh_rows_kernel, dim3((unsigned)((n * kFpfhBins + kFpfhFlatBlock - 1) / kFpfhFlatBlock)), dim3(kFpfhFlatBlock), 0, s, a);
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  if (second) {
    // pass 2 on its own counters (pass 1's are still on their way to the host where its lane kernel ran)
    FpfhArgs b = a;
    b.ws = a.ws + kRadWords;
    rad_walks<FpfhRule, FpfhLaneRule>(b, cu_count_, h_two, s);
  }
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->total = (int64_t)h_one[kRadTotal];
    info->max_row = (int64_t)h_one[kRadMaxRow];
    info->skipped_pairs = (int64_t)h_one[kRadOwn];
    info->fallback_items = (int64_t)(h_one[kRadLaneRows] + h_two[kRadLaneRows]);
    info->node_tests = (int64_t)(h_one[kRadNodeTests] + h_two[kRadNodeTests]);
    info->point_tests = (int64_t)(h_one[kRadPointTests] + h_two[kRadPointTests]);
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_d_));
    OWLMI_HIP(hipEventElapsedTime(&info->stage_ms, ev_a_, ev_b_));
    OWLMI_HIP(hipEventElapsedTime(&info->spfh_ms, ev_b_, ev_c_));
    if (second) OWLMI_HIP(hipEventElapsedTime(&info->fpfh_ms, ev_c_, ev_d_));  // (finish_ms stays 0: the finish is the pass's row_end)
  }
}

}  // namespace owlmi
