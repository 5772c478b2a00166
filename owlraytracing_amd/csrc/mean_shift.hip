// mean_shift.hip -- mean-shift mode seeking over the built set (tknnMeanShift, include/owlknn_meanshift.h).
//
// The loop a user writes in torch around tknnRadiusReduce -- reduce with the coordinates as values, shift, mask, compact -- inside
// the engine.  What that loop pays per iteration and this one does not: the curve sort of the queries, the stage that gathers the
// values (they are the tree's own points, the walk has p - x in registers), the torch mask and index compaction, and sums of
// absolute coordinates (sum w p in fp32 loses the mean of a cloud away from the origin; the sums here are over the offsets p - x).
//   0. the positions: a workspace array of m packed triples BY THE SEED'S j, a copy of d_seeds, or (d_seeds NULL) the tree's sorted
//      points scattered to their rows (ms_own_seeds_kernel).  The work list: external seeds get ONE query_order; the own points are
//      taken along prim_id, slot order being curve order.  TKNN_MEANSHIFT_REORDER=R sorts the work list again every R passes by
//      where the seeds are then (ms_code_kernel + the radix sort); a row's result cannot depend on it (below).
//   1. a pass: rad_walks (radius_walk.h: the walk, the box rule, the lane kernel for what the walk left) with
//      MeanShiftRule<WEIGHT> over the work list.  A lane adds w and w * (dx, dy, dz) into its OWN registers under the predicate --
//      no value load, no stage --; one team reduction per row; row_write forms the step, the new position, the shift and the
//      status, writes the seed's outputs and its "still moving" flag, by list position.  kArith is false: an inside box is
//      streamed through the range list, its points' offsets are needed.  The lane kernel has the weight as a run-time switch.
//   2. the rows still moving are counted in the walk's own counter word (kRadOwn), which the host reads together with the redo
//      count the walk makes it read anyway: the pass's one synchronisation (a second one only when the lane kernel ran).  That
//      count is the next pass's m -- rad_walks takes m by value --; the next pass starts with a stable compaction of the work list
//      by the flags (hipcub::DeviceSelect::Flagged), so the list keeps its curve order.  The loop ends at 0 rows or at
//      max_iterations.
//   3. ms_tally_kernel counts the seeds per status; the positions and the status are copied to the caller's arrays.
// In place: a row's position is read (Rule::query) and written (row_write) by exactly one team or one lane per pass, and by nobody
// else -- a walk's neighbours are the TREE's points, never another seed's position, and the own points' positions are a copy.  A row
// the walk leaves to the redo list is read by its team and written by nobody in that kernel; the lane kernel, which runs after it on
// the stream, reads the same unchanged position and writes it.  So the positions are updated in place, with the redo list as it is.
// A row's sums depend on the tree, the position and the kernel (walk or lane) only: the team's traversal, its lanes' shares and the
// DPP reduction are functions of (tree, q, r), not of the list position, the team or the pass.  So one call with max_iterations = T
// equals T chained calls of one step, bit for bit, and reordering changes no result.
// The call's workspace (Engine::workspace, one layout):
//      counters (kRadWords) + the four status counts | codes, sorted codes, list A, list B (m + 1 words each) | redo list, m |
//      flags, m bytes | status, m bytes | positions, 3 m floats | the temporary of the sort and the select | the select's count
#include "owlknn_meanshift.h"
#include "curve_key.h"
#include "query_order.h"
#include "radius_walk.h"
#include "radius_weights.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace owlmi {

namespace {

constexpr int kMsFlatBlock = 256;
constexpr int kMsAnyWeight = -1;  // MeanShiftRule's WEIGHT where the weight is Args::weight (the lane kernel)
static_assert(kHostCounterWords >= kRadWords + 4, "the host's copy of the counters holds a walk's words and the status counts");

struct MeanShiftArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const float *queries;   // the positions, m0 packed triples by the seed's j (read through rad_point)
  const uint32_t *order;  // the work list: the seed worked on at list position i
  int32_t m;              // its length
  float radius;
  float radius_wide;  // radius * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts
  float radius_in2;   // radius_inside2(radius)
  float coef;         // GAUSS: -1 / (2 h^2); EPANECHNIKOV: 1 / r^2
  float tol;
  int weight;          // TKNN_W_* (the lane kernel's switch)
  int pass;            // steps every row of the list has taken
  int max_iterations;
  int force_redo;      // TKNN_MEANSHIFT_FORCE_FALLBACK (tests): the walk leaves every row to the lane kernel
  float *pos;          // = queries, to write
  uint8_t *alive;      // by list position: 1 if the row is walked again
  uint8_t *status;     // by j
  int32_t *counts;     // by j, the caller's, may be null
  float *wsum;         // ...
  float *shift;
  int32_t *iterations;
  int32_t *redo;           // positions left to the lane kernel
  unsigned long long *ws;  // kRadWords counters
};

// ---- 1. the rule ---------------------------------------------------------------------------------------------------------------------
// WEIGHT: a TKNN_W_* the walk is compiled for, or kMsAnyWeight: Args::weight decides.
template <int WEIGHT>
struct MeanShiftRule {
  using Args = MeanShiftArgs;
  static constexpr bool kOne = WEIGHT == TKNN_W_ONE;
  static constexpr bool kArith = false, kRolled = false;
  static constexpr int kTeamLds = 0;
  struct Query {
    LbvhPoint q;
    int32_t row, self, pos;
    float r, r_wide, in2;
  };
  struct Lane {
    float w, ax, ay, az;  // my lane's share of W and of a
  };
  static __device__ __forceinline__ Query query(const Args &a, int32_t pos, bool has_q) {
    Query s;
    rad_point(a, pos, has_q, s.q, s.row);
    s.self = -1;
    s.pos = pos;
    s.r = a.radius, s.r_wide = a.radius_wide, s.in2 = a.radius_in2;
    return s;
  }
  static __device__ __forceinline__ void start(Lane &st, unsigned long long *) { st.w = st.ax = st.ay = st.az = 0.f; }
  static __device__ __forceinline__ bool one(const Args &a) { return WEIGHT == kMsAnyWeight ? a.weight == TKNN_W_ONE : kOne; }
  static __device__ __forceinline__ bool member(const Args &, const Query &s, int32_t, const LbvhPoint &, float d) { return d <= s.r; }
  static __device__ __forceinline__ void lane_take(const Args &a, const Query &, Lane &st, uint32_t, int64_t, const LbvhPoint &, float dx, float dy, float dz,
                                                   float d2, float d) {
#pragma clang fp contract(off)
    if constexpr (kOne) {
      st.ax += dx, st.ay += dy, st.az += dz;
    } else {
      const float w = WEIGHT == kMsAnyWeight ? rd_weight_of(a.weight, d2, d, a.coef) : rd_weight<WEIGHT>(d2, d, a.coef);
      st.w += w;
      st.ax += w * dx, st.ay += w * dy, st.az += w * dz;
    }
  }
  static __device__ __forceinline__ void take(const Args &a, const Query &s, Lane &st, uint32_t &part, bool hit, int64_t slot, const LbvhPoint &p, float dx,
                                              float dy, float dz, float d2, float d, int, int) {
    part = t_count(part, __ballot(hit));
    if (hit) lane_take(a, s, st, 0u, slot, p, dx, dy, dz, d2, d);
  }
  static __device__ __forceinline__ uint32_t row_end(const Args &, const Query &, Lane &st, uint32_t part, int, int) {
    if constexpr (!kOne) st.w = t_team_sum(st.w);
    st.ax = t_team_sum(st.ax), st.ay = t_team_sum(st.ay), st.az = t_team_sum(st.az);
    return t_team_sum(part);
  }
  // The finished walk of one row, by the one lane that holds its sums: the header's loop.  Returns 1 if the row is walked again
  // (the call's own counter word: the next pass's list length).
  static __device__ __forceinline__ unsigned long long row_write(const Args &a, const Query &s, const Lane &st, uint32_t cnt) {
#pragma clang fp contract(off)
    const int64_t j = s.row;
    const float x = s.q.x, y = s.q.y, z = s.q.z;
    const float inf = __uint_as_float(0x7f800000u);
    int status, steps = a.pass;
    bool alive = false, shifted = true;
    float W = 0.f, shift = inf;
    if (x != x || y != y || z != z) {
      status = TKNN_MS_INVALID, cnt = 0u;
    } else if (cnt == 0u) {
      status = TKNN_MS_EMPTY;
      shifted = a.pass == 0;  // a later pass: the last shift stays
    } else {
      W = one(a) ? (float)cnt : st.w;
      const float sx = st.ax / W, sy = st.ay / W, sz = st.az / W;
      shift = knn_sqrt((sx * sx + sy * sy) + sz * sz);
      if (shift != shift) {
        status = TKNN_MS_INVALID;
      } else {
        float *p = a.pos + 3 * j;
        p[0] = x + sx, p[1] = y + sy, p[2] = z + sz;
        steps = a.pass + 1;
        const bool converged = shift <= a.tol;
        status = converged ? TKNN_MS_CONVERGED : TKNN_MS_RUNNING;
        alive = !converged && steps < a.max_iterations;
      }
    }
    a.alive[s.pos] = alive ? 1 : 0;
    a.status[j] = (uint8_t)status;
    if (a.counts) a.counts[j] = (int32_t)cnt;
    if (a.wsum) a.wsum[j] = W;
    if (a.shift && shifted) a.shift[j] = shift;
    if (a.iterations) a.iterations[j] = steps;
    return alive ? 1ull : 0ull;
  }
  static __device__ __forceinline__ bool lane_arith(const Args &) { return false; }
};

template <class F>
void ms_weight_case(int weight, F &&f) {
  switch (weight) {
    case TKNN_W_GAUSS: f(std::integral_constant<int, TKNN_W_GAUSS>{}); break;
    case TKNN_W_EPANECHNIKOV: f(std::integral_constant<int, TKNN_W_EPANECHNIKOV>{}); break;
    default: f(std::integral_constant<int, TKNN_W_ONE>{}); break;
  }
}

// ---- 0. the own points as seeds: the position of row prim_id[slot] is the sorted point of that slot ----------------------------------
__global__ void __launch_bounds__(kMsFlatBlock) ms_own_seeds_kernel(LbvhView tv, float *__restrict__ pos) {
  const int64_t slot = (int64_t)blockIdx.x * kMsFlatBlock + threadIdx.x;
  if (slot >= (int64_t)tv.n) return;
  const LbvhPoint p = tv.points[slot];
  float *o = pos + 3 * (int64_t)tv.prim_id[slot];
  o[0] = p.x, o[1] = p.y, o[2] = p.z;
}

// the curve codes of the seeds of a work list where they are now (query_order.h's key), for the sort that reorders the list
__global__ void __launch_bounds__(kMsFlatBlock) ms_code_kernel(const float *__restrict__ pos, const uint32_t *__restrict__ list, int32_t count,
                                                              const float *__restrict__ scene, uint32_t *__restrict__ codes, int curve) {
  const int32_t i = blockIdx.x * kMsFlatBlock + threadIdx.x;
  if (i >= count) return;
  const float *c = pos + 3 * (int64_t)list[i];
  const float ext = fmaxf(fmaxf(scene[3] - scene[0], scene[4] - scene[1]), scene[5] - scene[2]);
  codes[i] = (uint32_t)curve_point_key(curve, c[0], c[1], c[2], scene[0], scene[1], scene[2], ext, kCodeBits / 3);
}

// ---- 3. the seeds per status, into counts[0 .. 4) ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMsFlatBlock) ms_tally_kernel(const uint8_t *__restrict__ status, int32_t m, unsigned long long *__restrict__ counts) {
  const int32_t j = blockIdx.x * kMsFlatBlock + threadIdx.x;
  const int st = j < m ? (int)status[j] : -1;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const unsigned long long mask = __ballot(st == v);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&counts[v], (unsigned long long)__popcll(mask));
  }
}

}  // namespace

void Engine::mean_shift(const tknnMeanShiftOptions &o, tknnMeanShiftInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const bool own = o.d_seeds == nullptr;
  int reorder = 0;  // (measured, not adopted as a default)
  if (const char *e = getenv("TKNN_MEANSHIFT_REORDER")) reorder = std::max(0, atoi(e));
  // the call's workspace (the layout: the file head)
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t sort_bytes = query_order_sort_bytes(m, s);
  size_t select_bytes = 0;
  {
    uint32_t *null_u32 = nullptr;
    uint8_t *null_u8 = nullptr;
    int *null_int = nullptr;
    OWLMI_HIP(hipcub::DeviceSelect::Flagged(nullptr, select_bytes, null_u32, null_u8, null_u32, null_int, (int)m, s));
  }
  const size_t words_b = align((kRadWords + 4) * sizeof(unsigned long long)), col_b = align(((size_t)m + 1) * sizeof(uint32_t)), byte_b = align((size_t)m),
               pos_b = align((size_t)m * 3 * sizeof(float)), tmp_b = align(std::max(sort_bytes, select_bytes));
  char *ws = (char *)workspace(words_b + 5 * col_b + 2 * byte_b + pos_b + tmp_b + 256);
  uint32_t *codes = (uint32_t *)(ws + words_b), *codes_alt = (uint32_t *)(ws + words_b + col_b);
  uint32_t *lists[2] = {(uint32_t *)(ws + words_b + 2 * col_b), (uint32_t *)(ws + words_b + 3 * col_b)};
  char *at = ws + words_b + 4 * col_b;
  int32_t *redo = (int32_t *)at;
  at += col_b;
  uint8_t *alive = (uint8_t *)at;
  at += byte_b;
  uint8_t *status = (uint8_t *)at;
  at += byte_b;
  float *pos = (float *)at;
  at += pos_b;
  void *tmp = at;
  at += tmp_b;
  int *selected = (int *)at;
  unsigned long long *words = (unsigned long long *)ws, *tally = words + kRadWords;

  const LbvhView tv = bvh_.view();
  MeanShiftArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = tv;
  a.wide = bvh_.wide_view();
  a.queries = pos;
  a.radius = o.radius;
  a.radius_wide = o.radius * 1.000001f;
  a.radius_in2 = radius_inside2(o.radius);
  if (o.weight == TKNN_W_GAUSS) a.coef = (float)(-0.5 / ((double)o.bandwidth * (double)o.bandwidth));
  if (o.weight == TKNN_W_EPANECHNIKOV) a.coef = (float)(1.0 / ((double)o.radius * (double)o.radius));
  a.tol = o.tol;
  a.weight = o.weight;
  a.max_iterations = o.max_iterations;
  if (const char *e = getenv("TKNN_MEANSHIFT_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.pos = pos;
  a.alive = alive;
  a.status = status;
  a.counts = o.d_counts;
  a.wsum = o.d_wsum;
  a.shift = o.d_shift;
  a.iterations = o.d_iterations;
  a.redo = redo;
  a.ws = words;

  const unsigned flat_blocks = (unsigned)((m + kMsFlatBlock - 1) / kMsFlatBlock);
  unsigned long long *h_words = h_counters_;
  tknnMeanShiftInfo r;
  std::memset(&r, 0, sizeof r);
  // a pass's walk lies between a pair of events of its own parity: the pair is read once the NEXT pass's synchronisation is through
  hipEvent_t walk_from[2] = {ev_c_, ev_f_}, walk_to[2] = {ev_d_, ev_g_};
  auto add_ms = [&](float &into, hipEvent_t from, hipEvent_t to) {
    float ms = 0;
    OWLMI_HIP(hipEventElapsedTime(&ms, from, to));
    into += ms;
  };
  const uint32_t *cur = nullptr;  // the work list
  auto other = [&]() { return cur == lists[0] ? lists[1] : lists[0]; };
  int64_t active = m;
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  int pass = 0;
  for (;; pass++) {
    OWLMI_HIP(hipEventRecord(ev_b_, s));
    if (pass > 0) {
      // the rows of the last pass that are walked again, in their order; `active` of them (the host knows: kRadOwn)
      uint32_t *next = other();
      size_t bytes = select_bytes;
      OWLMI_HIP(hipcub::DeviceSelect::Flagged(tmp, bytes, cur, alive, next, selected, (int)a.m, s));
      cur = next;
    }
    OWLMI_HIP(hipEventRecord(ev_h_, s));
    if (pass == 0) {
      if (own) {
        hipLaunchKernelGGL(ms_own_seeds_kernel, dim3((unsigned)((tv.n + kMsFlatBlock - 1) / kMsFlatBlock)), dim3(kMsFlatBlock), 0, s, tv, pos);
        OWLMI_HIP(hipGetLastError());
        cur = (const uint32_t *)tv.prim_id;
      } else {
        OWLMI_HIP(hipMemcpyAsync(pos, o.d_seeds, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
        query_order(pos, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, lists[1], lists[0], tmp, sort_bytes, s);
        cur = lists[0];
      }
    } else if (reorder > 0 && pass % reorder == 0) {
      uint32_t *next = other();
      hipLaunchKernelGGL(ms_code_kernel, dim3((unsigned)((active + kMsFlatBlock - 1) / kMsFlatBlock)), dim3(kMsFlatBlock), 0, s, (const float *)pos, cur,
                         (int32_t)active, bvh_.scene_device(), codes, bvh_.curve());
      OWLMI_HIP(hipGetLastError());
      size_t bytes = sort_bytes;
      OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, (const uint32_t *)codes, codes_alt, cur, next, (int)active, 0, kCodeBits + 1, s));
      cur = next;
    }
    OWLMI_HIP(hipEventRecord(walk_from[pass & 1], s));
    OWLMI_HIP(hipMemsetAsync(words, 0, kRadWords * sizeof(unsigned long long), s));
    a.order = cur;
    a.m = (int32_t)active;
    a.pass = pass;
    unsigned long long n_redo = 0;
    ms_weight_case(o.weight, [&](auto weight) { n_redo = rad_walks<MeanShiftRule<decltype(weight)::value>, MeanShiftRule<kMsAnyWeight>>(a, cu_count_, h_words, s); });
    OWLMI_HIP(hipEventRecord(walk_to[pass & 1], s));
    if (n_redo) OWLMI_HIP(hipStreamSynchronize(s));  // the counters as the lane kernel left them
    r.iterations = pass + 1;
    r.walks += active;
    r.fallback_items += (int64_t)h_words[kRadLaneRows];
    r.node_tests += (int64_t)h_words[kRadNodeTests];
    r.point_tests += (int64_t)h_words[kRadPointTests];
    add_ms(r.compact_ms, ev_b_, ev_h_);
    add_ms(r.order_ms, ev_h_, walk_from[pass & 1]);
    if (pass > 0) add_ms(r.walk_ms, walk_from[(pass - 1) & 1], walk_to[(pass - 1) & 1]);
    const int64_t moving = (int64_t)h_words[kRadOwn];
    if (moving == 0 || pass + 1 >= o.max_iterations) break;
    active = moving;
  }
  OWLMI_HIP(hipMemsetAsync(tally, 0, 4 * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(ms_tally_kernel, dim3(flat_blocks), dim3(kMsFlatBlock), 0, s, (const uint8_t *)status, (int32_t)m, tally);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipMemcpyAsync(h_words + kRadWords, tally, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  if (o.d_modes) OWLMI_HIP(hipMemcpyAsync(o.d_modes, pos, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (o.d_status) OWLMI_HIP(hipMemcpyAsync(o.d_status, status, (size_t)m, hipMemcpyDeviceToDevice, s));
  OWLMI_HIP(hipEventRecord(ev_e_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  add_ms(r.walk_ms, walk_from[pass & 1], walk_to[pass & 1]);
  add_ms(r.solve_ms, ev_a_, ev_e_);
  r.running = (int64_t)h_words[kRadWords + TKNN_MS_RUNNING];
  r.converged = (int64_t)h_words[kRadWords + TKNN_MS_CONVERGED];
  r.empty = (int64_t)h_words[kRadWords + TKNN_MS_EMPTY];
  r.invalid = (int64_t)h_words[kRadWords + TKNN_MS_INVALID];
  *info = r;
}

}  // namespace owlmi
