// plane.hip -- RANSAC plane segmentation of the built set (tknnSegmentPlane, include/owlknn_plane.h): the plane most active rows lie
// within a distance of, every hypothesis scored through the 64-ary box pyramid.
//
//   0. plane_flag_kernel copies the sorted points into a float4 column with every inactive slot (masked out, not finite, padding)
//      turned into NaN -- the distance test then fails for it with no flag to load -- and writes an active flag per sorted slot and
//      per row; two hipcub exclusive sums make them prefixes: "active rows under a box" is a difference of two words, which covers
//      NaN points, the ragged last block and the mask alike; plane_list_kernel writes the list A (as sorted slots, by rank of the row).
//      The host reads c;
//   per batch of TKNN_PLANE_BATCH trials:
//   a. plane_trial_kernel: one lane per trial samples (ransac_sample.h), builds the plane, sets the status; an OK trial is appended
//      to a compact list;
//   b. plane_walk_kernel, the hot path: a wave per OK trial walks the pyramid with the slab as its query -- the 64 lanes test the 64
//      children of a wide node, a child wholly outside is dropped, one wholly inside is counted by the prefix, the others go on an
//      LDS stack, leaf blocks are tested four at a time with lanes = points.  plane_sweep_kernel is the fallback and the yardstick: a
//      wave per OK trial over every slot, no tree;
//   c. plane_best_kernel / plane_pick_kernel: a 64-bit atomicMax over (inliers, ~trial), the winner's plane copied.  The host reads
//      the best and the counts: the batch's one synchronisation;
//   d. plane_moment_kernel: the inliers of a plane, their count, sum of d^2 and fp64 moments in a fixed order, and the inlier flag per
//      row; it evaluates the best plane, every refit and the final plane.  hipcub::DeviceSelect writes the sorted rows.
// The call's workspace (Engine::workspace): counters | points | slot prefix | row prefix | A | survivors | best | moment rows | flags | cub.
#include "owlknn_plane.h"
#include "plane_solve.h"
#include "ransac_sample.h"
#include "trueknn_engine.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kPlaneBlock = 256;
constexpr int kPlaneTrialBlock = 64;
constexpr int kPlaneMomentBlocksPerCu = 4;
// The walk's stack.  An entry is a node whose children are still to be tested; only nodes of the levels 1 .. top - 1 are pushed
// (a kept child of level 0 is a leaf block and is tested at once), top <= LBVH_WIDE_LEVELS = 6.  The walk is depth first: it pops
// one entry and pushes at most 64 children of the level below, so when a node of level l is popped the stack holds at most 63
// waiting siblings on each of the levels above l, and the push adds at most 64: never more than 63 * 4 + 64 = 316 entries.
constexpr int kPlaneStack = 320;
static_assert(LBVH_WIDE_LEVELS <= 6 && 63 * (LBVH_WIDE_LEVELS - 2) + 64 <= kPlaneStack, "the walk's stack cannot run out");
// the counters, 64-bit words
enum { kPsSurvivors = 0, kPsStatus = 1 /* .. 4 */, kPsBest = 5, kPsNodeTests = 6, kPsPointTests = 7, kPsBoxed = 8, kPsSelected = 9, kPsWords = 10 };

struct PlaneSurvivor {
  float n[3], a[3];
  int32_t trial, inliers;
};

size_t plane_align(size_t b) { return (b + 255) & ~(size_t)255; }

// the fp32 distance of a row to the plane, literally as the header states it
__device__ __forceinline__ float plane_dist(const float *n, const float *a, float x, float y, float z) {
#pragma clang fp contract(off)
  const float dx = x - a[0], dy = y - a[1], dz = z - a[2];
  return fabsf((n[0] * dx + n[1] * dy) + n[2] * dz);
}

// ---- 0. the active rows ------------------------------------------------------------------------------------------------------------
// slot s of [0, npad]: pts[s] = the point with its row in w, NaN coordinates where it is not active (w = -1 in the padding);
// pre_slot[s] and pre_row[row] = its flag, pre_slot[npad] = pre_row[n] = 0 (the sums run over one word more)
__global__ void __launch_bounds__(kPlaneBlock) plane_flag_kernel(const LbvhPoint *__restrict__ points, const int32_t *__restrict__ prim_id, int32_t n, int32_t npad,
                                                               const uint8_t *__restrict__ active, float4 *__restrict__ pts, int32_t *__restrict__ pre_slot,
                                                               int32_t *__restrict__ pre_row) {
  const int64_t s = (int64_t)blockIdx.x * kPlaneBlock + threadIdx.x;
  if (s > npad) return;
  if (s == npad) {
    pre_slot[npad] = 0, pre_row[n] = 0;
    return;
  }
  const float nan = __uint_as_float(0x7fc00000u);
  float4 v = make_float4(nan, nan, nan, __int_as_float(-1));
  int32_t flag = 0;
  if (s < n) {
    const LbvhPoint p = points[s];
    const int32_t row = prim_id[s];
    if (row >= 0 && row < n) {  // (a tree without ids names its points by row)
      flag = (isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && (!active || active[row] != 0)) ? 1 : 0;
      if (flag) v.x = p.x, v.y = p.y, v.z = p.z;
      v.w = __int_as_float(row);
      pre_row[row] = flag;
    }
  }
  pts[s] = v;
  pre_slot[s] = flag;
}

// A[rank of the row among the active rows] = its sorted slot
__global__ void __launch_bounds__(kPlaneBlock) plane_list_kernel(const float4 *__restrict__ pts, const int32_t *__restrict__ pre_row, int32_t n, int32_t *__restrict__ list) {
  const int64_t s = (int64_t)blockIdx.x * kPlaneBlock + threadIdx.x;
  if (s >= n) return;
  const float4 p = pts[s];
  if (!(p.x == p.x)) return;
  const int32_t at = pre_row[__float_as_int(p.w)];
  if (at >= 0 && at < n) list[at] = (int32_t)s;
}

// ---- a. the trials -----------------------------------------------------------------------------------------------------------------
struct PlaneTrialArgs {
  const float4 *pts;
  const int32_t *list;
  int32_t c;
  uint32_t seed;
  int32_t first, count;  // the batch: trials first .. first + count
  int32_t has_axis;
  float unit[3], min_cos;
  PlaneSurvivor *survivors;
  unsigned long long *counters;
  int32_t *status;   // the caller's, by trial; may be null
  int32_t *inliers;  // the caller's, by trial; may be null (-1 here: not scored)
};

__device__ int plane_trial(const PlaneTrialArgs &a, int32_t trial, float *n, float *anchor) {
#pragma clang fp contract(off)
  uint32_t idx[4];
  if (!ransac_sample(a.seed, (uint32_t)trial, 3, (uint32_t)a.c, idx)) return TKNN_PLANE_DUPLICATE;
  const float4 p0 = a.pts[a.list[idx[0]]], p1 = a.pts[a.list[idx[1]]], p2 = a.pts[a.list[idx[2]]];
  const float e1x = p1.x - p0.x, e1y = p1.y - p0.y, e1z = p1.z - p0.z;
  const float e2x = p2.x - p0.x, e2y = p2.y - p0.y, e2z = p2.z - p0.z;
  const float gx = e1y * e2z - e1z * e2y, gy = e1z * e2x - e1x * e2z, gz = e1x * e2y - e1y * e2x;
  const float l1 = (e1x * e1x + e1y * e1y) + e1z * e1z, l2 = (e2x * e2x + e2y * e2y) + e2z * e2z;
  const float g2 = (gx * gx + gy * gy) + gz * gz;
  if (!(isfinite(g2) && g2 > 0x1p-40f * (l1 * l2))) return TKNN_PLANE_DEGENERATE;
  const float q = __builtin_sqrtf(g2);
  n[0] = gx / q, n[1] = gy / q, n[2] = gz / q;
  anchor[0] = p0.x, anchor[1] = p0.y, anchor[2] = p0.z;
  if (a.has_axis && !(fabsf((n[0] * a.unit[0] + n[1] * a.unit[1]) + n[2] * a.unit[2]) >= a.min_cos)) return TKNN_PLANE_ANGLE;
  return TKNN_PLANE_OK;
}

__global__ void __launch_bounds__(kPlaneTrialBlock) plane_trial_kernel(PlaneTrialArgs a) {
  const int32_t i = blockIdx.x * kPlaneTrialBlock + threadIdx.x;
  if (i >= a.count) return;
  const int32_t trial = a.first + i;
  PlaneSurvivor sv;
  const int status = plane_trial(a, trial, sv.n, sv.a);
  atomicAdd(&a.counters[kPsStatus + status], 1ull);
  if (a.status) a.status[trial] = status;
  if (a.inliers) a.inliers[trial] = -1;
  if (status != TKNN_PLANE_OK) return;
  const int32_t at = (int32_t)atomicAdd(&a.counters[kPsSurvivors], 1ull);  // (< TKNN_PLANE_BATCH: one per lane of the batch at most)
  sv.trial = trial, sv.inliers = 0;
  a.survivors[at] = sv;
}

// ---- b. the scores -----------------------------------------------------------------------------------------------------------------
struct PlaneScoreArgs {
  LbvhWideView wide;
  const float4 *pts;        // npad
  const int32_t *pre_slot;  // npad + 1
  int32_t npad;
  float thr;
  PlaneSurvivor *survivors;
  unsigned long long *counters;
};

// The slab test of a box.  With l = lo - a and g = hi - a rounded per axis (relative to the anchor, as the distance expression
// takes a point), the products n*l and n*g rounded, t_lo = the sum of the smaller and t_hi = the sum of the larger products in the
// order (x + y) + z: every operation of the distance expression is monotone under round-to-nearest -- lo_i <= p_i <= hi_i gives
// l <= fl(p_i - a_i) <= g, so fl(n_i * fl(p_i - a_i)) lies between the two rounded products, and a rounded sum of two terms is
// monotone in each -- hence the fp32 value s(p) of EVERY point of the box lies in [t_lo, t_hi] exactly, with no margin.  A box is OUT
// iff t_lo > thr or t_hi < -thr: then |s(p)| > thr for all of its points; IN iff t_hi <= thr and t_lo >= -thr: then |s(p)| <= thr for
// all of them.  Both rules are one-sided.  W = the sum of |n*l| + |n*g| guards the bounds themselves: unless W < 2^100 -- an
// infinite or NaN bound, which fminf / fmaxf would hide, or a coordinate near overflow -- the box is left to its points.
__device__ __forceinline__ void plane_box_rule(const LbvhBox &bx, const float *n, const float *a, float thr, bool &out, bool &in) {
#pragma clang fp contract(off)
  float mn[3], mx[3], w[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float l = bx.lo[i] - a[i], g = bx.hi[i] - a[i];
    const float pl = n[i] * l, pg = n[i] * g;
    mn[i] = fminf(pl, pg), mx[i] = fmaxf(pl, pg);
    w[i] = fabsf(pl) + fabsf(pg);
  }
  const float t_lo = (mn[0] + mn[1]) + mn[2], t_hi = (mx[0] + mx[1]) + mx[2], W = (w[0] + w[1]) + w[2];
  const bool sure = W < 0x1p100f;  // (false for a NaN)
  out = sure && (t_lo > thr || t_hi < -thr);
  in = sure && t_hi <= thr && t_lo >= -thr;
}

// lanes of the wave below mine that are set in m
__device__ __forceinline__ int plane_rank(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// a wave per survivor (a workgroup past the list returns)
__global__ void __launch_bounds__(64) plane_walk_kernel(PlaneScoreArgs a) {
  __shared__ int32_t stack[kPlaneStack];
  __shared__ int32_t leaf[64];
  const int32_t count = (int32_t)a.counters[kPsSurvivors];
  const int32_t sv = blockIdx.x;
  if (sv >= count) return;
  const int lane = threadIdx.x;
  float n[3], anc[3];
  for (int i = 0; i < 3; i++) n[i] = a.survivors[sv].n[i], anc[i] = a.survivors[sv].a[i];
  const float thr = a.thr;
  const int top = a.wide.levels;
  int32_t inliers = 0;  // per lane; summed at the end
  uint32_t node_tests = 0, point_tests = 0, boxed = 0;
  int sp = 1;  // the same in every lane
  bool spilled = false;
  if (lane == 0) stack[0] = (top << 26) | 0;  // virtual root above the top level
  __syncthreads();
  while (sp > 0) {
    const int32_t e = stack[sp - 1];
    sp--;
    __syncthreads();  // (every lane has read the entry before a push can land on it)
    const int lvl = (e >> 26) - 1;  // level of the children
    const int32_t first_child = (e & 0x3ffffff) * 64;
    // the virtual root has the top level's few boxes as its children
    const int32_t nchild = a.wide.count[lvl];
    const int32_t c = first_child + lane;
    const bool valid = c < nchild;
    bool out = true, in = false;
    if (valid) {
      const LbvhBox bx = a.wide.level[lvl][c];
      plane_box_rule(bx, n, anc, thr, out, in);
      node_tests++;
      if (in) {
        const int64_t span = (int64_t)LBVH_BLOCK << (6 * lvl);  // slots under one child of this level
        const int64_t first = (int64_t)c * span;
        const int64_t end = first + span < (int64_t)a.npad ? first + span : (int64_t)a.npad;
        const int32_t rows = first < end ? a.pre_slot[end] - a.pre_slot[first] : 0;
        inliers += rows, boxed += (uint32_t)rows;
      }
    }
    const bool keep = valid && !out && !in;
    const unsigned long long keep_m = __ballot(keep);
    const int nkeep = __popcll(keep_m);
    if (lvl > 0) {
      if (sp + nkeep > kPlaneStack) {  // (cannot happen: kPlaneStack.  If it did, no count is lost: the wave sweeps every slot below)
        spilled = true;
        break;
      }
      if (keep) stack[sp + plane_rank(keep_m)] = (lvl << 26) | c;
      sp += nkeep;
    } else {
      // the children are leaf blocks: four at a time, a lane is point (lane & 15) of block (lane >> 4) of the four
      if (keep) leaf[plane_rank(keep_m)] = c;
      __syncthreads();
      for (int i = 0; i < nkeep; i += 4) {
        const int j = i + (lane >> 4);
        bool hit = false, live = false;
        if (j < nkeep) {
          const float4 p = a.pts[(int64_t)leaf[j] * LBVH_BLOCK + (lane & 15)];  // (block < ceil(n / 16): below npad)
          live = p.x == p.x;
          hit = plane_dist(n, anc, p.x, p.y, p.z) <= thr;
        }
        inliers += hit ? 1 : 0;
        point_tests += live ? 1u : 0u;
      }
    }
    __syncthreads();
  }
  if (spilled) {
    inliers = 0, boxed = 0, point_tests = 0;
    for (int64_t j = lane; j < a.npad; j += 64) {
      const float4 p = a.pts[j];
      inliers += plane_dist(n, anc, p.x, p.y, p.z) <= thr ? 1 : 0;
      point_tests += p.x == p.x ? 1u : 0u;
    }
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    inliers += __shfl_xor(inliers, off, 64);
    node_tests += __shfl_xor(node_tests, off, 64);
    point_tests += __shfl_xor(point_tests, off, 64);
    boxed += __shfl_xor(boxed, off, 64);
  }
  if (lane == 0) {
    a.survivors[sv].inliers = inliers;
    atomicAdd(&a.counters[kPsNodeTests], (unsigned long long)node_tests);
    atomicAdd(&a.counters[kPsPointTests], (unsigned long long)point_tests);
    atomicAdd(&a.counters[kPsBoxed], (unsigned long long)boxed);
  }
}

// the fallback: a wave per survivor, its lanes over every slot, no tree
__global__ void __launch_bounds__(64) plane_sweep_kernel(PlaneScoreArgs a) {
  const int32_t count = (int32_t)a.counters[kPsSurvivors];
  const int32_t sv = blockIdx.x;
  if (sv >= count) return;
  float n[3], anc[3];
  for (int i = 0; i < 3; i++) n[i] = a.survivors[sv].n[i], anc[i] = a.survivors[sv].a[i];
  int32_t inliers = 0;
  for (int64_t j = threadIdx.x; j < a.npad; j += 64) {
    const float4 p = a.pts[j];
    inliers += plane_dist(n, anc, p.x, p.y, p.z) <= a.thr ? 1 : 0;
  }
  for (int off = 1; off < 64; off <<= 1) inliers += __shfl_xor(inliers, off, 64);
  if (threadIdx.x == 0) a.survivors[sv].inliers = inliers;
}

// ---- c. the best -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long plane_order(int32_t inliers, int32_t trial) {
  return ((unsigned long long)(uint32_t)inliers << 32) | (unsigned long long)(0xffffffffu - (uint32_t)trial);
}

__global__ void __launch_bounds__(kPlaneBlock) plane_best_kernel(const PlaneSurvivor *__restrict__ survivors, unsigned long long *__restrict__ counters,
                                                               int32_t *__restrict__ trial_inliers) {
  const int32_t sv = blockIdx.x * kPlaneBlock + threadIdx.x;
  if (sv >= (int32_t)counters[kPsSurvivors]) return;
  const PlaneSurvivor &v = survivors[sv];
  if (trial_inliers) trial_inliers[v.trial] = v.inliers;
  atomicMax(&counters[kPsBest], plane_order(v.inliers, v.trial));
}

// (the best of an earlier batch is no survivor of this one: its plane stays)
__global__ void __launch_bounds__(kPlaneBlock) plane_pick_kernel(const PlaneSurvivor *__restrict__ survivors, const unsigned long long *__restrict__ counters,
                                                               float *__restrict__ best) {
  const int32_t sv = blockIdx.x * kPlaneBlock + threadIdx.x;
  if (sv >= (int32_t)counters[kPsSurvivors]) return;
  const PlaneSurvivor &v = survivors[sv];
  if (plane_order(v.inliers, v.trial) != counters[kPsBest]) return;
  for (int i = 0; i < 3; i++) best[i] = v.n[i], best[3 + i] = v.a[i];
}

// ---- d. the moments of the inliers of a plane --------------------------------------------------------------------------------------
struct PlaneMomentArgs {
  const float4 *pts;
  int32_t npad;
  float thr;
  float n[3], a[3];
  double centre[3];
  double *rows;    // gridDim.x rows of kPlMoments doubles, then the total
  uint8_t *flags;  // by row, may be null
};

__device__ __forceinline__ double plane_wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ void __launch_bounds__(kPlaneBlock) plane_moment_kernel(PlaneMomentArgs a) {
#pragma clang fp contract(off)
  __shared__ double part[kPlaneBlock / 64][kPlMoments];
  double acc[kPlMoments];
#pragma unroll
  for (int i = 0; i < kPlMoments; i++) acc[i] = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * kPlaneBlock + threadIdx.x; j < (int64_t)a.npad; j += (int64_t)gridDim.x * kPlaneBlock) {
    const float4 p = a.pts[j];
    const float d = plane_dist(a.n, a.a, p.x, p.y, p.z);
    const bool in = d <= a.thr;
    const int32_t row = __float_as_int(p.w);
    if (a.flags && row >= 0) a.flags[row] = in ? 1 : 0;
    if (!in) continue;
    const double x = (double)p.x - a.centre[0], y = (double)p.y - a.centre[1], z = (double)p.z - a.centre[2];
    acc[kPlCount] += 1.0;
    acc[kPlSumD2] += (double)d * (double)d;
    acc[kPlS1] += x, acc[kPlS1 + 1] += y, acc[kPlS1 + 2] += z;
    acc[kPlS2] += x * x, acc[kPlS2 + 1] += x * y, acc[kPlS2 + 2] += x * z;
    acc[kPlS2 + 3] += y * y, acc[kPlS2 + 4] += y * z, acc[kPlS2 + 5] += z * z;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kPlMoments; i++) {
    const double v = plane_wave_sum(acc[i]);
    if (lane == 0) part[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kPlMoments) {
    double v = 0.0;
    for (int w = 0; w < kPlaneBlock / 64; w++) v += part[w][threadIdx.x];
    a.rows[(int64_t)blockIdx.x * kPlMoments + threadIdx.x] = v;
  }
}

// rows[nrows] = the sum of rows[0 .. nrows), in index order
__global__ void __launch_bounds__(64) plane_moment_sum_kernel(double *rows, int32_t nrows) {
  if (threadIdx.x >= kPlMoments) return;
  double v = 0.0;
  for (int32_t b = 0; b < nrows; b++) v += rows[(int64_t)b * kPlMoments + threadIdx.x];
  rows[(int64_t)nrows * kPlMoments + threadIdx.x] = v;
}

}  // namespace

void Engine::segment_plane(const tknnPlaneOptions &o, tknnPlaneInfo *info, hipStream_t s) {
  const int32_t n = (int32_t)bvh_.size();
  const int32_t npad = (int32_t)(((int64_t)n + LBVH_BLOCK - 1) / LBVH_BLOCK * LBVH_BLOCK);  // (n <= 2^31 - 65: tknn_api.hip)
  const bool force_sweep = [] {
    const char *e = getenv("TKNN_PLANE_FORCE_FALLBACK");
    return e && !std::strcmp(e, "1");
  }();
  const LbvhView view = bvh_.view();
  const LbvhWideView wide = bvh_.wide_view();
  const bool sweep = force_sweep || n <= 64 || wide.levels < 1;
  const int moment_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)npad + kPlaneBlock - 1) / kPlaneBlock, (int64_t)cu_count_ * kPlaneMomentBlocksPerCu));
  size_t cub_bytes = 0, b1 = 0, b2 = 0;
  {
    int32_t *i32 = nullptr;
    uint8_t *u8 = nullptr;
    size_t b0 = 0;
    OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b1, i32, i32, npad + 1, s));
    OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b0, i32, i32, n + 1, s));
    b1 = std::max(b0, b1);
    OWLMI_HIP(hipcub::DeviceSelect::Flagged(nullptr, b2, hipcub::CountingInputIterator<int32_t>(0), u8, i32, i32, n, s));
    cub_bytes = std::max(b1, b2);
  }
  const size_t col_counters = plane_align(kPsWords * sizeof(unsigned long long)), col_pts = plane_align((size_t)npad * sizeof(float4)),
               col_pre_slot = plane_align(((size_t)npad + 1) * sizeof(int32_t)), col_pre_row = plane_align(((size_t)n + 1) * sizeof(int32_t)),
               col_list = plane_align((size_t)n * sizeof(int32_t)), col_surv = plane_align((size_t)TKNN_PLANE_BATCH * sizeof(PlaneSurvivor)),
               col_best = plane_align(8 * sizeof(float)), col_rows = plane_align((size_t)(moment_blocks + 1) * kPlMoments * sizeof(double)),
               col_flags = plane_align((size_t)n);
  char *ws = (char *)workspace(col_counters + col_pts + col_pre_slot + col_pre_row + col_list + col_surv + col_best + col_rows + col_flags + plane_align(cub_bytes));
  unsigned long long *counters = (unsigned long long *)ws;
  float4 *pts = (float4 *)(ws + col_counters);
  int32_t *pre_slot = (int32_t *)((char *)pts + col_pts);
  int32_t *pre_row = (int32_t *)((char *)pre_slot + col_pre_slot);
  int32_t *list = (int32_t *)((char *)pre_row + col_pre_row);
  PlaneSurvivor *survivors = (PlaneSurvivor *)((char *)list + col_list);
  float *best_plane = (float *)((char *)survivors + col_surv);
  double *rows = (double *)((char *)best_plane + col_best);
  uint8_t *flags = (uint8_t *)((char *)rows + col_rows);
  void *cub_tmp = (char *)flags + col_flags;
  static_assert(kCounterWords >= kPlMoments && kCounterWords >= kPsWords, "the host's copy of the counters holds a moment row");

  tknnPlaneInfo r;
  std::memset(&r, 0, sizeof r);
  r.best_trial = -1;
  float unit[3];
  const bool has_axis = plane_axis(o.axis, unit);
  double centre[3];
  for (int i = 0; i < 3; i++) {
    centre[i] = 0.5 * ((double)scene_[i] + (double)scene_[3 + i]);
    if (!std::isfinite(centre[i])) centre[i] = 0.0;
  }
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  // ---- 0. the active rows ----
  OWLMI_HIP(hipMemsetAsync(counters, 0, kPsWords * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(plane_flag_kernel, dim3((unsigned)(((int64_t)npad + 1 + kPlaneBlock - 1) / kPlaneBlock)), dim3(kPlaneBlock), 0, s, view.points, view.prim_id, n, npad,
                     o.d_active, pts, pre_slot, pre_row);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(cub_tmp, b1, pre_slot, pre_slot, npad + 1, s));
  OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(cub_tmp, b1, pre_row, pre_row, n + 1, s));
  hipLaunchKernelGGL(plane_list_kernel, dim3((unsigned)(((int64_t)n + kPlaneBlock - 1) / kPlaneBlock)), dim3(kPlaneBlock), 0, s, (const float4 *)pts, (const int32_t *)pre_row, n, list);
  OWLMI_HIP(hipGetLastError());
  int32_t c = 0;
  OWLMI_HIP(hipMemcpyAsync(h_counters_, pre_row + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  std::memcpy(&c, h_counters_, sizeof c);
  OWLMI_HIP(hipEventElapsedTime(&r.sample_ms, ev_a_, ev_b_));
  r.active = c;
  if (o.d_trial_status) OWLMI_HIP(hipMemsetAsync(o.d_trial_status, 0xff, (size_t)o.max_trials * sizeof(int32_t), s));
  if (o.d_trial_inliers) OWLMI_HIP(hipMemsetAsync(o.d_trial_inliers, 0xff, (size_t)o.max_trials * sizeof(int32_t), s));

  // ---- the batches ----
  PlaneTrialArgs ta;
  std::memset(&ta, 0, sizeof ta);
  ta.pts = pts, ta.list = list, ta.c = c, ta.seed = o.seed;
  ta.has_axis = has_axis ? 1 : 0, ta.min_cos = o.min_cos;
  std::memcpy(ta.unit, unit, sizeof unit);
  ta.survivors = survivors, ta.counters = counters;
  ta.status = o.d_trial_status, ta.inliers = o.d_trial_inliers;
  PlaneScoreArgs sa;
  std::memset(&sa, 0, sizeof sa);
  sa.wide = wide, sa.pts = pts, sa.pre_slot = pre_slot, sa.npad = npad, sa.thr = o.distance_threshold;
  sa.survivors = survivors, sa.counters = counters;
  unsigned long long best = 0;
  while (c >= 3 && r.trials_run < o.max_trials) {
    ta.first = r.trials_run, ta.count = std::min<int32_t>(TKNN_PLANE_BATCH, o.max_trials - r.trials_run);
    OWLMI_HIP(hipMemsetAsync(counters + kPsSurvivors, 0, sizeof(unsigned long long), s));
    OWLMI_HIP(hipEventRecord(ev_b_, s));
    hipLaunchKernelGGL(plane_trial_kernel, dim3((ta.count + kPlaneTrialBlock - 1) / kPlaneTrialBlock), dim3(kPlaneTrialBlock), 0, s, ta);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipEventRecord(ev_c_, s));
    if (sweep)
      hipLaunchKernelGGL(plane_sweep_kernel, dim3(ta.count), dim3(64), 0, s, sa);
    else
      hipLaunchKernelGGL(plane_walk_kernel, dim3(ta.count), dim3(64), 0, s, sa);
    OWLMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(plane_best_kernel, dim3((ta.count + kPlaneBlock - 1) / kPlaneBlock), dim3(kPlaneBlock), 0, s, (const PlaneSurvivor *)survivors, counters, o.d_trial_inliers);
    OWLMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(plane_pick_kernel, dim3((ta.count + kPlaneBlock - 1) / kPlaneBlock), dim3(kPlaneBlock), 0, s, (const PlaneSurvivor *)survivors,
                       (const unsigned long long *)counters, best_plane);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipEventRecord(ev_d_, s));
    OWLMI_HIP(hipMemcpyAsync(h_counters_, counters, kPsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));  // the batch's best: the stopping rule is the host's
    float sample_ms = 0, score_ms = 0;
    OWLMI_HIP(hipEventElapsedTime(&sample_ms, ev_b_, ev_c_));
    OWLMI_HIP(hipEventElapsedTime(&score_ms, ev_c_, ev_d_));
    r.sample_ms += sample_ms, r.score_ms += score_ms;
    r.trials_run += ta.count;
    r.batches++;
    best = h_counters_[kPsBest];
    const double f = (double)(best >> 32) / (double)c;
    double needed = INFINITY;
    if (o.confidence < 1.0 && f > 0.0) {
      const double miss = std::log(1.0 - std::pow(f, 3.0));  // (f = 1: -inf, needed = 0)
      needed = miss < 0.0 ? std::log(1.0 - o.confidence) / miss : INFINITY;
    }
    if ((double)r.trials_run >= needed) break;
  }
  if (r.trials_run > 0) {
    for (int i = 0; i < 4; i++) r.status_counts[i] = (int64_t)h_counters_[kPsStatus + i];
    r.node_tests = (int64_t)h_counters_[kPsNodeTests];
    r.boxes_counted = (int64_t)h_counters_[kPsBoxed];
    r.point_tests = sweep ? (int64_t)c * r.status_counts[TKNN_PLANE_OK] : (int64_t)h_counters_[kPsPointTests];
    r.lane_rows = sweep ? r.point_tests : 0;
  }

  // ---- evaluate, refit, the outputs ----
  OWLMI_HIP(hipEventRecord(ev_e_, s));
  if (r.status_counts[TKNN_PLANE_OK] > 0) {
    r.best_trial = (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffu));
    float cur[6];
    OWLMI_HIP(hipMemcpyAsync(h_counters_, best_plane, sizeof cur, hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
    std::memcpy(cur, h_counters_, sizeof cur);
    PlaneMomentArgs ma;
    std::memset(&ma, 0, sizeof ma);
    ma.pts = pts, ma.npad = npad, ma.thr = o.distance_threshold;
    std::memcpy(ma.centre, centre, sizeof centre);
    ma.rows = rows;
    double mom[kPlMoments];
    // the moments of the inliers of the plane `p` (normal, anchor), into mom
    auto evaluate = [&](const float *p, uint8_t *row_flags) {
      std::memcpy(ma.n, p, 3 * sizeof(float));
      std::memcpy(ma.a, p + 3, 3 * sizeof(float));
      ma.flags = row_flags;
      hipLaunchKernelGGL(plane_moment_kernel, dim3(moment_blocks), dim3(kPlaneBlock), 0, s, ma);
      OWLMI_HIP(hipGetLastError());
      hipLaunchKernelGGL(plane_moment_sum_kernel, dim3(1), dim3(64), 0, s, rows, (int32_t)moment_blocks);
      OWLMI_HIP(hipGetLastError());
      OWLMI_HIP(hipMemcpyAsync(h_counters_, rows + (size_t)moment_blocks * kPlMoments, kPlMoments * sizeof(double), hipMemcpyDeviceToHost, s));
      OWLMI_HIP(hipStreamSynchronize(s));
      std::memcpy(mom, h_counters_, sizeof mom);
    };
    evaluate(cur, nullptr);
    double kept[kPlMoments];
    std::memcpy(kept, mom, sizeof kept);
    for (int round = 0; round < o.refit_rounds; round++) {
      float next[6];
      if (!plane_refit(kept, centre, next, next + 3)) break;
      evaluate(next, nullptr);
      if (mom[kPlCount] < kept[kPlCount]) break;
      std::memcpy(cur, next, sizeof cur);
      std::memcpy(kept, mom, sizeof kept);
      r.refits_kept++;
    }
    if (o.d_inlier_mask || o.d_inlier_rows) evaluate(cur, flags);  // (the same sums once more, for the flags of the plane that was kept)
    const double sign = plane_output(cur, cur + 3, has_axis, unit, r.plane);
    for (int i = 0; i < 3; i++) r.normal[i] = sign < 0.0 ? -cur[i] : cur[i], r.anchor[i] = cur[3 + i];
    r.inliers = (int64_t)kept[kPlCount];
    r.fitness = kept[kPlCount] / (double)c;
    r.inlier_rmse = kept[kPlCount] > 0 ? std::sqrt(kept[kPlSumD2] / kept[kPlCount]) : 0.0;
    if (o.d_inlier_mask) OWLMI_HIP(hipMemcpyAsync(o.d_inlier_mask, flags, (size_t)n, hipMemcpyDeviceToDevice, s));
    if (o.d_inlier_rows) {
      OWLMI_HIP(hipMemsetAsync(o.d_inlier_rows, 0xff, (size_t)n * sizeof(int32_t), s));
      OWLMI_HIP(hipcub::DeviceSelect::Flagged(cub_tmp, b2, hipcub::CountingInputIterator<int32_t>(0), flags, o.d_inlier_rows, (int32_t *)(counters + kPsSelected), n, s));
    }
  } else {
    if (o.d_inlier_mask) OWLMI_HIP(hipMemsetAsync(o.d_inlier_mask, 0, (size_t)n, s));
    if (o.d_inlier_rows) OWLMI_HIP(hipMemsetAsync(o.d_inlier_rows, 0xff, (size_t)n * sizeof(int32_t), s));
  }
  OWLMI_HIP(hipEventRecord(ev_f_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  OWLMI_HIP(hipEventElapsedTime(&r.refit_ms, ev_e_, ev_f_));
  OWLMI_HIP(hipEventElapsedTime(&r.solve_ms, ev_a_, ev_f_));
  *info = r;
}

}  // namespace owlmi
