// icp.hip -- rigid registration of a cloud to the built set by iterated closest points (tknnIcp, include/owlknn_icp.h).
//
// The loop a user writes in torch around tknnKnn -- transform, search, gather, a dozen small reductions, a solve -- inside the
// engine: the pairs never leave the call's workspace and the sums are fp64.  One iteration:
//   1. icp_transform_kernel: s' = Tf s with the header's literal fp32 arithmetic, into the workspace;
//   2. the search of tknnKnn at k = 1 on s' -- query_order, rknn_slots, the seed pass (rknn_seed_kernel with the hooks below),
//      radius_knn_walks -- with one kernel between seed and walk: icp_clip_kernel takes min(seed bound, max_dist) per row, so the
//      walk's radius is the k = 1 bound wherever that is the smaller one and a large max_dist costs nothing (it can also take the
//      literal distance to the row's previous partner, an exact upper bound as well: measured, not adopted).  From the second
//      search on the first search's curve order is kept: the points have moved a little, the order is as good;
//   3. icp_moment_kernel<METHOD>: a grid-stride pass over j that gathers the partner (and its normal) by row and sums the pair's
//      contribution in double, the coordinates relative to the centre of the tree's scene box; per lane, per wave with shuffles,
//      per workgroup through LDS in wave order: one row of kIcpMoments doubles per workgroup.  icp_moment_sum_kernel, one
//      workgroup, adds the rows in index order.  No floating-point atomic anywhere: with the grid fixed by (m, the device) the
//      moments are bitwise reproducible;
//   4. the host reads those kIcpMoments doubles -- the iteration's one synchronisation besides the walk's redo count -- and
//      icp_solve.h makes the step.
// The call's workspace (Engine::workspace, one layout, RknnWorkspace's columns of m words):
//      counters | lane list, radii, codes (later: slots), sorted codes, order in, order | s' (three columns) | partner rows |
//      partner distances | the sort's temporary | moment rows, one per workgroup + the total
#include "owlknn_icp.h"
#include "curve_key.h"
#include "icp_solve.h"
#include "query_order.h"
#include "radius_knn_walk.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kIcpFlatBlock = 256;
constexpr int kIcpMomentBlock = 256;      // four waves
constexpr int kIcpMomentBlocksPerCu = 4;  // the grid: min(ceil(m / 256), 4 per compute unit)
static_assert(kCounterWords >= kRknnWsWords + kIcpMoments, "the host's copy of the counters holds a walk's words and a moment row");

struct IcpRows {
  float r[12];  // the top three rows of T in fp32
};

// ---- 1. s' = Tf s ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kIcpFlatBlock) icp_transform_kernel(const float *__restrict__ src, int32_t m, IcpRows t, float *__restrict__ out) {
#pragma clang fp contract(off)
  const int32_t j = blockIdx.x * kIcpFlatBlock + threadIdx.x;
  if (j >= m) return;
  const float x = src[3 * (int64_t)j], y = src[3 * (int64_t)j + 1], z = src[3 * (int64_t)j + 2];
  out[3 * (int64_t)j] = ((t.r[0] * x + t.r[1] * y) + t.r[2] * z) + t.r[3];
  out[3 * (int64_t)j + 1] = ((t.r[4] * x + t.r[5] * y) + t.r[6] * z) + t.r[7];
  out[3 * (int64_t)j + 2] = ((t.r[8] * x + t.r[9] * y) + t.r[10] * z) + t.r[11];
}

// ---- 2. the seed hooks: KnnSeedRule<false> of knn_seed.hip without a skipped point ----------------------------------------------------
struct IcpSeedArgs {
  LbvhView bvh;
  const float *queries;   // s', m packed triples
  const uint32_t *order;  // the query worked on at sorted position i
  const int32_t *slots;   // its place in the tree's order, by sorted position
  int32_t m;
  int k;                  // 1
  float *radii;           // out: the seed bound, by j
  unsigned long long *ws;
};

struct IcpSeedRule {
  using Args = IcpSeedArgs;
  struct Query {
    LbvhPoint q;
    int32_t skip;
  };
  static __device__ __forceinline__ int32_t item_at(const Args &a, int32_t pos) { return (int32_t)a.order[pos]; }
  static __device__ __forceinline__ void point(const Args &a, int32_t item, bool has_q, Query &s) {
    s.q = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
    s.skip = -1;
    if (!has_q) return;
    s.q.x = a.queries[3 * (int64_t)item], s.q.y = a.queries[3 * (int64_t)item + 1], s.q.z = a.queries[3 * (int64_t)item + 2];
  }
  static __device__ __forceinline__ float dist2(const Args &, const Query &s, const LbvhPoint &p) { return knn_dist2(p.x, p.y, p.z, s.q.x, s.q.y, s.q.z); }
  static __device__ __forceinline__ bool slot_ok(const Query &, int32_t) { return true; }
  static __device__ __forceinline__ void seed_range(const Args &a, const Query &, int32_t pos, bool has_q, int32_t clean_blocks, int32_t &blk_lo,
                                                    int32_t &blk_hi, int32_t &slot) {
    blk_lo = 0, blk_hi = clean_blocks;
    slot = min(has_q ? a.slots[pos] : 0, a.bvh.n - 1);
  }
  static __device__ __forceinline__ void seed_store(const Args &a, const Query &, int32_t item, float bound) { a.radii[item] = bound; }
};

// The walk's radius of row j: the seed bound, max_dist, and (prev given) the literal distance from s'_j to the partner the row had
// in the previous search -- each an upper bound of the distance of the partner the row can have, so their minimum is one.
__global__ void __launch_bounds__(kIcpFlatBlock) icp_clip_kernel(float *__restrict__ radii, int32_t m, float max_dist, const int32_t *__restrict__ prev,
                                                                const float *__restrict__ aligned, const LbvhPoint *__restrict__ points,
                                                                const int32_t *__restrict__ row_slot) {
  const int32_t j = blockIdx.x * kIcpFlatBlock + threadIdx.x;
  if (j >= m) return;
  float r = fminf(radii[j], max_dist);
  if (prev) {
    const int32_t c = prev[j];
    if (c >= 0) {
      const LbvhPoint p = points[row_slot[c]];
      const float d = knn_sqrt(knn_dist2(p.x, p.y, p.z, aligned[3 * (int64_t)j], aligned[3 * (int64_t)j + 1], aligned[3 * (int64_t)j + 2]));
      if (d <= FLT_MAX) r = fminf(r, d);  // (a NaN: no bound)
    }
  }
  radii[j] = r;
}

// ---- 3. the moments ----------------------------------------------------------------------------------------------------------------
struct IcpMomentArgs {
  const float *aligned;       // s', m x 3
  const int32_t *corr;        // c(j), m
  const LbvhPoint *points;    // the tree's sorted points
  const int32_t *row_slot;    // the sorted slot of a caller's row
  const float *normals;       // n x 3 by row (point-to-plane)
  int32_t m;
  int robust;
  double scale;               // robust_scale
  double centre[3];
  double *rows;               // gridDim.x rows of kIcpMoments doubles, then the total
};

__device__ __forceinline__ double icp_weight(int robust, double e, double c) {
  if (robust == TKNN_ICP_HUBER) return e <= c ? 1.0 : c / e;
  if (robust == TKNN_ICP_TUKEY) {
    const double u = e / c, v = 1.0 - u * u;
    return e <= c ? v * v : 0.0;
  }
  return 1.0;
}

__device__ __forceinline__ double icp_wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int METHOD>
__global__ void __launch_bounds__(kIcpMomentBlock) icp_moment_kernel(IcpMomentArgs a) {
  constexpr int NM = METHOD == TKNN_ICP_POINT_TO_PLANE ? kIcpPlaneWords : kIcpPointWords;
  __shared__ double part[kIcpMomentBlock / 64][kIcpMoments];
  double acc[NM];
#pragma unroll
  for (int i = 0; i < NM; i++) acc[i] = 0.0;
  const double cx = a.centre[0], cy = a.centre[1], cz = a.centre[2];
  for (int64_t j = (int64_t)blockIdx.x * kIcpMomentBlock + threadIdx.x; j < (int64_t)a.m; j += (int64_t)gridDim.x * kIcpMomentBlock) {
    const int32_t c = a.corr[j];
    if (c < 0) continue;
    const LbvhPoint p = a.points[a.row_slot[c]];
    const double sx = (double)a.aligned[3 * j], sy = (double)a.aligned[3 * j + 1], sz = (double)a.aligned[3 * j + 2];
    const double dx = sx - (double)p.x, dy = sy - (double)p.y, dz = sz - (double)p.z;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    acc[kIcpPairs] += 1.0;
    acc[kIcpSumD2] += d2;
    const double ax = sx - cx, ay = sy - cy, az = sz - cz;
    if (METHOD == TKNN_ICP_POINT_TO_POINT) {
      const double bx = (double)p.x - cx, by = (double)p.y - cy, bz = (double)p.z - cz;
      const double w = icp_weight(a.robust, sqrt(d2), a.scale);
      if (w > 0.0) acc[kIcpPositive] += 1.0;
      acc[4] += w;
      const double wa[3] = {w * ax, w * ay, w * az}, b[3] = {bx, by, bz};
#pragma unroll
      for (int i = 0; i < 3; i++) {
        acc[5 + i] += wa[i];
        acc[8 + i] += w * b[i];
#pragma unroll
        for (int t = 0; t < 3; t++) acc[11 + 3 * i + t] += wa[i] * b[t];
      }
    } else {
      const double nx = (double)a.normals[3 * (int64_t)c], ny = (double)a.normals[3 * (int64_t)c + 1], nz = (double)a.normals[3 * (int64_t)c + 2];
      if (!(fabs(nx) <= DBL_MAX && fabs(ny) <= DBL_MAX && fabs(nz) <= DBL_MAX)) {
        acc[kIcpSkipped] += 1.0;
        continue;
      }
      const double r = (dx * nx + dy * ny) + dz * nz;
      const double w = icp_weight(a.robust, fabs(r), a.scale);
      if (w > 0.0) acc[kIcpPositive] += 1.0;
      const double J[6] = {ay * nz - az * ny, az * nx - ax * nz, ax * ny - ay * nx, nx, ny, nz};
      int at = kIcpSystem;
#pragma unroll
      for (int i = 0; i < 6; i++) {
        const double wj = w * J[i];
#pragma unroll
        for (int t = i; t < 6; t++) acc[at++] += wj * J[t];
        acc[kIcpPlaneRhs + i] += wj * r;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NM; i++) {
    const double v = icp_wave_sum(acc[i]);
    if (lane == 0) part[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kIcpMoments) {
    double v = 0.0;
    if ((int)threadIdx.x < NM)
      for (int w = 0; w < kIcpMomentBlock / 64; w++) v += part[w][threadIdx.x];
    a.rows[(int64_t)blockIdx.x * kIcpMoments + threadIdx.x] = v;
  }
}

// rows[nrows] = the sum of rows[0 .. nrows), in index order
__global__ void __launch_bounds__(64) icp_moment_sum_kernel(double *rows, int32_t nrows) {
  if (threadIdx.x >= kIcpMoments) return;
  double v = 0.0;
  for (int32_t b = 0; b < nrows; b++) v += rows[(int64_t)b * kIcpMoments + threadIdx.x];
  rows[(int64_t)nrows * kIcpMoments + threadIdx.x] = v;
}

bool env_flag(const char *name, bool otherwise) {
  const char *e = getenv(name);
  return e ? atoi(e) != 0 : otherwise;
}

}  // namespace

void Engine::icp(const tknnIcpOptions &o, tknnIcpInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const bool plane = o.method == TKNN_ICP_POINT_TO_PLANE;
  // the two measured choices, read per call so that the measurement can be repeated: the first search's curve order
  // kept for the later ones (adopted: 4 - 6 % per iteration), and the previous partner's distance as a bound from the second
  // search on (not adopted: the seed bound is as tight already, the extra gather costs 0.5 % at 1 M).  Neither changes a result.
  const bool prev_bound = env_flag("TKNN_ICP_PREV_BOUND", false), reuse_order = env_flag("TKNN_ICP_REUSE_ORDER", true);
  const int moment_blocks = (int)std::min<int64_t>((m + kIcpMomentBlock - 1) / kIcpMomentBlock, (int64_t)cu_count_ * kIcpMomentBlocksPerCu);
  const size_t sort_bytes = query_order_sort_bytes(m, s), sort_b = RknnWorkspace::align(sort_bytes);
  const size_t moment_bytes = (size_t)(moment_blocks + 1) * kIcpMoments * sizeof(double);
  RknnWorkspace w(m, 11, sort_b + moment_bytes);
  w.base = (char *)workspace(w.bytes);
  float *radii = w.column<float>(1);
  uint32_t *codes = w.column<uint32_t>(2), *codes_alt = w.column<uint32_t>(3), *order_in = w.column<uint32_t>(4), *order = w.column<uint32_t>(5);
  int32_t *slots = w.column<int32_t>(2);  // (over the codes: the sort is through when the slots are written)
  float *aligned = w.column<float>(6);    // three columns
  int32_t *corr = w.column<int32_t>(9);
  float *corr_dist = w.column<float>(10);
  double *rows = (double *)(w.column<char>(11) + sort_b);

  const LbvhView tv = bvh_.view();
  IcpSeedArgs sa;
  std::memset(&sa, 0, sizeof sa);
  sa.bvh = tv;
  sa.queries = aligned;
  sa.order = order;
  sa.slots = slots;
  sa.m = (int32_t)m;
  sa.k = 1;
  sa.radii = radii;
  sa.ws = w.words();

  RadiusKnnKernelArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = tv;
  a.wide = bvh_.wide_view();
  a.queries = aligned;
  a.order = order;
  a.m = (int32_t)m;
  a.k = 1;
  a.radii = radii;
  a.force_redo = env_flag("TKNN_ICP_FORCE_FALLBACK", false);
  a.zero_radius_ok = 1;
  a.out_idx = corr;
  a.out_dist = corr_dist;
  a.redo = w.column<int32_t>(0);
  a.ws = w.words();

  IcpMomentArgs ma;
  std::memset(&ma, 0, sizeof ma);
  ma.aligned = aligned;
  ma.corr = corr;
  ma.points = tv.points;
  ma.row_slot = bvh_.row_slot_device();
  ma.normals = o.d_target_normals;
  ma.m = (int32_t)m;
  ma.robust = o.robust;
  ma.scale = (double)o.robust_scale;
  for (int i = 0; i < 3; i++) ma.centre[i] = 0.5 * ((double)scene_[i] + (double)scene_[3 + i]);
  ma.rows = rows;

  double T[16];
  if (o.init)
    std::memcpy(T, o.init, sizeof T);
  else
    icp_identity(T);
  const unsigned flat_blocks = (unsigned)((m + kIcpFlatBlock - 1) / kIcpFlatBlock);
  const double *h_mom = (const double *)(h_counters_ + kRknnWsWords);
  tknnIcpInfo r;
  std::memset(&r, 0, sizeof r);
  double prev_fitness = 0, prev_rmse = 0;
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  for (int pass = 0;; pass++) {
    // ---- the search at T ----
    IcpRows tf;
    icp_round_rows(T, tf.r);
    OWLMI_HIP(hipEventRecord(ev_a_, s));
    OWLMI_HIP(hipMemsetAsync(a.ws, 0, kRknnWsWords * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(icp_transform_kernel, dim3(flat_blocks), dim3(kIcpFlatBlock), 0, s, o.d_source, (int32_t)m, tf, aligned);
    OWLMI_HIP(hipGetLastError());
    if (pass == 0 || !reuse_order) query_order(aligned, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, w.column<void>(11), sort_bytes, s);
    rknn_slots(aligned, order, (int32_t)m, bvh_.scene_device(), bvh_.curve(), bvh_.keys_device(), tv.n, slots, s);
    rknn_seed<IcpSeedRule>(sa, cu_count_, s);
    hipLaunchKernelGGL(icp_clip_kernel, dim3(flat_blocks), dim3(kIcpFlatBlock), 0, s, radii, (int32_t)m, o.max_dist,
                       pass > 0 && prev_bound ? (const int32_t *)corr : nullptr, (const float *)aligned, tv.points, ma.row_slot);
    OWLMI_HIP(hipGetLastError());
    const unsigned long long n_redo = radius_knn_walks(a, cu_count_, h_counters_, s);
    OWLMI_HIP(hipEventRecord(ev_b_, s));
    // ---- the moments of its pairs ----
    if (plane)
      hipLaunchKernelGGL(icp_moment_kernel<TKNN_ICP_POINT_TO_PLANE>, dim3(moment_blocks), dim3(kIcpMomentBlock), 0, s, ma);
    else
      hipLaunchKernelGGL(icp_moment_kernel<TKNN_ICP_POINT_TO_POINT>, dim3(moment_blocks), dim3(kIcpMomentBlock), 0, s, ma);
    OWLMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(icp_moment_sum_kernel, dim3(1), dim3(64), 0, s, rows, (int32_t)moment_blocks);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipMemcpyAsync((void *)h_mom, rows + (size_t)moment_blocks * kIcpMoments, kIcpMoments * sizeof(double), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipEventRecord(ev_c_, s));
    OWLMI_HIP(hipStreamSynchronize(s));  // the iteration's moments (and the walk's counters as the lane kernel left them)
    float search_ms = 0, moment_ms = 0;
    OWLMI_HIP(hipEventElapsedTime(&search_ms, ev_a_, ev_b_));
    OWLMI_HIP(hipEventElapsedTime(&moment_ms, ev_b_, ev_c_));
    r.search_ms += search_ms, r.moment_ms += moment_ms;
    r.searches++;
    r.node_tests += (int64_t)h_counters_[kRknnWsNodeTests], r.point_tests += (int64_t)h_counters_[kRknnWsPointTests], r.lane_rows += (int64_t)n_redo;
    const double pairs = h_mom[kIcpPairs];
    r.correspondences = (int64_t)pairs;
    r.skipped_pairs = (int64_t)h_mom[kIcpSkipped];
    r.fitness = pairs / (double)m;
    r.inlier_rmse = pairs > 0 ? std::sqrt(h_mom[kIcpSumD2] / pairs) : 0.0;
    // ---- stop, or step ----
    if (pass > 0 && std::fabs(r.fitness - prev_fitness) < o.rel_fitness && std::fabs(r.inlier_rmse - prev_rmse) < o.rel_rmse) {
      r.converged = 1;
      break;
    }
    if (r.iterations == o.max_iterations) break;
    double dT[16], next[16];
    if (!(plane ? icp_solve_plane(h_mom, ma.centre, dT) : icp_solve_point(h_mom, ma.centre, dT))) {
      r.degenerate = 1;
      break;
    }
    icp_mul(dT, T, next);
    std::memcpy(T, next, sizeof T);
    r.iterations++;
    prev_fitness = r.fitness, prev_rmse = r.inlier_rmse;
  }
  if (o.d_corr) OWLMI_HIP(hipMemcpyAsync(o.d_corr, corr, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (o.d_corr_dist) OWLMI_HIP(hipMemcpyAsync(o.d_corr_dist, corr_dist, (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (o.d_aligned) OWLMI_HIP(hipMemcpyAsync(o.d_aligned, aligned, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  OWLMI_HIP(hipEventRecord(ev_e_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  OWLMI_HIP(hipEventElapsedTime(&r.solve_ms, ev_d_, ev_e_));
  std::memcpy(r.transform, T, sizeof T);
  *info = r;
}

}  // namespace owlmi
