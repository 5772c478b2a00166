// local_pca.hip -- the covariance of each query's neighbourhood, its eigenvalues, normal and surface variation, without the lists
// (tknnLocalPca, include/owlknn_pca.h).
//
// Row j sums, over the points p of its neighbourhood N_j, 1, the offset d = p - q_j and the six products of d: ten words.  The
// offsets are bounded by the neighbourhood's radius, so the covariance S2 / len - mean mean^T is a difference of numbers of the
// size r^2, never |p|^2; nothing is staged.  N_j is a radius row, a kNN row or their intersection (the header):
//   1. the bound (only with k): Engine::knn inside, its rows in DeviceBuffers (the inner call takes the workspace);
//      pca_bound_kernel turns each row into (R_j, last_j), the distance and the name of its last entry, R_j clipped to the radius
//      where one is given and smaller -- the name rule is then off for the row: every point within the radius is in it.  N_j is
//      "the own slot if it is in, plus every other point with (d, name) <= (R_j, last_j) lexicographically": the kNN row is never
//      gathered, no id is mapped back to a slot.  Without k: R_j = radius, the name rule off.
//   2. query_order (query_order.h): external queries along the tree's own curve; the own points in sorted-slot order.
//   3. rad_walks (radius_walk.h: the walk, the box rule, the lane kernel for what the walk left) with PcaRule: one bound R_j per
//      query; a lane adds, under the predicate, 1, d and the six products into its OWN ten registers.  A child box above the leaf
//      level wholly inside the sphere (radius_inside2(R_j)) holds only points strictly nearer than R_j -- the name rule cannot apply
//      to it --: its slots are streamed.  One DPP reduction per row; the team's lane 0 writes the row's ten words into the
//      workspace and does NOT solve it (fifteen idle lanes per eigen-solve otherwise).
//   4. pca_finish_kernel: flat, one row per lane: centroid, covariance, the eigen-solver (pca_eig3, the one place it exists), the
//      normal's sign, the curvature, the degenerate rows; only the outputs asked for, no solve where none of them needs one.
// The call's workspace (Engine::workspace, one layout):
//      counters (kRadWords) | codes, sorted codes, order in, order (m + 1 each; external queries only) | redo list, m |
//      moments, 10 columns of m words (external: by query, own points: by sorted slot) | the sort's temporary
#include "owlknn_pca.h"
#include "linkage.h"  // DeviceBuffer
#include "query_order.h"
#include "radius_walk.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kPcaFlatBlock = 256;
constexpr int kPcaMoments = 10;  // count, S1 (x y z), S2 (xx xy xz yy yz zz)
constexpr int kPcaSweeps = 6;    // cyclic Jacobi sweeps of the 3 x 3 solve

struct PcaArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const float *queries;   // m packed triples, caller order; null: the set's own points, position i = sorted slot i
  const uint32_t *order;  // external queries: the query worked on at sorted position i
  int32_t m;
  float radius;           // without bounds: every row's R_j
  const float *bound_r;   // by row: R_j, < 0 for a row that no other point enters (null: radius, the name rule off)
  const uint32_t *bound_last;  // by row: the largest name admitted at distance exactly R_j (0xffffffff: the name rule is off)
  int by_name;            // own points with k: the other points are told from the query by name, as tknnKnn tells them
  int self_in;            // ... and the query's own slot is a neighbour
  int skip_self;          // own points with a radius only: the query's slot is left out
  int force_redo;         // TKNN_PCA_FORCE_FALLBACK (tests): the walk leaves every query to the lane kernel
  int min_points;
  int orient;
  int solve;              // some output needs the eigen-solver
  float view[3];
  uint32_t *moments;      // kPcaMoments columns of m words
  int32_t *counts;        // the caller's outputs, any may be null
  float *centroid, *cov, *eigenvalues, *eigenvectors, *normals, *curvature;
  int32_t *redo;          // m: positions left to the lane kernel
  unsigned long long *ws; // kRadWords counters
};

// the query at position `pos` and how its neighbourhood is told
struct PcaQuery {
  LbvhPoint q;
  int32_t row;        // where the caller's results go
  int32_t at;         // where the moments go
  int32_t self;       // the query's own slot where it is treated apart (-1: no slot is)
  int32_t skip_name;  // the name no other neighbour may have (-1: none)
  float r;            // R_j
  float r_wide;       // max(R_j, 0) (1 + 1e-6): the query's box still holds the query
  float in2;          // radius_inside2(R_j) (-1: no box is inside)
  uint32_t last;
};
__device__ __forceinline__ PcaQuery pca_query(const PcaArgs &a, int32_t pos, bool has_q) {
  PcaQuery s;
  const int32_t slot = rad_point(a, pos, has_q, s.q, s.row);
  s.at = a.queries ? s.row : slot;
  s.self = has_q && (a.skip_self || a.by_name) ? slot : -1;
  s.skip_name = has_q && a.by_name ? s.q.id : -1;
  s.q.id = -1;
  s.r = a.bound_r ? a.bound_r[s.row] : a.radius;
  s.last = a.bound_last ? a.bound_last[s.row] : 0xffffffffu;
  s.r_wide = fmaxf(s.r, 0.f) * 1.000001f;
  s.in2 = s.r > 0.f ? radius_inside2(s.r) : -1.f;
  return s;
}

// Is the point p at sorted slot `slot`, at offset (dx, dy, dz) from the query, in N_j?  d: the literal fp32 distance.  A NaN on
// either side fails every compare.
__device__ __forceinline__ bool pca_member(const PcaArgs &a, const PcaQuery &s, int32_t slot, const LbvhPoint &p, float d) {
  if (slot == s.self) return a.self_in && d <= FLT_MAX;
  return p.id != s.skip_name && (d < s.r || (d == s.r && (uint32_t)p.id <= s.last));
}

// a neighbour's share of the row's nine float sums
__device__ __forceinline__ void pca_add(float (&acc)[9], float dx, float dy, float dz) {
#pragma clang fp contract(off)
  acc[0] += dx, acc[1] += dy, acc[2] += dz;
  acc[3] += dx * dx, acc[4] += dx * dy, acc[5] += dx * dz;
  acc[6] += dy * dy, acc[7] += dy * dz, acc[8] += dz * dz;
}

// one summed row, by the one lane that holds it
__device__ __forceinline__ void pca_store(const PcaArgs &a, int32_t at, uint32_t cnt, const float (&acc)[9]) {
  a.moments[at] = cnt;
#pragma unroll
  for (int c = 0; c < 9; c++) a.moments[(int64_t)(c + 1) * a.m + at] = __float_as_uint(acc[c]);
}

// ---- 1. the bound --------------------------------------------------------------------------------------------------------------------
// Row j of a kNN call with rows of kk: (R_j, last_j) = its last entry's distance and name; an empty row: R_j = -1, nothing passes.
__global__ void __launch_bounds__(kPcaFlatBlock) pca_bound_kernel(const int32_t *idx, const float *dist, const int32_t *counts, int32_t kk, int32_t m,
                                                                  float radius, float *bound_r, uint32_t *bound_last) {
  const int64_t j = (int64_t)blockIdx.x * kPcaFlatBlock + threadIdx.x;
  if (j >= m) return;
  const int32_t cnt = min(counts[j], kk);
  float r = -1.f;
  uint32_t last = 0u;
  if (cnt > 0) {
    r = dist[j * kk + cnt - 1];
    last = (uint32_t)idx[j * kk + cnt - 1];
    if (radius > 0.f && radius < r) r = radius, last = 0xffffffffu;  // the row reaches past the radius: all within it are in the row
  }
  bound_r[j] = r;
  bound_last[j] = last;
}

// ---- 3. the rule ---------------------------------------------------------------------------------------------------------------------
struct PcaRule {
  using Args = PcaArgs;
  using Query = PcaQuery;
  static constexpr bool kArith = false, kRolled = true;
  static constexpr int kTeamLds = 0;
  struct Lane {
    float acc[9];  // my lane's share of S1 and S2
  };
  static __device__ __forceinline__ Query query(const Args &a, int32_t pos, bool has_q) { return pca_query(a, pos, has_q); }
  static __device__ __forceinline__ void start(Lane &st, unsigned long long *) {
#pragma unroll
    for (int c = 0; c < 9; c++) st.acc[c] = 0.f;
  }
  static __device__ __forceinline__ bool member(const Args &a, const Query &s, int32_t slot, const LbvhPoint &p, float d) { return pca_member(a, s, slot, p, d); }
  static __device__ __forceinline__ void lane_take(const Args &, const Query &, Lane &st, uint32_t, int64_t, const LbvhPoint &, float dx, float dy, float dz, float,
                                                   float) {
    pca_add(st.acc, dx, dy, dz);
  }
  static __device__ __forceinline__ void take(const Args &, const Query &, Lane &st, uint32_t &part, bool hit, int64_t, const LbvhPoint &, float dx, float dy,
                                              float dz, float, float, int, int) {
    part = t_count(part, __ballot(hit));
    if (hit) pca_add(st.acc, dx, dy, dz);
  }
  static __device__ __forceinline__ uint32_t row_end(const Args &, const Query &, Lane &st, uint32_t part, int, int) {
#pragma unroll
    for (int c = 0; c < 9; c++) st.acc[c] = t_team_sum(st.acc[c]);
    return t_team_sum(part);
  }
  static __device__ __forceinline__ unsigned long long row_write(const Args &a, const Query &s, const Lane &st, uint32_t cnt) {
    pca_store(a, s.at, cnt, st.acc);
    return cnt < (uint32_t)a.min_points ? 1u : 0u;  // a degenerate row
  }
  static __device__ __forceinline__ bool lane_arith(const Args &) { return false; }
};

// ---- 4. the finish -------------------------------------------------------------------------------------------------------------------
// One Jacobi rotation of the pair (p, q) of a symmetric 3 x 3, r the third index: app, aqq, apq the pair's entries, arp, arq the
// third row's; the columns p and q of V turn with it.  Every operation fp32 and rounded on its own (tests/pca_spec.py jacobi32
// restates it operation for operation).
__device__ __forceinline__ void pca_rotate(float &app, float &aqq, float &apq, float &arp, float &arq, float &v0p, float &v0q, float &v1p, float &v1q, float &v2p,
                                           float &v2q) {
#pragma clang fp contract(off)
  if (apq == 0.f) return;
  const float theta = (aqq - app) / (2.f * apq);
  const float root = __builtin_sqrtf(theta * theta + 1.f);
  const float t = (theta >= 0.f ? 1.f : -1.f) / (fabsf(theta) + root);
  const float c = 1.f / __builtin_sqrtf(t * t + 1.f), sn = t * c;
  const float h = t * apq;
  app = app - h, aqq = aqq + h, apq = 0.f;
  const float rp = c * arp - sn * arq, rq = sn * arp + c * arq;
  arp = rp, arq = rq;
  const float x0 = c * v0p - sn * v0q, y0 = sn * v0p + c * v0q;
  const float x1 = c * v1p - sn * v1q, y1 = sn * v1p + c * v1q;
  const float x2 = c * v2p - sn * v2q, y2 = sn * v2p + c * v2q;
  v0p = x0, v0q = y0, v1p = x1, v1q = y1, v2p = x2, v2q = y2;
}

// Eigenvalues (ascending) and eigenvectors (row i of vec belongs to lam[i]) of the symmetric 3 x 3 with the entries xx, xy, xz,
// yy, yz, zz: scaled by the largest |entry|, kPcaSweeps cyclic Jacobi sweeps over (0,1), (0,2), (1,2), a three-element sort.
// A matrix of zeros (or one that is not finite at its largest entry) gives lam = 0 and the unit vectors.
__device__ __forceinline__ void pca_eig3(const float (&cv)[6], float (&lam)[3], float (&vec)[9]) {
#pragma clang fp contract(off)
  float scale = 0.f;
#pragma unroll
  for (int i = 0; i < 6; i++) scale = fmaxf(scale, fabsf(cv[i]));
  float a00 = 0.f, a01 = 0.f, a02 = 0.f, a11 = 0.f, a12 = 0.f, a22 = 0.f;
  if (scale > 0.f && scale <= FLT_MAX) {
    const float inv = 1.f / scale;
    a00 = cv[0] * inv, a01 = cv[1] * inv, a02 = cv[2] * inv, a11 = cv[3] * inv, a12 = cv[4] * inv, a22 = cv[5] * inv;
  } else {
    scale = 0.f;
  }
  float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;  // v[r][c]: component r of column c
#pragma unroll 1
  for (int sweep = 0; sweep < kPcaSweeps; sweep++) {
    pca_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    pca_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    pca_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  float l0 = a00 * scale, l1 = a11 * scale, l2 = a22 * scale;
  // column c of V is the eigenvector of l_c; sorted ascending by three compare-and-swaps (0,1), (1,2), (0,1)
  auto order = [](float &la, float &lb, float &xa, float &xb, float &ya, float &yb, float &za, float &zb) __attribute__((always_inline)) {
    if (lb < la) {
      float t = la; la = lb, lb = t;
      t = xa, xa = xb, xb = t;
      t = ya, ya = yb, yb = t;
      t = za, za = zb, zb = t;
    }
  };
  order(l0, l1, v00, v01, v10, v11, v20, v21);
  order(l1, l2, v01, v02, v11, v12, v21, v22);
  order(l0, l1, v00, v01, v10, v11, v20, v21);
  lam[0] = l0, lam[1] = l1, lam[2] = l2;
  vec[0] = v00, vec[1] = v10, vec[2] = v20;
  vec[3] = v01, vec[4] = v11, vec[5] = v21;
  vec[6] = v02, vec[7] = v12, vec[8] = v22;
}

__global__ void __launch_bounds__(kPcaFlatBlock) pca_finish_kernel(PcaArgs a) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * kPcaFlatBlock + threadIdx.x;
  if (t >= (int64_t)a.m) return;
  // external queries: lane t is query t; own points: sorted slot t, the results go to its row
  int64_t row = t;
  float qx, qy, qz;
  if (a.queries) {
    qx = a.queries[3 * t], qy = a.queries[3 * t + 1], qz = a.queries[3 * t + 2];
  } else {
    const LbvhPoint p = a.bvh.points[t];
    qx = p.x, qy = p.y, qz = p.z;
    row = a.bvh.prim_id[t];
  }
  const uint32_t cnt = a.moments[t];
  float mom[9];
#pragma unroll
  for (int c = 0; c < 9; c++) mom[c] = __uint_as_float(a.moments[(int64_t)(c + 1) * a.m + t]);
  if (a.counts) a.counts[row] = (int32_t)cnt;
  float mean[3] = {0.f, 0.f, 0.f}, cen[3] = {0.f, 0.f, 0.f}, cv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (cnt > 0u) {
    const float len = (float)cnt;
    mean[0] = mom[0] / len, mean[1] = mom[1] / len, mean[2] = mom[2] / len;
    cen[0] = qx + mean[0], cen[1] = qy + mean[1], cen[2] = qz + mean[2];
    cv[0] = mom[3] / len - mean[0] * mean[0], cv[1] = mom[4] / len - mean[0] * mean[1], cv[2] = mom[5] / len - mean[0] * mean[2];
    cv[3] = mom[6] / len - mean[1] * mean[1], cv[4] = mom[7] / len - mean[1] * mean[2], cv[5] = mom[8] / len - mean[2] * mean[2];
  }
  if (a.centroid) a.centroid[3 * row] = cen[0], a.centroid[3 * row + 1] = cen[1], a.centroid[3 * row + 2] = cen[2];
  if (a.cov) {
#pragma unroll
    for (int c = 0; c < 6; c++) a.cov[6 * row + c] = cv[c];
  }
  if (!a.solve) return;
  float lam[3] = {0.f, 0.f, 0.f}, vec[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, curv = 0.f;
  if (cnt >= (uint32_t)a.min_points) {
    pca_eig3(cv, lam, vec);
    // the normal's sign
    bool flip;
    if (a.orient) {
      const float vx = a.view[0] - qx, vy = a.view[1] - qy, vz = a.view[2] - qz;
      const float sgn = (vec[0] * vx + vec[1] * vy) + vec[2] * vz;
      flip = sgn < 0.f;
    } else {
      float big = vec[0];
      if (fabsf(vec[1]) > fabsf(big)) big = vec[1];
      if (fabsf(vec[2]) > fabsf(big)) big = vec[2];
      flip = big < 0.f;
    }
    if (flip) vec[0] = -vec[0], vec[1] = -vec[1], vec[2] = -vec[2];
    const float sum = (lam[0] + lam[1]) + lam[2];
    curv = sum > 0.f ? fmaxf(lam[0], 0.f) / sum : 0.f;
  }
  if (a.eigenvalues) a.eigenvalues[3 * row] = lam[0], a.eigenvalues[3 * row + 1] = lam[1], a.eigenvalues[3 * row + 2] = lam[2];
  if (a.eigenvectors) {
#pragma unroll
    for (int c = 0; c < 9; c++) a.eigenvectors[9 * row + c] = vec[c];
  }
  if (a.normals) a.normals[3 * row] = vec[0], a.normals[3 * row + 1] = vec[1], a.normals[3 * row + 2] = vec[2];
  if (a.curvature) a.curvature[row] = curv;
}

}  // namespace

void Engine::local_pca(const tknnLocalPcaOptions &o, tknnLocalPcaInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const bool own = o.d_queries == nullptr;
  const bool skip = (o.flags & TKNN_PCA_SKIP_SELF) != 0;
  const bool with_k = o.k > 0;
  const unsigned flat_blocks = (unsigned)((m + kPcaFlatBlock - 1) / kPcaFlatBlock);

  OWLMI_HIP(hipEventRecord(ev_e_, s));
  // 1. the bound.  (The call inside takes the engine's workspace, so what must outlive it is allocated for the length of this call.)
  DeviceBuffer bound_r(with_k ? (size_t)m * sizeof(float) : 0), bound_last(with_k ? (size_t)m * sizeof(uint32_t) : 0);
  if (with_k) {
    const int kk = own && !skip ? o.k - 1 : o.k;  // the own points without skip: the point itself and its k - 1 nearest others
    DeviceBuffer idx((size_t)m * kk * sizeof(int32_t)), dist((size_t)m * kk * sizeof(float)), counts((size_t)m * sizeof(int32_t));
    tknnKnnOptions ko;
    std::memset(&ko, 0, sizeof ko);
    ko.d_queries = o.d_queries;
    ko.m = m, ko.k = kk;
    ko.d_idx = (int32_t *)idx.p, ko.d_dist = (float *)dist.p, ko.d_counts = (int32_t *)counts.p;
    tknnKnnInfo knn_info;
    std::memset(&knn_info, 0, sizeof knn_info);
    knn(ko, &knn_info, s);
    hipLaunchKernelGGL(pca_bound_kernel, dim3(flat_blocks), dim3(kPcaFlatBlock), 0, s, (const int32_t *)idx.p, (const float *)dist.p, (const int32_t *)counts.p,
                       (int32_t)kk, (int32_t)m, o.radius, (float *)bound_r.p, (uint32_t *)bound_last.p);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipStreamSynchronize(s));  // (the rows are freed here)
  }
  OWLMI_HIP(hipEventRecord(ev_f_, s));

  // the call's workspace (the layout: the file head)
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t order_bytes = own ? 0 : query_order_sort_bytes(m, s);
  const size_t words_b = align(kRadWords * sizeof(unsigned long long)), col_b = align(((size_t)m + 1) * sizeof(uint32_t)), order_cols = own ? 0 : 4 * col_b,
               mom_b = align((size_t)m * kPcaMoments * sizeof(uint32_t)), tmp_b = align(order_bytes);
  char *ws = (char *)workspace(words_b + order_cols + col_b + mom_b + tmp_b);
  uint32_t *codes = (uint32_t *)(ws + words_b), *codes_alt = (uint32_t *)(ws + words_b + col_b), *order_in = (uint32_t *)(ws + words_b + 2 * col_b),
           *order = (uint32_t *)(ws + words_b + 3 * col_b);
  void *tmp = ws + words_b + order_cols + col_b + mom_b;

  PcaArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.wide = bvh_.wide_view();
  a.queries = o.d_queries;
  a.order = own ? nullptr : order;
  a.m = (int32_t)m;
  a.radius = o.radius;
  a.bound_r = with_k ? (const float *)bound_r.p : nullptr;
  a.bound_last = with_k ? (const uint32_t *)bound_last.p : nullptr;
  a.by_name = own && with_k;
  a.self_in = own && with_k && !skip;
  a.skip_self = own && skip;
  if (const char *e = getenv("TKNN_PCA_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.min_points = o.min_points > 0 ? o.min_points : 3;
  a.orient = (o.flags & TKNN_PCA_ORIENT) != 0;
  a.solve = o.d_eigenvalues || o.d_eigenvectors || o.d_normals || o.d_curvature;
  a.view[0] = o.viewpoint[0], a.view[1] = o.viewpoint[1], a.view[2] = o.viewpoint[2];
  a.moments = (uint32_t *)(ws + words_b + order_cols + col_b);
  a.counts = o.d_counts;
  a.centroid = o.d_centroid, a.cov = o.d_cov, a.eigenvalues = o.d_eigenvalues, a.eigenvectors = o.d_eigenvectors, a.normals = o.d_normals;
  a.curvature = o.d_curvature;
  a.redo = (int32_t *)(ws + words_b + order_cols);
  a.ws = (unsigned long long *)ws;

  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kRadWords * sizeof(unsigned long long), s));
  if (!own) query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, tmp, order_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_g_, s));
  // the walk, then the lane kernel for what the walk left
  unsigned long long *h_words = h_counters_;
  rad_walks<PcaRule>(a, cu_count_, h_words, s);
  OWLMI_HIP(hipEventRecord(ev_h_, s));
  hipLaunchKernelGGL(pca_finish_kernel, dim3(flat_blocks), dim3(kPcaFlatBlock), 0, s, a);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->total = (int64_t)h_words[kRadTotal];
    info->max_row = (int64_t)h_words[kRadMaxRow];
    info->degenerate_rows = (int64_t)h_words[kRadOwn];
    info->fallback_items = (int64_t)h_words[kRadLaneRows];
    info->node_tests = (int64_t)h_words[kRadNodeTests];
    info->point_tests = (int64_t)h_words[kRadPointTests];
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_e_, ev_a_));
    if (with_k) OWLMI_HIP(hipEventElapsedTime(&info->bound_ms, ev_e_, ev_f_));
    if (!own) OWLMI_HIP(hipEventElapsedTime(&info->order_ms, ev_f_, ev_g_));
    OWLMI_HIP(hipEventElapsedTime(&info->walk_ms, ev_g_, ev_h_));
    OWLMI_HIP(hipEventElapsedTime(&info->finish_ms, ev_h_, ev_a_));
  }
}

}  // namespace owlmi
