// local_pca.hip -- the covariance of each query's neighbourhood, its eigenvalues, normal and surface variation, without the lists
// (tknnLocalPca, include/owlknn_pca.h).
//
// Row j sums, over the points p of its neighbourhood N_j, 1, the offset d = p - q_j and the six products of d: ten words.  The
// offsets are bounded by the neighbourhood's radius, so the covariance S2 / len - mean mean^T is a difference of numbers of the
// size r^2, never |p|^2; nothing is staged.  N_j is a radius row, a kNN row or their intersection (the header); the walk is
// reduce_walk_kernel's (radius_reduce.hip) with one bound per query:
//   1. the bound (only with k): Engine::knn inside, its rows in DeviceBuffers (the inner call takes the workspace);
//      pca_bound_kernel turns each row into (R_j, last_j), the distance and the name of its last entry, R_j clipped to the radius
//      where one is given and smaller -- the name rule is then off for the row: every point within the radius is in it.  N_j is
//      "the own slot if it is in, plus every other point with (d, name) <= (R_j, last_j) lexicographically": the kNN row is never
//      gathered, no id is mapped back to a slot.  Without k: R_j = radius, the name rule off.
//   2. query_order (query_order.h): external queries along the tree's own curve; the own points in sorted-slot order.
//   3. pca_walk_kernel: persistent, one 16-lane team per query, four teams per wave, walk_tree (team_walk.h) with the query's box
//      of half-width R_j (1 + 1e-6).  Lane tl tests point tl of a leaf block and, under the predicate, adds 1, d and the six
//      products into its OWN ten registers.  A child box above the leaf level wholly inside the sphere of 0.999995 R_j^2
//      (reduce_inside2's rule) holds only points strictly nearer than R_j -- the name rule cannot apply to it --: it is noted in
//      the team's range list and streamed after the walk without further box tests; a full list means the box is walked.  One
//      DPP reduction per row; the team's lane 0 writes the row's ten words into the workspace and does NOT solve it (fifteen idle
//      lanes per eigen-solve otherwise).  Stack overflows go to a redo list.
//   4. pca_lane_kernel: one query per lane on the rope walk (lane_walk.h), for the redo list and for trees too small for a
//      pyramid; the same ten words.
//   5. pca_finish_kernel: flat, one row per lane: centroid, covariance, the eigen-solver (pca_eig3, the one place it exists), the
//      normal's sign, the curvature, the degenerate rows; only the outputs asked for, no solve where none of them needs one.
// The call's workspace (Engine::workspace, one layout):
//      counters (kPcaWords) | codes, sorted codes, order in, order (m + 1 each; external queries only) | redo list, m |
//      moments, 10 columns of m words (external: by query, own points: by sorted slot) | the sort's temporary
#include "owlknn_pca.h"
#include "lane_walk.h"
#include "linkage.h"  // DeviceBuffer
#include "query_order.h"
#include "team_lanes.h"
#include "team_walk.h"
#include "trueknn_engine.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kPcaBlock = 64;        // one wave per workgroup, four teams
constexpr int kPcaBlocksPerCu = 16;  // 6.3 KB of LDS each
constexpr int kPcaLaneBlock = 256;
constexpr int kPcaFlatBlock = 256;
constexpr int kPcaRanges = 16;  // inside boxes above the leaf level a team notes for streaming; a 17th is walked
constexpr int kPcaMoments = 10;  // count, S1 (x y z), S2 (xx xy xz yy yz zz)
constexpr int kPcaSweeps = 6;    // cyclic Jacobi sweeps of the 3 x 3 solve

// words of the call's own counters (in the workspace, zeroed per call)
enum { kPcaCursor = 0, kPcaRedo = 1, kPcaTotal = 2, kPcaMaxRow = 3, kPcaFallback = 4, kPcaNodeTests = 5, kPcaPointTests = 6, kPcaDegenerate = 7, kPcaWords = 8 };

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
  unsigned long long *ws; // kPcaWords counters
};

__device__ __forceinline__ float pca_nan() { return __uint_as_float(0x7fc00000u); }

// R^2 * 0.999995 in double, rounded DOWN to fp32 (radius_query.hip's box rule, reduce_inside2)
__device__ __forceinline__ float pca_inside2(float r) {
  const double want = (double)r * (double)r * 0.999995;
  float f = (float)want;
  if ((double)f > want) f = __uint_as_float(__float_as_uint(f) - 1u);  // (f > 0 here: want > 0)
  return f;
}

// sum over the 16 lanes of my team (lane 0 of the team reads it; the order of the additions differs by lane)
__device__ __forceinline__ float pca_team_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128 /*row_ror:8*/, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124 /*row_ror:4*/, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122 /*row_ror:2*/, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121 /*row_ror:1*/, 0xf, 0xf, false));
  return v;
}

// the query at position `pos` and how its neighbourhood is told
struct PcaQuery {
  LbvhPoint q;
  int32_t row;        // where the caller's results go
  int32_t at;         // where the moments go
  int32_t self_slot;  // the query's own slot where it is treated apart (-1: no slot is)
  int32_t skip_name;  // the name no other neighbour may have (-1: none)
  float r;            // R_j
  float r_walk;       // max(R_j, 0): the query's box still holds the query
  uint32_t last;
};
__device__ __forceinline__ PcaQuery pca_query(const PcaArgs &a, int32_t pos, bool has_q) {
  PcaQuery s;
  s.self_slot = -1, s.skip_name = -1;
  if (a.queries) {
    s.row = has_q ? (int32_t)a.order[pos] : 0;
    s.at = s.row;
    s.q.x = a.queries[3 * (int64_t)s.row], s.q.y = a.queries[3 * (int64_t)s.row + 1], s.q.z = a.queries[3 * (int64_t)s.row + 2];
  } else {
    const int32_t slot = has_q ? pos : 0;
    s.q = a.bvh.points[slot];
    s.row = a.bvh.prim_id[slot];
    s.at = slot;
    if (has_q && (a.skip_self || a.by_name)) s.self_slot = slot;
    if (has_q && a.by_name) s.skip_name = s.q.id;
  }
  s.q.id = -1;
  s.r = a.bound_r ? a.bound_r[s.row] : a.radius;
  s.last = a.bound_last ? a.bound_last[s.row] : 0xffffffffu;
  s.r_walk = fmaxf(s.r, 0.f);
  return s;
}

// Is the point p at sorted slot `slot`, at offset (dx, dy, dz) from the query, in N_j?  d: the literal fp32 distance.  A NaN on
// either side fails every compare.
__device__ __forceinline__ bool pca_member(const PcaArgs &a, const PcaQuery &s, int32_t slot, const LbvhPoint &p, float d) {
  if (slot == s.self_slot) return a.self_in && d <= FLT_MAX;
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

__device__ __forceinline__ void pca_add_stats(unsigned long long *ws, int lane, unsigned long long total, unsigned int max_row, unsigned long long fallback,
                                              unsigned long long degenerate, unsigned long long node_tests, unsigned long long point_tests) {
  const unsigned long long tsum = t_wave_sum(total), fb = t_wave_sum(fallback), dg = t_wave_sum(degenerate), nt = t_wave_sum(node_tests),
                           pt = t_wave_sum(point_tests);
  unsigned int mx = max_row;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, off));
  if (lane == 0) {
    if (tsum) atomicAdd(&ws[kPcaTotal], tsum);
    if (mx) atomicMax(&ws[kPcaMaxRow], (unsigned long long)mx);
    if (fb) atomicAdd(&ws[kPcaFallback], fb);
    if (dg) atomicAdd(&ws[kPcaDegenerate], dg);
    if (nt) atomicAdd(&ws[kPcaNodeTests], nt);
    if (pt) atomicAdd(&ws[kPcaPointTests], pt);
  }
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

// ---- 3. the walk ---------------------------------------------------------------------------------------------------------------------
// Teams of a wave loop in lock step: no __syncthreads, only t_wave_sync.
__global__ void __launch_bounds__(kPcaBlock) __attribute__((amdgpu_waves_per_eu(4))) pca_walk_kernel(PcaArgs a) {
  __shared__ int32_t stack_mem[4 * kWalkStack];
  __shared__ WalkLevel levels[LBVH_WIDE_LEVELS];
  __shared__ int32_t range_mem[4 * kPcaRanges];
  __shared__ uint32_t range_n_mem[4];
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  int32_t *stack = stack_mem + team * kWalkStack;
  int32_t *range = range_mem + team * kPcaRanges;
  uint32_t *range_n = range_n_mem + team;
  walk_fill_levels<1>(levels, &a.wide, lane);
  if (tl == 0) *range_n = 0u;
  t_wave_sync();
  const LbvhWideView &wv = a.wide;
  const int32_t clean_end = lane_clean_end(a.bvh);
  unsigned long long node_tests = 0, point_tests = 0, total = 0, degenerate = 0;
  unsigned int max_row = 0;
  for (;;) {
    int got = 0;
    if (lane == 0) got = (int)atomicAdd(&a.ws[kPcaCursor], 4ull);
    const int base = __builtin_amdgcn_readfirstlane(got);
    if (base >= a.m) break;
    const int32_t pos = base + team;
    const bool has_q = pos < a.m;
    const PcaQuery s = pca_query(a, pos, has_q);
    const LbvhPoint &q = s.q;
    const bool active = has_q && !a.force_redo;
    const WalkBox qb(q, s.r_walk * 1.000001f);  // the box prefilter must not cut what the rounded sphere test accepts
    const float radius_in2 = s.r > 0.f ? pca_inside2(s.r) : -1.f;
    uint32_t part = 0;  // my lane's share of the count
    float acc[9];       // ... of S1 and S2
#pragma unroll
    for (int c = 0; c < 9; c++) acc[c] = 0.f;
    // lane tl takes point tl of the sixteen slots from `slot0` (the sorted arrays are padded with NaN sentinels to whole blocks)
    auto test_points = [&](int64_t slot0, bool has_b) __attribute__((always_inline)) {
      const int64_t slot = slot0 + tl;
      LbvhPoint p = LbvhPoint{pca_nan(), 0.f, 0.f, -1};
      if (has_b) p = a.bvh.points[slot];
      const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
      const float d = knn_sqrt(t_dist2(dx, dy, dz));
      const bool hit = has_b && pca_member(a, s, (int32_t)slot, p, d);
      point_tests += has_b ? 1u : 0u;
      part = t_count(part, __ballot(hit));
      if (hit) pca_add(acc, dx, dy, dz);
    };
    bool overflow = wv.levels <= 0;
    if (wv.levels > 0)
      walk_tree<true>(
          levels, wv, stack, kWalkStack, active, q, qb, team, tl, node_tests,
          [&](const LbvhBox &bx, int32_t c, int lvl) {
            if (lvl == 0) return true;
            const float ax = fmaxf(fabsf(q.x - bx.lo[0]), fabsf(q.x - bx.hi[0])), ay = fmaxf(fabsf(q.y - bx.lo[1]), fabsf(q.y - bx.hi[1])),
                        az = fmaxf(fabsf(q.z - bx.lo[2]), fabsf(q.z - bx.hi[2]));
            const float far2 = t_dist2(ax, ay, az);
            const int64_t span = (int64_t)LBVH_BLOCK << (6 * lvl);  // points under one child of this level
            if (!(far2 <= radius_in2 && ((int64_t)c + 1) * span <= (int64_t)clean_end)) return true;
            const uint32_t at = atomicAdd(range_n, 1u);
            if (at >= (uint32_t)kPcaRanges) return true;
            range[at] = (lvl << 26) | c;
            return false;
          },
          [&](int32_t b, bool has_b) { test_points((int64_t)b * LBVH_BLOCK, has_b); }, [] {}, overflow);
    // the noted inside boxes, sixteen slots a step (every point but the query's own passes; the literal test decides all the same)
    t_wave_sync();
    const uint32_t nr = min(*range_n, (uint32_t)kPcaRanges);
    for (uint32_t i = 0; __ballot(i < nr) != 0ull; i++) {
      const bool has_r = i < nr;
      const int32_t e = has_r ? range[i] : 0;
      const int64_t span = has_r ? (int64_t)LBVH_BLOCK << (6 * (e >> 26)) : 0;
      const int64_t first = (int64_t)(e & 0x3ffffff) * span;
#pragma unroll 1
      for (int64_t t = 0; __ballot(t < span) != 0ull; t += LBVH_BLOCK) test_points(first + t, t < span);
    }
    t_wave_sync();
    if (tl == 0) *range_n = 0u;
    t_wave_sync();
    // the one reduction of the row
    const uint32_t cnt = t_team_sum(part);
#pragma unroll
    for (int c = 0; c < 9; c++) acc[c] = pca_team_sum(acc[c]);
    if (has_q && tl == 0) {
      if (overflow || a.force_redo) {
        // left to the lane kernel, which starts the row again: nothing of it is counted here
        a.redo[atomicAdd(&a.ws[kPcaRedo], 1ull)] = pos;
      } else {
        pca_store(a, s.at, cnt, acc);
        total += cnt;
        max_row = max(max_row, cnt);
        degenerate += cnt < (uint32_t)a.min_points ? 1u : 0u;
      }
    }
  }
  pca_add_stats(a.ws, lane, total, max_row, 0ull, degenerate, node_tests, point_tests);
}

// ---- 4. one query per lane: the queries of the redo list ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kPcaLaneBlock) pca_lane_kernel(PcaArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kPcaLaneBlock + threadIdx.x;
  const bool has_q = t < (int64_t)a.ws[kPcaRedo];
  const int32_t pos = has_q ? a.redo[t] : 0;
  const PcaQuery s = pca_query(a, pos, has_q);
  const LbvhPoint &q = s.q;
  const float r_wide = s.r_walk * 1.000001f;
  uint32_t cnt = 0;
  float acc[9];
#pragma unroll
  for (int c = 0; c < 9; c++) acc[c] = 0.f;
  unsigned long long node_tests = 0, point_tests = 0;
  if (has_q)
    lane_walk<LaneRope::kWithNode>(a.bvh,
        [&](int32_t, const LbvhNode &nd, int32_t) {
          node_tests++;
          return lane_box_hit(nd, q, r_wide) ? lane_descend() : lane_rope();
        },
        [&](int32_t slot, const LbvhPoint &p) {
          point_tests++;
          const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
          const float d = knn_sqrt(t_dist2(dx, dy, dz));
          if (pca_member(a, s, slot, p, d)) {
            cnt++;
            pca_add(acc, dx, dy, dz);
          }
          return lane_rope();
        });
  if (has_q) pca_store(a, s.at, cnt, acc);
  // (all lanes of the wave are here)
  pca_add_stats(a.ws, threadIdx.x & 63, has_q ? cnt : 0u, has_q ? cnt : 0u, has_q ? 1u : 0u, has_q && cnt < (uint32_t)a.min_points ? 1u : 0u, node_tests,
                point_tests);
}

// ---- 5. the finish -------------------------------------------------------------------------------------------------------------------
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
  const size_t words_b = align(kPcaWords * sizeof(unsigned long long)), col_b = align(((size_t)m + 1) * sizeof(uint32_t)), order_cols = own ? 0 : 4 * col_b,
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

  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kPcaWords * sizeof(unsigned long long), s));
  if (!own) query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, tmp, order_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_g_, s));
  // the walk, then the lane kernel for what the walk left
  const int blocks = (int)std::min<int64_t>((m + 3) / 4, (int64_t)cu_count_ * kPcaBlocksPerCu);
  hipLaunchKernelGGL(pca_walk_kernel, dim3(blocks), dim3(kPcaBlock), 0, s, a);
  OWLMI_HIP(hipGetLastError());
  unsigned long long *h_words = h_counters_;
  OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kPcaWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (const unsigned long long n_redo = h_words[kPcaRedo]) {
    const unsigned lane_blocks = (unsigned)((n_redo + kPcaLaneBlock - 1) / kPcaLaneBlock);
    hipLaunchKernelGGL(pca_lane_kernel, dim3(lane_blocks), dim3(kPcaLaneBlock), 0, s, a);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipMemcpyAsync(h_words, a.ws, kPcaWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  }
  OWLMI_HIP(hipEventRecord(ev_h_, s));
  hipLaunchKernelGGL(pca_finish_kernel, dim3(flat_blocks), dim3(kPcaFlatBlock), 0, s, a);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->total = (int64_t)h_words[kPcaTotal];
    info->max_row = (int64_t)h_words[kPcaMaxRow];
    info->degenerate_rows = (int64_t)h_words[kPcaDegenerate];
    info->fallback_items = (int64_t)h_words[kPcaFallback];
    info->node_tests = (int64_t)h_words[kPcaNodeTests];
    info->point_tests = (int64_t)h_words[kPcaPointTests];
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_e_, ev_a_));
    if (with_k) OWLMI_HIP(hipEventElapsedTime(&info->bound_ms, ev_e_, ev_f_));
    if (!own) OWLMI_HIP(hipEventElapsedTime(&info->order_ms, ev_f_, ev_g_));
    OWLMI_HIP(hipEventElapsedTime(&info->walk_ms, ev_g_, ev_h_));
    OWLMI_HIP(hipEventElapsedTime(&info->finish_ms, ev_h_, ev_a_));
  }
}

}  // namespace owlmi
