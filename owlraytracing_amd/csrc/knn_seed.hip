// knn_seed.hip -- the k nearest points, exactly, with no radius from the caller (tknnKnn, include/owlknn_knn.h), for query points
// that are not in the tree or for the tree's own points.
//
// Row j is the row tknnRadiusKnn gives q_j at radius FLT_MAX.  The radius the walk really starts with is found here: the tree's
// points are sorted along a space-filling curve, so the blocks of 16 around a query's place in that order are real points close to
// it.  If k of them are eligible for the row (finite distance, not the skipped point), the k-th smallest of their distances is
// an upper bound r_j of the row's k-th distance, whatever the data are: the row's k entries are the k smallest distances of ALL
// eligible points, of which the seeds are a subset.  Every entry of the row then lies within r_j, and the walk of radius_knn.hip
// at radius r_j returns the row of radius FLT_MAX: both are the first k of the same ascending sequence.  With fewer than k
// eligible seeds r_j is FLT_MAX itself.  Nothing here depends on the place being a good one; a bad one only costs a wider walk.
//   1. external queries: query_order (query_order.h), then rknn_slot_kernel: a query's full 21-level curve key, searched in the
//      tree's sorted keys (Lbvh::keys_device()), one query per lane; the kernel also serves tknnPeriodicKnn and, inside a batch's
//      range, tknnBatchKnn (rknn_slots).  The tree's own points are their slots: no such pass.
//   2. rknn_seed_kernel<NREG, KnnSeedRule<SELF>> (radius_knn_walk.h): the window around the slot, clipped to the blocks that hold
//      points without a NaN; r_j goes to a workspace column.  SELF: the teams work in slot order, and the query, its id as the
//      skipped point and r_j go to workspace columns by slot.
//   3. radius_knn_walks (radius_knn_walk.h): radius_knn.hip's walk and lane kernels with those columns as the rows' radii
//      (zero_radius_ok: k duplicates of a query give r_j = 0); SELF: rows written through prim_id, the caller's row of a slot.
#include "curve_key.h"
#include "query_order.h"
#include "radius_knn_walk.h"

#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

struct KnnSeedArgs {
  LbvhView bvh;              // the tree: its sorted points, padded with sentinels to whole blocks
  const float *queries;      // external: m packed triples, caller order
  const uint32_t *order;     // external: the query worked on at sorted position i
  const int32_t *slots;      // external: its place in the tree's order, by sorted position (0 .. n)
  const int32_t *skip_ids;   // external: m, by the caller's j (may be null)
  int32_t m;
  int k;
  float *radii;              // out: r_j, by the caller's j (SELF: by slot)
  float *self_queries;       // SELF, out: the slot's point as a query, packed triples by slot
  int32_t *self_skip;        // SELF, out: the slot's id, by slot
  unsigned long long *ws;    // kRknnWsWords counters
};

// ---- 1. a query's place in the tree's order ------------------------------------------------------------------------------------
// The first slot whose key is not below the query's: the tree's quantisation at all 21 levels (morton_kernel, lbvh.hip), queries
// outside the scene box clamped to its faces as query_code_kernel clamps them; a query with a NaN coordinate lands behind the last
// finite point.  With labels: the search runs inside the batch's range [starts[label], starts[label + 1]) for the batched key of
// (label, query), as the tree's key is made from its 21 levels; a query without a batch or with a NaN gets slot 0 (it has no seed
// pass).
__global__ void __launch_bounds__(kRknnLaneBlock) rknn_slot_kernel(const float *__restrict__ queries, const uint32_t *__restrict__ order, int32_t m,
                                                                  const float *__restrict__ scene, int curve, const uint64_t *__restrict__ keys, int32_t n,
                                                                  int32_t *__restrict__ slots, const int32_t *__restrict__ query_batch,
                                                                  const int32_t *__restrict__ starts, int32_t num_batches, int key_bits) {
  const int32_t i = blockIdx.x * kRknnLaneBlock + threadIdx.x;
  if (i >= m) return;
  const int64_t qi = order[i];
  const float ext = fmaxf(fmaxf(scene[3] - scene[0], scene[4] - scene[1]), scene[5] - scene[2]);
  const uint64_t key21 = curve_point_key(curve, queries[3 * qi], queries[3 * qi + 1], queries[3 * qi + 2], scene[0], scene[1], scene[2], ext, 21);
  uint32_t label = 0;
  int32_t lo = 0, hi = n;
  if (query_batch) {
    label = (uint32_t)query_batch[qi];
    hi = 0;
    if (label < (uint32_t)num_batches && !(key21 >> 63)) lo = starts[label], hi = starts[label + 1];
  }
  const uint64_t key = ((uint64_t)label << (63 - key_bits)) | (key21 >> key_bits);
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  slots[i] = lo;
}

// ---- 2. the seed hooks of the Euclidean rule -----------------------------------------------------------------------------------
template <bool SELF>
struct KnnSeedRule {
  using Args = KnnSeedArgs;
  struct Query {
    LbvhPoint q;
    int32_t skip;
  };
  static __device__ __forceinline__ int32_t item_at(const Args &a, int32_t pos) { return SELF ? pos : (int32_t)a.order[pos]; }
  static __device__ __forceinline__ void point(const Args &a, int32_t item, bool has_q, Query &s) {
    s.q = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
    s.skip = -1;
    if (!has_q) return;
    if (SELF) {
      s.q = a.bvh.points[item];
      s.skip = s.q.id;
    } else {
      s.q.x = a.queries[3 * (int64_t)item], s.q.y = a.queries[3 * (int64_t)item + 1], s.q.z = a.queries[3 * (int64_t)item + 2];
      s.skip = a.skip_ids ? a.skip_ids[item] : -1;
    }
  }
  static __device__ __forceinline__ float dist2(const Args &, const Query &s, const LbvhPoint &p) { return knn_dist2(p.x, p.y, p.z, s.q.x, s.q.y, s.q.z); }
  static __device__ __forceinline__ bool slot_ok(const Query &, int32_t) { return true; }
  // every block that holds a point without a NaN
  static __device__ __forceinline__ void seed_range(const Args &a, const Query &, int32_t pos, bool has_q, int32_t clean_blocks, int32_t &blk_lo,
                                                    int32_t &blk_hi, int32_t &slot) {
    blk_lo = 0, blk_hi = clean_blocks;
    slot = min(has_q ? (SELF ? pos : a.slots[pos]) : 0, a.bvh.n - 1);
  }
  static __device__ __forceinline__ void seed_store(const Args &a, const Query &s, int32_t item, float bound) {
    a.radii[item] = bound;
    if (SELF) {
      a.self_queries[3 * (int64_t)item] = s.q.x, a.self_queries[3 * (int64_t)item + 1] = s.q.y, a.self_queries[3 * (int64_t)item + 2] = s.q.z;
      a.self_skip[item] = s.skip;
    }
  }
};

}  // namespace

void rknn_slots(const float *queries, const uint32_t *order, int32_t m, const float *scene, int curve, const uint64_t *keys, int32_t n, int32_t *slots,
                hipStream_t s, const int32_t *query_batch, const int32_t *starts, int32_t num_batches, int key_bits) {
  hipLaunchKernelGGL(rknn_slot_kernel, dim3((unsigned)((m + kRknnLaneBlock - 1) / kRknnLaneBlock)), dim3(kRknnLaneBlock), 0, s, queries, order, m, scene, curve,
                     keys, n, slots, query_batch, starts, num_batches, key_bits);
  OWLMI_HIP(hipGetLastError());
}

void Engine::knn(const tknnKnnOptions &o, tknnKnnInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const bool self = o.d_queries == nullptr;
  // the call's workspace: counters | lane list, radii | external: codes, order (+ the sort's second halves), slots, sort space
  //                                                   | self: skipped ids, queries (three columns)
  const size_t sort_bytes = self ? 0 : query_order_sort_bytes(m, s);
  RknnWorkspace w(m, 6, sort_bytes);
  w.base = (char *)workspace(w.bytes);
  float *radii = w.column<float>(1);
  uint32_t *codes = w.column<uint32_t>(2), *codes_alt = w.column<uint32_t>(3), *order_in = w.column<uint32_t>(4), *order = w.column<uint32_t>(5);
  int32_t *slots = w.column<int32_t>(2);  // (over the codes: the sort is through when the slots are written)
  int32_t *self_skip = w.column<int32_t>(2);
  float *self_queries = w.column<float>(3);

  const LbvhView tv = bvh_.view();
  KnnSeedArgs sa;
  std::memset(&sa, 0, sizeof sa);
  sa.bvh = tv;
  sa.queries = o.d_queries;
  sa.order = self ? nullptr : order;
  sa.slots = self ? nullptr : slots;
  sa.skip_ids = o.d_skip_ids;
  sa.m = (int32_t)m;
  sa.k = o.k;
  sa.radii = radii;
  sa.self_queries = self ? self_queries : nullptr;
  sa.self_skip = self ? self_skip : nullptr;
  sa.ws = w.words();

  RadiusKnnKernelArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = tv;
  a.wide = bvh_.wide_view();
  a.queries = self ? self_queries : o.d_queries;
  a.order = self ? nullptr : order;
  a.m = (int32_t)m;
  a.k = o.k;
  a.radii = radii;
  a.skip_ids = self ? self_skip : o.d_skip_ids;
  a.out_row = self ? tv.prim_id : nullptr;
  if (const char *e = getenv("TKNN_KNN_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.zero_radius_ok = 1;
  a.out_idx = o.d_idx;
  a.out_dist = o.d_dist;
  a.out_counts = o.d_counts;
  a.redo = w.column<int32_t>(0);
  a.ws = w.words();

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kRknnWsWords * sizeof(unsigned long long), s));
  if (!self) query_order(o.d_queries, m, bvh_.scene_device(), bvh_.curve(), codes, codes_alt, order_in, order, w.column<void>(6), sort_bytes, s);
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  if (!self) rknn_slots(o.d_queries, order, (int32_t)m, bvh_.scene_device(), bvh_.curve(), bvh_.keys_device(), tv.n, slots, s);
  if (self)
    rknn_seed<KnnSeedRule<true>>(sa, cu_count_, s);
  else
    rknn_seed<KnnSeedRule<false>>(sa, cu_count_, s);
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  const unsigned long long n_redo = radius_knn_walks(a, cu_count_, h_counters_, s);
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  rknn_fill_info(info, h_counters_, n_redo, ev_a_, ev_b_, ev_c_, ev_d_);
}

}  // namespace owlmi
