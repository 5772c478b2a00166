// batch_knn.hip -- many labelled point clouds in one tree (tknnBuildBatched) and at most k nearest points inside the query's own
// cloud, with or without a radius, for labelled query points that are not in the tree or for the tree's own points (tknnBatchKnn,
// include/owlknn_batch.h).
//
// The tree is the ordinary one, sorted by a key that carries the label above the curve key (lbvh.hip, batch_key_kernel), so batch b
// is ONE range [starts[b], starts[b + 1]) of sorted slots.  Child c at level lvl of the 64-ary pyramid covers the slots
// [c * span, (c + 1) * span), span = LBVH_BLOCK << (6 * lvl) (walk_count_box's arithmetic, team_walk.h): "this box holds nothing of
// my batch" is two integer compares, no label is ever gathered in a walk, and nothing of the batch is dropped, because a slot of
// the range lies under exactly the children whose slot range holds it.  Boxes and blocks may straddle a batch boundary; the leaf
// test then takes only the lanes whose slot is in the range.
//   build. batch_label_check_kernel counts the labels outside [0, B) (one word read back), Engine::build builds with the labels,
//      batch_starts_kernel finds starts[b] as the lower bound of b << (63 - bb) in the sorted keys, one thread per batch.
//   1. external queries: batch_query_code_kernel and the radix sort of query_order.h's width -- the code is the label above the
//      leading 30 - bb bits of query_order's curve code, so the four teams of a wave walk the same batch and, inside it, neighbouring
//      nodes; without any radius also rknn_slots (knn_seed.hip), the search of the batched key of (label, query) inside the
//      batch's range.  The tree's own points are their slots and come in (label, curve) order: neither pass.
//   2. without any radius (d_radii == NULL, radius == FLT_MAX): rknn_seed_kernel<NREG, BatchRule> (radius_knn_walk.h), the window
//      around the slot, clipped to the blocks that touch the range; a seed has its slot inside the range.
//   3. rknn_walk_kernel<NREG, BatchRule> with the range rule in keep_box and at the leaf, and rknn_lane_kernel<K, BatchRule>,
//      nodes pruned by their slot range; every query goes to the lane kernel under TKNN_BATCH_KNN_FORCE_FALLBACK=1 (read per call).
#include "curve_key.h"
#include "owlknn_batch.h"
#include "query_order.h"
#include "radius_knn_walk.h"

#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

struct BatchKnnArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const uint64_t *keys;        // the tree's sorted keys: the batch of a slot is keys[slot] >> (63 - key_bits)
  const int32_t *starts;       // num_batches + 1: batch b is the sorted slots starts[b] .. starts[b + 1] - 1
  int32_t num_batches;
  int key_bits;
  const float *queries;        // external: m packed triples, by the caller's j; null: the tree's own points, an item is a sorted slot
  const int32_t *query_batch;  // external: m labels, by the caller's j
  const uint32_t *order;       // external: the query worked on at sorted position i
  const int32_t *slots;        // external, seed pass: its place in its batch's range, by sorted position
  int32_t m;
  int k;
  float radius;                // every row's radius if radii and bounds are null (FLT_MAX: none)
  const float *radii;          // m, by the caller's j (may be null)
  float *bounds;               // the seed pass's r_j, by item (null: no seed pass)
  const int32_t *skip_ids;     // external: m, by the caller's j (may be null)
  int force_redo;              // TKNN_BATCH_KNN_FORCE_FALLBACK (tests): the walk leaves every query to the lane kernel
  int32_t *out_idx;            // m*k
  float *out_dist;             // m*k (may be null)
  int32_t *out_counts;         // m (may be null)
  int32_t *redo;               // m: items left to the lane kernel
  unsigned long long *ws;      // kRknnWsWords counters
};

// ---- the build's two kernels ---------------------------------------------------------------------------------------------------------
// how many labels lie outside [0, num_batches): one word
__global__ void __launch_bounds__(kRknnLaneBlock) batch_label_check_kernel(const int32_t *__restrict__ batch, int64_t n, int32_t num_batches,
                                                                           unsigned long long *__restrict__ bad) {
  unsigned long long mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * kRknnLaneBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRknnLaneBlock)
    mine += (uint32_t)batch[i] >= (uint32_t)num_batches ? 1u : 0u;
  mine = t_wave_sum(mine);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(bad, mine);
}
// starts[b], 0 <= b <= num_batches: the first sorted slot whose key is not below b << (63 - key_bits); for b = num_batches that is
// the first slot of a point with a NaN (bit 63 alone is above every label), n if there is none
__global__ void __launch_bounds__(kRknnLaneBlock) batch_starts_kernel(const uint64_t *__restrict__ keys, int32_t n, int32_t num_batches, int key_bits,
                                                                      int32_t *__restrict__ starts) {
  const int32_t b = blockIdx.x * kRknnLaneBlock + threadIdx.x;
  if (b > num_batches) return;
  const uint64_t key = (uint64_t)b << (63 - key_bits);
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  starts[b] = lo;
}

// ---- the batch rule ------------------------------------------------------------------------------------------------------------------
// The range rule.  Child c of level lvl covers the slots [c << sh, (c + 1) << sh), sh = 4 + 6 lvl; it meets [s, e) iff
// (s >> sh) <= c <= ((e - 1) >> sh).  A child that does not is declined before its box is looked at; one that does goes through
// the Euclidean gate rule.  The rule drops no point of the batch: slot t lies under child t >> sh of every level, and s <= t < e
// gives (s >> sh) <= (t >> sh) <= ((e - 1) >> sh).  (Above level 4, sh exceeds 31; every slot is below 2^31, so a shift by 31
// gives the same zeros.)  Boxes and blocks may hold neighbours from other batches: a point is a seed or a candidate only if its
// slot lies in [s, e).
// The seed window.  The blocks that touch [s, e); a window that does not hold the whole batch has at most one edge block, so at
// least 16 * ceil(k / 16) + 1 slots of the batch, one of which may be the skipped point: k seeds.  With fewer (a batch of fewer
// than k eligible points) the bound is FLT_MAX, which costs a walk of the batch's range and no more.
struct BatchRule {
  using Args = BatchKnnArgs;
  struct Query {
    LbvhPoint q;
    float r;       // the predicate's radius: the caller's, or the seed bound (which may be 0: k duplicates of the query)
    float r_wide;  // r * (1 + 1e-6): the box prefilter must not cut what the rounded sphere test accepts (radius_knn.hip)
    float gate_r;  // the squared-distance gate of an empty list: every d2 whose rounded root can be <= r passes
    int32_t skip;  // the point left out of the row (no point has a negative id)
    int32_t row;   // the caller's j
    int32_t s, e;  // the batch's sorted slots [s, e) (0, 0: a label no batch has)
    bool valid;    // a radius the call takes, a query without a NaN and a batch with a point in it (a row without: empty)
  };
  static __device__ __forceinline__ int32_t item_at(const Args &a, int32_t pos) { return a.queries ? (int32_t)a.order[pos] : pos; }
  // the point, skipped id, row and batch range of an item: the caller's query j, or (the tree's own points) the point of a sorted slot
  static __device__ __forceinline__ void point(const Args &a, int32_t item, bool has_q, Query &t) {
    t.q = LbvhPoint{__uint_as_float(0x7fc00000u), 0.f, 0.f, -1};
    t.skip = -1, t.row = item, t.s = 0, t.e = 0;
    if (!has_q) return;
    uint32_t label;
    if (a.queries) {
      t.q.x = a.queries[3 * (int64_t)item], t.q.y = a.queries[3 * (int64_t)item + 1], t.q.z = a.queries[3 * (int64_t)item + 2];
      t.skip = a.skip_ids ? a.skip_ids[item] : -1;
      label = (uint32_t)a.query_batch[item];
    } else {
      t.q = a.bvh.points[item];
      t.skip = t.q.id;
      t.row = a.bvh.prim_id[item];
      label = (uint32_t)(a.keys[item] >> (63 - a.key_bits));  // (a NaN point: 2^key_bits, no batch)
    }
    if (label < (uint32_t)a.num_batches) t.s = a.starts[label], t.e = a.starts[label + 1];
  }
  static __device__ __forceinline__ Query query(const Args &a, int32_t item, bool has_q) {
    Query t;
    point(a, item, has_q, t);
    t.r = !has_q ? 0.f : a.bounds ? a.bounds[item] : a.radii ? a.radii[t.row] : a.radius;
    const bool no_nan = (t.q.x == t.q.x) & (t.q.y == t.q.y) & (t.q.z == t.q.z);
    t.valid = has_q && (t.r > 0.f || (a.bounds && t.r == 0.f)) && t.r <= FLT_MAX && no_nan && t.e > t.s;  // (a NaN radius: neither)
    t.r_wide = t.r * 1.000001f;
    t.gate_r = knn_gate_from_worst(t.r);
    return t;
  }
  static __device__ __forceinline__ bool keep_box(const Args &, const Query &t, const LbvhBox &bx, int32_t c, int lvl, float tau2) {
    const int sh = min(4 + 6 * lvl, 31);
    if (c < (t.s >> sh) || c > ((t.e - 1) >> sh)) return false;
    return !beyond_gate(box_min_dist2(bx, t.q), tau2);
  }
  static __device__ __forceinline__ float dist2(const Args &, const Query &t, const LbvhPoint &p) { return knn_dist2(p.x, p.y, p.z, t.q.x, t.q.y, t.q.z); }
  static __device__ __forceinline__ bool slot_ok(const Query &t, int32_t slot) { return slot >= t.s && slot < t.e; }
  static __device__ __forceinline__ LaneStep lane_node(const Args &, const Query &t, int32_t ref, const LbvhNode &nd, float gate) {
    if (lbvh_last(ref, nd.other) < t.s || lbvh_first(ref, nd.other) >= t.e) return lane_rope();
    return rknn_lane_box(nd, t.q, t.r_wide, gate);
  }
  static __device__ __forceinline__ void seed_range(const Args &a, const Query &t, int32_t pos, bool has_q, int32_t, int32_t &blk_lo, int32_t &blk_hi,
                                                    int32_t &slot) {
    blk_lo = t.s >> 4, blk_hi = t.e > t.s ? ((t.e - 1) >> 4) + 1 : blk_lo;
    slot = min(has_q ? (a.queries ? a.slots[pos] : pos) : 0, t.e - 1);
  }
  static __device__ __forceinline__ void seed_store(const Args &a, const Query &, int32_t item, float bound) { a.bounds[item] = bound; }
};

// ---- 1. the order of the queries ----------------------------------------------------------------------------------------------------
// query_code_kernel's code (query_order.h) under the label: (label << (30 - key_bits)) | (code >> key_bits), as the tree's key is made
// from its 21 levels.  A query with a NaN or with a label no batch has sorts last (bit 30), as NaN queries do there.
__global__ void __launch_bounds__(kRknnLaneBlock) batch_query_code_kernel(const float *__restrict__ queries, const int32_t *__restrict__ query_batch, int32_t m,
                                                                          const float *__restrict__ scene, int curve, int32_t num_batches, int key_bits,
                                                                          uint32_t *__restrict__ codes, uint32_t *__restrict__ order) {
  const int32_t i = blockIdx.x * kRknnLaneBlock + threadIdx.x;
  if (i >= m) return;
  const float ext = fmaxf(fmaxf(scene[3] - scene[0], scene[4] - scene[1]), scene[5] - scene[2]);
  uint32_t code = (uint32_t)curve_point_key(curve, queries[3 * (int64_t)i], queries[3 * (int64_t)i + 1], queries[3 * (int64_t)i + 2], scene[0], scene[1],
                                            scene[2], ext, kCodeBits / 3);
  const uint32_t label = (uint32_t)query_batch[i];
  if (label >= (uint32_t)num_batches) code = 1u << kCodeBits;
  if (!(code >> kCodeBits)) code = (label << (kCodeBits - key_bits)) | (code >> key_bits);
  codes[i] = code;
  order[i] = (uint32_t)i;
}

}  // namespace

void Engine::build_batched(const float *d_xyz, const int32_t *d_ids, const int32_t *d_batch, int32_t num_batches, int64_t n, tknnBuildInfo *info,
                           hipStream_t s) {
  int bits = 0;  // the smallest multiple of 3 with 2^bits >= num_batches: the key loses whole levels of cells
  while ((1 << bits) < num_batches) bits += 3;
  unsigned long long *d_bad = (unsigned long long *)workspace(256);
  OWLMI_HIP(hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), s));
  const int blocks = (int)std::min<int64_t>((n + kRknnLaneBlock - 1) / kRknnLaneBlock, (int64_t)cu_count_ * 8);
  hipLaunchKernelGGL(batch_label_check_kernel, dim3(blocks), dim3(kRknnLaneBlock), 0, s, d_batch, n, num_batches, d_bad);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipMemcpyAsync(h_counters_, d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (h_counters_[0]) {
    bvh_.clear();
    num_batches_ = 0;
    throw ArgError{TKNN_E_ARG, "tknnBuildBatched: " + std::to_string(h_counters_[0]) + " of the " + std::to_string(n) + " labels in d_batch lie outside [0, num_batches = " +
                                   std::to_string(num_batches) + ")"};
  }
  if ((int64_t)num_batches + 1 > batch_starts_cap_) {
    if (batch_starts_) (void)hipFree(batch_starts_);
    batch_starts_ = nullptr;
    batch_starts_cap_ = 0;
    bvh_.clear();  // (if the allocation fails: no tree rather than a batched one without its starts)
    OWLMI_HIP(hipMalloc((void **)&batch_starts_, ((size_t)num_batches + 1) * sizeof(int32_t)));
    batch_starts_cap_ = (int64_t)num_batches + 1;
  }
  build(d_xyz, d_ids, n, info, s, d_batch, bits);
  hipLaunchKernelGGL(batch_starts_kernel, dim3((unsigned)((num_batches + 1 + kRknnLaneBlock - 1) / kRknnLaneBlock)), dim3(kRknnLaneBlock), 0, s,
                     bvh_.keys_device(), (int32_t)n, num_batches, bits, batch_starts_);
  try {
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipStreamSynchronize(s));
  } catch (...) {
    bvh_.clear();
    throw;
  }
  num_batches_ = num_batches;
  batch_bits_ = bits;
}

void Engine::batch_layout(int32_t *num_batches, int32_t *key_bits, int32_t *d_starts, hipStream_t s) {
  if (num_batches) *num_batches = num_batches_;
  if (key_bits) *key_bits = batch_bits_;
  if (d_starts) {
    OWLMI_HIP(hipMemcpyAsync(d_starts, batch_starts_, ((size_t)num_batches_ + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    OWLMI_HIP(hipStreamSynchronize(s));
  }
}

void Engine::batch_knn(const tknnBatchKnnOptions &o, tknnBatchKnnInfo *info, hipStream_t s) {
  const int64_t m = o.m;
  const bool self = o.d_queries == nullptr;
  const bool seeded = !o.d_radii && o.radius == FLT_MAX;
  // the call's workspace: counters | lane list, bounds | external: codes, order (+ the sort's second halves), sort space
  const size_t sort_bytes = self ? 0 : query_order_sort_bytes(m, s);
  RknnWorkspace w(m, 6, sort_bytes);
  w.base = (char *)workspace(w.bytes);
  uint32_t *codes = w.column<uint32_t>(2), *codes_alt = w.column<uint32_t>(3), *order_in = w.column<uint32_t>(4), *order = w.column<uint32_t>(5);
  int32_t *slots = w.column<int32_t>(2);  // (over the codes: the sort is through when the slots are written)

  BatchKnnArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = bvh_.view();
  a.wide = bvh_.wide_view();
  a.keys = bvh_.keys_device();
  a.starts = batch_starts_;
  a.num_batches = num_batches_;
  a.key_bits = batch_bits_;
  a.queries = o.d_queries;
  a.query_batch = o.d_query_batch;
  a.order = self ? nullptr : order;
  a.slots = self ? nullptr : slots;
  a.m = (int32_t)m;
  a.k = o.k;
  a.radius = o.radius;
  a.radii = o.d_radii;
  a.bounds = seeded ? w.column<float>(1) : nullptr;
  a.skip_ids = o.d_skip_ids;
  if (const char *e = getenv("TKNN_BATCH_KNN_FORCE_FALLBACK")) a.force_redo = atoi(e) != 0;
  a.out_idx = o.d_idx;
  a.out_dist = o.d_dist;
  a.out_counts = o.d_counts;
  a.redo = w.column<int32_t>(0);
  a.ws = w.words();

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(a.ws, 0, kRknnWsWords * sizeof(unsigned long long), s));
  if (!self) {  // query_order (query_order.h) with the label above the code: one sort of the same width
    hipLaunchKernelGGL(batch_query_code_kernel, dim3((unsigned)((m + kRknnLaneBlock - 1) / kRknnLaneBlock)), dim3(kRknnLaneBlock), 0, s, o.d_queries,
                       o.d_query_batch, (int32_t)m, bvh_.scene_device(), bvh_.curve(), num_batches_, batch_bits_, codes, order_in);
    OWLMI_HIP(hipGetLastError());
    size_t bytes = sort_bytes;
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(w.column<void>(6), bytes, codes, codes_alt, order_in, order, (int)m, 0, kCodeBits + 1, s));
  }
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  if (seeded) {
    if (!self)
      rknn_slots(o.d_queries, order, (int32_t)m, bvh_.scene_device(), bvh_.curve(), a.keys, a.bvh.n, slots, s, o.d_query_batch, a.starts, num_batches_,
                 batch_bits_);
    rknn_seed<BatchRule>(a, cu_count_, s);
  }
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  const unsigned long long n_redo = rknn_walks<BatchRule>(a, cu_count_, h_counters_, s);
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  rknn_fill_info(info, h_counters_, n_redo, ev_a_, ev_b_, ev_c_, ev_d_);
}

}  // namespace owlmi
