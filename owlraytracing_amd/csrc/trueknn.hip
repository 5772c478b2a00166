// trueknn.hip -- the TrueKNN engine behind include/owlknn.h: LBVH build, the per-round "lane"
// kernel and the exact repair (one query per lane, the stackless rope traversal of lane_walk.h) and
// the result writers.  The persistent wave-packet kernel lives in trueknn_wave.hip, the C ABI's entry points in tknn_api.hip.
//
// Reference functions this file replaces (samples/s01-trueknn):
//   deviceCode.cu:140-153  __raygen__rayGen            -> active test + point query per lane
//   owl_device.h:150-174   optixTrace (RT cores)       -> rope traversal of the LBVH (lane_walk.h)
//   deviceCode.cu:62-138   __intersection__Spheres     -> box test + register k-list insert
//   hostCode.cpp:285-340   round loop                  -> Engine::solve_lane
#include "knn_thresholds.h"  // knn_gate_from_worst
#include "lane_walk.h"
#include "trueknn_engine.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kLaneBlock = 256;

struct LaneRoundArgs {
  LbvhView bvh;
  LbvhView halo;           // second point set searched by every query (n == 0: none)
  int level;               // 0-based radius level of this launch
  int32_t *out_level;      // n, caller order (may be null)
  float radius;
  int k;
  uint8_t *done;           // per sorted slot
  uint8_t *tie;            // per sorted slot: (1 + level) | 0x80 for rows finished with exact-distance ties (knn_flag_tie)
  int32_t *tie_list;
  const int32_t *next_level;  // per sorted slot: first level this query takes part in (may be null)
  int64_t *isect_sorted;   // per sorted slot, accumulated over rounds
  int32_t *out_idx;        // n*k, caller order (may be null)
  float *out_dist;         // n*k (may be null)
  int64_t *out_isect;      // n (may be null)
  tknnNeigh *out_fb;       // n*k (may be null)
  unsigned long long *counters;  // [0] unfinished, [1] node tests, [2] point tests, [3] sum isect, [4] active lanes, [5], [6] candidates of the active lanes, plain and squared
};

template <int K>
__device__ __forceinline__ void write_row(const LaneRoundArgs &a, int32_t row, const KList<K> &list,
                                          int64_t isect) {
  const int k = a.k;
  const int64_t base = (int64_t)row * k;
#pragma unroll
  for (int j = 0; j < K; j++) {
    if (j < k) {
      int32_t prim = knn_key_prim(list.key[j]);
      float d = knn_key_dist(list.key[j]);
      if (a.out_idx) a.out_idx[base + j] = prim;
      if (a.out_dist) a.out_dist[base + j] = d;
      if (a.out_fb) {
        // final state of the reference's frameBuffer: slot 0 carries numNeighbors (0 = done) and
        // the intersection counter, other slots keep their initial {k, 0}  (deviceCode.cu:74,118)
        tknnNeigh e;
        e.ind = prim;
        e.dist = d;
        e.numNeighbors = j == 0 ? 0 : k;
        e.pad_ = 0;
        e.intersections = j == 0 ? isect : 0;
        a.out_fb[base + j] = e;
      }
    }
  }
  if (a.out_isect) a.out_isect[row] = isect;
  if (a.out_level) a.out_level[row] = a.level;
}

// SUBTREES: count fully covered subtrees beyond the gate instead of walking them (lane_counts_subtree, lane_walk.h).  In a
// wave some lane is at a large node most of the time, so the test is paid on most steps: launches
// whose boxes hold few points run without it (Engine::lane_rounds decides per round).
template <int K, bool SUBTREES>
__global__ void __launch_bounds__(kLaneBlock) lane_round_kernel(LaneRoundArgs a) {
  const int32_t t = blockIdx.x * kLaneBlock + threadIdx.x;
  const LbvhView &bvh = a.bvh;
  // deviceCode.cu:148: finished queries launch no ray.  Inactive lanes fall through to the
  // wave-wide counter reduction at the end instead of returning.
  const bool active = t < bvh.n && !a.done[t] && (!a.next_level || a.next_level[t] <= a.level);
  LbvhPoint q = {0.f, 0.f, 0.f, -1};
  if (active) q = bvh.points[t];
  const float r = a.radius;
  KList<K> list;
  list.clear();
  int32_t cnt = 0, others = 0;
  uint32_t node_tests = 0, point_tests = 0;
  float tau2 = INFINITY;  // squared-distance gate from the list's last entry: beyond it nothing enters
  for (int tree = 0; tree < 2; tree++) {
    const LbvhView &tv = tree == 0 ? a.bvh : a.halo;
    if (tv.n <= 0 || !active) continue;
    const int32_t clean_end = lane_clean_end(tv);
    lane_walk<LaneRope::kWhenTaken>(tv,
        [&](int32_t ref, const LbvhNode &nd, int32_t) {
          node_tests++;
          const bool hit = lane_box_hit(nd, q, r);
          int32_t c;
          if (SUBTREES && hit && lane_counts_subtree(ref, nd, q, r, tau2, clean_end, c)) {
            cnt += c, others += c;
            return lane_rope();
          }
          return hit ? lane_descend() : lane_rope();
        },
        [&](int32_t, const LbvhPoint &p) {
          point_tests++;
          if (knn_in_box(p.x, p.y, p.z, r, q.x, q.y, q.z)) {
            cnt++;                 // deviceCode.cu:74
            if (p.id != q.id) {    // deviceCode.cu:103
              others++;
              float d = knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z));
              list.insert(knn_key(d, p.id));
              if (SUBTREES) tau2 = knn_gate_from_worst(knn_key_dist(list.worst()));
            }
          }
          return lane_rope();
        });
  }
  int64_t isect = 0;
  bool finished = false;
  if (active) {
    isect = a.isect_sorted[t] + cnt;
    a.isect_sorted[t] = isect;
    finished = others >= a.k;  // k insertions happened <=> numNeighbors reached 0
    if (finished) {
      a.done[t] = 1;
      write_row<K>(a, bvh.prim_id[t], list, isect);
      if (list.has_ties(a.k)) knn_flag_tie(a.tie, a.tie_list, a.counters, t, a.level);
    }
  }
  // wave-aggregated counters (all 64 lanes are here)
  const bool waiting = t < bvh.n && !a.done[t] && !active;  // handed over at a later level
  unsigned long long unfinished = __popcll(__ballot((active && !finished) || waiting));
  unsigned long long traced = __popcll(__ballot(active));
  unsigned long long nt = node_tests, pt = point_tests, si = finished ? (unsigned long long)isect : 0ull;
  // candidates of the active lanes, plain and squared (capped): sum c^2 / sum c is the box population
  // a random candidate TEST of this round saw, the figure that says where the round's work was
  const unsigned long long cc = active ? (unsigned long long)min(cnt, 65535) : 0ull;
  unsigned long long sc = cc, sc2 = cc * cc;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nt += __shfl_xor(nt, off);
    pt += __shfl_xor(pt, off);
    si += __shfl_xor(si, off);
    sc += __shfl_xor(sc, off);
    sc2 += __shfl_xor(sc2, off);
  }
  // the workgroup's sums in LDS, then one atomic per counter and workgroup on the workgroup's stripe (kStatBase, knn_device.h)
  __shared__ unsigned long long blk_sum[7];
  if (threadIdx.x < 7) blk_sum[threadIdx.x] = 0ull;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    if (unfinished) atomicAdd(&blk_sum[0], unfinished);
    if (nt) atomicAdd(&blk_sum[1], nt);
    if (pt) atomicAdd(&blk_sum[2], pt);
    if (si) atomicAdd(&blk_sum[3], si);
    if (traced) atomicAdd(&blk_sum[4], traced);
    if (sc) {
      atomicAdd(&blk_sum[5], sc);
      atomicAdd(&blk_sum[6], sc2);
    }
  }
  __syncthreads();
  if (threadIdx.x < 7 && blk_sum[threadIdx.x])
    atomicAdd(&a.counters[kStatBase + (blockIdx.x & (kStatStripes - 1)) * kStatStride + threadIdx.x], blk_sum[threadIdx.x]);
}

template <int K>
void launch_lane(const LaneRoundArgs &a, bool subtrees, hipStream_t s) {
  unsigned blocks = (unsigned)((a.bvh.n + kLaneBlock - 1) / kLaneBlock);
  if (subtrees)
    hipLaunchKernelGGL((lane_round_kernel<K, true>), dim3(blocks), dim3(kLaneBlock), 0, s, a);
  else
    hipLaunchKernelGGL((lane_round_kernel<K, false>), dim3(blocks), dim3(kLaneBlock), 0, s, a);
}

// ---- exact-kNN repair (opt-in, never part of tknnSolve) ----------------
// The reference's rows are box-candidate kNN: a query that finished with radius r_q only ever saw
// points inside its L-inf box, so when its k-th distance d_k exceeds r_q a closer point may sit
// outside the box (15-20 % of rows on uniform data).  Rows with d_k <= r_q are not exact
// either: candidates at equal distances keep the replay's order (first round seen, then index), and
// at the k-th place that order may keep another point than (dist, index) order does.  So every
// finished row is walked again.  Every true neighbour has Euclidean distance <= d_k, hence lies in
// the box of half-width d_k: one more traversal with that radius, (dist, index) order, gives the
// exact row.  The walk needs no r_q, so rows solved with per-query start radii are served alike.
struct RepairArgs {
  LbvhView bvh, halo;
  int k;
  const int32_t *levels;  // per caller row: level at which the query finished, -1: unfinished (row not written)
  int32_t *idx;           // n*k rows, read (d_k) and rewritten
  float *dist;
  unsigned long long *counters;  // [0] rows whose contents changed
};

template <int K>
__global__ void __launch_bounds__(kLaneBlock) repair_kernel(RepairArgs a) {
  const int32_t t = blockIdx.x * kLaneBlock + threadIdx.x;
  if (t >= a.bvh.n) return;
  const LbvhPoint q = a.bvh.points[t];
  const int32_t row = a.bvh.prim_id[t];
  if (a.levels[row] < 0) return;
  const int64_t base = (int64_t)row * a.k;
  const float dk = a.dist[base + a.k - 1];
  if (!(dk <= FLT_MAX)) return;  // NaN query, or a row without k finite distances: no box to walk
  // The rounded box test must not cut a point at computed distance <= d_k.  Its exact offset on every
  // axis is at most sqrt(d_k^2 (1 + 4 ulp) + 3 * 2^-150): each square rounds by a relative half ulp, or
  // by up to 2^-150 where it is subnormal.  d_k * 1.000001 covers the first term, + 2^-74 the second
  // (sqrt(3) * 2^-75 < 2^-74), so that rows of points closer than 1e-19 stay exact too.
  const float r = dk * 1.000001f + 0x1p-74f;
  KList<K> list;
  list.clear();
  for (int tree = 0; tree < 2; tree++) {
    const LbvhView &tv = tree == 0 ? a.bvh : a.halo;
    if (tv.n <= 0) continue;
    lane_walk<LaneRope::kWhenTaken>(tv, [&](int32_t, const LbvhNode &nd, int32_t) { return lane_box_hit(nd, q, r) ? lane_descend() : lane_rope(); },
        [&](int32_t, const LbvhPoint &p) {
          if (p.id != q.id && knn_in_box(p.x, p.y, p.z, r, q.x, q.y, q.z))
            list.insert(knn_key(knn_sqrt(knn_dist2(p.x, p.y, p.z, q.x, q.y, q.z)), p.id));
          return lane_rope();
        });
  }
  bool changed = false;
#pragma unroll
  for (int j = 0; j < K; j++)
    if (j < a.k) {
      const int32_t i = knn_key_prim(list.key[j]);
      const float d = knn_key_dist(list.key[j]);
      if (i != a.idx[base + j] || __float_as_uint(d) != __float_as_uint(a.dist[base + j])) {
        a.idx[base + j] = i;
        a.dist[base + j] = d;
        changed = true;
      }
    }
  if (changed) atomicAdd(&a.counters[0], 1ull);
}

template <int K>
void launch_repair(const RepairArgs &a, hipStream_t s) {
  unsigned blocks = (unsigned)((a.bvh.n + kLaneBlock - 1) / kLaneBlock);
  hipLaunchKernelGGL(repair_kernel<K>, dim3(blocks), dim3(kLaneBlock), 0, s, a);
}

}  // namespace

tknnSolveInfo solve_info(const KernelStats &st, float start_radius, int kernel, int list_capacity, float ms) {
  tknnSolveInfo info;
  std::memset(&info, 0, sizeof info);
  info.rounds = (int)st.rounds;
  info.final_radius = final_radius(start_radius, info.rounds);
  info.node_tests = (int64_t)st.node_tests;
  info.point_tests = (int64_t)st.point_tests;
  info.total_intersections = (int64_t)st.intersections;
  info.total_active_rounds = (int64_t)st.active_rounds;
  info.solve_ms = ms;
  info.dominant_kernel_ms = ms;
  info.dominant_kernel_launches = 1;
  info.kernel_used = kernel;
  info.list_capacity = list_capacity;
  info.unfinished = (int64_t)st.unfinished;
  return info;
}

void merge_tail(tknnSolveInfo &into, const tknnSolveInfo &tail, float start_radius, bool count_launches) {
  into.rounds = std::max(into.rounds, tail.rounds);
  into.final_radius = final_radius(start_radius, into.rounds);
  into.node_tests += tail.node_tests;
  into.point_tests += tail.point_tests;
  into.total_intersections += tail.total_intersections;
  into.total_active_rounds += tail.total_active_rounds;
  into.unfinished += tail.unfinished;
  into.solve_ms += tail.solve_ms;
  if (count_launches) into.dominant_kernel_launches += tail.dominant_kernel_launches;
}

Engine::Engine() {
  OWLMI_HIP(hipGetDevice(&device_));
  OWLMI_HIP(hipDeviceGetAttribute(&cu_count_, hipDeviceAttributeMultiprocessorCount, device_));
  OWLMI_HIP(hipEventCreate(&ev_a_));
  OWLMI_HIP(hipEventCreate(&ev_b_));
  OWLMI_HIP(hipEventCreate(&ev_c_));
  OWLMI_HIP(hipEventCreate(&ev_d_));
  OWLMI_HIP(hipEventCreate(&ev_e_));
  OWLMI_HIP(hipEventCreate(&ev_f_));
  OWLMI_HIP(hipEventCreate(&ev_g_));
  OWLMI_HIP(hipEventCreate(&ev_h_));
  OWLMI_HIP(hipMalloc((void **)&counters_, kCounterWords * sizeof(unsigned long long)));  // (the team kernel's per-XCD packet counters sit in the stripes' words, 32 words apart: trueknn_team.hip) [32]: tie rows
  OWLMI_HIP(hipMalloc((void **)&tie_list_, kTieListCap * sizeof(int32_t)));
  OWLMI_HIP(hipHostMalloc((void **)&h_counters_, kHostCounterWords * sizeof(unsigned long long)));
  if (const char *e = getenv("TKNN_WAVE_FORCE_REDO")) wave_force_redo_ = atoi(e) != 0;
  if (const char *e = getenv("TKNN_LEAF_MAX")) {
    int v = atoi(e);
    if (v >= 1 && v <= 64) wave_leaf_max_ = v;
  }
}

Engine::~Engine() {
  if (done_) (void)hipFree(done_);
  if (isect_sorted_) (void)hipFree(isect_sorted_);
  if (next_level_) (void)hipFree(next_level_);
  if (tie_) (void)hipFree(tie_);
  if (boundary_) (void)hipFree(boundary_);
  if (tie_list_) (void)hipFree(tie_list_);
  if (counters_) (void)hipFree(counters_);
  if (halo_mask_) (void)hipFree(halo_mask_);
  if (slot_list_) (void)hipFree(slot_list_);
  if (batch_starts_) (void)hipFree(batch_starts_);
  if (h_counters_) (void)hipHostFree(h_counters_);
  if (wave_ws_) (void)hipFree(wave_ws_);
  if (ev_a_) (void)hipEventDestroy(ev_a_);
  if (ev_b_) (void)hipEventDestroy(ev_b_);
  if (ev_c_) (void)hipEventDestroy(ev_c_);
  if (ev_d_) (void)hipEventDestroy(ev_d_);
  if (ev_e_) (void)hipEventDestroy(ev_e_);
  if (ev_f_) (void)hipEventDestroy(ev_f_);
  if (ev_g_) (void)hipEventDestroy(ev_g_);
  if (ev_h_) (void)hipEventDestroy(ev_h_);
  if (ev_side_a_) (void)hipEventDestroy(ev_side_a_);
  if (ev_side_b_) (void)hipEventDestroy(ev_side_b_);
  if (db_side_) (void)hipStreamDestroy(db_side_);
}

// Pointer and size are cleared before the allocation: if it fails (it throws), the next smaller request allocates
// again instead of finding a null buffer behind a stale size.
void *Engine::workspace(size_t bytes) {
  if (bytes > wave_ws_bytes_) {
    if (wave_ws_) (void)hipFree(wave_ws_);
    wave_ws_ = nullptr;
    wave_ws_bytes_ = 0;
    OWLMI_HIP(hipMalloc(&wave_ws_, bytes));
    wave_ws_bytes_ = bytes;
  }
  return wave_ws_;
}

int32_t *Engine::slot_list(int64_t n) {
  if (n > slot_list_cap_) {
    if (slot_list_) (void)hipFree(slot_list_);
    slot_list_ = nullptr;
    slot_list_cap_ = 0;
    OWLMI_HIP(hipMalloc((void **)&slot_list_, ((size_t)n + 1) * sizeof(int32_t)));
    slot_list_cap_ = n;
  }
  return slot_list_;
}

void Engine::join_side(hipStream_t s) {
  if (!db_side_pending_) return;
  OWLMI_HIP(hipStreamWaitEvent(s, ev_side_b_, 0));
  db_side_pending_ = false;
}

// What is filled is scratch and nothing else: no call may read a word of it that it has not written itself ("State that
// carries from one call to the next").  The trees, batch_starts_, boundary_ and the host's flags carry meaning and are left alone.
int64_t Engine::debug_poison(unsigned what, int byte, size_t min_workspace_bytes, hipStream_t s) {
  join_side(s);
  int64_t filled = 0;
  const auto fill = [&](void *p, size_t bytes) {
    if (!p || bytes == 0) return;
    OWLMI_HIP(hipMemsetAsync(p, byte, bytes, s));
    filled += (int64_t)bytes;
  };
  if (what & TKNN_POISON_WORKSPACE) {
    if (min_workspace_bytes > 0) workspace(min_workspace_bytes);
    fill(wave_ws_, wave_ws_bytes_);
  }
  if (what & TKNN_POISON_COUNTERS) fill(counters_, kCounterWords * sizeof(unsigned long long));
  if (what & TKNN_POISON_LISTS) {
    fill(slot_list_, slot_list_ ? ((size_t)slot_list_cap_ + 1) * sizeof(int32_t) : 0);
    fill(tie_list_, kTieListCap * sizeof(int32_t));
    fill(halo_mask_, halo_mask_ ? halo_mask_bytes(halo_mask_cap_) : 0);
  }
  if (what & TKNN_POISON_SOLVE) {
    const size_t cap = (size_t)state_cap_;
    fill(done_, cap);
    fill(isect_sorted_, cap * sizeof(int64_t));
    fill(next_level_, cap * sizeof(int32_t));
    fill(tie_, (cap + 3) & ~(size_t)3);
  }
  OWLMI_HIP(hipStreamSynchronize(s));
  if (what & TKNN_POISON_COUNTERS) {
    std::memset(h_counters_, byte, kHostCounterWords * sizeof(unsigned long long));
    filled += (int64_t)(kHostCounterWords * sizeof(unsigned long long));
  }
  return filled;
}

void Engine::set_halo(const float *d_xyz, const int32_t *d_ids, int64_t m, hipStream_t s) {
  halo_n_ = 0;
  if (m <= 0) return;
  halo_.build_from_points(d_xyz, m, s, d_ids);
  halo_n_ = m;
}

LbvhView Engine::halo_view() const {
  if (halo_count() > 0) return halo_.view();
  LbvhView v;
  std::memset(&v, 0, sizeof v);
  v.root = LBVH_END;
  return v;
}

void Engine::build(const float *d_xyz, const int32_t *d_ids, int64_t n, tknnBuildInfo *info, hipStream_t s, const int32_t *d_batch, int batch_bits) {
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  num_batches_ = 0;  // a plain tree until build_batched says otherwise
  halo_n_ = 0;
  boundary_valid_ = false;
  ids_given_ = d_ids != nullptr;
  // Per-slot solve state first: if one of these allocations fails (a 100 M-point rebuild on a full
  // card) the engine must not be left "built" with null state arrays behind a stale capacity.
  if (n > state_cap_) {
    state_cap_ = 0;
    if (done_) (void)hipFree(done_);
    if (isect_sorted_) (void)hipFree(isect_sorted_);
    if (next_level_) (void)hipFree(next_level_);
    if (tie_) (void)hipFree(tie_);
    if (boundary_) (void)hipFree(boundary_);
    boundary_ = nullptr;
    tie_ = nullptr;
    done_ = nullptr;
    isect_sorted_ = nullptr;
    next_level_ = nullptr;
    try {
      OWLMI_HIP(hipMalloc((void **)&done_, (size_t)n));
      OWLMI_HIP(hipMalloc((void **)&isect_sorted_, (size_t)n * sizeof(int64_t)));
      OWLMI_HIP(hipMalloc((void **)&next_level_, (size_t)n * sizeof(int32_t)));
      OWLMI_HIP(hipMalloc((void **)&tie_, ((size_t)n + 3) & ~(size_t)3));  // (whole words: knn_flag_tie's atomics work on the byte's word)
      OWLMI_HIP(hipMalloc((void **)&boundary_, (size_t)n));
    } catch (...) {
      bvh_.clear();  // unbuilt: tknnSolve then answers TKNN_E_STATE instead of launching on null arrays
      throw;
    }
    state_cap_ = n;
  }
  try {
    bvh_.build_from_points(d_xyz, n, s, d_ids, d_batch, batch_bits);
  } catch (...) {
    bvh_.clear();
    throw;
  }
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  OWLMI_HIP(hipMemcpyAsync(scene_, bvh_.scene_device(), 6 * sizeof(float), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  OWLMI_HIP(hipEventSynchronize(ev_b_));
  if (info) {
    float ms = 0;
    OWLMI_HIP(hipEventElapsedTime(&ms, ev_a_, ev_b_));
    info->build_ms = ms;
    info->device_bytes = (int64_t)bvh_.device_bytes();
    info->n = (int32_t)n;
  }
}

// points a candidate box of this radius holds at the mean density of the built set (a work estimate)
double Engine::expected_box_population(float radius) const {
  double measure = 1.0;
  int dims = 0;
  for (int a = 0; a < 3; a++) {
    const double e = (double)scene_[3 + a] - (double)scene_[a];
    if (e > 0) {
      measure *= e;
      dims++;
    }
  }
  if (dims == 0 || !(measure > 0)) return (double)bvh_.size();
  return (double)bvh_.size() / measure * std::pow(2.0 * (double)radius, dims);
}

void Engine::solve_lane(const SolveArgs &sa, tknnSolveInfo *info, hipStream_t s) { lane_rounds(sa, 0, true, info, s); }

void Engine::continue_lane(const SolveArgs &sa, int first_level, tknnSolveInfo *info, hipStream_t s) {
  lane_rounds(sa, first_level, false, info, s);
}

void Engine::lane_rounds(const SolveArgs &sa, int first_level, bool fresh, tknnSolveInfo *info, hipStream_t s) {
  const int64_t n = bvh_.size();
  const int cap = list_capacity_for(sa.k);
  if (fresh) {
    OWLMI_HIP(hipMemsetAsync(done_, 0, (size_t)n, s));
    OWLMI_HIP(hipMemsetAsync(isect_sorted_, 0, (size_t)n * sizeof(int64_t), s));
    if (sa.d_levels) OWLMI_HIP(hipMemsetAsync(sa.d_levels, 0xff, (size_t)n * sizeof(int32_t), s));
  }
  OWLMI_HIP(hipMemsetAsync(counters_, 0, 16 * sizeof(unsigned long long), s));
  reset_stat_stripes(s);
  LaneRoundArgs a;
  a.bvh = bvh_.view();
  a.halo = halo_view();
  a.out_level = sa.d_levels;
  a.k = sa.k;
  a.done = done_;
  a.tie = tie_;
  a.tie_list = tie_list_;
  a.isect_sorted = isect_sorted_;
  a.next_level = fresh ? nullptr : next_level_;
  a.out_idx = sa.d_idx;
  a.out_dist = sa.d_dist;
  a.out_isect = sa.d_isect;
  a.out_fb = sa.d_fb;
  a.counters = counters_;
  float radius = sa.start_radius, total_ms = 0;
  int rounds = first_level, launches = 0;
  for (int t = 0; t < first_level; t++) radius *= 2;
  double predicted_candidates = expected_box_population(radius);
  const double growth = expected_box_population(2.0f) / std::max(expected_box_population(1.0f), 1e-300);  // 2^dims
  unsigned long long c1_before = 0, c2_before = 0;
  for (;;) {
    if (rounds >= sa.max_rounds) {
      if (sa.allow_unfinished) break;
      throw RoundsExceeded{};
    }
    a.level = rounds;
    rounds++;
    launches++;
    a.radius = radius;
    // Subtree counting pays when boxes hold hundreds of points.  Stragglers handed over by the team
    // kernel are exactly those queries; otherwise predict from the round before -- the population of
    // the box an average candidate test worked in, times 2^dims -- and for the first round from
    // the scene's mean density.
    const bool subtrees = !fresh || predicted_candidates >= 256.0;
    // (the kernel's counters are striped: [0] of every stripe = unfinished is reset per round, the others accumulate over the rounds)
    OWLMI_HIP(hipMemset2DAsync(counters_ + kStatBase, kStatStride * sizeof(unsigned long long), 0, sizeof(unsigned long long), kStatStripes, s));
    OWLMI_HIP(hipEventRecord(ev_a_, s));
    ListCapacities::dispatch(cap, [&](auto c) { launch_lane<decltype(c)::value>(a, subtrees, s); });
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipEventRecord(ev_b_, s));
    // hostCode.cpp:310-330: the host decides about another round from the result state
    fetch_stat_stripes(s);
    OWLMI_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 7; i++) {
      h_counters_[i] = 0;
      for (int j = 0; j < kStatStripes; j++) h_counters_[i] += h_counters_[kHostStripes + j * kStatStride + i];
    }
    float ms = 0;
    OWLMI_HIP(hipEventElapsedTime(&ms, ev_a_, ev_b_));
    total_ms += ms;
    if (h_counters_[0] == 0) break;
    if (rounds >= sa.max_rounds && sa.allow_unfinished) break;
    {
      // counters [5], [6] accumulate over rounds: this round's share is the difference
      const double c1 = (double)(h_counters_[5] - c1_before), c2 = (double)(h_counters_[6] - c2_before);
      c1_before = h_counters_[5];
      c2_before = h_counters_[6];
      predicted_candidates = (c1 > 0 ? c2 / c1 : 0.0) * growth;
    }
    radius *= 2;  // hostCode.cpp:321 (fp32)
  }
  if (info) {
    info->rounds = rounds;
    info->final_radius = radius;
    info->node_tests = (int64_t)h_counters_[1];
    info->point_tests = (int64_t)h_counters_[2];
    info->total_intersections = (int64_t)h_counters_[3];
    info->total_active_rounds = (int64_t)h_counters_[4];
    info->solve_ms = total_ms;
    info->dominant_kernel_ms = total_ms / std::max(launches, 1);
    info->dominant_kernel_launches = launches;
    info->kernel_used = TKNN_KERNEL_LANE;
    info->list_capacity = cap;
    info->unfinished = (int64_t)h_counters_[0];
  }
}

int64_t Engine::repair_exact(int k, const int32_t *d_levels, int32_t *d_idx, float *d_dist, hipStream_t s) {
  RepairArgs a;
  a.bvh = bvh_.view();
  a.halo = halo_view();
  a.k = k;
  a.levels = d_levels;
  a.idx = d_idx;
  a.dist = d_dist;
  a.counters = counters_;
  OWLMI_HIP(hipMemsetAsync(counters_, 0, sizeof(unsigned long long), s));
  ListCapacities::dispatch(list_capacity_for(k), [&](auto c) { launch_repair<decltype(c)::value>(a, s); });
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipMemcpyAsync(h_counters_, counters_, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  return (int64_t)h_counters_[0];
}

// tknnSolveOptions.phase == 3: per sorted slot, 1 for the queries an earlier call left unfinished (level -1 at their row)
__global__ void __launch_bounds__(256) unfinished_mask_kernel(const int32_t *levels, const int32_t *prim_id, int64_t n, uint8_t *mask) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) mask[t] = levels[prim_id[t]] < 0 ? 1 : 0;
}

void Engine::solve(const SolveArgs &sa, int kernel, tknnSolveInfo *info, hipStream_t s) {
  // 64 < k <= TKNN_MAX_K: the team walk with the lists in memory, rows final (three-word keys: no tie pass)
  const bool bigk = bigk_supports(sa.k);
  if (bigk) {
    if (kernel != TKNN_KERNEL_AUTO && kernel != TKNN_KERNEL_TEAM)
      throw ArgError{TKNN_E_UNSUPPORTED, "the lane and wave kernels keep their lists in registers: k <= 64 (k up to TKNN_MAX_K: TKNN_KERNEL_AUTO or TKNN_KERNEL_TEAM)"};
  } else {
    if (kernel == TKNN_KERNEL_TEAM && !team_kernel_supports(sa.k))
      throw ArgError{TKNN_E_UNSUPPORTED, "the team kernels hold up to four neighbours per lane of a 16-lane team: k <= 64"};
    if (kernel == TKNN_KERNEL_AUTO) {
      // team kernels for every k the engine takes (<= 64): they hand what it cannot hold (outliers, dense duplicates, start radii
      // far too large) to lane rounds or the wave kernel by itself; measured fastest from r0 = 2e-5 to
      // r0 = 0.04 on 10 M uniform points and on the clustered sets of profiles/
      if (team_kernel_supports(sa.k))
        kernel = TKNN_KERNEL_TEAM;
      else
        kernel = wave_kernel_available() ? TKNN_KERNEL_WAVE : TKNN_KERNEL_LANE;
    }
  }
  // per-query start radii and phases: the team kernels only (solve_team takes n < 2^28)
  const bool team = bigk || (kernel == TKNN_KERNEL_TEAM && bvh_.size() < (1ll << 28));
  if (sa.d_start_radii && !team)
    throw ArgError{TKNN_E_UNSUPPORTED, "tknnSolveEx: per-query start radii are served by the team kernels only (k <= 64)"};
  if (sa.d_start_radii && halo_count() > 0)
    throw ArgError{TKNN_E_UNSUPPORTED, "tknnSolveEx: per-query start radii and a halo tree do not combine (the halo is exchanged for ONE radius)"};
  if (sa.phase != 0) {
    if (!team)
      throw ArgError{TKNN_E_UNSUPPORTED, "tknnSolveEx: phases (interior / boundary / unfinished queries) are served by the team kernels only"};
    if (sa.phase == 3) {
      // the queries an earlier call (allow_unfinished) left without a row: d_levels[row] < 0, marked per sorted slot
      if (!sa.d_levels) throw ArgError{TKNN_E_ARG, "tknnSolveEx: phase 3 (unfinished queries only) needs the d_levels of the call that left them"};
      const int64_t n = bvh_.size();
      hipLaunchKernelGGL(unfinished_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sa.d_levels, bvh_.view().prim_id, n, boundary_);
      OWLMI_HIP(hipGetLastError());
      boundary_valid_ = false;  // (the marks of the last tknnHaloSelect are gone)
    } else if (!boundary_valid_) {
      throw ArgError{TKNN_E_STATE, "tknnSolveEx: phase 1 / 2 need a tknnHaloSelect count pass since the last build (it marks the boundary queries)"};
    }
  }
  struct HaloOff {  // phase 1 runs beside tknnSetHalo: it must not look at the halo tree
    bool &flag;
    explicit HaloOff(bool &f, bool on) : flag(f) { flag = on; }
    ~HaloOff() { flag = false; }
  } halo_off(ignore_halo_, sa.phase == 1);
  if (bigk) {
    solve_bigk(sa, info, s);
    return;
  }
  // Rows whose order depends on how bit-identical fp32 distances are ordered: every kernel lists by
  // (dist, index) and flags them in tie_; fix_ties redoes them in the reference's order, by the round in
  // which each neighbour was first a candidate (deviceCode.cu:77-85 -- lists persist over rounds).
  tknnSolveInfo mine;
  std::memset(&mine, 0, sizeof mine);
  bool solved = false;
  ties_early_ = false;
  if (kernel == TKNN_KERNEL_TEAM) {
    solved = solve_team(sa, &mine, s);  // (resets tie_ and the tie counters together with its own state, one launch)
    if (!solved) kernel = TKNN_KERNEL_WAVE;  // n >= 2^28
  }
  if (!solved) {
    OWLMI_HIP(hipMemsetAsync(tie_, 0, (size_t)bvh_.size(), s));
    OWLMI_HIP(hipMemsetAsync(counters_ + kTieCounter, 0, 3 * sizeof(unsigned long long), s));
    if (kernel == TKNN_KERNEL_WAVE)
      solve_wave(sa, &mine, s);
    else
      solve_lane(sa, &mine, s);
  }
  fix_ties(sa, &mine, s);
  if (info) *info = mine;
}

}  // namespace owlmi
