// radius_knn_walk.h -- the walk of radius_knn.hip as its two callers launch it: tknnRadiusKnn (radius_knn.hip) with the caller's
// radii, tknnKnn (knn_seed.hip) with the bounds its seed kernel found.  The kernels themselves are in radius_knn.hip, once.
// The counter words, the gate, the statistics and the k-th distance below also serve the periodic walk (periodic_knn.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knn_thresholds.h"  // knn_gate_from_worst
#include "owl/lbvh_device.h"
#include "team_lanes.h"  // t_lane_read, t_wave_sum

namespace owlmi {

// words of a call's own counters (in the workspace, zeroed per call); the last two are tknnKnn's
enum {
  kRknnWsCursor = 0,
  kRknnWsRedo = 1,
  kRknnWsTotal = 2,
  kRknnWsFullRows = 3,
  kRknnWsNodeTests = 4,
  kRknnWsPointTests = 5,
  kRknnWsTightened = 6,  // full rows whose k-th distance ended below their radius
  kRknnWsSeedTests = 7,  // knn_seed_kernel's point tests
  kRknnWsWords = 8
};

struct RadiusKnnKernelArgs {
  LbvhView bvh;
  LbvhWideView wide;
  const float *queries;     // m packed triples, by query index
  const uint32_t *order;    // m: the query worked on at sorted position i (null: query i)
  int32_t m;
  int k;
  float radius;             // every row's radius if radii is null
  const float *radii;       // m, by query index (may be null)
  const int32_t *skip_ids;  // m, by query index (may be null)
  const int32_t *out_row;   // m: the row of the output a query's answer goes to (null: the query's own index)
  int force_redo;           // TKNN_RADIUS_KNN_FORCE_FALLBACK / TKNN_KNN_FORCE_FALLBACK (tests): the walk leaves every query to the lane kernel
  int zero_radius_ok;       // a radius of 0 is a row's radius like any other (tknnKnn: k duplicates of the query); else such a row is empty
  int32_t *out_idx;         // m*k
  float *out_dist;          // m*k (may be null)
  int32_t *out_counts;      // m (may be null)
  int32_t *redo;            // m: queries left to the lane kernel
  unsigned long long *ws;   // kRknnWsWords counters
};

// radius_knn.hip: radius_knn_walk_kernel over the m queries of `a`, then radius_knn_lane_kernel over what the walk left; one host
// sync before the caller's last -- the redo list's length, which is returned.  h_words: kRknnWsWords words of pinned host
// memory, the counters as they stand once the stream has been synchronised again.
unsigned long long radius_knn_walks(const RadiusKnnKernelArgs &a, int cu_count, unsigned long long *h_words, hipStream_t s);

namespace {

// The gate of a list whose k-th entry lies at distance `kth` (FLT_MAX: fewer than k entries, the gate stays the radius's).  A
// candidate beyond it is farther than r or farther than the k-th entry; one AT the k-th distance passes, the index decides.
__device__ __forceinline__ float rknn_gate(float gate_r, float kth) { return fminf(gate_r, knn_gate_from_worst(kth)); }

__device__ __forceinline__ void rknn_add_stats(unsigned long long *ws, int lane, unsigned long long total, unsigned long long full_rows,
                                               unsigned long long node_tests, unsigned long long point_tests, unsigned long long tightened) {
  const unsigned long long tsum = t_wave_sum(total), fsum = t_wave_sum(full_rows), nt = t_wave_sum(node_tests), pt = t_wave_sum(point_tests),
                           tight = t_wave_sum(tightened);
  if (lane == 0) {
    if (tsum) atomicAdd(&ws[kRknnWsTotal], tsum);
    if (fsum) atomicAdd(&ws[kRknnWsFullRows], fsum);
    if (nt) atomicAdd(&ws[kRknnWsNodeTests], nt);
    if (pt) atomicAdd(&ws[kRknnWsPointTests], pt);
    if (tight) atomicAdd(&ws[kRknnWsTightened], tight);
  }
}

// t_kth_dist (team_walk.h) with the register picked by masks instead of a chain of selects: the compiler turns that chain into a load
// through a selected address, which keeps registers 1 .. NREG - 1 of the list in scratch (16 / 32 bytes for NREG = 3 / 4 in
// query_walk_kernel); picked this way the list stays in registers for every NREG.
template <int NREG>
__device__ __forceinline__ float rknn_kth_dist(const uint32_t (&bd)[NREG], int k, int team) {
  const uint32_t sel = (uint32_t)(k - 1) >> 4;
  uint32_t reg = 0u;
#pragma unroll
  for (int j = 0; j < NREG; j++) reg |= bd[j] & (0u - (uint32_t)(sel == (uint32_t)j));
  return __uint_as_float(t_lane_read(reg, (team << 4) + ((k - 1) & 15)));
}

}  // namespace

}  // namespace owlmi
