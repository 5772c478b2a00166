// trueknn_engine.h -- host-side engine object behind include/owlknn.h
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "knn_device.h"
#include "lbvh.h"
#include "owlknn.h"
#include "owlknn_batch.h"
#include "owlknn_debug.h"
#include "owlknn_emst.h"
#include "owlknn_fpfh.h"
#include "owlknn_fps.h"
#include "owlknn_global.h"
#include "owlknn_hdbscan.h"
#include "owlknn_icp.h"
#include "owlknn_knn.h"
#include "owlknn_meanshift.h"
#include "owlknn_nms.h"
#include "owlknn_orient.h"
#include "owlknn_pca.h"
#include "owlknn_periodic.h"
#include "owlknn_plane.h"
#include "owlknn_reduce.h"
#include "owlknn_voxel.h"

namespace owlmi {

struct TeamArgs;  // team_args.h: the team kernels' argument block

struct RoundsExceeded {};
struct ArgError {
  int code;
  std::string what;
};

struct SolveArgs {
  int k = 0;
  float start_radius = 0;
  int max_rounds = 64;
  int32_t *d_idx = nullptr;
  float *d_dist = nullptr;
  int64_t *d_isect = nullptr;
  tknnNeigh *d_fb = nullptr;
  int32_t *d_levels = nullptr;
  bool allow_unfinished = false;
  const float *d_start_radii = nullptr;  // tknnSolveOptions.d_start_radii: per row, or null (one start radius for all)
  int phase = 0;  // tknnSolveOptions.phase: 0 every query, 1 interior queries in the own tree only, 2 boundary queries
};

// tknnSolveOptions.max_rounds and tknnQueryOptions.max_rounds as the solves take them: 64 where the caller gives none, and
// at most 127 (more doublings than fp32 has binades for a radius; the tie flags keep the level in seven bits)
inline int resolve_max_rounds(int asked) { return asked > 0 ? (asked < 127 ? asked : 127) : 64; }

template <int... C>
struct CapacityTable {
  // smallest capacity >= k, or -1
  static constexpr int smallest_for(int k) {
    int cap = -1;
    (void)((k <= C ? (cap = C, true) : false) || ...);
    return cap;
  }
  // f(std::integral_constant<int, cap>{}): cap as a compile-time constant; one not in the table takes 64
  template <class F>
  static void dispatch(int cap, F &&f) {
    if (!((cap == C ? (f(std::integral_constant<int, C>{}), true) : false) || ...)) f(std::integral_constant<int, 64>{});
  }
};
// the register-list capacities the lane, wave and repair kernels are instantiated for
using ListCapacities = CapacityTable<1, 2, 4, 5, 8, 10, 16, 24, 32, 64>;

// smallest register-list capacity instantiated for k, or -1
inline int list_capacity_for(int k) { return ListCapacities::smallest_for(k); }

// counters_ words [1] .. [9] as the team and wave kernels leave them (TeamArgs::counters, WaveArgs::counters)
struct KernelStats {
  unsigned long long rounds = 0;         // [1] max levels
  unsigned long long node_tests = 0;     // [2]
  unsigned long long point_tests = 0;    // [3]
  unsigned long long intersections = 0;  // [4] sum of the finished rows' intersections
  unsigned long long flags = 0;          // [5] error flags: 1 max_rounds, 2 (wave kernel) LDS stack exhausted
  unsigned long long active_rounds = 0;  // [6] sum of levels
  unsigned long long unfinished = 0;     // [7]
  unsigned long long handed_over = 0;    // [8] packet kernel: handed over; walks: stack exhausted (state untouched)
  unsigned long long first_handover_level = 0;  // [9] packet kernel: min hand-over level
  static KernelStats from_words(const unsigned long long *w) {
    KernelStats st;
    st.rounds = w[1];
    st.node_tests = w[2];
    st.point_tests = w[3];
    st.intersections = w[4];
    st.flags = w[5];
    st.active_rounds = w[6];
    st.unfinished = w[7];
    st.handed_over = w[8];
    st.first_handover_level = w[9];
    return st;
  }
};

// the radius of level `rounds - 1`: start_radius doubled in fp32 (hostCode.cpp:321)
inline float final_radius(float start_radius, int rounds) {
  float radius = start_radius;
  for (int t = 1; t < rounds; t++) radius *= 2;
  return radius;
}
// the info of one kernel launch (the tie fields: fix_ties)
tknnSolveInfo solve_info(const KernelStats &st, float start_radius, int kernel, int list_capacity, float ms);
// folds the info of a tail (the queries another launch handed over) into the solve's: the larger round count and
// its radius, work, time and unfinished queries summed; launches only with `count_launches`
void merge_tail(tknnSolveInfo &into, const tknnSolveInfo &tail, float start_radius, bool count_launches);

// dbscan_label.hip: out[seg[i]] = min(out[seg[i]], val[i]) for seg[i] >= 0 (tknnSegmentMin)
void db_segment_min(const int32_t *d_seg, const int64_t *d_val, int64_t n, int64_t *d_out, hipStream_t s);

// test hook: the wave kernel's exact candidate thresholds for (q, r) pairs (trueknn_wave.hip)
void debug_thresholds(const float *d_q, const float *d_r, int64_t n, float *d_lo, float *d_hi, hipStream_t s);

// test hook (tknnDebugTeamLanes, include/owlknn_debug.h): one team helper on caller-supplied lanes (debug_lanes.hip).  The words
// per lane that `op` with `variant` takes and returns, false if the op has no such variant or there is no such op
bool debug_team_lanes_words(int op, int variant, int *win, int *wout);
void debug_team_lanes(int op, int variant, const uint32_t *d_in, uint32_t *d_out, int64_t teams, hipStream_t s);

class Engine {
 public:
  Engine();
  ~Engine();
  Engine(const Engine &) = delete;
  Engine &operator=(const Engine &) = delete;

  // d_batch, batch_bits: build_batched's (Lbvh::build_from_points); every build through here leaves a plain tree behind
  void build(const float *d_xyz, const int32_t *d_ids, int64_t n, tknnBuildInfo *info, hipStream_t s, const int32_t *d_batch = nullptr,
             int batch_bits = 0);
  // batch_knn.hip: a tree over num_batches labelled clouds, each one range of sorted slots (tknnBuildBatched); the labels are
  // checked on the device first, one outside [0, num_batches) is an ArgError that leaves the engine without a tree
  void build_batched(const float *d_xyz, const int32_t *d_ids, const int32_t *d_batch, int32_t num_batches, int64_t n, tknnBuildInfo *info,
                     hipStream_t s);
  // batch_knn.hip: the batches' ranges of sorted slots, num_batches + 1 words copied to d_starts (device; may be null)
  void batch_layout(int32_t *num_batches, int32_t *key_bits, int32_t *d_starts, hipStream_t s);
  void set_halo(const float *d_xyz, const int32_t *d_ids, int64_t m, hipStream_t s);
  LbvhView halo_view() const;
  // halo_select.hip: my points inside any box of each peer, as 16-byte wire rows (count pass: d_rows == nullptr)
  // (d_caps: the one-pass form -- rows into segments of those capacities, exact counts out, what does not fit dropped)
  void halo_select(const float *d_boxes, const int32_t *d_box_peer, int32_t nboxes, int32_t npeers, int64_t *d_counts,
                   const int64_t *d_offsets, float *d_rows, hipStream_t s, const int64_t *d_caps = nullptr);
  double expected_box_population(float radius) const;
  void solve(const SolveArgs &sa, int kernel, tknnSolveInfo *info, hipStream_t s);
  // rewrites every finished row with the exact kNN (a walk of the box of half-width d_k); returns how many rows changed
  int64_t repair_exact(int k, const int32_t *d_levels, int32_t *d_idx, float *d_dist, hipStream_t s);
  // dbscan.hip; with core_label (per row: the label the caller gave each core point, < 0 for others) only
  // the assignment runs: core points keep their label, others take the smallest among their core neighbours
  void dbscan(float eps, int min_pts, int32_t *d_labels, uint8_t *d_core, int32_t *d_counts, tknnDbscanInfo *info,
              hipStream_t s, const int32_t *core_label = nullptr);
  // dbscan.hip: labels (and neighbour counts) for m points that are not in the tree (tknnDbscanQuery); m > 0
  void dbscan_query(float eps, const float *d_queries, int64_t m, const int32_t *core_label, int32_t *d_labels, int32_t *d_counts,
                    tknnDbscanInfo *info, hipStream_t s);
  // "eps auto-grown" (BASELINE config 5; spec: oracle/dbscan_oracle.c dbref_dbscan_auto)
  int64_t dbscan_noise(float eps, int min_pts, uint8_t *d_noise, hipStream_t s);  // tknnDbscanNoise
  void db_read_stats(hipStream_t s);
  void dbscan_auto(float eps0, int min_pts, double max_noise, int max_rounds, int32_t *d_labels, uint8_t *d_core,
                   tknnDbscanAutoInfo *info, hipStream_t s);
  // The three calls below take the caller's options record as tknn_api.hip has validated it (m > 0 among the rest).
  // trueknn_query.hip: TrueKNN rows for m points that are not in the tree (tknnQuery); per-slot solve state is not touched
  void query(const tknnQueryOptions &o, tknnSolveInfo *info, hipStream_t s);
  // radius_query.hip: the points within a radius of m points that are not in the tree, as CSR rows (tknnRadiusQuery); m > 0
  void radius_query(const tknnRadiusOptions &o, tknnRadiusInfo *info, hipStream_t s);
  // radius_knn.hip: at most k nearest points within a radius of m points that are not in the tree, as dense rows (tknnRadiusKnn); m > 0
  void radius_knn(const tknnRadiusKnnOptions &o, tknnRadiusKnnInfo *info, hipStream_t s);
  // knn_seed.hip: the k nearest points, exactly, of m points that are not in the tree or (d_queries null) of the tree's own points,
  // with no radius from the caller (tknnKnn); m > 0
  void knn(const tknnKnnOptions &o, tknnKnnInfo *info, hipStream_t s);
  // periodic_knn.hip: at most k nearest points under a per-axis periodic metric, with or without a radius, of m points that are
  // not in the tree or (d_queries null) of the tree's own points (tknnPeriodicKnn); m > 0
  void periodic_knn(const tknnPeriodicKnnOptions &o, tknnPeriodicKnnInfo *info, hipStream_t s);
  // batch_knn.hip: at most k nearest points of the query's own batch, with or without a radius, of m labelled points that are
  // not in the tree or (d_queries null) of the tree's own points (tknnBatchKnn); m > 0, the tree a batched one
  void batch_knn(const tknnBatchKnnOptions &o, tknnBatchKnnInfo *info, hipStream_t s);
  // emst.hip: the minimum spanning forest of the tree's own points, Euclidean or under the caller's core distances, in Boruvka
  // rounds (tknnEmst); throws RoundsExceeded, with info filled and nothing written, when max_rounds rounds do not finish it
  void emst(const tknnEmstOptions &o, tknnEmstInfo *info, hipStream_t s);
  // linkage.hip: the single-linkage dendrogram of a sorted forest, in contraction rounds (tknnLinkage); needs no tree
  void linkage(const tknnLinkageOptions &o, tknnLinkageInfo *info, hipStream_t s);
  // hdbscan.hip: HDBSCAN's labels of a sorted forest (tknnHdbscanLabels; needs no tree), and the pipeline on the built set: knn for
  // the core distances, emst under them, the labels of its records (tknnHdbscan)
  void hdbscan_labels(const tknnHdbscanLabelsOptions &o, tknnHdbscanLabelsInfo *info, hipStream_t s);
  void hdbscan(const tknnHdbscanOptions &o, tknnHdbscanInfo *info, hipStream_t s);
  // fps.hip: farthest point sampling inside each cloud of the tree -- the batches of a batched tree, one cloud otherwise --,
  // one workgroup per cloud, pruned by the box pyramid (tknnFps); the tree a point tree
  void fps(const tknnFpsOptions &o, tknnFpsInfo *info, hipStream_t s);
  // nms.hip: greedy suppression within a radius inside each cloud of the tree, in rounds of early-exit walks (tknnRadiusNms); the
  // tree a point tree.  An ArgError of TKNN_E_STATE, with info->rounds set and no output written, when max_rounds do not finish it
  void radius_nms(const tknnRadiusNmsOptions &o, tknnRadiusNmsInfo *info, hipStream_t s);
  // radius_reduce.hip: counts, weight sums and weighted value sums over the points within a radius of m points that are not in the
  // tree or (d_queries null) of the tree's own points, no lists written (tknnRadiusReduce); m > 0, the tree a point tree
  void radius_reduce(const tknnRadiusReduceOptions &o, tknnRadiusReduceInfo *info, hipStream_t s);
  // local_pca.hip: count, centroid, covariance, eigenvalues, eigenvectors, normal and surface variation of the neighbourhood -- a
  // radius row, a kNN row or both -- of m points that are not in the tree or (d_queries null) of the tree's own points, no lists
  // written (tknnLocalPca); m > 0, the tree a point tree
  void local_pca(const tknnLocalPcaOptions &o, tknnLocalPcaInfo *info, hipStream_t s);
  // icp.hip: rigid registration of m source points to the tree's points by iterated closest points -- tknnKnn's search at k = 1
  // clipped to max_dist, fp64 moments of the pairs, the step solved on the host (icp_solve.h) -- with no list leaving the call
  // (tknnIcp); m > 0, the tree a point tree without ids
  void icp(const tknnIcpOptions &o, tknnIcpInfo *info, hipStream_t s);
  // mean_shift.hip: every seed -- m points that are not in the tree, or (d_seeds null) the tree's own points -- moved to the
  // kernel-weighted mean of the points within a radius of it until it stops, the loop and its shrinking work list on the device
  // (tknnMeanShift); m > 0, the tree a point tree
  void mean_shift(const tknnMeanShiftOptions &o, tknnMeanShiftInfo *info, hipStream_t s);
  // fpfh.hip: the 33-bin point-feature histogram of each of the tree's own points from the caller's normals -- a walk that bins
  // the pair features of every neighbour within the radius, a second that sums the neighbours' histograms by 1 / d^2 --, no
  // lists written (tknnFpfh); n > 0, the tree a point tree
  void fpfh(const tknnFpfhOptions &o, tknnFpfhInfo *info, hipStream_t s);
  // feature_match.hip: the nearest and second-nearest target row of m source rows in D <= 64 dimensions, dense brute force through
  // registers and LDS (tknnFeatureMatch); m > 0, needs no tree
  void feature_match(const tknnFeatureMatchOptions &o, tknnFeatureMatchInfo *info, hipStream_t s);
  // ransac.hip: RANSAC over c correspondences in batches of trials -- sample, edge check, solve (icp_solve.h on the device), score
  // against every record, stop by confidence, refit -- (tknnRansac); needs no tree.  An ArgError of TKNN_E_ARG, with nothing the
  // caller can see written, when a pair names a row out of range
  void ransac(const tknnRansacOptions &o, tknnRansacInfo *info, hipStream_t s);
  // voxel_grid.hip: one point per occupied grid cell of every cloud -- a cell key per row, a stable radix sort, head flags and a
  // scan, fp64 sums per voxel by a lane or by a wave -- (tknnVoxelGrid); needs no tree.  An ArgError of TKNN_E_ARG, with nothing
  // the caller can see written, when the voxels outnumber the capacity
  void voxel_grid(const tknnVoxelGridOptions &o, tknnVoxelGridInfo *info, hipStream_t s);
  // orient.hip: one sign per normal, agreed along the minimum spanning forest of the kNN graph (and the EMST's records) weighted
  // by 1 - |n_i . n_j| -- knn and emst, one sort of the candidates by the strict key, Boruvka rounds over the ranked list with the
  // sign parity carried through the merges -- (tknnOrientNormals); the tree a point tree.  Throws RoundsExceeded, with nothing
  // written, info included, when max_rounds rounds do not finish it
  void orient_normals(const tknnOrientOptions &o, tknnOrientInfo *info, hipStream_t s);
  // plane.hip: the plane most active rows of the built set lie within a distance of, by RANSAC in batches of trials -- the active
  // list and its prefixes, a lane per trial for the planes, a wave per plane walking the box pyramid with the slab as its query (or
  // sweeping every row: the fallback), stop by confidence, refit by the inliers' fp64 moments (plane_solve.h) -- (tknnSegmentPlane);
  // the tree a point tree without ids
  void segment_plane(const tknnPlaneOptions &o, tknnPlaneInfo *info, hipStream_t s);
  // The top of every call (tknn_api.hip): a DBSCAN call that threw between its side launch and its rejoin has left
  // db_border_walk_kernel running on the workspace and the counters; `s` waits for it before the call touches either.
  void join_side(hipStream_t s);
  // test hook (tknnDebugPoison, include/owlknn_debug.h): fills the scratch named in `what` with `byte`; returns the bytes filled
  int64_t debug_poison(unsigned what, int byte, size_t min_workspace_bytes, hipStream_t s);
  bool batched() const { return bvh_.built() && num_batches_ > 0; }
  int32_t num_clouds() const { return batched() ? num_batches_ : 1; }  // the clouds tknnFps samples
  bool has_halo() const { return halo_n_ > 0; }
  bool ids_given() const { return ids_given_; }  // the tree names its points by the caller's ids, not by row
  bool built() const { return bvh_.built(); }
  int device() const { return device_; }
  int64_t size() const { return bvh_.size(); }
  const float *scene() const { return scene_; }  // lo xyz, hi xyz of the built set, NaN points ignored (host copy)
  const Lbvh &tree() const { return bvh_; }
  const Lbvh &halo_tree() const { return halo_; }  // meaningful while has_halo()

 private:
  struct DbCall;  // db_call.h: one RT-DBSCAN call -- its knobs, its kernels' argument block and its launches, in steps
  void solve_lane(const SolveArgs &sa, tknnSolveInfo *info, hipStream_t s);
  // lane rounds over the queries another kernel left with done_[slot] == 0, each from next_level_[slot]
  void continue_lane(const SolveArgs &sa, int first_level, tknnSolveInfo *info, hipStream_t s);
  void lane_rounds(const SolveArgs &sa, int first_level, bool fresh, tknnSolveInfo *info, hipStream_t s);
  void solve_wave(const SolveArgs &sa, tknnSolveInfo *info, hipStream_t s, bool only_unfinished = false);  // trueknn_wave.hip
  static bool wave_kernel_available();                                        // trueknn_wave.hip
  // trueknn_team.hip; returns false if a packet needed more leaf blocks than the kernel can name
  bool solve_team(const SolveArgs &sa, tknnSolveInfo *info, hipStream_t s);
  static bool team_kernel_supports(int k);
  // trueknn_bigk.hip: 64 < k <= TKNN_MAX_K, the lists in memory (bigk_walk_kernel)
  static bool bigk_supports(int k);
  void solve_bigk(const SolveArgs &sa, tknnSolveInfo *info, hipStream_t s);
  // trueknn_tail.hip: redo the rows flagged in tie_ with the reference's order of exact-distance ties
  void fix_ties(const SolveArgs &sa, tknnSolveInfo *info, hipStream_t s);
  // trueknn_tail.hip: the team kernels' end-of-wave statistics, striped (kStatBase)
  void reset_stat_stripes(hipStream_t s);
  void fetch_stat_stripes(hipStream_t s);
  KernelStats fold_stat_stripes(bool with_min) const;
  // trueknn_tail.hip: a solve from level 0 without the packet kernel's prep launch (levels: preset to -1 if not null)
  void reset_solve_state(int32_t *levels, hipStream_t s);
  // trueknn_tail.hip: a zeroed TeamArgs (the team kernels' argument block) with the fields every team launch reads ...
  TeamArgs team_args(const SolveArgs &sa) const;
  // ... and the fields only the solves read (team_kernel, team_walk_kernel, bigk_walk_kernel; not tie_fix_kernel)
  void set_solve_args(TeamArgs &a, const SolveArgs &sa) const;
  // trueknn_tail.hip: team_walk_kernel over nslots sorted slots (slots null: every slot), lane rounds for what outgrew its stack
  tknnSolveInfo walk(const SolveArgs &sa, TeamArgs a, int nreg, const int32_t *slots, int32_t nslots, int lane_level,
                     bool count_lane_launches, hipStream_t s);
  // trueknn_tail.hip: the sorted slots that were handed over (done_[slot] == 0) or, with `ties`, flagged in tie_, ascending,
  // into slot_list_; returns their count's device address
  int32_t *compact_slots(bool ties, hipStream_t s);
  void launch_tie_fix(const SolveArgs &sa, const int32_t *slots, int32_t nslots, int blocks, hipStream_t s,
                      const int32_t *d_slot_count = nullptr, int64_t expected_rows = 0);
  int first_step_estimate(const SolveArgs &sa) const;
  // wave_ws_ / slot_list_ (n slots + their count) grown to at least this size; a failed allocation leaves them empty
  void *workspace(size_t bytes);
  int32_t *slot_list(int64_t n);
  float scene_[6] = {0, 0, 0, 0, 0, 0};  // bounds of the built point set (host copy)

  int device_ = 0;
  int cu_count_ = 0;  // compute units of device_ (the launches size their grids by it)
  Lbvh bvh_;
  // the last build was given ids (tknnBuildIds with d_ids): neighbour lists then name points by id, not by input row
  bool ids_given_ = false;
  // the last build was build_batched: the batches, the bits their labels take at the top of the keys, and the first sorted
  // slot of each (num_batches_ + 1 words on the device; the last: the points without a NaN).  0 batches: a plain tree.
  int32_t num_batches_ = 0;
  int batch_bits_ = 0;
  int32_t *batch_starts_ = nullptr;
  int64_t batch_starts_cap_ = 0;
  Lbvh halo_;
  int64_t halo_n_ = 0;
  // A phase-1 solve (queries no halo point can reach) runs beside the halo exchange: tknnSetHalo may rebuild
  // halo_ on another host thread meanwhile, so that solve never looks at it.
  bool ignore_halo_ = false;
  int64_t halo_count() const { return ignore_halo_ ? 0 : halo_n_; }
  uint8_t *boundary_ = nullptr;  // per sorted slot: 1 if the last tknnHaloSelect count pass found the point inside a peer's box
  bool boundary_valid_ = false;
  uint8_t *done_ = nullptr;
  int64_t *isect_sorted_ = nullptr;
  int32_t *next_level_ = nullptr;
  int32_t *tie_list_ = nullptr;  // the first kTieListCap flagged slots, in the order the kernels met them
  uint8_t *tie_ = nullptr;  // per sorted slot: 0, or 1 + the level at which the query finished with exact-distance ties in reach of its row
  int64_t state_cap_ = 0;
  // counters_: kCounterWords words, h_counters_: the host's copy (the layouts of both: knn_device.h)
  unsigned long long *counters_ = nullptr, *h_counters_ = nullptr;
  void *wave_ws_ = nullptr;
  size_t wave_ws_bytes_ = 0;
  int db_union_resident_ = 0;     // workgroups of db_group_union_kernel this engine's device holds at once (0: not asked yet)
  bool wave_force_redo_ = false;  // TKNN_WAVE_FORCE_REDO (tests): treat every wave-kernel solve as if its LDS stack had overflowed
  int wave_leaf_max_ = 16;  // subtrees of at most this many points are streamed as one range (TKNN_LEAF_MAX)
  int32_t *slot_list_ = nullptr;  // compact list of the sorted slots the team kernel handed over (+ its length)
  int64_t slot_list_cap_ = 0;
  unsigned long long *halo_mask_ = nullptr;  // per leaf block: peers it may have points for (+ 64 cursors)
  int64_t halo_mask_cap_ = 0;
  static size_t halo_mask_bytes(int64_t blocks);  // halo_select.hip: what halo_mask_ takes for that many leaf blocks
  hipEvent_t ev_a_ = nullptr, ev_b_ = nullptr, ev_c_ = nullptr, ev_d_ = nullptr, ev_e_ = nullptr, ev_f_ = nullptr;
  // dbscan(): the walks of the points that are not core run beside the group unions on a stream of their own
  hipStream_t db_side_ = nullptr;
  hipEvent_t ev_side_a_ = nullptr, ev_side_b_ = nullptr;
  bool db_side_pending_ = false;  // a side launch was recorded in ev_side_b_ and no stream has been made to wait for it yet
  hipEvent_t ev_g_ = nullptr, ev_h_ = nullptr;  // dbscan(): around what runs between the two union launches
  // the packet kernel's solve launches the tie pass behind itself, before its one host round trip: set if
  // that launch has seen every flagged row (no tail ran, the list held them all)
  bool ties_early_ = false;
  int64_t early_tie_rows_ = 0, early_tie_left_ = 0;
  float early_tie_ms_ = 0;
};

}  // namespace owlmi
