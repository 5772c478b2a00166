// dbscan.hip -- RT-DBSCAN on the MI355X LBVH.
//
// The reference tree has no RT-DBSCAN source (samples/s02-rtdbscan is absent); its README only
// says distance computations go to the RT cores and "other clustering operations" to shader
// cores.  The spec implemented here is written down in oracle/dbscan_oracle.c (neighbourhood
// includes the point, fp32 distance arithmetic of the TrueKNN intersection program, clusters
// numbered by ascending smallest core index, border -> lowest adjacent cluster) and equals
// sklearn.cluster.DBSCAN wherever no pair sits within rounding of eps.
//
// Same machinery as TrueKNN: points are primitives with box c +- eps (deviceCode.cu:38-56
// pattern), every point is also a query, the "intersection program" does the true sphere test.
// Three traversal launches over the point LBVH (one query per lane, stackless ropes: lane_walk.h has the walk and
// the node tests, the kernels here say what happens at a node and at a point):
//   1. core flags: count neighbours, stop at minPts unless counts were asked for
//   2. union: every core point unites with each core neighbour of smaller index (lock-free
//      union-find; the smaller index stays root, so a root is its cluster's smallest core index)
//   3. labels: roots ranked by an exclusive scan; border points take the smallest adjacent root
// TIGHT NODES keep step 2 from costing O(n x neighbours) in dense sets (BASELINE config 3: 5 000
// neighbours per point).  A tree node whose box diagonal is below eps holds points that are pairwise
// within eps, so its core points are one cluster: every core point unites with the first core point
// of the first tight node on its own root path, and a traversal that meets a tight node settles it
// as a whole -- farthest corner within eps: unite with that representative; nearest face beyond
// eps: nothing; otherwise test its core points one by one until the first within eps.  The
// components, and so the labels, are those of the full neighbour graph.  Step 3 and the full
// neighbour counts use the same node tests (a node inside the sphere is counted, not walked).
// Union-find reads/writes go through agent-scope atomics: a workgroup's L1 (and another XCD's L2)
// would otherwise keep serving a stale parent and a failed CAS could retry forever.
//
// The files: db_device.h   DbArgs (the kernels' argument block) and the device helpers more than one pass uses
//            db_call.h     DbKnobs and Engine::DbCall, one call on the host: each step that launches is defined beside its kernels
//            dbscan_core.hip / dbscan_union.hip / dbscan_label.hip   the kernels of steps 1, 2 and 3 (and what else a call
//                          needs at that stage: next_core and the noise probe; the group list; rows, assign, query, tknnSegmentMin)
//            dbscan.hip    the host side: what a call sets up, the order of its steps, what it reports -- no kernel
#include "db_call.h"
#include "query_order.h"

#include <hipcub/hipcub.hpp>

#include <vector>

namespace owlmi {

// the work counters of the launches so far: the stripes to the host (synchronises the stream), summed into h_counters_'s first words
void Engine::db_read_stats(hipStream_t s) {
  OWLMI_HIP(hipMemcpyAsync(h_counters_ + kHostStripes, counters_ + kDbStats, kDbStripes * kDbStripeWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < kDbStripeWords; i++) {
    unsigned long long sum = 0;
    for (int st = 0; st < kDbStripes; st++) sum += h_counters_[kHostStripes + st * kDbStripeWords + i];
    h_counters_[i] = sum;
  }
}

// what every call sets
Engine::DbCall::DbCall(Engine &engine, int min_pts, hipStream_t stream) : e(engine), s(stream) {
  std::memset(&a, 0, sizeof a);
  a.bvh = e.bvh_.view();
  a.block_paths = knobs.paths ? e.bvh_.block_paths_device() : nullptr;
  a.stats = e.counters_ + kDbStats;  // striped (db_add_stats)
  a.min_pts = min_pts;
  common = a;
  exclusive_sum(nullptr, nullptr, (int)n);  // (no storage yet: the library says how much it wants)
}
void Engine::DbCall::exclusive_sum(const int32_t *in, int32_t *out, int count) {
  OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, in, out, count, s));
}
void Engine::DbCall::reserve(size_t layout_bytes) {
  const size_t scan_at = db_round_up(layout_bytes, kDbScanAlign);
  ws = e.workspace(scan_at + scan_bytes);
  scan_tmp = db_at<void>(ws, scan_at);
}
void Engine::DbCall::set_eps(float eps) {
  a.eps = eps, a.eps_wide = eps * 1.000001f;
  a.eps_in2 = eps * eps * (1.0f - 1e-5f), a.eps_out2 = eps * eps * (1.0f + 1e-5f);
}
void Engine::DbCall::reset_counters() { OWLMI_HIP(hipMemsetAsync(e.counters_, 0, kCounterWords * sizeof(unsigned long long), s)); }

// a growth round's scratch and arguments (probe_round: dbscan_core.hip)
void Engine::DbCall::probe_setup() {
  const DbProbeWs w = DbProbeWs::of((size_t)n);
  reserve(w.end);
  // (a.parent stays null: no unions here; near_node: where each point's noise probe starts, db_has_core_neighbour)
  a.near_node = db_at<int32_t>(ws, w.near_node), a.rank = db_at<int32_t>(ws, w.pos), a.next_core = next_core = db_at<int32_t>(ws, w.next_core);
  a.core_sorted = db_at<uint8_t>(ws, w.core_sorted), noise = db_at<uint8_t>(ws, w.noise), block_places = db_at<int32_t>(ws, w.block_places);
}

// scratch, arguments, the side stream, a clean start of the stream: everything before the first launch
void Engine::DbCall::cluster_setup(float eps, int32_t *d_labels, uint8_t *d_core, int32_t *d_counts, bool with_side, bool by_point, bool groups_wanted) {
  const DbClusterWs w = DbClusterWs::of((size_t)n, TKNN_DIAG_BUILD != 0);
  reserve(w.end);
  a = common, union_launches = 1, between_passes = false;
  set_eps(eps);
  a.want_counts = d_counts != nullptr, a.diag = knobs.diag;
  a.parent = db_at<int32_t>(ws, w.parent), roots = db_at<int32_t>(ws, w.roots), a.rank = db_at<int32_t>(ws, w.ranks);
  a.next_core = next_core = db_at<int32_t>(ws, w.next_core), a.core_sorted = db_at<uint8_t>(ws, w.core_sorted);
  a.min_row = db_at<int32_t>(ws, w.min_row), not_core = db_at<int32_t>(ws, w.not_core), border_lists = db_at<int32_t>(ws, w.border_lists);
  uni = db_at<int32_t>(ws, w.uni), block_places = db_at<int32_t>(ws, w.block_places);
  if (TKNN_DIAG_BUILD && (a.diag & 512) && groups_wanted) a.pk_diag = db_at<int32_t>(ws, w.pk_diag);
  border_per = std::max(2, a.min_pts), side = with_side, per_point = by_point;
  if (side && !e.db_side_) {
    OWLMI_HIP(hipStreamCreateWithFlags(&e.db_side_, hipStreamNonBlocking));
    OWLMI_HIP(hipEventCreateWithFlags(&e.ev_side_a_, hipEventDisableTiming));
    OWLMI_HIP(hipEventCreateWithFlags(&e.ev_side_b_, hipEventDisableTiming));
  }
  a.core = d_core, a.counts = d_counts, a.labels = d_labels;
  // every point's group, for the union pass; kept in the caller's label array, which is written last
  a.group_of = groups_wanted ? d_labels : nullptr;
  a.diag_out = e.counters_ + kDbDiag;
  reset_counters();
  OWLMI_HIP(hipEventRecord(e.ev_a_, s));
}
// the counters to the host; returns when the stream has run dry
void Engine::DbCall::read_back() {
  OWLMI_HIP(hipMemcpyAsync(e.h_counters_ + kHostDbGroups, e.counters_ + kDbGroups, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipMemcpyAsync(e.h_counters_ + kHostDbOverflows, e.counters_ + kDbOverflows, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipMemcpyAsync(e.h_counters_ + kHostDbNotCore, e.counters_ + kDbNotCore, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  e.db_read_stats(s);
  OWLMI_HIP(hipStreamSynchronize(s));
}
// one clustering from the first launch to the last
void Engine::DbCall::cluster(float eps, int32_t *d_labels, uint8_t *d_core, int32_t *d_counts, bool by_point) {
  cluster_setup(eps, d_labels, d_core, d_counts, knobs.side, by_point, !by_point);
  core_flags();
  build_next_core(false, not_core);
  border_walk();
  per_point ? unions() : group_unions();
  number_clusters();
  labels();
  read_back();
}
// tknnDbscanAssign: the caller's labels decide the core flags; a core point keeps its label, any other point takes the
// smallest among its core neighbours
void Engine::DbCall::assign(float eps, int32_t *d_labels, const int32_t *core_label, tknnDbscanInfo *info) {
  cluster_setup(eps, d_labels, nullptr, nullptr, false, false, false);
  core_from_labels(core_label);
  OWLMI_HIP(hipEventRecord(e.ev_c_, s));
  build_next_core(true, nullptr);
  assign_labels(core_label);
  OWLMI_HIP(hipEventRecord(e.ev_b_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  e.db_read_stats(s);
  if (!info) return;
  float ms = 0;
  OWLMI_HIP(hipEventElapsedTime(&ms, e.ev_a_, e.ev_b_));
  std::memset(info, 0, sizeof *info);
  info->clusters = -1, info->solve_ms = ms, info->label_ms = ms;
  info->node_tests = (int64_t)e.h_counters_[kDbStatLabel];
  info->point_tests = info->label_point_tests = (int64_t)e.h_counters_[kDbStatLabel + 1];
}
// tknnDbscanQuery: the core flags and next_core as assign() makes them, the queries put in order along the tree's curve,
// one traversal for their labels (and counts).  The tree, the solve state and core_label are only read.
void Engine::DbCall::query(float eps, const float *d_queries, int64_t m, const int32_t *core_label, int32_t *d_labels, int32_t *d_counts, tknnDbscanInfo *info) {
  const size_t sort_bytes = query_order_sort_bytes(m, s);
  scan_bytes = std::max(scan_bytes, sort_bytes);  // one after the other in the same place
  const DbQueryWs w = DbQueryWs::of((size_t)n, (size_t)m);
  reserve(w.end);
  a = common;
  set_eps(eps);
  a.rank = db_at<int32_t>(ws, w.pos), a.next_core = next_core = db_at<int32_t>(ws, w.next_core);
  a.core_sorted = db_at<uint8_t>(ws, w.core_sorted), block_places = db_at<int32_t>(ws, w.block_places);
  uint32_t *order = db_at<uint32_t>(ws, w.order);
  reset_counters();
  OWLMI_HIP(hipEventRecord(e.ev_a_, s));
  core_from_labels(core_label);
  build_next_core(true, nullptr);
  OWLMI_HIP(hipGetLastError());
  query_order(d_queries, m, e.bvh_.scene_device(), e.bvh_.curve(), db_at<uint32_t>(ws, w.codes), db_at<uint32_t>(ws, w.codes_sorted),
              db_at<uint32_t>(ws, w.order_in), order, scan_tmp, sort_bytes, s);
  OWLMI_HIP(hipEventRecord(e.ev_c_, s));
  query_labels(d_queries, order, m, core_label, d_labels, d_counts);
  OWLMI_HIP(hipEventRecord(e.ev_b_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  e.db_read_stats(s);
  if (!info) return;
  std::memset(info, 0, sizeof *info);
  info->clusters = -1;
  OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, e.ev_a_, e.ev_b_));
  OWLMI_HIP(hipEventElapsedTime(&info->label_ms, e.ev_c_, e.ev_b_));
  info->node_tests = (int64_t)e.h_counters_[kDbStatLabel];
  info->point_tests = info->label_point_tests = (int64_t)e.h_counters_[kDbStatLabel + 1];
}

void Engine::DbCall::cluster_info(tknnDbscanInfo *info) const {
  const unsigned long long *h = e.h_counters_;
  float ms = 0;
  std::memset(info, 0, sizeof *info);
  OWLMI_HIP(hipEventElapsedTime(&ms, e.ev_a_, e.ev_b_));
  info->clusters = last[0] + last[1];
  info->solve_ms = ms;
  OWLMI_HIP(hipEventElapsedTime(&info->core_ms, e.ev_a_, e.ev_c_));
  OWLMI_HIP(hipEventElapsedTime(&info->union_ms, e.ev_d_, e.ev_e_));
  if (between_passes) {  // union_ms: the two launches of the union kernel
    float between = 0;
    OWLMI_HIP(hipEventElapsedTime(&between, e.ev_g_, e.ev_h_));
    info->union_ms -= between;
  }
  OWLMI_HIP(hipEventElapsedTime(&info->label_ms, e.ev_f_, e.ev_b_));
  info->node_tests = (int64_t)(h[kDbStatCore] + h[kDbStatUnion] + h[kDbStatLabel]);
  info->point_tests = (int64_t)(h[kDbStatCore + 1] + h[kDbStatUnion + 1] + h[kDbStatLabel + 1]);
  info->core_point_tests = (int64_t)h[kDbStatCore + 1];
  info->union_point_tests = (int64_t)h[kDbStatUnion + 1];
  info->label_point_tests = (int64_t)h[kDbStatLabel + 1];
  info->union_launches = union_launches;
  info->union_node_tests = (int64_t)h[kDbStatUnion];
  info->groups = per_point ? 0 : (int64_t)h[kHostDbGroups];
}

// what TKNN_DB_DIAG (diagnostic library) and TKNN_DB_VERBOSE ask for, on stderr (scripts/db_probe.py, db_packet_stats.py,
// diag_sweep.sh and db_fallback_check.py read it)
void Engine::DbCall::print_diagnostics() const {
  const unsigned long long *h = e.h_counters_;
  if ((a.diag & 512) && a.pk_diag) {
    // what the packets of the timed pass took, and when the launch would end if the waves took them longest first
    // (TKNN_DB_DUMP=<file>: four int32 per packet -- ticks, extent in 1e-6, rounds, settles -- for scripts/db_packet_stats.py)
    const size_t np = ((size_t)h[kHostDbGroups] + 63) / 64;
    std::vector<int32_t> d(np * 4);
    OWLMI_HIP(hipMemcpy(d.data(), a.pk_diag, np * 16, hipMemcpyDeviceToHost));
    if (knobs.dump) {
      if (FILE *f = std::fopen(knobs.dump, "wb")) {
        std::fwrite(d.data(), 16, np, f);
        std::fclose(f);
      }
    }
    std::vector<size_t> order(np);
    for (size_t i = 0; i < np; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return d[x * 4] > d[y * 4]; });
    double sum = 0;
    for (size_t i = 0; i < np; i++) sum += d[i * 4];
    const int machines = union_waves();
    std::vector<double> load(machines, 0.0);
    for (size_t i = 0; i < np; i++) load[std::min_element(load.begin(), load.end()) - load.begin()] += d[order[i] * 4];
    std::fprintf(stderr, "[dbscan] %zu packets, %d waves: sum %.3g ticks, mean per wave %.0f, longest packet %d; longest-first would end at %.0f ticks\n", np, machines, sum,
                 sum / machines, np ? d[order[0] * 4] : 0, *std::max_element(load.begin(), load.end()));
    for (int i = 0; i < 6 && (size_t)i < np; i++)
      std::fprintf(stderr, "[dbscan]   packet %zu: %d ticks, extent %.4f, %d rounds, %d settles\n", order[i], d[order[i] * 4], d[order[i] * 4 + 1] * 1e-6, d[order[i] * 4 + 2], d[order[i] * 4 + 3]);
  }
  if (a.diag & 512) {
    unsigned long long t[kDbDiagWords];  // (the block's words: knn_device.h)
    OWLMI_HIP(hipMemcpy(t, e.counters_ + kDbDiag, sizeof t, hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[dbscan] union kernel: %llu waves, mean time in the kernel %.0f ticks, longest %llu ticks (%.0f %% of it filled on average), in packets %.0f ticks\n", t[15],
                 (double)t[13] / (double)t[15], t[14], 100.0 * (double)t[13] / (double)t[15] / (double)t[14], (double)(t[0] + t[1] + t[2] + t[3] + t[4]) / (double)t[15]);
    if (!(a.diag & 1024)) std::fprintf(stderr, "[dbscan] union kernel: longest packet %llu ticks; %llu packets above 2^20 ticks, %llu above 2^21\n", t[12], t[10], t[11]);
    if (!(a.diag & 1024) && t[11]) std::fprintf(stderr, "[dbscan] union kernel: the packets above 2^21 ticks, each on average: %.1f rounds, %.1f settles (%.0f ticks in them), %.1f entries the long way, %.1f point tests\n",
                 (double)t[16] / t[11], (double)t[17] / t[11], (double)t[9] / t[11], (double)t[18] / t[11], (double)t[19] / t[11]);
    const double tot = (double)(t[0] + t[1] + t[2] + t[3] + t[4]);
    std::fprintf(stderr, "[dbscan] union kernel wave time: loads %.1f%%  tests %.1f%%  settles %.1f%%  pushes %.1f%%  packet set-up %.1f%%;  %.1f rounds and %.1f settles per packet, %llu packet walks, %.1f us per packet walk (s_memtime at 100 MHz)\n",
                 100 * t[0] / tot, 100 * t[1] / tot, 100 * t[2] / tot, 100 * t[3] / tot, 100 * t[4] / tot, (double)t[5] / (double)t[7], (double)t[6] / (double)t[7], t[7], tot / 100.0 / (double)t[7]);
  }
  if (knobs.verbose)
    std::fprintf(stderr, "[dbscan] node / point tests: core flags %llu / %llu, unions %llu / %llu, labels %llu / %llu; %llu slots not core\n", h[kDbStatCore],
                 h[kDbStatCore + 1], h[kDbStatUnion], h[kDbStatUnion + 1], h[kDbStatLabel], h[kDbStatLabel + 1], h[kHostDbNotCore]);
  if (a.diag & 1024) {
    unsigned long long t[5];
    OWLMI_HIP(hipMemcpy(t, e.counters_ + kDbDiag + kDbDiagSets, sizeof t, hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[dbscan] second union pass: %llu packets of one set, %llu mixed; %llu nodes popped, %llu of them dropped as the packet's own set, %llu known to be of one set\n", t[0], t[1], t[3], t[2], t[4]);
  }
  if (a.diag & 8)
    std::fprintf(stderr, "[dbscan] groups %llu  union-phase node tests %llu  longest walk %llu  mean of the waves' longest %.0f\n", h[kHostDbGroups],
                 h[kDbStatUnion], h[kDbStatLongestWalk], (double)h[kDbStatWalkSum] / ((double)((h[kHostDbGroups] + 63) / 64) + 1e-9));
}

// tknnDbscanNoise: one growth round of the auto-eps loop without the loop.  Returns the number of noise points; d_noise is
// indexed by row.
int64_t Engine::dbscan_noise(float eps, int min_pts, uint8_t *d_noise, hipStream_t s) {
  DbCall c(*this, min_pts, s);
  c.probe_setup();
  const int64_t count = c.probe_round(eps, true);
  c.noise_rows(d_noise);
  OWLMI_HIP(hipStreamSynchronize(s));
  return count;
}

void Engine::dbscan(float eps, int min_pts, int32_t *d_labels, uint8_t *d_core, int32_t *d_counts,
                    tknnDbscanInfo *info, hipStream_t s, const int32_t *core_label) {
  DbCall c(*this, min_pts, s);
  if (core_label) return c.assign(eps, d_labels, core_label, info);
  c.cluster(eps, d_labels, d_core, d_counts, c.knobs.per_point);
  // a packet's walk ran out of stack (a tree some 250 levels deep): the whole call again with the per-point unions
  if (!c.per_point && h_counters_[kHostDbOverflows] != 0) c.cluster(eps, d_labels, d_core, d_counts, true);
  if (info) {
    c.cluster_info(info);
    c.print_diagnostics();
  }
}

void Engine::dbscan_query(float eps, const float *d_queries, int64_t m, const int32_t *core_label, int32_t *d_labels, int32_t *d_counts,
                          tknnDbscanInfo *info, hipStream_t s) {
  DbCall c(*this, 1, s);
  c.query(eps, d_queries, m, core_label, d_labels, d_counts, info);
}

// tknnDbscanAuto: the growth loop of the spec -- rounds of (core flags of the points not core yet, noise probe of the
// points still noise) with eps doubling, then ONE full clustering at the eps that brought the noise under the bound.
void Engine::dbscan_auto(float eps0, int min_pts, double max_noise, int max_rounds, int32_t *d_labels, uint8_t *d_core,
                         tknnDbscanAutoInfo *info, hipStream_t s) {
  const int64_t bound = (int64_t)std::floor(max_noise * (double)bvh_.size());
  float eps = eps0;
  int rounds = 0;
  int64_t noise_now = bvh_.size();
  bool reached = false;
  {
    DbCall c(*this, min_pts, s);
    c.probe_setup();
    c.a.keep_core = 1;  // slots flagged core by a round with a smaller eps stay core (N(p) only grows)
    OWLMI_HIP(hipMemsetAsync(c.a.core_sorted, 0, (size_t)c.n, s));
    OWLMI_HIP(hipEventRecord(ev_a_, s));
    for (int t = 0; t < max_rounds; t++) {
      noise_now = c.probe_round(eps, t == 0);
      rounds = t + 1;
      if (noise_now <= bound) {
        reached = true;
        break;
      }
      if (t + 1 < max_rounds) eps = eps * 2.0f;  // hostCode.cpp:321
    }
  }
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  OWLMI_HIP(hipEventSynchronize(ev_b_));
  float probe_ms = 0;
  OWLMI_HIP(hipEventElapsedTime(&probe_ms, ev_a_, ev_b_));
  // the clusters of the final eps (also when the rounds ran out: the caller gets the last round's labelling and an error)
  tknnDbscanInfo last;
  std::memset(&last, 0, sizeof last);
  dbscan(eps, min_pts, d_labels, d_core, nullptr, &last, s);
  if (info) {
    std::memset(info, 0, sizeof *info);
    info->last = last;
    info->rounds = rounds, info->eps = eps, info->noise = noise_now, info->probe_ms = probe_ms;
  }
  if (!reached) throw RoundsExceeded{};
}

}  // namespace owlmi
