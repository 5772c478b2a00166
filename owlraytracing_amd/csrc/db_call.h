// db_call.h -- one RT-DBSCAN call on the host: its knobs (DbKnobs), its kernels' argument block and its launches as steps
// (Engine::DbCall).  A step that launches kernels is defined in the file that holds those kernels (dbscan_core.hip,
// dbscan_union.hip, dbscan_label.hip), every other step and the order of the steps in dbscan.hip.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "db_device.h"
#include "db_workspace.h"
#include "trueknn_engine.h"

namespace owlmi {

// RT-DBSCAN's environment knobs -- this is the list.  Read at the top of every call (DbCall): tests and measurement scripts
// switch them between calls.  Not here: TKNN_DB_PER_CU (union workgroups per CU, at most what fits; read once per engine
// with Engine::db_union_resident_) and the build macros (TKNN_DB_STACK, TKNN_DB_BUF, TKNN_DB_BOXES, TKNN_DB_UNION_BLOCK:
// dbscan_union.hip).
struct DbKnobs {
  static int num(const char *name, int otherwise) { return getenv(name) ? atoi(getenv(name)) : otherwise; }
  static bool is(const char *name, const char *value) { return getenv(name) && std::strcmp(getenv(name), value) == 0; }
  bool paths = num("TKNN_DB_PATHS", 1) != 0;               // 0: a point's walk down to its group starts at the root (measurements)
  bool side = num("TKNN_DB_SIDE", 1) != 0;                 // 0: no side stream, the label kernel walks for the points that are not core (measurements)
  bool uniform = num("TKNN_DB_UNIFORM", 1) != 0;           // 0: the second union pass without the one-set shortcut (measurements)
  bool per_point = is("TKNN_DBSCAN_UNION", "point");       // the per-point union walk (A/B measurements, tests)
  bool scatter = is("TKNN_DB_LABEL", "scatter");           // labels straight to the rows instead of by slot and a gather (A/B)
  int chunk = std::max(1, num("TKNN_DB_CHUNK", 64));       // packets per chunk dealt to an XCD
  int short_way = num("TKNN_DB_SHORT", 1);                 // 0: the group-union kernel's settle the long way only (measurements)
  int scan_budget = std::max(0, num("TKNN_DB_SCAN", 12));  // steps a probe's quick scan may take
  int grid = num("TKNN_DB_GRID", INT_MAX);                 // at most this many workgroups of the group-union kernel (at least 1; measurements)
  float split = getenv("TKNN_DB_SPLIT") ? (float)atof(getenv("TKNN_DB_SPLIT")) : 0.25f;  // the first union pass takes faces up to this fraction of eps apart; >= 1: one pass
  int diag = TKNN_DIAG_BUILD ? num("TKNN_DB_DIAG", 0) : 0;  // the diagnostic library only (DbArgs::diag)
  const char *dump = getenv("TKNN_DB_DUMP");               // <file>: the timed pass's packet records (TKNN_DB_DIAG & 512; scripts/db_packet_stats.py)
  bool verbose = getenv("TKNN_DB_VERBOSE") != nullptr;     // the traversals' work counters on stderr
};

struct Engine::DbCall {
  Engine &e;
  const hipStream_t s;
  const DbKnobs knobs;  // (reads the environment)
  const int64_t n = e.bvh_.size();
  const unsigned blocks = (unsigned)((n + kDbBlock - 1) / kDbBlock);  // of a launch over the slots
  const unsigned blocks_per = (unsigned)(((n + kDbPer - 1) / kDbPer + kDbBlock - 1) / kDbBlock);  // ... kDbPer slots per thread
  const unsigned walk_grid = blocks < 2048u ? blocks : 2048u;  // grid-stride over lists whose lengths only the device knows
  size_t scan_bytes = 0;  // the library's exclusive sum over up to n words: its temporary storage, behind the layout
  void *ws = nullptr, *scan_tmp = nullptr;
  DbArgs a, common;  // common: what every call sets, as the constructor leaves it
  int32_t *block_places = nullptr, *next_core = nullptr;  // build_next_core (next_core: a.next_core, to write through)
  uint8_t *noise = nullptr;  // a growth round: per slot
  // the full clustering, and the assign step (which shares its first steps)
  int32_t *roots = nullptr, *not_core = nullptr, *border_lists = nullptr, *uni = nullptr;
  int border_per = 0;
  bool side = false, per_point = false, between_passes = false;
  int union_launches = 1;
  int32_t last[2] = {0, 0};  // rank and root flag of the last row: their sum is the number of clusters

  // ---- dbscan.hip: what a call sets up, the order of its steps, what it reports
  DbCall(Engine &engine, int min_pts, hipStream_t stream);
  void reserve(size_t layout_bytes);
  void set_eps(float eps);
  void reset_counters();
  void exclusive_sum(const int32_t *in, int32_t *out, int count);  // the library's, over at most n words (scan_tmp, scan_bytes)
  void probe_setup();
  void cluster_setup(float eps, int32_t *d_labels, uint8_t *d_core, int32_t *d_counts, bool with_side, bool by_point, bool groups_wanted);
  void read_back();
  void cluster(float eps, int32_t *d_labels, uint8_t *d_core, int32_t *d_counts, bool by_point);
  void assign(float eps, int32_t *d_labels, const int32_t *core_label, tknnDbscanInfo *info);
  void query(float eps, const float *d_queries, int64_t m, const int32_t *core_label, int32_t *d_labels, int32_t *d_counts, tknnDbscanInfo *info);
  void cluster_info(tknnDbscanInfo *info) const;
  void print_diagnostics() const;
  // ---- dbscan_core.hip: what is known before any union
  void core_flags();
  void core_from_labels(const int32_t *core_label);
  void build_next_core(bool count, int32_t *not_core);
  int64_t probe_round(float eps, bool first_round);
  // ---- dbscan_union.hip: a walk per core point, or a walk per packet of groups in two passes
  void unions();
  void group_unions();
  int union_waves() const;
  // ---- dbscan_label.hip: from "the roots are final" to the caller's rows
  void border_walk();
  void number_clusters();
  void labels();
  void assign_labels(const int32_t *core_label);
  void query_labels(const float *d_queries, const uint32_t *order, int64_t m, const int32_t *core_label, int32_t *d_labels, int32_t *d_counts);
  void noise_rows(uint8_t *d_noise);
};

}  // namespace owlmi
