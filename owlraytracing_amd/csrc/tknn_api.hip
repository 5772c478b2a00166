// tknn_api.hip -- the C ABI of include/owlknn.h, include/owlknn_knn.h, include/owlknn_periodic.h, include/owlknn_batch.h, include/owlknn_emst.h, include/owlknn_fps.h, include/owlknn_nms.h, include/owlknn_reduce.h, include/owlknn_pca.h, include/owlknn_fpfh.h, include/owlknn_global.h, include/owlknn_voxel.h, include/owlknn_orient.h, include/owlknn_plane.h, include/owlknn_icp.h, include/owlknn_meanshift.h, include/owlknn_hdbscan.h and include/owlknn_debug.h and nothing else: every entry point checks its arguments and hands over to
// the Engine (trueknn_engine.h).  No kernel is in here and none depends on this file.
//
// What every entry point keeps to: a NULL engine is refused before any device is touched; then the engine's device is made
// current (a failure of that is TKNN_E_HIP, whatever else is wrong with the call), required pointers are checked, then the
// engine's state (TKNN_E_STATE before tknnBuild), then values; a refused call has written nothing, its info included (info is zeroed once the arguments are
// accepted); a message starts with the function's name and names the argument or the constraint.
#include "periodic_metric.h"  // periodic_in_cell
#include "trueknn_engine.h"

#include <cmath>
#include <cstring>
#include <string>

using owlmi::Engine;

static thread_local std::string g_last_error;

struct tknnEngine_t {
  Engine impl;
};

namespace {

// Every engine call runs on the device the engine was created on (the caller's current device at
// tknnCreate), whatever device is current in the calling thread now; the caller's choice is restored.
struct DeviceScope {
  int prev = -1, want;
  explicit DeviceScope(int device) : want(device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != want && hipSetDevice(want) != hipSuccess) throw owlmi::HipError{"hipSetDevice(engine's device) failed"};
  }
  ~DeviceScope() {
    if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
  }
};

// The checks of one call: each throws the refusal, said in the function's name.
struct Call {
  const char *fn;
  tknnEngine e;
  [[noreturn]] void refuse(int code, const std::string &why) const { throw owlmi::ArgError{code, std::string(fn) + ": " + why}; }
  void require(bool ok, const char *why) const {
    if (!ok) refuse(TKNN_E_ARG, why);
  }
  void need(const void *p, const char *name) const {
    if (!p) refuse(TKNN_E_ARG, std::string(name) + " is NULL");
  }
  template <typename T>
  const T &record(const T *options) const {
    need(options, "options");
    return *options;
  }
  void built() const {
    if (!e->impl.built()) refuse(TKNN_E_STATE, "call tknnBuild first");
  }
  void batched() const {
    if (!e->impl.batched()) refuse(TKNN_E_STATE, "call tknnBuildBatched first (the engine's tree is not a batched one)");
  }
  void positive(float x, const char *name) const {
    if (!(x > 0.f) || !std::isfinite(x)) refuse(TKNN_E_ARG, std::string(name) + " must be finite and > 0");
  }
  void count(int64_t m, const char *name, int64_t least = 0) const {
    if (m < least || m >= 0x7fffffffLL) refuse(TKNN_E_ARG, "need " + std::to_string(least) + " <= " + name + " < 2^31-1");
  }
  // 1 <= k <= limit; above the limit with `code_above` (TKNN_E_UNSUPPORTED where another call or kernel serves that k)
  void k_up_to(int k, int limit, int code_above) const {
    if (k < 1) refuse(TKNN_E_ARG, "k must be positive");
    if (k > limit) refuse(code_above, "k out of range (1 .. " + std::to_string(limit) + ")");
  }
};

int failed(int code, const std::string &what) {
  g_last_error = what;
  return code;
}

// runs f; what it throws becomes the call's code and tknnLastError()
template <typename F>
int guarded(F &&f) {
  try {
    f();
    return TKNN_OK;
  } catch (const owlmi::LbvhStateError &e) {
    return failed(TKNN_E_STATE, e.what);
  } catch (const owlmi::HipError &e) {
    return failed(TKNN_E_HIP, e.what);
  } catch (const owlmi::RoundsExceeded &) {
    return failed(TKNN_E_ROUNDS, "max_rounds reached with unfinished queries (the reference loops forever here, e.g. n <= k)");
  } catch (const owlmi::ArgError &e) {
    return failed(e.code, e.what);
  } catch (const std::exception &e) {
    return failed(TKNN_E_HIP, e.what());
  }
}

// One call on an engine: a NULL engine is refused before any device is touched, `f(call)` runs on the engine's device.  The
// call's stream first waits for a DBSCAN side launch that an earlier call left without a rejoin (Engine::join_side): whatever
// the call is, it is about to lay its own columns over the workspace that kernel works on.
template <typename F>
int api(const char *fn, tknnEngine e, void *stream, F &&f) {
  return guarded([&] {
    const Call c{fn, e};
    c.need(e, "the engine");
    DeviceScope scope(e->impl.device());
    e->impl.join_side((hipStream_t)stream);
    f(c);
  });
}

template <typename T>
void zero(T *info) {
  if (info) std::memset(info, 0, sizeof(*info));
}

}  // namespace

extern "C" {

const char *tknnLastError(void) { return g_last_error.c_str(); }

int tknnDeviceCount(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int tknnCreate(tknnEngine *out) {
  return guarded([&] {
    Call{"tknnCreate", nullptr}.need(out, "out");
    *out = nullptr;
    int n = 0;
    OWLMI_HIP(hipGetDeviceCount(&n));
    if (n <= 0) throw owlmi::HipError{"no HIP device visible: the TrueKNN engine has no CPU fallback"};
    *out = new tknnEngine_t();
  });
}

void tknnDestroy(tknnEngine e) {
  if (!e) return;
  try {
    DeviceScope scope(e->impl.device());
    delete e;
  } catch (...) {
    delete e;
  }
}

int tknnBuildIds(tknnEngine e, const float *d_xyz, const int32_t *d_ids, int64_t n, tknnBuildInfo *info, void *stream) {
  return api("tknnBuild", e, stream, [&](const Call &c) {
    c.need(d_xyz, "d_xyz");
    c.count(n, "n", 1);
    e->impl.build(d_xyz, d_ids, n, info, (hipStream_t)stream);
  });
}

int tknnBuild(tknnEngine e, const float *d_xyz, int64_t n, tknnBuildInfo *info, void *stream) {
  return tknnBuildIds(e, d_xyz, nullptr, n, info, stream);
}

int tknnSetHalo(tknnEngine e, const float *d_xyz, const int32_t *d_ids, int64_t m, void *stream) {
  return api("tknnSetHalo", e, stream, [&](const Call &c) {
    c.count(m, "m");
    if (m > 0) c.need(d_xyz, "d_xyz"), c.need(d_ids, "d_ids");
    c.built();
    e->impl.set_halo(d_xyz, d_ids, m, (hipStream_t)stream);
  });
}

// the boxes of both forms of tknnHaloSelect
static void need_boxes(const Call &c, const float *d_boxes, const int32_t *d_box_peer, int32_t nboxes) {
  c.require(nboxes >= 0, "nboxes must not be negative");
  if (nboxes > 0) c.need(d_boxes, "d_boxes"), c.need(d_box_peer, "d_box_peer");
}

int tknnHaloSelect(tknnEngine e, const float *d_boxes, const int32_t *d_box_peer, int32_t nboxes, int32_t npeers,
                   int64_t *d_counts, const int64_t *d_offsets, float *d_rows, void *stream) {
  return api("tknnHaloSelect", e, stream, [&](const Call &c) {
    need_boxes(c, d_boxes, d_box_peer, nboxes);
    c.require(d_rows || d_counts, "need d_counts (count pass) or d_offsets + d_rows (write pass)");
    if (d_rows) c.need(d_offsets, "d_offsets");
    c.built();
    e->impl.halo_select(d_boxes, d_box_peer, nboxes, npeers, d_counts, d_offsets, d_rows, (hipStream_t)stream);
  });
}

int tknnHaloSelectFixed(tknnEngine e, const float *d_boxes, const int32_t *d_box_peer, int32_t nboxes, int32_t npeers,
                        const int64_t *d_caps, const int64_t *d_offsets, float *d_rows, int64_t *d_counts, void *stream) {
  return api("tknnHaloSelectFixed", e, stream, [&](const Call &c) {
    need_boxes(c, d_boxes, d_box_peer, nboxes);
    c.need(d_caps, "d_caps"), c.need(d_offsets, "d_offsets"), c.need(d_rows, "d_rows"), c.need(d_counts, "d_counts");
    c.built();
    e->impl.halo_select(d_boxes, d_box_peer, nboxes, npeers, d_counts, d_offsets, d_rows, (hipStream_t)stream, d_caps);
  });
}

int tknnSolve(tknnEngine e, int k, float start_radius, int kernel, int max_rounds, int32_t *d_idx,
              float *d_dist, int64_t *d_intersections, tknnNeigh *d_fb, tknnSolveInfo *info, void *stream) {
  tknnSolveOptions o = {};
  o.k = k;
  o.start_radius = start_radius;
  o.kernel = kernel;
  o.max_rounds = max_rounds;
  o.d_idx = d_idx;
  o.d_dist = d_dist;
  o.d_intersections = d_intersections;
  o.d_fb = d_fb;
  return tknnSolveEx(e, &o, info, stream);
}

int tknnSolveEx(tknnEngine e, const tknnSolveOptions *options, tknnSolveInfo *info, void *stream) {
  return api("tknnSolve", e, stream, [&](const Call &c) {
    const tknnSolveOptions &o = c.record(options);
    c.built();
    c.k_up_to(o.k, TKNN_MAX_K, TKNN_E_UNSUPPORTED);
    c.require((int64_t)o.k < e->impl.size() || o.allow_unfinished, "need n > k (the reference never terminates otherwise)");
    c.positive(o.start_radius, "start_radius");
    c.require(o.kernel == TKNN_KERNEL_AUTO || o.kernel == TKNN_KERNEL_LANE || o.kernel == TKNN_KERNEL_WAVE || o.kernel == TKNN_KERNEL_TEAM,
              "unknown kernel selector");
    c.require(o.phase >= 0 && o.phase <= 3, "phase must be 0 (all), 1 (interior), 2 (boundary) or 3 (unfinished)");
    owlmi::SolveArgs sa;
    sa.k = o.k;
    sa.start_radius = o.start_radius;
    sa.max_rounds = owlmi::resolve_max_rounds(o.max_rounds);
    sa.d_idx = o.d_idx;
    sa.d_dist = o.d_dist;
    sa.d_isect = o.d_intersections;
    sa.d_fb = o.d_fb;
    sa.d_levels = o.d_levels;
    sa.allow_unfinished = o.allow_unfinished != 0;
    sa.phase = o.phase;
    sa.d_start_radii = o.d_start_radii;
    zero(info);
    e->impl.solve(sa, o.kernel, info, (hipStream_t)stream);
  });
}

int tknnRepairExact(tknnEngine e, int k, float start_radius, const int32_t *d_levels, int32_t *d_idx,
                    float *d_dist, int64_t *repaired, void *stream) {
  return api("tknnRepairExact", e, stream, [&](const Call &c) {
    c.need(d_levels, "d_levels"), c.need(d_idx, "d_idx"), c.need(d_dist, "d_dist");
    c.built();
    c.k_up_to(k, TKNN_MAX_K_REGISTERS, TKNN_E_ARG);  // (the repair pass keeps its lists in registers)
    c.positive(start_radius, "start_radius");
    const int64_t n = e->impl.repair_exact(k, d_levels, d_idx, d_dist, (hipStream_t)stream);
    if (repaired) *repaired = n;
  });
}

int tknnQuery(tknnEngine e, const tknnQueryOptions *options, tknnSolveInfo *info, void *stream) {
  return api("tknnQuery", e, stream, [&](const Call &c) {
    const tknnQueryOptions &o = c.record(options);
    if (o.m > 0) c.need(o.d_queries, "d_queries");
    c.built();
    c.require(o.k >= 1, "k must be positive");
    c.require((int64_t)o.k <= e->impl.size(), "need n >= k (no query can finish otherwise)");
    c.positive(o.start_radius, "start_radius");
    c.count(o.m, "m");
    c.require(!o.allow_unfinished || o.d_levels, "allow_unfinished needs d_levels (they say which rows were written)");
    c.k_up_to(o.k, TKNN_MAX_K_REGISTERS, TKNN_E_UNSUPPORTED);  // (the query kernels keep their lists in registers)
    if (e->impl.has_halo()) c.refuse(TKNN_E_UNSUPPORTED, "a halo tree is set (queries over tiles are not served yet)");
    zero(info);
    if (o.m > 0) e->impl.query(o, info, (hipStream_t)stream);
  });
}

int tknnDbscan(tknnEngine e, float eps, int min_pts, int32_t *d_labels, uint8_t *d_core, int32_t *d_counts,
               tknnDbscanInfo *info, void *stream) {
  return api("tknnDbscan", e, stream, [&](const Call &c) {
    c.need(d_labels, "d_labels");
    c.built();
    c.positive(eps, "eps");
    c.require(min_pts >= 1, "min_pts must be >= 1");
    e->impl.dbscan(eps, min_pts, d_labels, d_core, d_counts, info, (hipStream_t)stream);
  });
}

int tknnDbscanAssign(tknnEngine e, float eps, const int32_t *d_core_label, int32_t *d_labels, tknnDbscanInfo *info,
                     void *stream) {
  return api("tknnDbscanAssign", e, stream, [&](const Call &c) {
    c.need(d_labels, "d_labels"), c.need(d_core_label, "d_core_label");
    c.built();
    c.positive(eps, "eps");
    e->impl.dbscan(eps, 1, d_labels, nullptr, nullptr, info, (hipStream_t)stream, d_core_label);
  });
}

int tknnDbscanQuery(tknnEngine e, const tknnDbscanQueryOptions *options, tknnDbscanInfo *info, void *stream) {
  return api("tknnDbscanQuery", e, stream, [&](const Call &c) {
    const tknnDbscanQueryOptions &o = c.record(options);
    c.need(o.d_core_label, "d_core_label"), c.need(o.d_labels, "d_labels");
    if (o.m > 0) c.need(o.d_queries, "d_queries");
    c.built();
    c.positive(o.eps, "eps");
    c.count(o.m, "m");
    zero(info);
    if (o.m > 0) e->impl.dbscan_query(o.eps, o.d_queries, o.m, o.d_core_label, o.d_labels, o.d_counts, info, (hipStream_t)stream);
  });
}

int tknnRadiusQuery(tknnEngine e, const tknnRadiusOptions *options, tknnRadiusInfo *info, void *stream) {
  return api("tknnRadiusQuery", e, stream, [&](const Call &c) {
    const tknnRadiusOptions &o = c.record(options);
    c.need(o.d_offsets, "d_offsets");
    if (o.m > 0) c.need(o.d_queries, "d_queries");
    c.built();
    c.positive(o.radius, "radius");
    c.count(o.m, "m");
    c.require(!o.d_dist || o.d_idx, "d_dist needs d_idx (both NULL: the count pass)");
    c.require(o.capacity >= 0, "capacity must not be negative");
    zero(info);
    if (o.m > 0) {
      e->impl.radius_query(o, info, (hipStream_t)stream);
    } else if (!o.d_idx) {  // the count pass of no queries: the one offset
      OWLMI_HIP(hipMemsetAsync(o.d_offsets, 0, sizeof(int64_t), (hipStream_t)stream));
      OWLMI_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
  });
}

int tknnRadiusKnn(tknnEngine e, const tknnRadiusKnnOptions *options, tknnRadiusKnnInfo *info, void *stream) {
  return api("tknnRadiusKnn", e, stream, [&](const Call &c) {
    const tknnRadiusKnnOptions &o = c.record(options);
    c.need(o.d_idx, "d_idx");
    if (o.m > 0) c.need(o.d_queries, "d_queries");
    c.built();
    c.require(o.k >= 1, "k must be positive");
    c.count(o.m, "m");
    if (!o.d_radii) c.positive(o.radius, "radius (or give d_radii)");
    c.k_up_to(o.k, TKNN_MAX_K_REGISTERS, TKNN_E_UNSUPPORTED);  // (the kernels keep their lists in registers)
    zero(info);
    if (o.m > 0) e->impl.radius_knn(o, info, (hipStream_t)stream);
  });
}

int tknnKnn(tknnEngine e, const tknnKnnOptions *options, tknnKnnInfo *info, void *stream) {
  return api("tknnKnn", e, stream, [&](const Call &c) {
    const tknnKnnOptions &o = c.record(options);
    c.need(o.d_idx, "d_idx");
    if (!o.d_queries) {  // the set's own points
      c.require(o.m == e->impl.size(), "d_queries is NULL (the set's own points): m must equal n");
      c.require(!o.d_skip_ids, "d_queries is NULL (the set's own points): d_skip_ids must be NULL, every point is left out of its own row");
    }
    c.built();
    c.require(o.k >= 1, "k must be positive");
    c.count(o.m, "m");
    c.k_up_to(o.k, TKNN_MAX_K_REGISTERS, TKNN_E_UNSUPPORTED);  // (the kernels keep their lists in registers)
    zero(info);
    if (o.m > 0) e->impl.knn(o, info, (hipStream_t)stream);
  });
}

int tknnPeriodicKnn(tknnEngine e, const tknnPeriodicKnnOptions *options, tknnPeriodicKnnInfo *info, void *stream) {
  return api("tknnPeriodicKnn", e, stream, [&](const Call &c) {
    const tknnPeriodicKnnOptions &o = c.record(options);
    c.need(o.d_idx, "d_idx");
    if (!o.d_queries) {  // the set's own points
      c.require(o.m == e->impl.size(), "d_queries is NULL (the set's own points): m must equal n");
      c.require(!o.d_skip_ids, "d_queries is NULL (the set's own points): d_skip_ids must be NULL, every point is left out of its own row");
    }
    c.built();
    c.require(o.k >= 1, "k must be positive");
    c.count(o.m, "m");
    c.k_up_to(o.k, TKNN_MAX_K_REGISTERS, TKNN_E_UNSUPPORTED);  // (the kernels keep their lists in registers)
    static const char *const axis[3] = {"x", "y", "z"};
    for (int a = 0; a < 3; a++) {
      if (!(o.period[a] >= 0.f) || !std::isfinite(o.period[a])) c.refuse(TKNN_E_ARG, std::string("period of axis ") + axis[a] + " must be finite and >= 0 (0: an open axis)");
      if (o.period[a] > 0.f && !std::isfinite(o.lo[a])) c.refuse(TKNN_E_ARG, std::string("lo of the periodic axis ") + axis[a] + " must be finite");
    }
    if (!o.d_radii) c.positive(o.radius, "radius (FLT_MAX: none; or give d_radii)");
    const float *scene = e->impl.scene();
    for (int a = 0; a < 3; a++) {
      if (!(o.period[a] > 0.f) || !(scene[a] <= scene[3 + a])) continue;  // (an open axis; a set of NaN points only: no box)
      const bool inside = periodic_in_cell(scene[a], o.lo[a], o.period[a]) && periodic_in_cell(scene[3 + a], o.lo[a], o.period[a]);  // (then so is every point between)
      if (!inside) c.refuse(TKNN_E_ARG, std::string("the built set does not lie in the cell on the periodic axis ") + axis[a] + " (nothing is wrapped for the caller)");
    }
    zero(info);
    if (o.m > 0) e->impl.periodic_knn(o, info, (hipStream_t)stream);
  });
}

int tknnBuildBatched(tknnEngine e, const float *d_xyz, const int32_t *d_ids, const int32_t *d_batch, int32_t num_batches, int64_t n, tknnBuildInfo *info,
                     void *stream) {
  return api("tknnBuildBatched", e, stream, [&](const Call &c) {
    c.need(d_xyz, "d_xyz"), c.need(d_batch, "d_batch");
    c.count(n, "n", 1);
    c.require(num_batches >= 1, "num_batches must be positive");
    if (num_batches > TKNN_MAX_BATCHES) c.refuse(TKNN_E_UNSUPPORTED, "num_batches out of range (1 .. " + std::to_string(TKNN_MAX_BATCHES) + ")");
    e->impl.build_batched(d_xyz, d_ids, d_batch, num_batches, n, info, (hipStream_t)stream);
  });
}

int tknnBatchLayout(tknnEngine e, int32_t *num_batches, int32_t *key_bits, int32_t *d_starts, void *stream) {
  return api("tknnBatchLayout", e, stream, [&](const Call &c) {
    c.batched();
    e->impl.batch_layout(num_batches, key_bits, d_starts, (hipStream_t)stream);
  });
}

int tknnBatchKnn(tknnEngine e, const tknnBatchKnnOptions *options, tknnBatchKnnInfo *info, void *stream) {
  return api("tknnBatchKnn", e, stream, [&](const Call &c) {
    const tknnBatchKnnOptions &o = c.record(options);
    c.need(o.d_idx, "d_idx");
    if (!o.d_queries) {  // the set's own points
      c.require(o.m == e->impl.size(), "d_queries is NULL (the set's own points): m must equal n");
      c.require(!o.d_skip_ids, "d_queries is NULL (the set's own points): d_skip_ids must be NULL, every point is left out of its own row");
    }
    c.require(!o.d_queries == !o.d_query_batch, "d_queries and d_query_batch go together: both given, or both NULL (the set's own points)");
    c.batched();
    c.require(o.k >= 1, "k must be positive");
    c.count(o.m, "m");
    c.k_up_to(o.k, TKNN_MAX_K_REGISTERS, TKNN_E_UNSUPPORTED);  // (the kernels keep their lists in registers)
    if (!o.d_radii) c.positive(o.radius, "radius (FLT_MAX: none; or give d_radii)");
    zero(info);
    if (o.m > 0) e->impl.batch_knn(o, info, (hipStream_t)stream);
  });
}

int tknnFps(tknnEngine e, const tknnFpsOptions *options, tknnFpsInfo *info, void *stream) {
  return api("tknnFps", e, stream, [&](const Call &c) {
    const tknnFpsOptions &o = c.record(options);
    c.need(o.d_idx, "d_idx");
    if (!e->impl.built() || !e->impl.tree().has_points()) c.refuse(TKNN_E_STATE, "call tknnBuild first (the engine has no point tree)");
    c.require(o.num_samples >= 1, "num_samples must be positive");
    c.require((int64_t)e->impl.num_clouds() * o.num_samples < (1ll << 31), "need clouds * num_samples < 2^31");
    zero(info);
    e->impl.fps(o, info, (hipStream_t)stream);
  });
}

int tknnRadiusNms(tknnEngine e, const tknnRadiusNmsOptions *options, tknnRadiusNmsInfo *info, void *stream) {
  return api("tknnRadiusNms", e, stream, [&](const Call &c) {
    const tknnRadiusNmsOptions &o = c.record(options);
    c.need(o.d_keep, "d_keep");
    if (!e->impl.built() || !e->impl.tree().has_points()) c.refuse(TKNN_E_STATE, "call tknnBuild first (the engine has no point tree)");
    c.positive(o.radius, "radius");
    c.require(!(o.d_scores && (o.flags & TKNN_NMS_BY_NAME)), "d_scores and TKNN_NMS_BY_NAME exclude each other");
    c.require((o.flags & ~TKNN_NMS_BY_NAME) == 0u, "flags has a bit no flag of this call has");
    c.require(o.max_rounds >= 0, "max_rounds must not be negative (0: no limit)");
    zero(info);
    e->impl.radius_nms(o, info, (hipStream_t)stream);
  });
}

int tknnRadiusReduce(tknnEngine e, const tknnRadiusReduceOptions *options, tknnRadiusReduceInfo *info, void *stream) {
  return api("tknnRadiusReduce", e, stream, [&](const Call &c) {
    const tknnRadiusReduceOptions &o = c.record(options);
    c.require(o.d_counts || o.d_wsum || o.d_out, "no output: give d_counts, d_wsum or d_out");
    if (!o.d_queries) c.require(o.m == e->impl.size(), "d_queries is NULL (the set's own points): m must equal n");
    if (!e->impl.built() || !e->impl.tree().has_points()) c.refuse(TKNN_E_STATE, "call tknnBuild first (the engine has no point tree)");
    c.positive(o.radius, "radius");
    c.require(o.weight >= TKNN_W_ONE && o.weight <= TKNN_W_CUBIC_SPLINE, "weight must be one of TKNN_W_ONE, TKNN_W_GAUSS, TKNN_W_EPANECHNIKOV, TKNN_W_CUBIC_SPLINE");
    c.require((o.flags & ~(TKNN_REDUCE_NORMALIZE | TKNN_REDUCE_SKIP_SELF)) == 0u, "flags has a bit no flag of this call has");
    if (o.weight == TKNN_W_GAUSS) c.positive(o.bandwidth, "bandwidth (TKNN_W_GAUSS)");
    c.require(o.channels >= 0 && o.channels <= TKNN_REDUCE_MAX_CHANNELS, "channels must be 0 .. 16");
    if (o.channels > 0) c.need(o.d_values, "d_values (channels > 0)"), c.need(o.d_out, "d_out (channels > 0)");
    c.require(o.channels > 0 || o.d_counts || o.d_wsum, "channels = 0 writes no d_out: give d_counts or d_wsum");
    c.require(!((o.flags & TKNN_REDUCE_SKIP_SELF) && o.d_queries), "TKNN_REDUCE_SKIP_SELF goes with d_queries = NULL (the set's own points) only");
    c.count(o.m, "m");
    zero(info);
    if (o.m > 0) e->impl.radius_reduce(o, info, (hipStream_t)stream);
  });
}

int tknnLocalPca(tknnEngine e, const tknnLocalPcaOptions *options, tknnLocalPcaInfo *info, void *stream) {
  return api("tknnLocalPca", e, stream, [&](const Call &c) {
    const tknnLocalPcaOptions &o = c.record(options);
    c.require(o.d_counts || o.d_centroid || o.d_cov || o.d_eigenvalues || o.d_eigenvectors || o.d_normals || o.d_curvature,
              "no output: give d_counts, d_centroid, d_cov, d_eigenvalues, d_eigenvectors, d_normals or d_curvature");
    if (!o.d_queries) c.require(o.m == e->impl.size(), "d_queries is NULL (the set's own points): m must equal n");
    if (!e->impl.built() || !e->impl.tree().has_points()) c.refuse(TKNN_E_STATE, "call tknnBuild first (the engine has no point tree)");
    c.require(o.radius != 0.f || o.k != 0, "give a radius, k or both (radius = 0 and k = 0: no neighbourhood)");
    c.require(o.radius >= 0.f && std::isfinite(o.radius), "radius must be finite and > 0 (0: none)");
    c.require(o.k >= 0, "k must not be negative (0: none)");
    c.require(!(!o.d_queries && !(o.flags & TKNN_PCA_SKIP_SELF) && o.k == 1),
              "k = 1 with the set's own points is the point alone: k counts the point itself, give k >= 2 or TKNN_PCA_SKIP_SELF");
    c.require((o.flags & ~(TKNN_PCA_SKIP_SELF | TKNN_PCA_ORIENT)) == 0u, "flags has a bit no flag of this call has");
    c.require(!((o.flags & TKNN_PCA_SKIP_SELF) && o.d_queries), "TKNN_PCA_SKIP_SELF goes with d_queries = NULL (the set's own points) only");
    if (o.flags & TKNN_PCA_ORIENT)
      c.require(std::isfinite(o.viewpoint[0]) && std::isfinite(o.viewpoint[1]) && std::isfinite(o.viewpoint[2]), "viewpoint must be finite (TKNN_PCA_ORIENT)");
    c.require(o.min_points >= 0, "min_points must not be negative (0: 3)");
    c.count(o.m, "m");
    if (o.k > TKNN_MAX_K_REGISTERS) c.refuse(TKNN_E_UNSUPPORTED, "k out of range (1 .. " + std::to_string(TKNN_MAX_K_REGISTERS) + ")");
    zero(info);
    if (o.m > 0) e->impl.local_pca(o, info, (hipStream_t)stream);
  });
}

int tknnFpfh(tknnEngine e, const tknnFpfhOptions *options, tknnFpfhInfo *info, void *stream) {
  return api("tknnFpfh", e, stream, [&](const Call &c) {
    const tknnFpfhOptions &o = c.record(options);
    c.require(o.d_fpfh || o.d_spfh || o.d_spfh_counts || o.d_counts, "no output: give d_fpfh, d_spfh, d_spfh_counts or d_counts");
    c.need(o.d_normals, "d_normals");
    if (!e->impl.built() || !e->impl.tree().has_points()) c.refuse(TKNN_E_STATE, "call tknnBuild first (the engine has no point tree)");
    c.positive(o.radius, "radius");
    c.require((o.flags & ~TKNN_FPFH_NO_SELF_TERM) == 0u, "flags has a bit no flag of this call has");
    zero(info);
    if (e->impl.size() > 0) e->impl.fpfh(o, info, (hipStream_t)stream);
  });
}

int tknnIcp(tknnEngine e, const tknnIcpOptions *options, tknnIcpInfo *info, void *stream) {
  return api("tknnIcp", e, stream, [&](const Call &c) {
    const tknnIcpOptions &o = c.record(options);
    c.need(info, "info");
    if (o.m > 0) c.need(o.d_source, "d_source");
    if (!e->impl.built() || !e->impl.tree().has_points()) c.refuse(TKNN_E_STATE, "call tknnBuild first (the engine has no point tree)");
    if (e->impl.ids_given()) c.refuse(TKNN_E_UNSUPPORTED, "the tree was built with ids: a partner is fetched by the caller's row, build with tknnBuild");
    c.positive(o.max_dist, "max_dist");
    c.require(o.method == TKNN_ICP_POINT_TO_POINT || o.method == TKNN_ICP_POINT_TO_PLANE, "method must be TKNN_ICP_POINT_TO_POINT or TKNN_ICP_POINT_TO_PLANE");
    c.require(o.robust >= TKNN_ICP_L2 && o.robust <= TKNN_ICP_TUKEY, "robust must be one of TKNN_ICP_L2, TKNN_ICP_HUBER, TKNN_ICP_TUKEY");
    c.require(o.flags == 0u, "flags has a bit no flag of this call has");
    if (o.method == TKNN_ICP_POINT_TO_PLANE) c.need(o.d_target_normals, "d_target_normals (TKNN_ICP_POINT_TO_PLANE)");
    if (o.robust != TKNN_ICP_L2) c.positive(o.robust_scale, "robust_scale (TKNN_ICP_HUBER, TKNN_ICP_TUKEY)");
    c.require(o.max_iterations >= 0, "max_iterations must not be negative (0: evaluate at init)");
    c.require(o.rel_fitness >= 0.0 && std::isfinite(o.rel_fitness), "rel_fitness must be finite and not negative");
    c.require(o.rel_rmse >= 0.0 && std::isfinite(o.rel_rmse), "rel_rmse must be finite and not negative");
    if (o.init)
      for (int i = 0; i < 16; i++) c.require(std::isfinite(o.init[i]), "init has an entry that is not finite");
    c.count(o.m, "m");
    zero(info);
    if (o.m > 0) {
      e->impl.icp(o, info, (hipStream_t)stream);
    } else {
      for (int i = 0; i < 16; i++) info->transform[i] = o.init ? o.init[i] : (i % 5 == 0 ? 1.0 : 0.0);
    }
  });
}

int tknnFeatureMatch(tknnEngine e, const tknnFeatureMatchOptions *options, tknnFeatureMatchInfo *info, void *stream) {
  return api("tknnFeatureMatch", e, stream, [&](const Call &c) {
    const tknnFeatureMatchOptions &o = c.record(options);
    c.need(info, "info");
    c.require(o.d_best || o.d_best_d2 || o.d_second_d2, "no output: give d_best, d_best_d2 or d_second_d2");
    if (o.m > 0) c.need(o.d_source, "d_source");
    if (o.n > 0) c.need(o.d_target, "d_target");
    c.require(o.D >= 1 && o.D <= TKNN_MATCH_MAX_D, "D must be 1 .. 64");
    c.count(o.m, "m");
    c.count(o.n, "n");
    c.require(o.flags == 0u, "flags has a bit no flag of this call has");
    zero(info);
    if (o.m > 0) e->impl.feature_match(o, info, (hipStream_t)stream);
  });
}

int tknnRansac(tknnEngine e, const tknnRansacOptions *options, tknnRansacInfo *info, void *stream) {
  return api("tknnRansac", e, stream, [&](const Call &c) {
    const tknnRansacOptions &o = c.record(options);
    c.need(info, "info");
    if (o.ms > 0) c.need(o.d_source, "d_source");
    if (o.mt > 0) c.need(o.d_target, "d_target");
    if (o.c > 0) c.need(o.d_pairs, "d_pairs");
    c.require(o.ransac_n == 3 || o.ransac_n == 4, "ransac_n must be 3 or 4");
    c.positive(o.max_dist, "max_dist");
    c.require(o.edge_similarity >= 0.f && o.edge_similarity <= 1.f, "edge_similarity must be 0 .. 1 (0: no edge check)");
    c.require(o.confidence > 0.0 && o.confidence <= 1.0, "confidence must be in (0, 1] (1: never stop early)");
    c.require(o.max_trials >= 1, "max_trials must be at least 1");
    c.require(o.refit_rounds >= 0 && o.refit_rounds <= 8, "refit_rounds must be 0 .. 8");
    c.count(o.ms, "ms");
    c.count(o.mt, "mt");
    c.count(o.c, "c");
    c.require(o.flags == 0u, "flags has a bit no flag of this call has");
    e->impl.ransac(o, info, (hipStream_t)stream);  // (refuses a pair row out of range itself, and writes info at its end only)
  });
}

int tknnVoxelGrid(tknnEngine e, const tknnVoxelGridOptions *options, tknnVoxelGridInfo *info, void *stream) {
  return api("tknnVoxelGrid", e, stream, [&](const Call &c) {
    const tknnVoxelGridOptions &o = c.record(options);
    c.need(info, "info");
    if (o.n > 0) c.need(o.d_points, "d_points");
    if (o.channels > 0) c.need(o.d_values, "d_values (channels > 0)");
    c.require(!(o.d_value_mean && o.channels == 0), "d_value_mean is given with channels = 0");
    c.count(o.n, "n");
    c.positive(o.voxel, "voxel");
    c.require(std::isfinite(o.origin[0]) && std::isfinite(o.origin[1]) && std::isfinite(o.origin[2]), "origin must be finite");
    c.require(o.num_batches >= 1 && o.num_batches <= TKNN_MAX_BATCHES, "num_batches must be 1 .. 32768");
    c.require(o.d_batch || o.num_batches == 1, "num_batches must be 1 without d_batch");
    c.require(o.channels >= 0 && o.channels <= TKNN_VOXEL_MAX_CHANNELS, "channels must be 0 .. 16");
    c.count(o.capacity, "capacity");
    c.require(o.flags == 0u, "flags has a bit no flag of this call has");
    e->impl.voxel_grid(o, info, (hipStream_t)stream);  // (refuses voxels beyond the capacity itself, and writes info at its end only)
  });
}

int tknnMeanShift(tknnEngine e, const tknnMeanShiftOptions *options, tknnMeanShiftInfo *info, void *stream) {
  return api("tknnMeanShift", e, stream, [&](const Call &c) {
    const tknnMeanShiftOptions &o = c.record(options);
    c.need(info, "info");
    c.require(o.d_modes || o.d_counts || o.d_wsum || o.d_shift || o.d_iterations || o.d_status,
              "no output: give d_modes, d_counts, d_wsum, d_shift, d_iterations or d_status");
    if (!o.d_seeds) c.require(o.m == e->impl.size(), "d_seeds is NULL (the set's own points): m must equal n");
    if (!e->impl.built() || !e->impl.tree().has_points()) c.refuse(TKNN_E_STATE, "call tknnBuild first (the engine has no point tree)");
    c.positive(o.radius, "radius");
    c.require(o.weight == TKNN_W_ONE || o.weight == TKNN_W_GAUSS || o.weight == TKNN_W_EPANECHNIKOV,
              "weight must be one of TKNN_W_ONE, TKNN_W_GAUSS, TKNN_W_EPANECHNIKOV (TKNN_W_CUBIC_SPLINE is no mean-shift kernel)");
    if (o.weight == TKNN_W_GAUSS) c.positive(o.bandwidth, "bandwidth (TKNN_W_GAUSS)");
    c.require(o.tol >= 0.f && std::isfinite(o.tol), "tol must be finite and not negative");
    c.require(o.max_iterations >= 1, "max_iterations must be at least 1");
    c.require(o.flags == 0u, "flags has a bit no flag of this call has");
    c.count(o.m, "m");
    zero(info);
    if (o.m > 0) e->impl.mean_shift(o, info, (hipStream_t)stream);
  });
}

int tknnEmst(tknnEngine e, const tknnEmstOptions *options, tknnEmstInfo *info, void *stream) {
  const int rc = api("tknnEmst", e, stream, [&](const Call &c) {
    const tknnEmstOptions &o = c.record(options);
    if (e->impl.built() && e->impl.size() > 1) c.need(o.d_u, "d_u"), c.need(o.d_v, "d_v");
    c.built();
    c.count(e->impl.size(), "n", 1);
    zero(info);
    e->impl.emst(o, info, (hipStream_t)stream);
  });
  if (rc == TKNN_E_ROUNDS) g_last_error = "tknnEmst: max_rounds reached with components still merging (nothing was written)";
  return rc;
}

int tknnOrientNormals(tknnEngine e, const tknnOrientOptions *options, tknnOrientInfo *info, void *stream) {
  const int rc = api("tknnOrientNormals", e, stream, [&](const Call &c) {
    const tknnOrientOptions &o = c.record(options);
    c.require(o.d_out_normals || o.d_flip, "no output: give d_out_normals or d_flip");
    c.need(o.d_normals, "d_normals");
    if (!e->impl.built() || !e->impl.tree().has_points()) c.refuse(TKNN_E_STATE, "call tknnBuild first (the engine has no point tree)");
    c.k_up_to(o.k, TKNN_MAX_K_REGISTERS, TKNN_E_ARG);
    c.require((o.flags & ~TKNN_ORIENT_NO_EMST) == 0u, "flags has a bit no flag of this call has");
    c.require(std::isfinite(o.direction[0]) && std::isfinite(o.direction[1]) && std::isfinite(o.direction[2]), "direction must be finite");
    if (e->impl.size() * ((int64_t)o.k + 1) >= (1ll << 31)) c.refuse(TKNN_E_UNSUPPORTED, "need n * (k + 1) < 2^31");
    e->impl.orient_normals(o, info, (hipStream_t)stream);  // (writes info at its end only)
  });
  if (rc == TKNN_E_ROUNDS) g_last_error = "tknnOrientNormals: max_rounds reached with components still merging (nothing was written)";
  return rc;
}

int tknnSegmentPlane(tknnEngine e, const tknnPlaneOptions *options, tknnPlaneInfo *info, void *stream) {
  return api("tknnSegmentPlane", e, stream, [&](const Call &c) {
    const tknnPlaneOptions &o = c.record(options);
    c.need(info, "info");
    if (!e->impl.built() || !e->impl.tree().has_points()) c.refuse(TKNN_E_STATE, "call tknnBuild first (the engine has no point tree)");
    if (e->impl.ids_given()) c.refuse(TKNN_E_UNSUPPORTED, "the tree was built with ids: a row is named by the caller's row, build with tknnBuild");
    if (e->impl.size() > 0x7fffffffLL - 64) c.refuse(TKNN_E_UNSUPPORTED, "need n <= 2^31 - 65 (the slots, padded to whole blocks, are counted in 31 bits)");
    c.positive(o.distance_threshold, "distance_threshold");
    c.require(o.max_trials >= 1, "max_trials must be at least 1");
    c.require(o.confidence > 0.0 && o.confidence <= 1.0, "confidence must be in (0, 1] (1: never stop early)");
    c.require(o.refit_rounds >= 0 && o.refit_rounds <= 8, "refit_rounds must be 0 .. 8");
    c.require(std::isfinite(o.axis[0]) && std::isfinite(o.axis[1]) && std::isfinite(o.axis[2]), "axis must be finite");
    if (o.axis[0] != 0.f || o.axis[1] != 0.f || o.axis[2] != 0.f) c.require(o.min_cos > 0.f && o.min_cos <= 1.f, "min_cos must be in (0, 1] with an axis");
    c.require(o.flags == 0u, "flags has a bit no flag of this call has");
    e->impl.segment_plane(o, info, (hipStream_t)stream);  // (writes info at its end only)
  });
}

// the forest of tknnLinkage and tknnHdbscanLabels
static void need_forest(const Call &c, int64_t n, int64_t edges) {
  c.require(n >= 1 && n < (1ll << 30), "need 1 <= n < 2^30");
  c.require(edges >= 0 && edges <= n - 1, "need 0 <= edges <= n - 1 (a forest)");
}

int tknnLinkage(tknnEngine e, const tknnLinkageOptions *options, tknnLinkageInfo *info, void *stream) {
  return api("tknnLinkage", e, stream, [&](const Call &c) {
    const tknnLinkageOptions &o = c.record(options);
    if (o.edges > 0) c.need(o.d_u, "d_u"), c.need(o.d_v, "d_v");
    c.require(o.d_parent || o.d_left || o.d_right || o.d_size, "need one of d_parent, d_left, d_right, d_size");
    need_forest(c, o.n, o.edges);
    zero(info);
    e->impl.linkage(o, info, (hipStream_t)stream);
  });
}

int tknnHdbscanLabels(tknnEngine e, const tknnHdbscanLabelsOptions *options, tknnHdbscanLabelsInfo *info, void *stream) {
  return api("tknnHdbscanLabels", e, stream, [&](const Call &c) {
    const tknnHdbscanLabelsOptions &o = c.record(options);
    c.need(o.d_labels, "d_labels");
    if (o.edges > 0) c.need(o.d_u, "d_u"), c.need(o.d_v, "d_v"), c.need(o.d_w, "d_w");
    need_forest(c, o.n, o.edges);
    c.require(o.min_cluster_size >= 2, "min_cluster_size must be >= 2");
    zero(info);
    e->impl.hdbscan_labels(o, info, (hipStream_t)stream);
  });
}

int tknnHdbscan(tknnEngine e, const tknnHdbscanOptions *options, tknnHdbscanInfo *info, void *stream) {
  return api("tknnHdbscan", e, stream, [&](const Call &c) {
    const tknnHdbscanOptions &o = c.record(options);
    c.need(o.d_labels, "d_labels");
    c.built();
    c.require(e->impl.size() < (1ll << 30), "need n < 2^30");
    c.require(o.min_cluster_size >= 2, "min_cluster_size must be >= 2");
    c.require(o.min_samples >= 1, "min_samples must be >= 1");
    if (o.min_samples - 1 > TKNN_MAX_K_REGISTERS)
      c.refuse(TKNN_E_UNSUPPORTED, "min_samples out of range (1 .. " + std::to_string(TKNN_MAX_K_REGISTERS + 1) + ": the core distances are tknnKnn's)");
    zero(info);
    e->impl.hdbscan(o, info, (hipStream_t)stream);
  });
}

int tknnDbscanAuto(tknnEngine e, float eps0, int min_pts, double max_noise, int max_rounds, int32_t *d_labels, uint8_t *d_core,
                   tknnDbscanAutoInfo *info, void *stream) {
  const int rc = api("tknnDbscanAuto", e, stream, [&](const Call &c) {
    c.need(d_labels, "d_labels");
    c.built();
    c.positive(eps0, "eps0");
    c.require(min_pts >= 1, "min_pts must be >= 1");
    c.require(max_noise >= 0.0 && max_noise <= 1.0, "max_noise is a share of the points, 0 .. 1");
    c.require(max_rounds >= 1, "max_rounds must be >= 1");
    e->impl.dbscan_auto(eps0, min_pts, max_noise, max_rounds, d_labels, d_core, info, (hipStream_t)stream);
  });
  if (rc == TKNN_E_ROUNDS) g_last_error = "tknnDbscanAuto: max_rounds doublings of eps did not bring the noise under the bound";
  return rc;
}

int tknnDbscanNoise(tknnEngine e, float eps, int min_pts, uint8_t *d_noise, int64_t *noise_count, void *stream) {
  return api("tknnDbscanNoise", e, stream, [&](const Call &c) {
    c.need(d_noise, "d_noise");
    c.built();
    c.positive(eps, "eps");
    c.require(min_pts >= 1, "min_pts must be >= 1");
    const int64_t count = e->impl.dbscan_noise(eps, min_pts, d_noise, (hipStream_t)stream);
    if (noise_count) *noise_count = count;
  });
}

int tknnSegmentMin(tknnEngine e, const int32_t *d_segment, const int64_t *d_value, int64_t n, int64_t *d_out, void *stream) {
  return api("tknnSegmentMin", e, stream, [&](const Call &c) {
    c.require(n >= 0, "n must not be negative");
    if (n > 0) c.need(d_segment, "d_segment"), c.need(d_value, "d_value"), c.need(d_out, "d_out");
    owlmi::db_segment_min(d_segment, d_value, n, d_out, (hipStream_t)stream);
  });
}

int tknnExportTree(tknnEngine e, void *nodes, int32_t *rope_node, int32_t *rope_leaf, int32_t *prim_id,
                   void *stream) {
  return api("tknnExportTree", e, stream, [&](const Call &c) {
    c.built();
    e->impl.tree().download((LbvhNode *)nodes, rope_node, rope_leaf, prim_id, (hipStream_t)stream);
  });
}

int tknnExportTreeTables(tknnEngine e, int32_t *split_owner, int32_t *block_paths, void *stream) {
  return api("tknnExportTreeTables", e, stream, [&](const Call &c) {
    c.built();
    e->impl.tree().download_tables(split_owner, block_paths, (hipStream_t)stream);
  });
}

int tknnExportTreeEx(tknnEngine e, tknnTreeExport *x, void *stream) {
  return api("tknnExportTreeEx", e, stream, [&](const Call &c) {
    c.need(x, "the export record");
    c.require(x->which == 0 || x->which == 1, "which must be 0 (own tree) or 1 (halo tree)");
    c.require(!x->wide_boxes || x->wide_capacity >= 0, "wide_capacity must not be negative");
    c.built();
    if (x->which == 1 && !(e->impl.has_halo() && e->impl.halo_tree().built())) c.refuse(TKNN_E_STATE, "no halo tree is set");
    const owlmi::Lbvh &t = x->which == 1 ? e->impl.halo_tree() : e->impl.tree();
    static_assert(sizeof(x->wide_count) == sizeof(owlmi::Lbvh::DebugInfo::wide_count), "wide levels");
    owlmi::Lbvh::DebugInfo d;
    t.download_debug(&d, x->keys, (LbvhPoint *)x->points, x->row_slot, (LbvhBox *)x->wide_boxes, x->wide_capacity, (hipStream_t)stream);
    t.download((LbvhNode *)x->nodes, x->rope_node, x->rope_leaf, x->prim_id, (hipStream_t)stream);
    t.download_tables(x->split_owner, nullptr, (hipStream_t)stream);
    x->n = t.size();
    x->curve = d.curve;
    x->nan_count = d.nan_count;
    x->wide_levels = d.wide_levels;
    for (int l = 0; l < LBVH_WIDE_LEVELS; l++) x->wide_count[l] = d.wide_count[l];
    for (int a = 0; a < 6; a++) x->scene[a] = d.scene[a];
  });
}

int tknnDebugPoison(tknnEngine e, unsigned what, int byte, size_t min_workspace_bytes, int64_t *poisoned_bytes, void *stream) {
  return api("tknnDebugPoison", e, stream, [&](const Call &c) {
    c.require((what & ~TKNN_POISON_ALL) == 0u, "what has a bit no part of the scratch has");
    c.require(byte >= 0 && byte <= 255, "byte must be 0 .. 255");
    const int64_t filled = e->impl.debug_poison(what, byte, min_workspace_bytes, (hipStream_t)stream);
    if (poisoned_bytes) *poisoned_bytes = filled;
  });
}

// the debug entry points below need no engine

int tknnDebugBoxTree(const float *d_boxes, int64_t n, const float *d_boxes_refit, int mode, void *nodes, int32_t *rope_node,
                     int32_t *rope_leaf, int32_t *prim_id, float *sorted_boxes, void *stream) {
  return guarded([&] {
    const Call c{"tknnDebugBoxTree", nullptr};
    c.need(d_boxes, "d_boxes");
    c.count(n, "n", 1);
    c.require(mode >= 0 && mode <= 2, "mode must be 0, 1 or 2");
    const hipStream_t s = (hipStream_t)stream;
    owlmi::Lbvh tree;
    if (mode == 0) tree.build_from_boxes((const LbvhBox *)d_boxes, n, s);
    if (mode == 2) tree.build_from_points(d_boxes, 2 * n, s);
    if (d_boxes_refit || mode != 0) tree.refit_boxes((const LbvhBox *)(d_boxes_refit ? d_boxes_refit : d_boxes), s);
    tree.download((LbvhNode *)nodes, rope_node, rope_leaf, prim_id, s);
    if (sorted_boxes) tree.download_boxes((LbvhBox *)sorted_boxes, s);
    OWLMI_HIP(hipStreamSynchronize(s));
  });
}

int tknnDebugThresholds(const float *d_q, const float *d_r, int64_t n, float *d_lo, float *d_hi, void *stream) {
  return guarded([&] {
    const Call c{"tknnDebugThresholds", nullptr};
    c.need(d_q, "d_q"), c.need(d_r, "d_r"), c.need(d_lo, "d_lo"), c.need(d_hi, "d_hi");
    c.require(n >= 0, "n must not be negative");
    owlmi::debug_thresholds(d_q, d_r, n, d_lo, d_hi, (hipStream_t)stream);
    OWLMI_HIP(hipStreamSynchronize((hipStream_t)stream));
  });
}

int tknnDebugTeamLanes(int op, int variant, const uint32_t *d_in, uint32_t *d_out, int64_t teams, void *stream) {
  return guarded([&] {
    const Call c{"tknnDebugTeamLanes", nullptr};
    c.need(d_in, "d_in"), c.need(d_out, "d_out");
    c.require(teams >= 0 && teams <= TKNN_LANES_MAX_TEAMS, "need 0 <= teams <= 2^20");
    c.require(op >= 0 && op < TKNN_LANES_OPS, "no such op");
    c.require(owlmi::debug_team_lanes_words(op, variant, nullptr, nullptr), "the op has no such variant");
    if (teams == 0) return;
    owlmi::debug_team_lanes(op, variant, d_in, d_out, teams, (hipStream_t)stream);
    OWLMI_HIP(hipStreamSynchronize((hipStream_t)stream));
  });
}

}  // extern "C"
