"""ctypes binding of libowl_mi355x.so (the C-ABI declared in include/owlknn.h).

There is no fallback: if the library has not been built, or no MI355X is visible when an engine is
created, the call raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C owlraytracing_amd/csrc``.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OWL_MI355X_LIB") or os.path.join(_HERE, "libowl_mi355x.so")  # override: diagnostic builds

KERNEL_AUTO, KERNEL_LANE, KERNEL_WAVE, KERNEL_TEAM = 0, 1, 2, 3
KERNEL_QUERY = 4  # info["kernel_used"] of tknnQuery; not a selector for solve
MAX_K = 1024  # include/owlknn.h TKNN_MAX_K (k <= 64: register lists; above: the team walk with the lists in memory)


class TknnError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("tknn error %d: %s" % (code, message))
        self.code = code


class _Record(ctypes.Structure):
    """A record of include/owlknn.h."""

    def as_dict(self):
        """The record's fields by name, without its reserved_ and pad_ words."""
        return {name: getattr(self, name) for name, _ in self._fields_ if name not in ("reserved_", "pad_")}


class SolveInfo(_Record):
    _fields_ = [
        ("rounds", ctypes.c_int32),
        ("final_radius", ctypes.c_float),
        ("total_intersections", ctypes.c_int64),
        ("node_tests", ctypes.c_int64),
        ("point_tests", ctypes.c_int64),
        ("total_active_rounds", ctypes.c_int64),
        ("solve_ms", ctypes.c_float),
        ("dominant_kernel_ms", ctypes.c_float),
        ("dominant_kernel_launches", ctypes.c_int32),
        ("kernel_used", ctypes.c_int32),
        ("list_capacity", ctypes.c_int32),
        ("unfinished", ctypes.c_int64),
        ("tie_rows", ctypes.c_int64),
        ("tie_rows_left", ctypes.c_int64),
        ("tie_ms", ctypes.c_float),
        ("reserved_", ctypes.c_int32),
    ]


class SolveOptions(_Record):
    _fields_ = [
        ("k", ctypes.c_int32),
        ("start_radius", ctypes.c_float),
        ("kernel", ctypes.c_int32),
        ("max_rounds", ctypes.c_int32),
        ("allow_unfinished", ctypes.c_int32),
        ("phase", ctypes.c_int32),
        ("d_idx", ctypes.c_void_p),
        ("d_dist", ctypes.c_void_p),
        ("d_intersections", ctypes.c_void_p),
        ("d_fb", ctypes.c_void_p),
        ("d_levels", ctypes.c_void_p),
        ("d_start_radii", ctypes.c_void_p),
    ]


class QueryOptions(_Record):
    _fields_ = [
        ("d_queries", ctypes.c_void_p),
        ("m", ctypes.c_int64),
        ("k", ctypes.c_int32),
        ("start_radius", ctypes.c_float),
        ("max_rounds", ctypes.c_int32),
        ("allow_unfinished", ctypes.c_int32),
        ("exact", ctypes.c_int32),
        ("reserved_", ctypes.c_int32),
        ("d_idx", ctypes.c_void_p),
        ("d_dist", ctypes.c_void_p),
        ("d_intersections", ctypes.c_void_p),
        ("d_levels", ctypes.c_void_p),
    ]


class DbscanQueryOptions(_Record):
    _fields_ = [
        ("d_queries", ctypes.c_void_p),
        ("m", ctypes.c_int64),
        ("eps", ctypes.c_float),
        ("reserved_", ctypes.c_int32),
        ("d_core_label", ctypes.c_void_p),
        ("d_labels", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
    ]


class RadiusOptions(_Record):
    _fields_ = [
        ("d_queries", ctypes.c_void_p),
        ("m", ctypes.c_int64),
        ("radius", ctypes.c_float),
        ("sort", ctypes.c_int32),
        ("d_offsets", ctypes.c_void_p),
        ("d_idx", ctypes.c_void_p),
        ("d_dist", ctypes.c_void_p),
        ("capacity", ctypes.c_int64),
    ]


class RadiusInfo(_Record):
    _fields_ = [("total", ctypes.c_int64), ("max_row", ctypes.c_int64), ("mismatched", ctypes.c_int64),
                ("node_tests", ctypes.c_int64), ("point_tests", ctypes.c_int64), ("solve_ms", ctypes.c_float),
                ("order_ms", ctypes.c_float), ("walk_ms", ctypes.c_float), ("sort_ms", ctypes.c_float)]


class RadiusKnnOptions(_Record):
    _fields_ = [
        ("d_queries", ctypes.c_void_p),
        ("m", ctypes.c_int64),
        ("k", ctypes.c_int32),
        ("radius", ctypes.c_float),
        ("d_radii", ctypes.c_void_p),
        ("d_skip_ids", ctypes.c_void_p),
        ("d_idx", ctypes.c_void_p),
        ("d_dist", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
    ]


class RadiusKnnInfo(_Record):
    _fields_ = [("total", ctypes.c_int64), ("full_rows", ctypes.c_int64), ("node_tests", ctypes.c_int64),
                ("point_tests", ctypes.c_int64), ("lane_rows", ctypes.c_int64), ("solve_ms", ctypes.c_float),
                ("order_ms", ctypes.c_float), ("walk_ms", ctypes.c_float), ("reserved_", ctypes.c_int32)]


class DbscanInfo(_Record):
    _fields_ = [("clusters", ctypes.c_int32), ("solve_ms", ctypes.c_float), ("core_ms", ctypes.c_float),
                ("union_ms", ctypes.c_float), ("label_ms", ctypes.c_float), ("union_launches", ctypes.c_int32),
                ("node_tests", ctypes.c_int64), ("point_tests", ctypes.c_int64), ("core_point_tests", ctypes.c_int64),
                ("union_point_tests", ctypes.c_int64), ("label_point_tests", ctypes.c_int64),
                ("union_node_tests", ctypes.c_int64), ("groups", ctypes.c_int64)]


class DbscanAutoInfo(_Record):
    _fields_ = [("last", DbscanInfo), ("rounds", ctypes.c_int32), ("eps", ctypes.c_float), ("noise", ctypes.c_int64),
                ("probe_ms", ctypes.c_float), ("pad_", ctypes.c_int32)]

    def as_dict(self):
        d = {"rounds": self.rounds, "eps": self.eps, "noise": self.noise, "probe_ms": self.probe_ms}
        d.update(self.last.as_dict())
        return d


class BuildInfo(_Record):
    _fields_ = [("build_ms", ctypes.c_float), ("device_bytes", ctypes.c_int64), ("n", ctypes.c_int32)]


class TreeExport(_Record):
    _fields_ = [("which", ctypes.c_int32), ("curve", ctypes.c_int32), ("n", ctypes.c_int64), ("nan_count", ctypes.c_int32),
                ("wide_levels", ctypes.c_int32), ("wide_count", ctypes.c_int32 * 6), ("scene", ctypes.c_float * 6),
                ("wide_capacity", ctypes.c_int64), ("keys", ctypes.c_void_p), ("points", ctypes.c_void_p),
                ("row_slot", ctypes.c_void_p), ("wide_boxes", ctypes.c_void_p), ("nodes", ctypes.c_void_p),
                ("rope_node", ctypes.c_void_p), ("rope_leaf", ctypes.c_void_p), ("prim_id", ctypes.c_void_p),
                ("split_owner", ctypes.c_void_p)]


# every symbol include/owlknn.h declares, with its signature
SIGNATURES = {
    "tknnLastError": (ctypes.c_char_p, []),
    "tknnDeviceCount": (ctypes.c_int, []),
    "tknnCreate": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p)]),
    "tknnDestroy": (None, [ctypes.c_void_p]),
    "tknnBuild": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                 ctypes.POINTER(BuildInfo), ctypes.c_void_p]),
    "tknnSolve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.POINTER(SolveInfo), ctypes.c_void_p]),
    "tknnBuildIds": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                    ctypes.POINTER(BuildInfo), ctypes.c_void_p]),
    "tknnSetHalo": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                   ctypes.c_void_p]),
    "tknnSolveEx": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SolveOptions), ctypes.POINTER(SolveInfo),
                                   ctypes.c_void_p]),
    "tknnHaloSelect": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tknnRepairExact": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    "tknnQuery": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(QueryOptions), ctypes.POINTER(SolveInfo), ctypes.c_void_p]),
    "tknnDbscan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.POINTER(DbscanInfo), ctypes.c_void_p]),
    "tknnDbscanAssign": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.POINTER(DbscanInfo), ctypes.c_void_p]),
    "tknnDbscanQuery": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(DbscanQueryOptions), ctypes.POINTER(DbscanInfo), ctypes.c_void_p]),
    "tknnRadiusQuery": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RadiusOptions), ctypes.POINTER(RadiusInfo), ctypes.c_void_p]),
    "tknnRadiusKnn": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RadiusKnnOptions), ctypes.POINTER(RadiusKnnInfo), ctypes.c_void_p]),
    "tknnDbscanAuto": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.POINTER(DbscanAutoInfo), ctypes.c_void_p]),
    "tknnHaloSelectFixed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tknnSegmentMin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "tknnDbscanNoise": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                       ctypes.c_void_p]),
    "tknnExportTree": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tknnExportTreeTables": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tknnExportTreeEx": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(TreeExport), ctypes.c_void_p]),
    "tknnDebugBoxTree": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tknnDebugThresholds": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
}

_lib = None


def load():
    """Load the shared library (no GPU needed for loading itself).

    Order matters in a process that also uses torch: torch brings a HIP runtime of its own, the library is linked against the
    system's.  With torch imported first the library binds to torch's runtime and both see the GPU; with the library loaded
    first the process holds two runtimes, and the one that starts second reports "no ROCm-capable device is detected"
    (tknnCreate then returns TKNN_E_HIP).  Import torch before the first call of load()."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: build the HIP extension first (make -C owlraytracing_amd/csrc); "
                "there is no CPU fallback" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise TknnError(rc, (load().tknnLastError() or b"").decode())


# native sources a kernel's code does NOT depend on, by kernel-name prefix (the FIRST matching prefix counts: team_walk_ stands
# before team_): a committed profile of the packet kernel stays valid when only the tie pass, the k > 64 walk or the
# clustering kernels change, and the other way round; one of the label pass when only the union pass changes; every one when
# only the C ABI's argument checks and messages (tknn_api.hip, which holds no kernel) change
_NOT_TEAM = ("dbscan.hip", "dbscan_core.hip", "dbscan_union.hip", "dbscan_label.hip", "db_device.h", "db_call.h", "halo_select.hip", "radius_query.hip", "radius_walk.h",
             "radius_knn.hip", "radius_knn_walk.h", "knn_seed.hip", "owlknn_knn.h", "periodic_knn.hip", "periodic_metric.h", "owlknn_periodic.h", "batch_knn.hip", "owlknn_batch.h",
             "emst.hip", "owlknn_emst.h", "linkage.hip", "linkage.h", "hdbscan.hip", "owlknn_hdbscan.h", "tknn_api.hip", "owl_runtime.cpp",
             "debug_lanes.hip")  # (the lane harness of tknnDebugTeamLanes: kernels of its own around the shared headers)
# RT-DBSCAN's kernels are in three files by pass; dbscan.hip, the host side that decides their grids and arguments, counts for all
_NOT_DB = ("trueknn_team.hip", "trueknn_tail.hip", "trueknn_bigk.hip", "trueknn_wave.hip", "halo_select.hip", "radius_query.hip", "radius_walk.h", "radius_knn.hip",
           "radius_knn_walk.h", "knn_seed.hip", "owlknn_knn.h", "periodic_knn.hip", "periodic_metric.h", "owlknn_periodic.h", "batch_knn.hip",
           "owlknn_batch.h", "emst.hip", "owlknn_emst.h", "linkage.hip", "linkage.h", "hdbscan.hip", "owlknn_hdbscan.h", "tknn_api.hip", "owl_runtime.cpp",
           "debug_lanes.hip", "bigk_keys.h")
_NOT_DB_CORE, _NOT_DB_UNION = _NOT_DB + ("dbscan_union.hip", "dbscan_label.hip"), _NOT_DB + ("dbscan_core.hip", "dbscan_label.hip")
_NOT_IN = {
    "team_walk_": _NOT_TEAM + ("trueknn_team.hip", "trueknn_bigk.hip", "bigk_keys.h"),  # trueknn_tail.hip
    "tie_fix_": _NOT_TEAM + ("trueknn_team.hip", "trueknn_bigk.hip", "bigk_keys.h"),
    "bigk_": _NOT_TEAM + ("trueknn_team.hip", "trueknn_tail.hip"),  # trueknn_bigk.hip
    "team_": _NOT_TEAM + ("trueknn_tail.hip", "trueknn_bigk.hip", "bigk_keys.h"),  # trueknn_team.hip: team_kernel, team_prep_kernel
    "db_core_": _NOT_DB_CORE,  # dbscan_core.hip: db_core_kernel, db_core_pos_blocks_kernel, db_core_from_labels_kernel
    "db_flag_count_": _NOT_DB_CORE,
    "db_next_core_": _NOT_DB_CORE,
    "db_noise_probe_": _NOT_DB_CORE,
    "db_union_": _NOT_DB_UNION,  # dbscan_union.hip
    "db_group_": _NOT_DB_UNION,  # db_group_kernel, db_group_list_kernel, db_group_union_kernel
    "db_uniform_": _NOT_DB_UNION,
    "db_": _NOT_DB + ("dbscan_core.hip", "dbscan_union.hip"),  # dbscan_label.hip: every other db_ kernel (db_rows_kernel and db_rows_from_slots_kernel among them)
}


def source_fingerprint(kernel=None):
    """16 hex digits naming the native sources the library -- or, with `kernel`, that kernel -- is built from (csrc/ and
    include/owlknn.h, include/owl/lbvh_device.h; without `kernel` also the other owl headers): what a committed rocprofv3 record must carry for bench.py
    to attach it to a run (profiles/hbm_traffic.json)."""
    import glob
    import hashlib

    root = os.path.dirname(_HERE)
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h"))
                   + glob.glob(os.path.join(_HERE, "csrc", "*.cpp")) + glob.glob(os.path.join(_HERE, "csrc", "Makefile"))
                   + glob.glob(os.path.join(root, "include", "**", "*.h"), recursive=True))
    if kernel is not None:
        skip = next((v for k, v in _NOT_IN.items() if kernel.startswith(k)), ())
        owl_headers = os.path.join(root, "include", "owl") + os.sep
        files = [f for f in files if os.path.basename(f) not in skip
                 and (not f.startswith(owl_headers) or os.path.basename(f) == "lbvh_device.h")]  # the tree's device layout
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, root).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]
