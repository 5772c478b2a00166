"""ctypes binding of tknnFeatureMatch and tknnRansac (include/owlknn_global.h), entry points of libowl_mi355x.so next to the C-ABI
of include/owlknn.h: their records and signatures.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

# include/owlknn_global.h
MATCH_MAX_D = 64
RANSAC_BATCH = 4096
STATUS = ("ok", "duplicate", "edge", "degenerate", "far")  # TKNN_RANSAC_OK .. TKNN_RANSAC_FAR


class FeatureMatchOptions(_lib._Record):
    _fields_ = [
        ("m", ctypes.c_int64),
        ("n", ctypes.c_int64),
        ("d_source", ctypes.c_void_p),
        ("d_target", ctypes.c_void_p),
        ("D", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("d_best", ctypes.c_void_p),
        ("d_best_d2", ctypes.c_void_p),
        ("d_second_d2", ctypes.c_void_p),
    ]


class FeatureMatchInfo(_lib._Record):
    _fields_ = [("pair_tests", ctypes.c_int64), ("bad_source_rows", ctypes.c_int64), ("bad_target_rows", ctypes.c_int64), ("chunks", ctypes.c_int32),
                ("solve_ms", ctypes.c_float), ("match_ms", ctypes.c_float), ("merge_ms", ctypes.c_float)]


class RansacOptions(_lib._Record):
    _fields_ = [
        ("ms", ctypes.c_int64),
        ("mt", ctypes.c_int64),
        ("c", ctypes.c_int64),
        ("d_source", ctypes.c_void_p),
        ("d_target", ctypes.c_void_p),
        ("d_pairs", ctypes.c_void_p),
        ("ransac_n", ctypes.c_int32),
        ("max_dist", ctypes.c_float),
        ("edge_similarity", ctypes.c_float),
        ("max_trials", ctypes.c_int32),
        ("confidence", ctypes.c_double),
        ("seed", ctypes.c_uint32),
        ("refit_rounds", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("pad_", ctypes.c_int32),
        ("d_inlier_mask", ctypes.c_void_p),
        ("d_trial_status", ctypes.c_void_p),
        ("d_trial_inliers", ctypes.c_void_p),
    ]


class RansacInfo(_lib._Record):
    _fields_ = [("transform", ctypes.c_double * 16), ("fitness", ctypes.c_double), ("inlier_rmse", ctypes.c_double), ("inliers", ctypes.c_int64),
                ("status_counts", ctypes.c_int64 * 5), ("best_trial", ctypes.c_int32), ("trials_run", ctypes.c_int32), ("batches", ctypes.c_int32),
                ("refits_kept", ctypes.c_int32), ("solve_ms", ctypes.c_float), ("sample_ms", ctypes.c_float), ("score_ms", ctypes.c_float),
                ("refit_ms", ctypes.c_float)]


# every symbol include/owlknn_global.h declares, with its signature
SIGNATURES = {
    "tknnFeatureMatch": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(FeatureMatchOptions), ctypes.POINTER(FeatureMatchInfo), ctypes.c_void_p]),
    "tknnRansac": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RansacOptions), ctypes.POINTER(RansacInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_global.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
