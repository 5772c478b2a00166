"""ctypes binding of tknnSegmentPlane (include/owlknn_plane.h), an entry point of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its records and signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

# include/owlknn_plane.h
PLANE_BATCH = 1024
PLANE_OK, PLANE_DUPLICATE, PLANE_DEGENERATE, PLANE_ANGLE = 0, 1, 2, 3
STATUS = ("ok", "duplicate", "degenerate", "angle")


class PlaneOptions(_lib._Record):
    _fields_ = [
        ("d_active", ctypes.c_void_p),
        ("distance_threshold", ctypes.c_float),
        ("min_cos", ctypes.c_float),
        ("axis", ctypes.c_float * 3),
        ("max_trials", ctypes.c_int32),
        ("confidence", ctypes.c_double),
        ("seed", ctypes.c_uint32),
        ("refit_rounds", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("pad_", ctypes.c_int32),
        ("d_inlier_mask", ctypes.c_void_p),
        ("d_inlier_rows", ctypes.c_void_p),
        ("d_trial_status", ctypes.c_void_p),
        ("d_trial_inliers", ctypes.c_void_p),
    ]


class PlaneInfo(_lib._Record):
    _fields_ = [
        ("plane", ctypes.c_double * 4),
        ("fitness", ctypes.c_double),
        ("inlier_rmse", ctypes.c_double),
        ("inliers", ctypes.c_int64),
        ("active", ctypes.c_int64),
        ("status_counts", ctypes.c_int64 * 4),
        ("node_tests", ctypes.c_int64),
        ("point_tests", ctypes.c_int64),
        ("boxes_counted", ctypes.c_int64),
        ("lane_rows", ctypes.c_int64),
        ("normal", ctypes.c_float * 3),
        ("anchor", ctypes.c_float * 3),
        ("best_trial", ctypes.c_int32),
        ("trials_run", ctypes.c_int32),
        ("batches", ctypes.c_int32),
        ("refits_kept", ctypes.c_int32),
        ("solve_ms", ctypes.c_float),
        ("sample_ms", ctypes.c_float),
        ("score_ms", ctypes.c_float),
        ("refit_ms", ctypes.c_float),
    ]


# every symbol include/owlknn_plane.h declares, with its signature
SIGNATURES = {
    "tknnSegmentPlane": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(PlaneOptions), ctypes.POINTER(PlaneInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_plane.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
