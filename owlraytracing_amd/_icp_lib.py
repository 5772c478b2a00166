"""ctypes binding of tknnIcp (include/owlknn_icp.h), an entry point of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its two records and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

# include/owlknn_icp.h
METHODS = {"point_to_point": 0, "point_to_plane": 1}
ROBUST = {None: 0, "l2": 0, "huber": 1, "tukey": 2}


class IcpOptions(_lib._Record):
    _fields_ = [
        ("m", ctypes.c_int64),
        ("d_source", ctypes.c_void_p),
        ("d_target_normals", ctypes.c_void_p),
        ("init", ctypes.POINTER(ctypes.c_double)),
        ("max_dist", ctypes.c_float),
        ("robust_scale", ctypes.c_float),
        ("method", ctypes.c_int32),
        ("robust", ctypes.c_int32),
        ("max_iterations", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("rel_fitness", ctypes.c_double),
        ("rel_rmse", ctypes.c_double),
        ("d_corr", ctypes.c_void_p),
        ("d_corr_dist", ctypes.c_void_p),
        ("d_aligned", ctypes.c_void_p),
    ]


class IcpInfo(_lib._Record):
    _fields_ = [("transform", ctypes.c_double * 16), ("fitness", ctypes.c_double), ("inlier_rmse", ctypes.c_double),
                ("correspondences", ctypes.c_int64), ("skipped_pairs", ctypes.c_int64), ("node_tests", ctypes.c_int64),
                ("point_tests", ctypes.c_int64), ("lane_rows", ctypes.c_int64), ("iterations", ctypes.c_int32), ("searches", ctypes.c_int32),
                ("converged", ctypes.c_int32), ("degenerate", ctypes.c_int32), ("solve_ms", ctypes.c_float), ("search_ms", ctypes.c_float),
                ("moment_ms", ctypes.c_float), ("pad_", ctypes.c_int32)]


# every symbol include/owlknn_icp.h declares, with its signature
SIGNATURES = {
    "tknnIcp": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IcpOptions), ctypes.POINTER(IcpInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_icp.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
