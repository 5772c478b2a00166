"""ctypes binding of tknnPeriodicKnn (include/owlknn_periodic.h), an entry point of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its two records and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib


class PeriodicKnnOptions(_lib._Record):
    _fields_ = [
        ("d_queries", ctypes.c_void_p),
        ("m", ctypes.c_int64),
        ("k", ctypes.c_int32),
        ("radius", ctypes.c_float),
        ("d_radii", ctypes.c_void_p),
        ("d_skip_ids", ctypes.c_void_p),
        ("lo", ctypes.c_float * 3),
        ("period", ctypes.c_float * 3),
        ("d_idx", ctypes.c_void_p),
        ("d_dist", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
    ]


class PeriodicKnnInfo(_lib._Record):
    _fields_ = [("total", ctypes.c_int64), ("full_rows", ctypes.c_int64), ("node_tests", ctypes.c_int64),
                ("point_tests", ctypes.c_int64), ("seed_point_tests", ctypes.c_int64), ("tightened_rows", ctypes.c_int64),
                ("lane_rows", ctypes.c_int64), ("solve_ms", ctypes.c_float), ("order_ms", ctypes.c_float),
                ("seed_ms", ctypes.c_float), ("walk_ms", ctypes.c_float)]


# every symbol include/owlknn_periodic.h declares, with its signature
SIGNATURES = {
    "tknnPeriodicKnn": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(PeriodicKnnOptions), ctypes.POINTER(PeriodicKnnInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_periodic.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
