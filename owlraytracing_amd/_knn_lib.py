"""ctypes binding of tknnKnn (include/owlknn_knn.h), an entry point of libowl_mi355x.so next to the C-ABI of include/owlknn.h:
its two records and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib


class KnnOptions(_lib._Record):
    _fields_ = [
        ("d_queries", ctypes.c_void_p),
        ("m", ctypes.c_int64),
        ("k", ctypes.c_int32),
        ("reserved_", ctypes.c_int32),
        ("d_skip_ids", ctypes.c_void_p),
        ("d_idx", ctypes.c_void_p),
        ("d_dist", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
    ]


class KnnInfo(_lib._Record):
    _fields_ = [("total", ctypes.c_int64), ("full_rows", ctypes.c_int64), ("node_tests", ctypes.c_int64),
                ("point_tests", ctypes.c_int64), ("seed_point_tests", ctypes.c_int64), ("tightened_rows", ctypes.c_int64),
                ("lane_rows", ctypes.c_int64), ("solve_ms", ctypes.c_float), ("order_ms", ctypes.c_float),
                ("seed_ms", ctypes.c_float), ("walk_ms", ctypes.c_float)]


# every symbol include/owlknn_knn.h declares, with its signature
SIGNATURES = {
    "tknnKnn": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(KnnOptions), ctypes.POINTER(KnnInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_knn.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
