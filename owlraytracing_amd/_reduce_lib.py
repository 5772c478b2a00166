"""ctypes binding of tknnRadiusReduce (include/owlknn_reduce.h), an entry point of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its two records and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

# include/owlknn_reduce.h
REDUCE_NORMALIZE, REDUCE_SKIP_SELF = 1, 2
W_ONE, W_GAUSS, W_EPANECHNIKOV, W_CUBIC_SPLINE = 0, 1, 2, 3
WEIGHTS = {"one": W_ONE, "gauss": W_GAUSS, "epanechnikov": W_EPANECHNIKOV, "cubic_spline": W_CUBIC_SPLINE}
MAX_CHANNELS = 16  # TKNN_REDUCE_MAX_CHANNELS


class RadiusReduceOptions(_lib._Record):
    _fields_ = [
        ("m", ctypes.c_int64),
        ("radius", ctypes.c_float),
        ("bandwidth", ctypes.c_float),
        ("weight", ctypes.c_int32),
        ("channels", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("pad_", ctypes.c_int32),
        ("d_queries", ctypes.c_void_p),
        ("d_values", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
        ("d_wsum", ctypes.c_void_p),
        ("d_out", ctypes.c_void_p),
    ]


class RadiusReduceInfo(_lib._Record):
    _fields_ = [("total", ctypes.c_int64), ("max_row", ctypes.c_int64), ("fallback_items", ctypes.c_int64), ("node_tests", ctypes.c_int64),
                ("point_tests", ctypes.c_int64), ("solve_ms", ctypes.c_float), ("order_ms", ctypes.c_float), ("stage_ms", ctypes.c_float),
                ("walk_ms", ctypes.c_float)]


# every symbol include/owlknn_reduce.h declares, with its signature
SIGNATURES = {
    "tknnRadiusReduce": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RadiusReduceOptions), ctypes.POINTER(RadiusReduceInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_reduce.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
