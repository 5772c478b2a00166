"""ctypes binding of tknnMeanShift (include/owlknn_meanshift.h), an entry point of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its two records and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib
from ._reduce_lib import W_EPANECHNIKOV, W_GAUSS, W_ONE

# include/owlknn_meanshift.h
MS_RUNNING, MS_CONVERGED, MS_EMPTY, MS_INVALID = 0, 1, 2, 3
KERNELS = {"flat": W_ONE, "gauss": W_GAUSS, "epanechnikov": W_EPANECHNIKOV}
OUTPUTS = ("modes", "counts", "wsum", "shift", "iterations", "status")


class MeanShiftOptions(_lib._Record):
    _fields_ = [
        ("m", ctypes.c_int64),
        ("d_seeds", ctypes.c_void_p),
        ("radius", ctypes.c_float),
        ("bandwidth", ctypes.c_float),
        ("tol", ctypes.c_float),
        ("weight", ctypes.c_int32),
        ("max_iterations", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("d_modes", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
        ("d_wsum", ctypes.c_void_p),
        ("d_shift", ctypes.c_void_p),
        ("d_iterations", ctypes.c_void_p),
        ("d_status", ctypes.c_void_p),
    ]


class MeanShiftInfo(_lib._Record):
    _fields_ = [("iterations", ctypes.c_int64), ("walks", ctypes.c_int64), ("converged", ctypes.c_int64), ("empty", ctypes.c_int64),
                ("running", ctypes.c_int64), ("invalid", ctypes.c_int64), ("fallback_items", ctypes.c_int64), ("node_tests", ctypes.c_int64),
                ("point_tests", ctypes.c_int64), ("solve_ms", ctypes.c_float), ("order_ms", ctypes.c_float), ("walk_ms", ctypes.c_float),
                ("compact_ms", ctypes.c_float)]


# every symbol include/owlknn_meanshift.h declares, with its signature
SIGNATURES = {
    "tknnMeanShift": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(MeanShiftOptions), ctypes.POINTER(MeanShiftInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_meanshift.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
