"""ctypes binding of tknnBuildBatched, tknnBatchLayout and tknnBatchKnn (include/owlknn_batch.h), entry points of
libowl_mi355x.so next to the C-ABI of include/owlknn.h: their two records and their signatures.  The handle is _lib.load()'s;
there is no fallback."""
import ctypes

from . import _lib

MAX_BATCHES = 32768  # include/owlknn_batch.h TKNN_MAX_BATCHES


class BatchKnnOptions(_lib._Record):
    _fields_ = [
        ("d_queries", ctypes.c_void_p),
        ("m", ctypes.c_int64),
        ("k", ctypes.c_int32),
        ("radius", ctypes.c_float),
        ("d_radii", ctypes.c_void_p),
        ("d_skip_ids", ctypes.c_void_p),
        ("d_query_batch", ctypes.c_void_p),
        ("d_idx", ctypes.c_void_p),
        ("d_dist", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
    ]


class BatchKnnInfo(_lib._Record):
    _fields_ = [("total", ctypes.c_int64), ("full_rows", ctypes.c_int64), ("node_tests", ctypes.c_int64),
                ("point_tests", ctypes.c_int64), ("seed_point_tests", ctypes.c_int64), ("tightened_rows", ctypes.c_int64),
                ("lane_rows", ctypes.c_int64), ("solve_ms", ctypes.c_float), ("order_ms", ctypes.c_float),
                ("seed_ms", ctypes.c_float), ("walk_ms", ctypes.c_float)]


# every symbol include/owlknn_batch.h declares, with its signature
SIGNATURES = {
    "tknnBuildBatched": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                        ctypes.POINTER(_lib.BuildInfo), ctypes.c_void_p]),
    "tknnBatchLayout": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "tknnBatchKnn": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(BatchKnnOptions), ctypes.POINTER(BatchKnnInfo), ctypes.c_void_p]),
}

_bound = None


def key_bits(num_batches):
    """The bits the labels of ``num_batches`` batches take at the top of the tree's keys: the smallest multiple of 3 with
    2**bits >= num_batches (the key loses whole levels of cells)."""
    bits = 0
    while (1 << bits) < num_batches:
        bits += 3
    return bits


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_batch.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
