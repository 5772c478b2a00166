"""ctypes binding of tknnFps (include/owlknn_fps.h), an entry point of libowl_mi355x.so next to the C-ABI of include/owlknn.h:
its two records and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

FPS_NO_PRUNE = 1  # include/owlknn_fps.h TKNN_FPS_NO_PRUNE


class FpsOptions(_lib._Record):
    _fields_ = [
        ("num_samples", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("d_num", ctypes.c_void_p),
        ("d_start_rows", ctypes.c_void_p),
        ("d_idx", ctypes.c_void_p),
        ("d_dist", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
    ]


class FpsInfo(_lib._Record):
    _fields_ = [("samples", ctypes.c_int64), ("point_tests", ctypes.c_int64), ("node_tests", ctypes.c_int64),
                ("bad_starts", ctypes.c_int64), ("lds_clouds", ctypes.c_int64), ("solve_ms", ctypes.c_float),
                ("init_ms", ctypes.c_float), ("walk_ms", ctypes.c_float)]


# every symbol include/owlknn_fps.h declares, with its signature
SIGNATURES = {
    "tknnFps": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(FpsOptions), ctypes.POINTER(FpsInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_fps.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
