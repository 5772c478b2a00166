"""ctypes binding of tknnRadiusNms (include/owlknn_nms.h), an entry point of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its two records and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

NMS_BY_NAME = 1  # include/owlknn_nms.h TKNN_NMS_BY_NAME


class RadiusNmsOptions(_lib._Record):
    _fields_ = [
        ("radius", ctypes.c_float),
        ("flags", ctypes.c_uint32),
        ("max_rounds", ctypes.c_int32),
        ("pad_", ctypes.c_int32),
        ("d_scores", ctypes.c_void_p),
        ("d_keep", ctypes.c_void_p),
        ("d_cover", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
    ]


class RadiusNmsInfo(_lib._Record):
    _fields_ = [("kept", ctypes.c_int64), ("eligible", ctypes.c_int64), ("bad_scores", ctypes.c_int64), ("rounds", ctypes.c_int64),
                ("fallback_items", ctypes.c_int64), ("undecided", ctypes.c_int64), ("point_tests", ctypes.c_int64), ("node_tests", ctypes.c_int64),
                ("solve_ms", ctypes.c_float), ("init_ms", ctypes.c_float), ("rounds_ms", ctypes.c_float), ("cover_ms", ctypes.c_float)]


# every symbol include/owlknn_nms.h declares, with its signature
SIGNATURES = {
    "tknnRadiusNms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RadiusNmsOptions), ctypes.POINTER(RadiusNmsInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_nms.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
