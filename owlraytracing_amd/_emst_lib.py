"""ctypes binding of tknnEmst (include/owlknn_emst.h), an entry point of libowl_mi355x.so next to the C-ABI of include/owlknn.h:
its two records and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib


class EmstOptions(_lib._Record):
    _fields_ = [
        ("d_core_dist", ctypes.c_void_p),
        ("d_u", ctypes.c_void_p),
        ("d_v", ctypes.c_void_p),
        ("d_w", ctypes.c_void_p),
        ("d_component", ctypes.c_void_p),
        ("max_rounds", ctypes.c_int32),
        ("reserved_", ctypes.c_int32),
    ]


class EmstInfo(_lib._Record):
    _fields_ = [("edges", ctypes.c_int64), ("components", ctypes.c_int64), ("excluded", ctypes.c_int64),
                ("node_tests", ctypes.c_int64), ("point_tests", ctypes.c_int64), ("skipped_subtrees", ctypes.c_int64),
                ("rounds", ctypes.c_int32), ("reserved_", ctypes.c_int32), ("solve_ms", ctypes.c_float),
                ("walk_ms", ctypes.c_float), ("merge_ms", ctypes.c_float), ("sort_ms", ctypes.c_float)]


# every symbol include/owlknn_emst.h declares, with its signature
SIGNATURES = {
    "tknnEmst": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(EmstOptions), ctypes.POINTER(EmstInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_emst.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
