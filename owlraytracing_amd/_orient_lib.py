"""ctypes binding of tknnOrientNormals (include/owlknn_orient.h), an entry point of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its records and signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

# include/owlknn_orient.h
ORIENT_NO_EMST = 1


class OrientOptions(_lib._Record):
    _fields_ = [
        ("d_normals", ctypes.c_void_p),
        ("k", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("direction", ctypes.c_float * 3),
        ("max_rounds", ctypes.c_int32),
        ("d_out_normals", ctypes.c_void_p),
        ("d_flip", ctypes.c_void_p),
        ("d_component", ctypes.c_void_p),
        ("d_u", ctypes.c_void_p),
        ("d_v", ctypes.c_void_p),
        ("d_w", ctypes.c_void_p),
    ]


class OrientInfo(_lib._Record):
    _fields_ = [("candidates", ctypes.c_int64), ("tree_edges", ctypes.c_int64), ("components", ctypes.c_int64), ("excluded", ctypes.c_int64),
                ("flipped", ctypes.c_int64), ("rounds", ctypes.c_int32), ("reserved_", ctypes.c_int32), ("solve_ms", ctypes.c_float),
                ("knn_ms", ctypes.c_float), ("emst_ms", ctypes.c_float), ("sort_ms", ctypes.c_float), ("forest_ms", ctypes.c_float),
                ("apply_ms", ctypes.c_float)]


# every symbol include/owlknn_orient.h declares, with its signature
SIGNATURES = {
    "tknnOrientNormals": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(OrientOptions), ctypes.POINTER(OrientInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_orient.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
