"""ctypes binding of tknnFpfh (include/owlknn_fpfh.h), an entry point of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its two records and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

# include/owlknn_fpfh.h
FPFH_NO_SELF_TERM = 1
FPFH_BINS = 33


class FpfhOptions(_lib._Record):
    _fields_ = [
        ("radius", ctypes.c_float),
        ("flags", ctypes.c_uint32),
        ("d_normals", ctypes.c_void_p),
        ("d_fpfh", ctypes.c_void_p),
        ("d_spfh", ctypes.c_void_p),
        ("d_spfh_counts", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
    ]


class FpfhInfo(_lib._Record):
    _fields_ = [("total", ctypes.c_int64), ("max_row", ctypes.c_int64), ("skipped_pairs", ctypes.c_int64), ("fallback_items", ctypes.c_int64),
                ("node_tests", ctypes.c_int64), ("point_tests", ctypes.c_int64), ("solve_ms", ctypes.c_float), ("stage_ms", ctypes.c_float),
                ("spfh_ms", ctypes.c_float), ("fpfh_ms", ctypes.c_float), ("finish_ms", ctypes.c_float), ("pad_", ctypes.c_int32)]


# every symbol include/owlknn_fpfh.h declares, with its signature
SIGNATURES = {
    "tknnFpfh": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(FpfhOptions), ctypes.POINTER(FpfhInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_fpfh.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
