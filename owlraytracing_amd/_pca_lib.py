"""ctypes binding of tknnLocalPca (include/owlknn_pca.h), an entry point of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its two records and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

# include/owlknn_pca.h
PCA_SKIP_SELF, PCA_ORIENT = 1, 2
# the outputs by the names TrueKNN.local_pca takes in ``want``: the record's field, the floats (or ints) per row
OUTPUTS = {"counts": ("d_counts", 1), "centroid": ("d_centroid", 3), "cov": ("d_cov", 6), "eigenvalues": ("d_eigenvalues", 3),
           "eigenvectors": ("d_eigenvectors", 9), "normals": ("d_normals", 3), "curvature": ("d_curvature", 1)}


class LocalPcaOptions(_lib._Record):
    _fields_ = [
        ("m", ctypes.c_int64),
        ("radius", ctypes.c_float),
        ("k", ctypes.c_int32),
        ("min_points", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("viewpoint", ctypes.c_float * 3),
        ("pad_", ctypes.c_int32),
        ("d_queries", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
        ("d_centroid", ctypes.c_void_p),
        ("d_cov", ctypes.c_void_p),
        ("d_eigenvalues", ctypes.c_void_p),
        ("d_eigenvectors", ctypes.c_void_p),
        ("d_normals", ctypes.c_void_p),
        ("d_curvature", ctypes.c_void_p),
    ]


class LocalPcaInfo(_lib._Record):
    _fields_ = [("total", ctypes.c_int64), ("max_row", ctypes.c_int64), ("degenerate_rows", ctypes.c_int64), ("fallback_items", ctypes.c_int64),
                ("node_tests", ctypes.c_int64), ("point_tests", ctypes.c_int64), ("solve_ms", ctypes.c_float), ("order_ms", ctypes.c_float),
                ("bound_ms", ctypes.c_float), ("walk_ms", ctypes.c_float), ("finish_ms", ctypes.c_float), ("pad_", ctypes.c_int32)]


# every symbol include/owlknn_pca.h declares, with its signature
SIGNATURES = {
    "tknnLocalPca": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LocalPcaOptions), ctypes.POINTER(LocalPcaInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_pca.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
