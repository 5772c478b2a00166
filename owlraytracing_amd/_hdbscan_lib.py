"""ctypes binding of tknnLinkage, tknnHdbscanLabels and tknnHdbscan (include/owlknn_hdbscan.h), entry points of libowl_mi355x.so
next to the C-ABI of include/owlknn.h: their records and signatures.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib


class LinkageOptions(_lib._Record):
    _fields_ = [
        ("n", ctypes.c_int64),
        ("edges", ctypes.c_int64),
        ("d_u", ctypes.c_void_p),
        ("d_v", ctypes.c_void_p),
        ("d_w", ctypes.c_void_p),
        ("d_parent", ctypes.c_void_p),
        ("d_left", ctypes.c_void_p),
        ("d_right", ctypes.c_void_p),
        ("d_size", ctypes.c_void_p),
        ("max_rounds", ctypes.c_int32),
        ("reserved_", ctypes.c_int32),
    ]


class LinkageInfo(_lib._Record):
    _fields_ = [("absorbed", ctypes.c_int64), ("host_edges", ctypes.c_int64), ("roots", ctypes.c_int64), ("rounds", ctypes.c_int32),
                ("reserved_", ctypes.c_int32), ("solve_ms", ctypes.c_float), ("pad_", ctypes.c_float)]


class HdbscanLabelsOptions(_lib._Record):
    _fields_ = [
        ("n", ctypes.c_int64),
        ("edges", ctypes.c_int64),
        ("d_u", ctypes.c_void_p),
        ("d_v", ctypes.c_void_p),
        ("d_w", ctypes.c_void_p),
        ("min_cluster_size", ctypes.c_int32),
        ("max_rounds", ctypes.c_int32),
        ("d_labels", ctypes.c_void_p),
        ("d_parent", ctypes.c_void_p),
        ("d_left", ctypes.c_void_p),
        ("d_right", ctypes.c_void_p),
        ("d_size", ctypes.c_void_p),
        ("d_lambda", ctypes.c_void_p),
        ("d_stability", ctypes.c_void_p),
    ]


class HdbscanLabelsInfo(_lib._Record):
    _fields_ = [("clusters", ctypes.c_int64), ("noise", ctypes.c_int64), ("condensed_clusters", ctypes.c_int64), ("absorbed", ctypes.c_int64),
                ("host_edges", ctypes.c_int64), ("rounds", ctypes.c_int32), ("reserved_", ctypes.c_int32), ("solve_ms", ctypes.c_float),
                ("linkage_ms", ctypes.c_float), ("condense_ms", ctypes.c_float), ("select_ms", ctypes.c_float), ("label_ms", ctypes.c_float),
                ("pad_", ctypes.c_float)]


class HdbscanOptions(_lib._Record):
    _fields_ = [
        ("min_cluster_size", ctypes.c_int32),
        ("min_samples", ctypes.c_int32),
        ("max_rounds", ctypes.c_int32),
        ("reserved_", ctypes.c_int32),
        ("d_labels", ctypes.c_void_p),
        ("d_core_dist", ctypes.c_void_p),
        ("d_u", ctypes.c_void_p),
        ("d_v", ctypes.c_void_p),
        ("d_w", ctypes.c_void_p),
        ("d_parent", ctypes.c_void_p),
        ("d_left", ctypes.c_void_p),
        ("d_right", ctypes.c_void_p),
        ("d_size", ctypes.c_void_p),
        ("d_lambda", ctypes.c_void_p),
        ("d_stability", ctypes.c_void_p),
    ]


class HdbscanInfo(_lib._Record):
    _fields_ = [("labels", HdbscanLabelsInfo), ("edges", ctypes.c_int64), ("excluded", ctypes.c_int64), ("knn_ms", ctypes.c_float),
                ("emst_ms", ctypes.c_float)]

    def as_dict(self):
        d = self.labels.as_dict()
        d.update(edges=self.edges, excluded=self.excluded, knn_ms=self.knn_ms, emst_ms=self.emst_ms)
        return d


# every symbol include/owlknn_hdbscan.h declares, with its signature
SIGNATURES = {
    "tknnLinkage": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LinkageOptions), ctypes.POINTER(LinkageInfo), ctypes.c_void_p]),
    "tknnHdbscanLabels": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HdbscanLabelsOptions), ctypes.POINTER(HdbscanLabelsInfo), ctypes.c_void_p]),
    "tknnHdbscan": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HdbscanOptions), ctypes.POINTER(HdbscanInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_hdbscan.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
