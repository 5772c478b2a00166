"""ctypes binding of tknnVoxelGrid (include/owlknn_voxel.h), an entry point of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its records and signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

# include/owlknn_voxel.h
VOXEL_MAX_CHANNELS = 16
VOXEL_CELL_BITS = 21
VOXEL_LANE_ROWS = 24
VOXEL_WAVE_ROWS = 2048


class VoxelGridOptions(_lib._Record):
    _fields_ = [
        ("n", ctypes.c_int64),
        ("d_points", ctypes.c_void_p),
        ("d_batch", ctypes.c_void_p),
        ("d_values", ctypes.c_void_p),
        ("voxel", ctypes.c_float),
        ("origin", ctypes.c_float * 3),
        ("num_batches", ctypes.c_int32),
        ("channels", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("pad_", ctypes.c_int32),
        ("capacity", ctypes.c_int64),
        ("d_cell", ctypes.c_void_p),
        ("d_count", ctypes.c_void_p),
        ("d_centroid", ctypes.c_void_p),
        ("d_value_mean", ctypes.c_void_p),
        ("d_first", ctypes.c_void_p),
        ("d_nearest", ctypes.c_void_p),
        ("d_voxel_label", ctypes.c_void_p),
        ("d_offsets", ctypes.c_void_p),
        ("d_map", ctypes.c_void_p),
    ]


class VoxelGridInfo(_lib._Record):
    _fields_ = [("voxels", ctypes.c_int64), ("rows_in_grid", ctypes.c_int64), ("bad_rows", ctypes.c_int64), ("bad_labels", ctypes.c_int64),
                ("out_of_grid", ctypes.c_int64), ("wave_voxels", ctypes.c_int64), ("block_voxels", ctypes.c_int64), ("max_count", ctypes.c_int32), ("key_ms", ctypes.c_float),
                ("sort_ms", ctypes.c_float), ("reduce_ms", ctypes.c_float), ("solve_ms", ctypes.c_float), ("pad_", ctypes.c_int32)]


# every symbol include/owlknn_voxel.h declares, with its signature
SIGNATURES = {
    "tknnVoxelGrid": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(VoxelGridOptions), ctypes.POINTER(VoxelGridInfo), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_voxel.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
