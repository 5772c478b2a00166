"""ctypes binding of tknnDebugPoison (include/owlknn_debug.h), a test hook of libowl_mi355x.so next to the C-ABI of
include/owlknn.h: its constants and its signature.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

# include/owlknn_debug.h
POISON_WORKSPACE, POISON_COUNTERS, POISON_LISTS, POISON_SOLVE = 1, 2, 4, 8
POISON_ALL = 15

# every symbol include/owlknn_debug.h declares, with its signature
SIGNATURES = {
    "tknnDebugPoison": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
}

_bound = None


def load():
    """_lib.load()'s handle with the symbols of include/owlknn_debug.h bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib


def poison(engine, what=POISON_ALL, byte=0x5A, min_workspace_bytes=0, stream=None):
    """Fill the scratch of ``engine`` (a TrueKNN) named in ``what`` with ``byte`` on the engine's current stream (or ``stream``, a
    torch.cuda.Stream); returns the bytes filled.  The call returns with the fills done."""
    torch = engine._torch
    filled = ctypes.c_int64(0)
    with torch.cuda.device(engine.device):
        on = engine._stream() if stream is None else ctypes.c_void_p(stream.cuda_stream)
        _lib.check(load().tknnDebugPoison(engine._h, int(what), int(byte), int(min_workspace_bytes), ctypes.byref(filled), on))
    return int(filled.value)
