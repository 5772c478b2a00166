"""ctypes binding of tknnDebugPoison and tknnDebugTeamLanes (include/owlknn_debug.h), the test hooks of libowl_mi355x.so next to
the C-ABI of include/owlknn.h: their constants and signatures.  The handle is _lib.load()'s; there is no fallback."""
import ctypes

from . import _lib

# include/owlknn_debug.h
POISON_WORKSPACE, POISON_COUNTERS, POISON_LISTS, POISON_SOLVE = 1, 2, 4, 8
POISON_ALL = 15
(LANES_SORT16, LANES_CLEAN16, LANES_SORT16_U32, LANES_SORTED_ROW, LANES_MERGE, LANES_KTH, LANES_ROW_TIES, LANES_STRADDLE, LANES_FIRST_LEVEL,
 LANES_REDUCE, LANES_MOVES, LANES_SORT16_3, LANES_CLEAN16_3) = range(13)
LANES_OPS = 13
LANES_MAX_TEAMS = 1 << 20

# every symbol include/owlknn_debug.h declares, with its signature
SIGNATURES = {
    "tknnDebugPoison": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    "tknnDebugTeamLanes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
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


def team_lanes(op, variant, in_tensor, teams):
    """One team helper (``op``, ``variant``: the table of include/owlknn_debug.h) on ``teams`` teams of caller-supplied lanes:
    ``in_tensor`` is a contiguous int32 device tensor (teams, WIN, 16) of the words' bits; returns the (teams, WOUT, 16) int32
    outcome.  The call returns with the kernel done."""
    import torch

    wout = {LANES_SORT16: 2, LANES_CLEAN16: 2, LANES_SORT16_U32: 1, LANES_SORTED_ROW: 2, LANES_MERGE: 2 * variant + 1, LANES_KTH: 1,
            LANES_ROW_TIES: 2, LANES_STRADDLE: 1, LANES_FIRST_LEVEL: 1, LANES_REDUCE: 8, LANES_MOVES: 15, LANES_SORT16_3: 3, LANES_CLEAN16_3: 3}[op]
    assert in_tensor.is_cuda and in_tensor.is_contiguous() and in_tensor.dtype == torch.int32 and in_tensor.shape[0] >= teams
    out = torch.zeros((max(int(teams), 1), wout, 16), dtype=torch.int32, device=in_tensor.device)
    with torch.cuda.device(in_tensor.device):
        on = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(load().tknnDebugTeamLanes(int(op), int(variant), ctypes.c_void_p(in_tensor.data_ptr()), ctypes.c_void_p(out.data_ptr()), int(teams), on))
    return out[:int(teams)]
