"""owlraytracing_amd/csrc/curve_key.h compiled for the host: the one sort key of the LBVH, as the builder's kernels compute
it, callable from numpy.  Shared by tests/test_curve_key.py and tests/lbvh_spec.py.  No tests here."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HILBERT, MORTON = 0, 1

_SHIM = r"""
#include "curve_key.h"
extern "C" {
void keys(int curve, int levels, long n, const unsigned *x, const unsigned *y, const unsigned *z, unsigned long long *out) {
  for (long i = 0; i < n; i++) out[i] = curve_key3(curve, x[i], y[i], z[i], levels);
}
void point_keys(int curve, int levels, long n, const float *xyz, const float *lo, float ext, unsigned long long *out) {
  for (long i = 0; i < n; i++)
    out[i] = curve_point_key(curve, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], lo[0], lo[1], lo[2], ext, levels);
}
}
"""

_lib = None


def compile_shim(directory):
    """The shim as a shared library in ``directory`` (-ffp-contract=off, as the device build); returns the loaded library."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, so = os.path.join(str(directory), "shim.cpp"), os.path.join(str(directory), "libcurvekey.so")
    with open(src, "w") as fh:
        fh.write(_SHIM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "owlraytracing_amd", "csrc"),
                    src, "-o", so], check=True, capture_output=True, text=True)
    return ctypes.CDLL(so)


def load():
    """One library per process, in a temporary directory that goes away with the process."""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="curve_key_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        _lib = compile_shim(d)
    return _lib


def keys(lib, curve, levels, x, y, z):
    x, y, z = (np.ascontiguousarray(v, dtype=np.uint32) for v in (x, y, z))
    out = np.empty(len(x), np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.keys(ctypes.c_int(curve), ctypes.c_int(levels), ctypes.c_long(len(x)), p(x), p(y), p(z), p(out))
    return out


def point_keys(lib, curve, levels, xyz, lo, ext):
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    lo = np.ascontiguousarray(lo, dtype=np.float32)
    out = np.empty(len(xyz), np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.point_keys(ctypes.c_int(curve), ctypes.c_int(levels), ctypes.c_long(len(xyz)), p(xyz), p(lo), ctypes.c_float(ext), p(out))
    return out
