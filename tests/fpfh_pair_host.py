"""owlraytracing_amd/csrc/fpfh_pair.h compiled for the host (-ffp-contract=off, as the device build): the pair features and their
bins as the kernels of fpfh.hip compute them, callable from numpy.  No tests here."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SHIM = r"""
#include "fpfh_pair.h"
extern "C" {
// ni, nj, dp: n x 3; d2, f4: n; out: valid n bytes, bins n x 3, features n x 3
void pairs(long n, const float *ni, const float *nj, const float *dp, const float *d2, const float *f4, unsigned char *valid, int *bins, float *features) {
  for (long i = 0; i < n; i++) {
    FpfhFeatures f = {0.f, 0.f, 0.f, 0, 0, 0};
    valid[i] = fpfh_pair(ni[3 * i], ni[3 * i + 1], ni[3 * i + 2], nj[3 * i], nj[3 * i + 1], nj[3 * i + 2], dp[3 * i], dp[3 * i + 1], dp[3 * i + 2], d2[i], f4[i], f) ? 1 : 0;
    bins[3 * i] = f.b1, bins[3 * i + 1] = f.b2, bins[3 * i + 2] = f.b3;
    features[3 * i] = f.f1, features[3 * i + 1] = f.f2, features[3 * i + 2] = f.f3;
  }
}
}
"""

_lib = None


def load():
    """One library per process, in a temporary directory that goes away with the process."""
    global _lib
    if _lib is None:
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        assert cxx, "no host C++ compiler"
        d = tempfile.mkdtemp(prefix="fpfh_pair_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "libfpfhpair.so")
        with open(src, "w") as fh:
            fh.write(_SHIM)
        subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "owlraytracing_amd", "csrc"),
                        src, "-o", so], check=True, capture_output=True, text=True)
        _lib = ctypes.CDLL(so)
    return _lib


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pairs(ni, nj, dp, d2, f4):
    """fpfh_pair of the pairs (ni[i], nj[i], dp[i], d2[i], f4[i]): valid (n,) bool, bins (n, 3) int32, features (n, 3) float32."""
    ni, nj, dp, d2, f4 = _f(ni), _f(nj), _f(dp), _f(d2), _f(f4)
    n = len(d2)
    valid, bins, feats = np.zeros(n, np.uint8), np.zeros((n, 3), np.int32), np.zeros((n, 3), np.float32)
    load().pairs(ctypes.c_long(n), _p(ni), _p(nj), _p(dp), _p(d2), _p(f4), _p(valid), _p(bins), _p(feats))
    return valid.astype(bool), bins, feats
