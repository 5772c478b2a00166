"""owlraytracing_amd/csrc/ransac_sample.h compiled for the host: the sample of a trial as the kernel of ransac.hip draws it, callable
from numpy.  No tests here."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SHIM = r"""
#include "ransac_sample.h"
extern "C" {
// seed, trial, n, c: count words each; idx: count x 4; ok: count bytes
void samples(long count, const uint32_t *seed, const uint32_t *trial, const int *n, const uint32_t *c, uint32_t *idx, unsigned char *ok) {
  for (long i = 0; i < count; i++) ok[i] = ransac_sample(seed[i], trial[i], n[i], c[i], idx + 4 * i) ? 1 : 0;
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
        d = tempfile.mkdtemp(prefix="ransac_sample_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "libransacsample.so")
        with open(src, "w") as fh:
            fh.write(_SHIM)
        subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "owlraytracing_amd", "csrc"), src, "-o", so],
                       check=True, capture_output=True, text=True)
        _lib = ctypes.CDLL(so)
    return _lib


def samples(seed, trial, n, c):
    """ransac_sample of the (seed[i], trial[i], n[i], c[i]): (idx (count, 4) uint32 -- the first n[i] meaningful --, ok (count,) bool)."""
    seed, trial, c = (np.ascontiguousarray(a, dtype=np.uint32) for a in (seed, trial, c))
    n = np.ascontiguousarray(n, dtype=np.int32)
    count = len(seed)
    idx, ok = np.zeros((count, 4), np.uint32), np.zeros(count, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    load().samples(ctypes.c_long(count), p(seed), p(trial), p(n), p(c), p(idx), p(ok))
    return idx, ok.astype(bool)
