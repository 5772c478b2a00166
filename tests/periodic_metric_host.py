"""owlraytracing_amd/csrc/periodic_metric.h compiled for the host (-ffp-contract=off, as the device build): the wrapped distance
and its lower bound over a box, as the kernels of periodic_knn.hip compute them, callable from numpy.  No tests here."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SHIM = r"""
#include "periodic_metric.h"
struct Box { float lo[3], hi[3]; };
static PeriodicCell cell_of(const float *lo, const float *period) {
  PeriodicCell c;
  for (int a = 0; a < 3; a++) c.lo[a] = lo[a], c.period[a] = period[a];
  return c;
}
extern "C" {
void dist2(long n, const float *p, const float *q, const float *lo, const float *period, float *out) {
  const PeriodicCell c = cell_of(lo, period);
  for (long i = 0; i < n; i++) out[i] = periodic_dist2(p[3 * i], p[3 * i + 1], p[3 * i + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2], c);
}
void box_min_dist2(long n, const float *blo, const float *bhi, const float *q, const float *lo, const float *period, float *out) {
  const PeriodicCell c = cell_of(lo, period);
  for (long i = 0; i < n; i++) {
    Box b;
    for (int a = 0; a < 3; a++) b.lo[a] = blo[3 * i + a], b.hi[a] = bhi[3 * i + a];
    out[i] = periodic_box_min_dist2(b, q[3 * i], q[3 * i + 1], q[3 * i + 2], c);
  }
}
void in_cell(long n, const float *x, float lo, float period, unsigned char *out) {
  for (long i = 0; i < n; i++) out[i] = periodic_in_cell(x[i], lo, period) ? 1 : 0;
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
        d = tempfile.mkdtemp(prefix="periodic_metric_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "libperiodicmetric.so")
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


def dist2(P, Q, lo, period):
    """periodic_dist2 of the pairs (P[i], Q[i])."""
    P, Q, lo, period = _f(P), _f(Q), _f(lo), _f(period)
    out = np.empty(len(P), np.float32)
    load().dist2(ctypes.c_long(len(P)), _p(P), _p(Q), _p(lo), _p(period), _p(out))
    return out


def box_min_dist2(blo, bhi, Q, lo, period):
    """periodic_box_min_dist2 of the pairs (box i, Q[i])."""
    blo, bhi, Q, lo, period = _f(blo), _f(bhi), _f(Q), _f(lo), _f(period)
    out = np.empty(len(Q), np.float32)
    load().box_min_dist2(ctypes.c_long(len(Q)), _p(blo), _p(bhi), _p(Q), _p(lo), _p(period), _p(out))
    return out


def in_cell(x, lo, period):
    x = _f(x)
    out = np.empty(len(x), np.uint8)
    load().in_cell(ctypes.c_long(len(x)), _p(x), ctypes.c_float(lo), ctypes.c_float(period), _p(out))
    return out.astype(bool)
