"""owlraytracing_amd/csrc/icp_solve.h compiled for the host (-ffp-contract=off, as the device build): the step of tknnIcp from a
moment row, as Engine::icp calls it, callable from numpy.  No tests here."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SHIM = r"""
#include "icp_solve.h"
extern "C" {
int moments_len(void) { return owlmi::kIcpMoments; }
int solve_point(const double *mom, const double *c, double *dT) { return owlmi::icp_solve_point(mom, c, dT) ? 1 : 0; }
int solve_plane(const double *mom, const double *c, double *dT) { return owlmi::icp_solve_plane(mom, c, dT) ? 1 : 0; }
void mul(const double *A, const double *B, double *C) { owlmi::icp_mul(A, B, C); }
void round_rows(const double *T, float *Tf) { owlmi::icp_round_rows(T, Tf); }
}
"""

_lib = None


def load():
    """One library per process, in a temporary directory that goes away with the process."""
    global _lib
    if _lib is None:
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        assert cxx, "no host C++ compiler"
        d = tempfile.mkdtemp(prefix="icp_solve_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "libicpsolve.so")
        with open(src, "w") as fh:
            fh.write(_SHIM)
        subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "owlraytracing_amd", "csrc"), src, "-o", so], check=True, capture_output=True, text=True)
        _lib = ctypes.CDLL(so)
    return _lib


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def solve(method, mom, c):
    """dT (4,4) of the step from the moment row, or None where the header's solver calls it degenerate (dT is then untouched)."""
    mom, c = _d(mom), _d(c)
    assert mom.shape == (load().moments_len(),) and c.shape == (3,)
    dT = np.full(16, -7.0)
    fn = load().solve_plane if method == "point_to_plane" else load().solve_point
    if not fn(_p(mom), _p(c), _p(dT)):
        assert (dT == -7.0).all(), "a degenerate solve writes nothing"
        return None
    return dT.reshape(4, 4)


def mul(A, B):
    A, B = _d(A), _d(B)
    C = np.empty((4, 4))
    load().mul(_p(A), _p(B), _p(C))
    return C


def round_rows(T):
    T = _d(T)
    Tf = np.empty(12, np.float32)
    load().round_rows(_p(T), _p(Tf))
    return Tf.reshape(3, 4)
