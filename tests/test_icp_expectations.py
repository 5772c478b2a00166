"""tests/icp_spec.py against cases small enough to know the answer, and include/owlknn_icp.h against
owlraytracing_amd/_icp_lib.py and the built library (no GPU needed)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import torch  # noqa: F401  before the library is loaded (tests/test_cabi.py says why)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_spec as spec  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETRA = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])


def _rot_z(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])


def test_four_points_by_hand():
    """The unit tetrahedron and its copy moved by 0.1 along x: every point's partner is its original at distance 0.1; the sums
    about the centre (0.5, 0.5, 0.5) are W = 4, sum a = (1.4, 1, 1) - 2 = (-0.6, -1, -1), sum b = (-1, -1, -1); H is that of the
    tetrahedron with itself, so dR = I and dt = mu_p - mu_s = (-0.1, 0, 0)."""
    S = TETRA + np.float32([0.1, 0, 0])
    corr, dist = spec.correspond(TETRA, S, 0.5)
    assert corr.tolist() == [0, 1, 2, 3] and np.allclose(dist, 0.1, atol=1e-7)
    c = spec.centre(TETRA)
    assert c.tolist() == [0.5, 0.5, 0.5]
    mom = spec.moments(TETRA, S, corr, c)
    assert mom[spec.PAIRS] == 4 and mom[spec.POSITIVE] == 4 and mom[4] == 4 and abs(mom[spec.SUM_D2] - 0.04) < 1e-7
    assert np.allclose(mom[5:8], [-0.6, -1, -1], atol=1e-7) and np.allclose(mom[8:11], [-1, -1, -1])
    dT, aux = spec.solve_point(mom, c)
    assert np.allclose(dT[:3, :3], np.eye(3), atol=1e-7) and np.allclose(dT[:3, 3], [-0.1, 0, 0], atol=1e-7)  # (1.1f - 1 is not 0.1f)
    assert np.allclose(aux["H"], np.float64(TETRA - 0.25).T @ np.float64(TETRA - 0.25), atol=1e-6)
    r = spec.icp(TETRA, S, 0.5, max_iterations=1)
    assert r["iterations"] == 1 and r["fitness"] == 1.0 and r["inlier_rmse"] < 1e-7 and len(r["history"]) == 2
    # a point beyond max_dist has no partner; a distance equal to max_dist has one; a NaN has none
    far = np.float32([[0.5, 0, 0], [3, 3, 3], [np.nan, 0, 0]])
    corr, dist = spec.correspond(TETRA, far, 0.5)
    assert corr.tolist() == [0, -1, -1] and dist[0] == 0.5 and np.isinf(dist[1:]).all()  # (the tie of rows 0 and 1: the smaller)


def test_translation_and_rotation_in_one_step_from_exact_pairs():
    rng = np.random.default_rng(1)
    P = rng.uniform(-1, 1, size=(200, 3)).astype(np.float32)
    c = spec.centre(P)
    everyone = np.arange(200, dtype=np.int32)
    t = np.array([0.3, -0.2, 0.1])
    X = (P - t).astype(np.float32)
    dT, _ = spec.solve_point(spec.moments(P, X, everyone, c), c)
    assert np.allclose(dT[:3, :3], np.eye(3), atol=1e-7) and np.allclose(dT[:3, 3], t, atol=1e-6)
    R = _rot_z(25) @ np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    X = (P.astype(np.float64) @ R).astype(np.float32)  # x = R^T p: the step must find R
    dT, _ = spec.solve_point(spec.moments(P, X, everyone, c), c)
    assert np.allclose(dT[:3, :3], R, atol=1e-6) and np.allclose(dT[:3, 3], 0, atol=1e-6)
    # point-to-plane is a linearisation: a small motion comes back to first order, and the angles follow Rz Ry Rx
    small = np.array([1e-3, -2e-3, 1.5e-3, 1e-3, 2e-3, -1e-3])
    Rs = spec.euler(small[:3])
    nrm = rng.normal(size=(200, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    X = ((P.astype(np.float64) - c - small[3:]) @ Rs + c).astype(np.float32)  # p = Rs (x - c) + c + t: the step turns about c
    dT, aux = spec.solve_plane(spec.moments(P, X, everyone, c, "point_to_plane", normals=nrm), c)
    assert np.allclose(aux["x"], small, atol=2e-5) and np.allclose(dT[:3, :3], spec.euler(aux["x"]))
    assert np.allclose(dT[:3, 3], c - dT[:3, :3] @ c + aux["x"][3:])
    assert np.allclose(spec.euler([0.1, 0, 0])[1:, 1:], [[np.cos(0.1), -np.sin(0.1)], [np.sin(0.1), np.cos(0.1)]])
    assert np.allclose(spec.euler([0, 0, 0.1])[:2, :2], [[np.cos(0.1), -np.sin(0.1)], [np.sin(0.1), np.cos(0.1)]])


def test_the_reflection_guard():
    rng = np.random.default_rng(2)
    P = np.concatenate([rng.uniform(-1, 1, size=(60, 2)), np.zeros((60, 1))], axis=1).astype(np.float32)
    X = P * np.float32([1, -1, 1])
    c = spec.centre(P)
    dT, aux = spec.solve_point(spec.moments(P, X, np.arange(60, dtype=np.int32), c), c)
    assert abs(np.linalg.det(dT[:3, :3]) - 1) < 1e-12 and np.allclose(dT[:3, :3], np.diag([1.0, -1.0, -1.0]), atol=1e-12)
    assert np.allclose(X.astype(np.float64) @ dT[:3, :3].T + dT[:3, 3], P, atol=1e-6)
    assert abs(aux["sigma"][2]) < 1e-12 * aux["sigma"][0]


def test_robust_weights():
    e = np.array([0.0, 0.5, 1.0, 2.0, 4.0])
    assert spec.weights(None, e, None).tolist() == [1, 1, 1, 1, 1] and spec.weights("l2", e, 1.0).tolist() == [1, 1, 1, 1, 1]
    assert spec.weights("huber", e, 1.0).tolist() == [1, 1, 1, 0.5, 0.25]
    assert spec.weights("tukey", e, 1.0).tolist() == [1, 0.5625, 0, 0, 0]
    # a pair at e = c counts for Huber and has no weight for Tukey
    S = TETRA + np.float32([0.25, 0, 0])
    corr, _ = spec.correspond(TETRA, S, 0.5)
    assert spec.moments(TETRA, S, corr, spec.centre(TETRA), robust="huber", scale=0.25)[[spec.POSITIVE, 4]].tolist() == [4, 4]
    assert spec.moments(TETRA, S, corr, spec.centre(TETRA), robust="tukey", scale=0.25)[[spec.POSITIVE, 4]].tolist() == [0, 0]


def test_the_degenerate_stops_and_the_evaluation():
    rng = np.random.default_rng(4)
    P = rng.uniform(0, 1, size=(300, 3)).astype(np.float32)
    T0 = spec.rigid(_rot_z(3), [0.01, 0, 0])
    far = P[:50] + np.float32(10)
    r = spec.icp(P, far, 0.1, init=T0)
    assert (r["correspondences"], r["fitness"], r["inlier_rmse"], r["degenerate"], r["iterations"], r["converged"]) == (0, 0, 0, 1, 0, 0)
    assert np.array_equal(r["transform"], T0) and (r["corr"] == -1).all()
    r = spec.icp(P, P[:2], 0.1)
    assert r["correspondences"] == 2 and r["degenerate"] == 1 and r["iterations"] == 0 and np.array_equal(r["transform"], np.eye(4))
    line = (np.linspace(0, 1, 30)[:, None] * np.float32([1, 1, 1])).astype(np.float32)
    r = spec.icp(line, line[3:20] + np.float32([0.001, 0, 0]), 0.1)
    assert r["correspondences"] == 17 and r["degenerate"] == 1 and r["iterations"] == 0
    flat = np.tile(np.float32([0, 0, 1]), (300, 1))
    r = spec.icp(P, P[:100] + np.float32(0.001), 0.1, method="point_to_plane", normals=flat)
    assert r["correspondences"] == 100 and r["degenerate"] == 1 and r["iterations"] == 0
    # a normal that is not finite leaves the system, not the evaluation
    nrm = rng.normal(size=(300, 3)).astype(np.float32)
    nrm[:10, 1] = np.nan
    r = spec.icp(P, P[:100] + np.float32(0.001), 0.1, method="point_to_plane", normals=nrm, max_iterations=1)
    assert r["history"][0]["corr"].tolist() == list(range(100)) and r["iterations"] == 1
    assert spec.moments(P, P[:100] + np.float32(0.001), r["history"][0]["corr"], spec.centre(P), "point_to_plane", normals=nrm)[spec.SKIPPED] == 10
    # max_iterations = 0: one search, no step, also where a step would be degenerate
    r = spec.icp(P, P[:100] + np.float32(0.001), 0.1, init=T0, max_iterations=0)
    assert r["iterations"] == 0 and len(r["history"]) == 1 and r["degenerate"] == 0 and r["converged"] == 0 and np.array_equal(r["transform"], T0)
    assert spec.icp(P, far, 0.1, max_iterations=0)["degenerate"] == 0
    r = spec.icp(P, np.zeros((0, 3), np.float32), 0.1, init=T0)
    assert r["fitness"] == 0 and r["iterations"] == 0 and np.array_equal(r["transform"], T0)
    # the loop stops by itself once nothing changes any more
    r = spec.icp(P, (P[:150].astype(np.float64) @ _rot_z(1).T + 0.002).astype(np.float32), 0.05)
    assert r["converged"] == 1 and 0 < r["iterations"] < 30 and len(r["history"]) == r["iterations"] + 1


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_binding_and_struct_layouts_agree(tmp_path):
    """tknnIcp is declared in its own header, exported and bound with its signature, nothing was added to owlknn.h or to _lib's
    tables, and the ctypes records have the header's sizes and offsets (gcc, C99)."""
    from owlraytracing_amd import _icp_lib, _lib

    assert _declared("owlknn_icp.h") == set(_icp_lib.SIGNATURES) == {"tknnIcp"}
    assert "tknnIcp" not in _declared("owlknn.h") and "tknnIcp" not in _lib.SIGNATURES
    res, args = _icp_lib.SIGNATURES["tknnIcp"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.POINTER(_icp_lib.IcpOptions), ctypes.POINTER(_icp_lib.IcpInfo), ctypes.c_void_p]
    pairs = {"tknnIcpOptions": _icp_lib.IcpOptions, "tknnIcpInfo": _icp_lib.IcpInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_icp.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    consts = {"TKNN_ICP_POINT_TO_POINT": _icp_lib.METHODS["point_to_point"], "TKNN_ICP_POINT_TO_PLANE": _icp_lib.METHODS["point_to_plane"],
              "TKNN_ICP_L2": _icp_lib.ROBUST["l2"], "TKNN_ICP_HUBER": _icp_lib.ROBUST["huber"], "TKNN_ICP_TUKEY": _icp_lib.ROBUST["tukey"]}
    for cname in consts:
        lines.append('  printf("const %s %%ld\\n", (long)%s);' % (cname, cname))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, what, value = line.split()
        if cname == "const":
            assert consts[what] == int(value), what
        elif what == "size":
            assert ctypes.sizeof(pairs[cname]) == int(value), cname
        else:
            assert getattr(pairs[cname], what).offset == int(value), (cname, what)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values()) + len(consts)
    assert ctypes.sizeof(_icp_lib.IcpOptions) == 96 and ctypes.sizeof(_icp_lib.IcpInfo) == 216
    assert _icp_lib.ROBUST[None] == _icp_lib.ROBUST["l2"]
    lib = _icp_lib.load()
    assert lib is _lib.load() and lib.tknnIcp.restype is ctypes.c_int and lib.tknnIcp.argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT tknnIcp$", exported, flags=re.M), "the library exports the symbol"


def test_a_null_engine_is_refused_without_a_device():
    from owlraytracing_amd import _icp_lib

    lib = _icp_lib.load()
    o, info = _icp_lib.IcpOptions(), _icp_lib.IcpInfo()
    info.correspondences = 77
    assert lib.tknnIcp(None, ctypes.byref(o), ctypes.byref(info), None) == -1
    assert lib.tknnLastError().decode().startswith("tknnIcp: ") and "engine" in lib.tknnLastError().decode() and info.correspondences == 77


def test_the_package_exports_the_one_shot():
    import owlraytracing_amd
    from owlraytracing_amd import trueknn

    assert callable(owlraytracing_amd.icp) and callable(trueknn.icp)
    assert callable(trueknn.TrueKNN.icp) and callable(trueknn.TrueKNN.evaluate_registration)
