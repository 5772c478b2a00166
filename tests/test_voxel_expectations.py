"""The numpy definition of tknnVoxelGrid (tests/voxel_spec.py) on cases whose every expected value is written out by hand, and what
can be checked of the call without a GPU: its header is strict C99 and declares the call in its own file, the library exports the
symbol, the ctypes records have the header's layout, and the shared cases are what the GPU tests say they are."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np

import voxel_spec as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_point_on_a_cell_face_belongs_to_the_cell_above():
    # voxel 0.125 is a power of two: every quotient is exact.  0.25 / 0.125 = 2 exactly, the fp32 below 0.25 gives 1.99999988 -> 1.
    below = np.nextafter(np.float32(0.25), np.float32(0))
    P = np.float32([[0.25, 0.125, 0.0], [below, 0.125, 0.0], [0.25, 0.125, 0.0], [0.0, 0.0, 0.0]])
    g = vs.grid(P, 0.125, (0, 0, 0))
    assert g["V"] == 3 and g["cells"].tolist() == [[0, 0, 0], [1, 1, 0], [2, 1, 0]]
    assert g["counts"].tolist() == [1, 1, 2] and g["first"].tolist() == [3, 1, 0] and g["map"].tolist() == [2, 1, 2, 0]
    assert g["offsets"].tolist() == [0, 3] and g["labels"].tolist() == [0, 0, 0] and g["max_count"] == 2
    assert (g["bad_rows"], g["bad_labels"], g["out_of_grid"], g["rows_in_grid"]) == (0, 0, 0, 4)
    assert g["centroid"].tolist() == [[0.0, 0.0, 0.0], [float(below), 0.125, 0.0], [0.25, 0.125, 0.0]]
    # an origin that is no multiple of the voxel: (0.25 - 0.0625) / 0.125 = 1.5 -> 1
    assert vs.grid(P[:1], 0.125, (0.0625, 0, 0))["cells"].tolist() == [[1, 1, 0]]


def test_voxel_one_tenth_rounds_as_fp32_does():
    # fp32(0.1) = 0.100000001490116.  fp32(0.3) / it = 3.00000007..., which rounds to 3.0; fp32(0.7) / it = 6.99999977..., less than
    # half an ulp (2.38e-7) below 7: the fp32 quotient IS 7.0 and the cell 7, where real numbers say 0.7 / 0.1 < 7; fp32(0.6) / it
    # = 6.00000015 -> 6; fp32(0.5) / it = 4.99999993 -> 5.0 -> 5; fp32(0.9) / it = 8.99999964: above 9 - half an ulp (4.77e-7)? yes
    # -> 9.0 -> 9; fp32(0.8) / it = 8.00000000 -> 8.
    x = np.float32([0.3, 0.7, 0.6, 0.5, 0.9, 0.8])
    P = np.stack([x, np.zeros(6, np.float32), np.zeros(6, np.float32)], axis=1)
    c, finite = vs.cells_of(P, 0.1, (0, 0, 0))
    assert finite.all() and c[:, 0].tolist() == [3.0, 7.0, 6.0, 5.0, 9.0, 8.0]
    g = vs.grid(P, 0.1, (0, 0, 0))
    assert g["cells"][:, 0].tolist() == [3, 5, 6, 7, 8, 9] and g["map"].tolist() == [0, 3, 2, 1, 5, 4]
    # the same quotients in double, rounded afterwards, would not do: the spec divides in fp32
    assert np.floor(np.float64(np.float32(0.7)) / np.float64(np.float32(0.1))) == 6.0


def test_the_grid_ends_at_two_to_the_21_cells_and_starts_at_the_origin():
    P = np.float32([[2097151.5, 0, 0], [2097152.0, 0, 0], [-0.001, 0, 0], [0, 0, 2097151.0], [0, -1e-30, 0], [0, 0, 0]])
    g = vs.grid(P, 1.0, (0, 0, 0))
    assert g["map"].tolist() == [2, -1, -1, 1, -1, 0], "cell 2^21 - 1 is in the grid, cell 2^21 and cell -1 are not"
    assert g["cells"].tolist() == [[0, 0, 0], [0, 0, 2097151], [2097151, 0, 0]]
    assert (g["bad_rows"], g["bad_labels"], g["out_of_grid"], g["rows_in_grid"]) == (0, 0, 3, 3)
    # a row below the origin by less than a voxel: floor(-0.25) = -1
    g = vs.grid(np.float32([[0.75, 1, 1], [1, 1, 1]]), 1.0, (1, 1, 1))
    assert g["map"].tolist() == [-1, 0] and g["out_of_grid"] == 1


def test_rows_left_out_are_counted_once_and_clouds_keep_apart():
    nan, inf = np.nan, np.inf
    P = np.float32([[0.5, 0.5, 0.5], [nan, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, inf, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [9.5, 0.5, 0.5], [-5, 0.5, 0.5]])
    batch = np.int32([1, 0, 0, 7, 2, 1, 1, -3])
    g = vs.grid(P, 1.0, (0, 0, 0), batch=batch, B=2, values=np.float32([[1], [2], [3], [4], [5], [6], [7], [8]]))
    # rows 1 and 3 are bad rows (row 3 has a bad label too: counted once, as a bad row); rows 4 and 7 have bad labels (row 7 lies
    # outside the grid too); nobody is out of the grid alone
    assert (g["bad_rows"], g["bad_labels"], g["out_of_grid"], g["rows_in_grid"]) == (2, 2, 0, 4)
    assert g["V"] == 3 and g["labels"].tolist() == [0, 1, 1] and g["cells"].tolist() == [[0, 0, 0], [0, 0, 0], [9, 0, 0]]
    assert g["map"].tolist() == [1, -1, 0, -1, -1, 1, 2, -1] and g["offsets"].tolist() == [0, 1, 3]
    assert g["counts"].tolist() == [1, 2, 1] and g["first"].tolist() == [2, 0, 6] and g["means"].tolist() == [[3.0], [3.5], [7.0]]
    assert vs.grid(P, 1.0, (0, 0, 0), batch=batch, B=2, reverse=True)["centroid"].tolist() == g["centroid"].tolist()


def test_nearest_takes_the_smaller_row_at_equal_distance():
    P = np.float32([[0.75, 0.5, 0.5], [0.25, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [1.5, 0.5, 0.5]])
    g = vs.grid(P, 1.0, (0, 0, 0))
    assert g["centroid"].tolist() == [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]]
    assert vs.nearest(P, g["members"], g["centroid"]).tolist() == [2, 4]
    assert vs.nearest(P, [np.array([0, 1])], np.float32([[0.5, 0.5, 0.5]])).tolist() == [0], "rows 0 and 1 are both 0.25 away: the smaller row"
    assert vs.nearest(P, [np.array([0, 1])], np.float32([[0.45, 0.5, 0.5]])).tolist() == [1]
    assert vs.ulps_apart(np.float32([1.0, -0.0, np.nan]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0, np.nan])).tolist() == [1, 0, 0]


def test_the_shared_cases_are_what_the_gpu_tests_say():
    """Rows per voxel of the three 1 025-row cases, and: summed in reverse order the spec gives every centroid and mean of every
    case within one fp32 value of itself, at least 99 % of them bit for bit -- the bound the GPU tests hold the library's own order
    to (an fp64 sum of at most 2^20 terms errs by at most 2^-33 of the largest operand, far below an fp32 half-ulp of 2^-25: the
    two roundings differ only where the exact mean lies that close to a rounding boundary)."""
    cases = vs.cases()
    one, many, all_in_one = (vs.spec_of(cases[k]) for k in ("u1025_one_per_voxel", "u1025_128_per_voxel", "u1025_one_voxel"))
    assert one["V"] > 900 and one["max_count"] <= 4
    assert many["V"] == 8 and many["counts"].min() > 64 and many["max_count"] < 256
    assert all_in_one["V"] == 1 and all_in_one["counts"].tolist() == [1025]
    assert vs.spec_of(cases["n0"])["V"] == 0 and vs.spec_of(cases["n0"])["offsets"].tolist() == [0, 0]
    assert vs.spec_of(cases["twins"])["counts"].tolist() == [2]
    left = vs.spec_of(cases["left_out"])
    assert left["bad_rows"] == 4 and left["bad_labels"] == 3 and left["out_of_grid"] == 4 and left["rows_in_grid"] == 600 - 11
    three = vs.spec_of(cases["three_clouds"])
    assert three["V"] % 3 == 0 and np.array_equal(three["cells"][: three["V"] // 3], three["cells"][three["V"] // 3: 2 * three["V"] // 3])
    assert three["offsets"].tolist() == [0, three["V"] // 3, 2 * three["V"] // 3, three["V"]]
    assert vs.spec_of(cases["empty_clouds"])["offsets"][[0, 1, 2, 4, 5, 7]].tolist()[0] == 0
    lattice = vs.spec_of(cases["lattice_on_faces"])
    assert lattice["V"] == 343 and sorted(set(lattice["counts"].tolist())) == [1, 2]
    assert vs.spec_of(cases["at_1000"])["V"] > 800
    for name, case in cases.items():
        a, b = vs.spec_of(case), vs.spec_of(case, reverse=True)
        for key in ("centroid", "means"):
            d = vs.ulps_apart(a[key], b[key])
            finite = np.isfinite(a[key])
            assert np.array_equal(np.isnan(a[key]), np.isnan(b[key])) and (d[finite] <= 1).all(), (name, key)
            assert d.size == 0 or (d == 0).mean() >= 0.99, (name, key)


def test_the_header_is_strict_c99_and_the_records_have_its_layout(tmp_path):
    from owlraytracing_amd import _lib, _voxel_lib

    pairs = {"tknnVoxelGridOptions": _voxel_lib.VoxelGridOptions, "tknnVoxelGridInfo": _voxel_lib.VoxelGridInfo}
    mirrors = {c for c in vars(_voxel_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and getattr(c, "_fields_", None)}
    assert mirrors == set(pairs.values())
    consts = {"TKNN_VOXEL_MAX_CHANNELS": _voxel_lib.VOXEL_MAX_CHANNELS, "TKNN_VOXEL_CELL_BITS": _voxel_lib.VOXEL_CELL_BITS,
              "TKNN_VOXEL_LANE_ROWS": _voxel_lib.VOXEL_LANE_ROWS, "TKNN_VOXEL_WAVE_ROWS": _voxel_lib.VOXEL_WAVE_ROWS}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_voxel.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    for cname in consts:
        lines.append('  printf("const %s %%ld\\n", (long)%s);' % (cname, cname))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = 0
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, what, value = line.split()
        if cname == "const":
            assert consts[what] == int(value), what
        elif what == "size":
            assert ctypes.sizeof(pairs[cname]) == int(value), cname
        else:
            assert getattr(pairs[cname], what).offset == int(value), (cname, what)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values()) + len(consts)
    assert ctypes.sizeof(_voxel_lib.VoxelGridOptions) == 144 and ctypes.sizeof(_voxel_lib.VoxelGridInfo) == 80
    assert (1 << _voxel_lib.VOXEL_CELL_BITS) == vs.CELLS
    res, args = _voxel_lib.SIGNATURES["tknnVoxelGrid"]
    lib = _voxel_lib.load()
    assert lib is _lib.load() and lib.tknnVoxelGrid.restype is res is ctypes.c_int and lib.tknnVoxelGrid.argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT tknnVoxelGrid$", exported, flags=re.M), "the library exports the symbol"


def test_the_call_is_declared_in_its_own_header_only():
    from owlraytracing_amd import _lib

    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        text = open(path).read()
        assert ("tknnVoxelGrid" in text) == (os.path.basename(path) == "owlknn_voxel.h"), path
    assert "oxel" not in open(os.path.join(ROOT, "include", "owlknn.h")).read(), "nothing was added to owlknn.h"
    assert "oxel" not in open(os.path.join(ROOT, "owlraytracing_amd", "_lib.py")).read(), "nor to _lib.py's table"
    assert not hasattr(_lib, "VoxelGridOptions")


def test_a_null_engine_is_refused_without_a_device():
    from owlraytracing_amd import _voxel_lib

    lib = _voxel_lib.load()
    o, info = _voxel_lib.VoxelGridOptions(), _voxel_lib.VoxelGridInfo()
    info.voxels = 77
    assert lib.tknnVoxelGrid(None, ctypes.byref(o), ctypes.byref(info), None) == -1
    assert lib.tknnLastError().decode().startswith("tknnVoxelGrid: ") and "engine" in lib.tknnLastError().decode() and info.voxels == 77
