"""OWL C-ABI boundary: symbol coverage (CPU) and the program model on the GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build", "owl_tests")
DRIVER = os.path.join(BUILD, "owl_host_driver")
RADIUS_HSACO = os.path.join(BUILD, "radius_programs.hsaco")
REF_HSACO = os.path.join(ROOT, "oracle", "_ref", "deviceCode.hsaco")
REF_SAMPLE = os.path.join(ROOT, "oracle", "_ref", "sample01-trueknn")


def _declared_owl_symbols():
    out = subprocess.run(
        ["g++", "-E", "-P", "-x", "c++", "-I" + os.path.join(ROOT, "include"),
         "-I" + os.path.join(ROOT, "include", "owl_shims"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__=1",
         os.path.join(ROOT, "include", "owl", "owl_host.h")], capture_output=True, text=True, check=True).stdout
    names = set(re.findall(r'extern "C"[^;{]*?\b(owl[A-Z]\w*)\s*\(', out))
    assert len(names) > 400
    return names


def test_library_exports_every_owl_host_symbol():
    import ctypes
    from owlraytracing_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in sorted(_declared_owl_symbols()) if not hasattr(lib, n)]
    assert not missing, missing[:10]


def test_header_covers_the_entry_points_the_sample_calls():
    # the C-ABI symbols samples/s01-trueknn/hostCode.cpp:141-362 needs
    needed = """owlContextCreate owlContextDestroy owlModuleCreate owlGeomTypeCreate owlGeomTypeSetIntersectProg
    owlGeomTypeSetBoundsProg owlBuildPrograms owlBuildPipeline owlBuildSBT owlManagedMemoryBufferCreate
    owlDeviceBufferCreate owlBufferGetPointer owlGeomCreate owlGeomSetPrimCount owlGeomSetBuffer owlGeomSet1f
    owlParamsCreate owlParamsSetBuffer owlParamsSet1i owlParamsSet1f owlUserGeomGroupCreate owlInstanceGroupCreate
    owlGroupBuildAccel owlGroupRefitAccel owlRayGenCreate owlRayGenSet2i owlRayGenSet3f owlRayGenSetGroup
    owlRayGenSetBuffer owlLaunch2D""".split()
    names = _declared_owl_symbols()
    assert not [n for n in needed if n not in names]


def test_c99_header_compiles_as_plain_c(tmp_path):
    # reference tests/t00-c99-compliant-header: owl.h must be includable from strict C99
    src = tmp_path / "c99.c"
    src.write_text('#include <owl/owl.h>\nint main(void){ OWLContext c = 0; (void)c; return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o",
                    str(tmp_path / "c99.o"), "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "include", "owl_shims"), "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__=1"], check=True)


def _need_driver():
    if not (os.path.exists(DRIVER) and os.path.exists(RADIUS_HSACO)):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "owl_programs", "build.sh")])


@pytest.mark.gpu
def test_error_conventions():
    _need_driver()
    r = subprocess.run([DRIVER, "errors", RADIUS_HSACO, os.path.join(BUILD, "stale_abi_programs.hsaco")], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures=0" in r.stdout and "FAIL" not in r.stdout


@pytest.mark.gpu
def test_program_model_count_closest_hit_and_miss(tmp_path):
    """bounds + intersect + closest-hit + miss + launch params + two geometries in one group."""
    _need_driver()
    from owlraytracing_amd import datasets
    n, radius = 20000, np.float32(0.03)
    pts = datasets.uniform3d(n, seed=42)
    (tmp_path / "pts.f32").write_bytes(pts.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([DRIVER, "count", RADIUS_HSACO, str(tmp_path / "pts.f32"), str(n), repr(float(radius)), str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = out.read_bytes()
    count = np.frombuffer(raw, np.int32, n, 0)
    nearest = np.frombuffer(raw, np.float32, n, 4 * n)
    calls = np.frombuffer(raw, np.int64, n, 8 * n)
    first = np.frombuffer(raw, np.int32, n, 16 * n)
    n0 = n // 3
    # reference answers with numpy (float32 arithmetic as written in the program)
    from scipy.spatial import cKDTree
    tree = cKDTree(pts.astype(np.float64))
    want_count = np.zeros(n, np.int32)
    want_near = np.full(n, np.inf, np.float32)
    want_calls = np.zeros(n, np.int64)
    prop = tree.query_ball_point(pts.astype(np.float64), float(radius) * 1.001 + 1e-6, p=np.inf)
    for q in range(n):
        p = np.asarray(prop[q])
        lo, hi = (pts[p] - radius).astype(np.float32), (pts[p] + radius).astype(np.float32)
        inside = np.all((lo <= pts[q]) & (pts[q] <= hi), axis=1)
        p = p[inside]
        want_calls[q] = len(p)
        # the program excludes 'prim == launch index': primitive ids are per geometry
        local = np.where(p < n0, p, p - n0)
        p = p[local != q]
        d = pts[p] - pts[q]
        dist = np.sqrt(((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2]), dtype=np.float32)
        ok = dist <= radius
        want_count[q] = ok.sum()
        if ok.any():
            want_near[q] = dist[ok].min()
    assert np.array_equal(calls, want_calls)
    assert np.array_equal(count, want_count)
    assert np.array_equal(nearest, want_near)
    # first-hit pass: +z ray from each point; nearest ball in front whose disc covers (x,y); ids per geometry
    dxy = pts[:, None, :2] if n <= 2000 else None
    sample = np.arange(0, n, 40)
    for q in sample:
        d2 = (pts[:, 0] - pts[q, 0]) ** 2 + (pts[:, 1] - pts[q, 1]) ** 2
        t = pts[:, 2] - pts[q, 2]
        cand = np.flatnonzero((d2 <= radius * radius) & (t > 0))
        if len(cand) == 0:
            assert first[q] == -1
        else:
            best = cand[np.argmin(t[cand])]
            assert first[q] == (best if best < n0 else best - n0)


@pytest.mark.gpu
@pytest.mark.parametrize("launch_order", ["morton", "thread"])
def test_reference_device_programs_through_owl_api_match_the_checker(tmp_path, launch_order):
    """The reference's own deviceCode.cu (compiled in place by oracle/build_ref.sh, never copied)
    driven through owl* by our host driver: frameBuffer equals the CPU checker's, modulo tie order -- with the launch
    indices handed to the threads in the traced geometry's Morton order (the default for a 1-D launch of as many indices
    as the geometry has primitives, LaunchDesc::order) and in thread order (OWL_LAUNCH_ORDER=0)."""
    env = dict(os.environ)
    env.pop("OWL_LAUNCH_ORDER", None)
    if launch_order == "thread":
        env["OWL_LAUNCH_ORDER"] = "0"
    if not os.path.exists(REF_HSACO):
        pytest.skip("oracle/_ref/deviceCode.hsaco not built (no reference tree at build time)")
    _need_driver()
    import oracle
    from owlraytracing_amd import datasets
    for n, k, r0, seed in ((20000, 5, None, 3), (6000, 10, 0.004, 4)):
        pts = datasets.uniform3d(n, seed=seed) if seed == 3 else datasets.gaussian_mixture3d(n, 8, 0.03, seed)
        r0 = datasets.start_radius(n, k) if r0 is None else r0
        (tmp_path / "pts.f32").write_bytes(pts.tobytes())
        out = tmp_path / "fb.bin"
        r = subprocess.run([DRIVER, "knn", REF_HSACO, str(tmp_path / "pts.f32"), str(n), str(k), repr(float(np.float32(r0))), str(out)],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        fb = np.frombuffer(out.read_bytes(), dtype=oracle.NEIGH_DTYPE).reshape(n, k)
        ref = oracle.trueknn(pts, k, float(np.float32(r0)))
        assert "rounds=%d " % ref["rounds"] in r.stdout
        assert np.array_equal(fb["dist"], ref["dist"])
        assert np.array_equal(fb["intersections"][:, 0], ref["intersections"])
        assert np.all(fb["numNeighbors"][:, 0] == 0)
        # visit order is the LBVH's, not ascending index: indices may differ only inside ties
        same = np.all(fb["ind"] == ref["idx"], axis=1)
        for q in np.flatnonzero(~same):
            d = fb["dist"][q].view(np.int32)
            for pos in np.flatnonzero(fb["ind"][q] != ref["idx"][q]):
                run = np.flatnonzero(d == d[pos])  # the positions holding this very distance
                # a permutation inside a run of bit-identical distances, or -- at the row's last distance -- another of
                # the candidates tied for the last places (which of them is listed depends on the visit order)
                assert (len(run) >= 2 and sorted(fb["ind"][q][run]) == sorted(ref["idx"][q][run])) or d[pos] == d[-1], (q, pos)


@pytest.mark.gpu
@pytest.mark.parametrize("policy", ["mirror", "managed"])
def test_managed_buffer_pointer_held_across_launches(tmp_path, policy):
    """owlManagedMemoryBufferCreate gives ONE address that stays coherent after a synchronising launch
    (owl/Buffer.cpp:307-360, cudaMallocManaged).  A host program that fetches owlBufferGetPointer once and re-reads it
    after later launches must see their results, and what it writes through the pointer between two launches must
    reach the device -- in the default mirror form as with plain managed memory (OWL_MANAGED_POLICY=0)."""
    if not os.path.exists(REF_HSACO):
        pytest.skip("oracle/_ref/deviceCode.hsaco not built (no reference tree at build time)")
    _need_driver()
    import oracle
    from owlraytracing_amd import datasets
    n, k = 15000, 6
    pts = datasets.uniform3d(n, seed=17)
    r0 = float(np.float32(datasets.start_radius(n, k)))
    (tmp_path / "pts.f32").write_bytes(pts.tobytes())
    out = tmp_path / "fb.bin"
    env = dict(os.environ)
    env.pop("OWL_MANAGED_POLICY", None)
    if policy == "managed":
        env["OWL_MANAGED_POLICY"] = "0"
    r = subprocess.run([DRIVER, "knn", REF_HSACO, str(tmp_path / "pts.f32"), str(n), str(k), repr(r0), str(out), "held"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    ref = oracle.trueknn(pts, k, r0)
    assert ref["rounds"] >= 2, "the case must need a second launch"
    assert "rounds=%d " % ref["rounds"] in r.stdout, r.stdout
    assert "held_marker=ok" in r.stdout, r.stdout
    fb = np.frombuffer(out.read_bytes(), dtype=oracle.NEIGH_DTYPE).reshape(n, k)
    assert np.array_equal(fb["dist"], ref["dist"])
    assert np.array_equal(fb["intersections"][:, 0], ref["intersections"])
    assert np.all(fb["intersections"][:, 1:] == 0)
    assert np.all(fb["numNeighbors"][:, 0] == 0)


@pytest.mark.gpu
def test_read_only_mirror_policy_gives_the_same_rows(tmp_path):
    """OWL_MANAGED_POLICY=5 (opt-in, for applications whose host code only reads its managed buffers): no mirror -> device
    copy before a launch.  The TrueKNN loop (it only reads its frameBuffer) gets the rows of the default policy."""
    if not os.path.exists(REF_HSACO):
        pytest.skip("oracle/_ref/deviceCode.hsaco not built (no reference tree at build time)")
    _need_driver()
    import oracle
    from owlraytracing_amd import datasets
    n, k = 15000, 6
    pts = datasets.uniform3d(n, seed=18)
    r0 = float(np.float32(datasets.start_radius(n, k)))
    (tmp_path / "pts.f32").write_bytes(pts.tobytes())
    out = tmp_path / "fb.bin"
    r = subprocess.run([DRIVER, "knn", REF_HSACO, str(tmp_path / "pts.f32"), str(n), str(k), repr(r0), str(out)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, OWL_MANAGED_POLICY="5"))
    assert r.returncode == 0, r.stdout + r.stderr
    ref = oracle.trueknn(pts, k, r0)
    assert "rounds=%d " % ref["rounds"] in r.stdout, r.stdout
    fb = np.frombuffer(out.read_bytes(), dtype=oracle.NEIGH_DTYPE).reshape(n, k)
    assert np.array_equal(fb["dist"], ref["dist"]) and np.array_equal(fb["intersections"][:, 0], ref["intersections"])


@pytest.mark.gpu
def test_rtdbscan_sample_on_the_program_model(tmp_path):
    """samples/s02-rtdbscan -- RT-DBSCAN written as an OWL application (host code on owl* only; ONE intersection program
    that counts neighbours, unites core points with atomics in a union-find and assigns border points; two launches
    without rays for the flags and the roots): the boundary BASELINE's north_star names carries the second workload too.
    Labels and core flags equal the CPU spec's on a 3-D mixture and on a 2-D set with duplicates read as dim = 2."""
    exe = os.path.join(ROOT, "build", "owl_tests", "sample02-rtdbscan")
    if not os.path.exists(exe):
        pytest.fail("build/owl_tests/sample02-rtdbscan is not built (__graft_entry__.build() -> tests/owl_programs/build.sh)")
    import oracle
    from owlraytracing_amd import datasets
    cases = [("mixture3d", datasets.gaussian_mixture3d(20_000, components=8, sigma=0.03, seed=11), 3, 0.012, 5),
             ("taxi2d", datasets.taxi_like2d(15_000, components=10, seed=12), 2, 0.004, 4)]
    for name, pts, dim, eps, min_pts in cases:
        csv = tmp_path / (name + ".csv")
        datasets.write_csv_points(str(csv), pts)
        # the sample parses the text with operator>>: the oracle must see the values it read
        seen = datasets.read_csv_points(str(csv), len(pts), dim)
        eps32 = float(np.float32(eps))
        ref = oracle.dbscan(datasets.pad_to_3d(seen), eps32, min_pts)
        out = tmp_path / (name + ".bin")
        r = subprocess.run([exe, str(csv), str(len(pts)), str(dim), repr(eps32), str(min_pts), str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = out.read_bytes()
        labels = np.frombuffer(raw, np.int32, len(pts), 0)
        core = np.frombuffer(raw, np.uint8, len(pts), 4 * len(pts)).astype(bool)
        assert np.array_equal(core, ref["core"].astype(bool)), name
        assert np.array_equal(labels, ref["labels"]), name
        assert "clusters=%d " % ref["clusters"] in r.stdout, r.stdout


@pytest.mark.gpu
def test_unchanged_reference_sample_runs(tmp_path):
    """samples/s01-trueknn (hostCode.cpp + deviceCode.cu, unchanged) linked against libowl_mi355x."""
    if not os.path.exists(REF_SAMPLE):
        pytest.skip("oracle/_ref/sample01-trueknn not built (no reference tree at build time)")
    import oracle
    from owlraytracing_amd import datasets
    n, k = 30000, 5
    pts = datasets.uniform3d(n, seed=11)
    csv = tmp_path / "pts.csv"
    datasets.write_csv_points(str(csv), pts)
    r0 = datasets.start_radius(n, k)
    timefile = tmp_path / "time.txt"
    dump = tmp_path / "dump"
    dump.mkdir()
    r = subprocess.run([REF_SAMPLE, str(csv), str(n), "3", repr(r0), str(k), str(timefile)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, OWL_MI355X_DUMP_BUFFERS=str(dump)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ref = oracle.trueknn(pts, k, float(np.float32(r0)))
    assert r.stdout.count("Round: ") == 2 * ref["rounds"]  # header line + timing line per round
    assert "True KNN time" in r.stdout and "Build time" in r.stdout
    assert float(timefile.read_text().split()[0]) > 0
    # ... and the ROWS (the test never looked at one).  The sample exports nothing -- its dump loop is commented
    # out (hostCode.cpp:312-321) --, so the runtime's opt-in hook leaves the managed frameBuffer's final contents when the sample
    # destroys its context: n * k Neigh records (GeomTypes.h:22-28), compared field by field with the replay, neighbour
    # indices modulo the order inside exact distance ties (the program model visits in tree order, section 1 of DESIGN.md)
    files = [f for f in os.listdir(dump) if f.endswith("_%d.bin" % (n * k * 24))]
    assert len(files) == 1, os.listdir(dump)
    fb = np.fromfile(os.path.join(dump, files[0]), dtype=oracle.NEIGH_DTYPE).reshape(n, k)
    want = ref["fb"].reshape(n, k)
    assert np.array_equal(fb["dist"], want["dist"])
    assert np.array_equal(fb["numNeighbors"], want["numNeighbors"]) and np.array_equal(fb["intersections"], want["intersections"])
    same = np.all(fb["ind"] == want["ind"], axis=1)
    for q in np.flatnonzero(~same):  # rows that differ: the same neighbours, permuted inside groups of equal distance
        assert sorted(zip(fb["dist"][q].tolist(), fb["ind"][q].tolist())) == sorted(zip(want["dist"][q].tolist(), want["ind"][q].tolist())), q
    assert same.mean() > 0.99


API_HSACO = os.path.join(BUILD, "api_programs.hsaco")


@pytest.mark.gpu
def test_rest_of_the_owl_surface(tmp_path):
    """SURVEY 8f-1 on the GPU (tests/owl_programs/api_programs.cu + `owl_host_driver api`): OWL_BUFFER / OWL_BUFFER_SIZE /
    OWL_DEVICE variables, a host-pinned output buffer read in place, owlBufferResize + two partial owlBufferUpload,
    owlBufferDestroy, instance transforms and ids, any-hit programs (optixIgnoreIntersection), and two OWLParams
    launched asynchronously on one raygen -- each launch sees its own parameters although the code object has a
    single `optixLaunchParams` (reference: a device buffer per LaunchParams, owl/LaunchParams.cpp:38-49)."""
    if not os.path.exists(API_HSACO) or not os.path.exists(DRIVER):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "owl_programs", "build.sh")])
    out = tmp_path / "api.bin"
    r = subprocess.run([DRIVER, "api", API_HSACO, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # a context asked to span two devices spans one (owlGetDeviceCount says so, OWL_DEVICE variables read 0)
    assert "device_count=1" in r.stdout
    raw = out.read_bytes()
    n = 4
    rec = np.dtype([("hit", np.int32, (n, 4)), ("t", np.float32, (n,))])
    a, b, c = np.frombuffer(raw, dtype=rec)
    # pass A, OWLParams A and B launched back to back: same hits, each with ITS tag
    for got, tag in ((a, 1001), (b, 2002)):
        assert got["hit"][:, 3].tolist() == [tag] * n
        assert got["hit"][:, 2].tolist() == [0] * n                      # OWL_DEVICE
        assert got["hit"][0].tolist()[:2] == [0, 70] and got["t"][0] == np.float32(0.75)   # instance 0, cube 0
        assert got["hit"][1].tolist()[:2] == [0, 71] and got["t"][1] == np.float32(1.25)   # moved instance: (1 + 0.5 - 0.25) - 0
        assert got["hit"][2].tolist()[:2] == [1, 70] and got["t"][2] == np.float32(0.25)   # starts inside cube 0's shadow: next is cube 1 at x = 1.75
        assert got["hit"][3].tolist()[:2] == [-1, -1] and got["t"][3] == np.float32(-1.0)  # between the instances: miss program
    # pass B: the any-hit program ignores odd primitives
    assert c["hit"][0].tolist()[:2] == [0, 70]
    assert c["hit"][2].tolist()[:2] == [2, 70] and c["t"][2] == np.float32(1.25)           # cube 1 ignored, cube 2 at x = 2.75
    assert c["hit"][1].tolist()[:2] == [0, 71]
    assert c["hit"][3].tolist()[:2] == [-1, -1]


@pytest.mark.gpu
def test_command_line_tool_with_a_sampled_start_radius(tmp_path):
    """tools/trueknn_cli.py (the reference sample's argv, hostCode.cpp:66-73) with `auto`: the start radius comes from
    owlraytracing_amd.radius.sample_start_radius (counterpart of samples/s01-trueknn/Util/random_sample.py), the rows
    equal the CPU checker's for that radius, the reference's report lines are printed and the total is appended."""
    import sys

    import oracle
    from owlraytracing_amd import datasets
    from owlraytracing_amd.radius import sample_start_radius
    n, k = 40_000, 7
    pts = datasets.gaussian_mixture3d(n, components=9, sigma=0.04, seed=21)
    csv = tmp_path / "pts.csv"
    datasets.write_csv_points(str(csv), pts)
    back = datasets.pad_to_3d(datasets.read_csv_points(str(csv), n, 3))
    timefile, rows = tmp_path / "time.txt", tmp_path / "rows.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "trueknn_cli.py"), str(csv), str(n), "3", "auto", str(k),
                        str(timefile), "--out", str(rows)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for needle in ("num spheres: %d" % n, "Build time:", "True KNN time:", "Total time:"):
        assert needle in r.stdout
    assert float(timefile.read_text().split()[0]) > 0
    r0 = sample_start_radius(back)
    ref = oracle.trueknn(back, k, r0)
    z = np.load(rows)
    assert np.array_equal(z["idx"], ref["idx"]) and np.array_equal(z["dist"], ref["dist"])
    assert np.array_equal(z["intersections"], ref["intersections"])
    assert "Rounds: %d " % ref["rounds"] in r.stdout


def test_reference_sample_configures_and_builds_through_the_cmake_module(tmp_path):
    """cmake/owl_mi355x.cmake stands in for the reference's owl/cmake/configure_owl.cmake + configure_optix.cmake: a
    sample CMakeLists.txt in the reference's form (cuda_compile_and_embed(ptxCode deviceCode.cu), an executable of
    hostCode.cpp + ${ptxCode} linked to ${OWL_LIBRARIES}, as samples/s01-trueknn/CMakeLists.txt:19-30 there) configures
    and builds against it -- hipcc cross-compiles deviceCode.cu for gfx950, no GPU needed.  The sample is this
    repository's samples/s02-rtdbscan, written in that form, so the test needs nothing outside the repository."""
    sample = os.path.join(ROOT, "samples", "s02-rtdbscan")
    import shutil
    if not shutil.which("cmake") or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("cmake or hipcc missing")
    from owlraytracing_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    (tmp_path / "CMakeLists.txt").write_text(
        "cmake_minimum_required(VERSION 3.16)\nproject(owl_on_mi355x C CXX)\nenable_testing()\n"
        "include(%s)\nadd_subdirectory(%s ${CMAKE_BINARY_DIR}/s02-rtdbscan)\n" % (os.path.join(ROOT, "cmake", "owl_mi355x.cmake"), sample))
    build = tmp_path / "build"
    r = subprocess.run(["cmake", "-S", str(tmp_path), "-B", str(build), "-DCMAKE_BUILD_TYPE=Release"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run(["cmake", "--build", str(build), "-j", "4"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    exe = build / "s02-rtdbscan" / "sample02-rtdbscan"
    assert exe.exists()
    # the embedded device code is a gfx950 code object under the symbol the sample declares (hostCode.cpp:21)
    syms = subprocess.run(["nm", "-C", str(exe)], capture_output=True, text=True).stdout
    assert " ptxCode" in syms
