"""TrueKNN.voxel_down_sample (tknnVoxelGrid, include/owlknn_voxel.h) against tests/voxel_spec.py.  Cells, counts, first, labels,
offsets, map, the number of voxels and the four counters equal the spec exactly; `nearest` equals the spec's exactly with the spec fed
the call's own centroid; centroids and value means are equal or adjacent fp32 values to the spec's, at least 99 % of them bit for
bit.

That bound is derived, not measured: an fp64 sum of at most 2^20 terms errs by at most 2^-33 relative to the largest operand, far
below an fp32 half-ulp (2^-25), so two orders of summation round differently only where the exact mean lies that close to a rounding
boundary.  On these very inputs the spec summed in reverse row order stays within the bound and the share against itself
(tests/test_voxel_expectations.py::test_the_shared_cases_are_what_the_gpu_tests_say, run on the CPU)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import voxel_spec as vs

pytestmark = pytest.mark.gpu

ARG = -1
FORCE_WAVE = "TKNN_VOXEL_FORCE_WAVE"
LANE_ROWS = 24  # TKNN_VOXEL_LANE_ROWS
PER_VOXEL = {"d_cell": (3, np.int32), "d_count": (1, np.int32), "d_centroid": (3, np.float32), "d_first": (1, np.int32), "d_nearest": (1, np.int32),
             "d_voxel_label": (1, np.int32)}
CASES = vs.cases()
_SPECS = {}


def spec(name):
    if name not in _SPECS:
        _SPECS[name] = vs.spec_of(CASES[name])
    return _SPECS[name]


@contextlib.contextmanager
def forced(on, variable=FORCE_WAVE, value="1"):
    """The variable set (it is read at call time), or unset."""
    before = os.environ.pop(variable, None)
    if on:
        os.environ[variable] = value
    try:
        yield
    finally:
        os.environ.pop(variable, None)
        if before is not None:
            os.environ[variable] = before


@pytest.fixture(scope="module")
def eng():
    from owlraytracing_amd.trueknn import TrueKNN

    e = TrueKNN(device=0)  # no tree: the call needs none
    yield e
    e.close()


def raw(eng, case, capacity=None, outputs=None, fill=None, empty=None):
    """The call through its C ABI with every output (or those of `outputs`) at `capacity` entries (None: n): (rc, {name: numpy},
    info).  `fill`: the byte the outputs hold before the call; `empty`: the allocator (torch.empty, or a Guarded's)."""
    import torch

    from owlraytracing_amd import _voxel_lib

    dev = eng.device
    P = np.ascontiguousarray(case["P"], np.float32).reshape(-1, 3)
    n, B = len(P), case.get("B", 1)
    values = case.get("values")
    C = 0 if values is None else values.shape[1]
    cap = n if capacity is None else capacity
    empty = torch.empty if empty is None else empty
    spare = torch.zeros((4,), dtype=torch.int32, device=dev)
    keep = [torch.from_numpy(P).to(dev)]
    o = _voxel_lib.VoxelGridOptions()
    o.n, o.d_points = n, keep[0].data_ptr() if n else spare.data_ptr()
    if case.get("batch") is not None:
        keep.append(torch.from_numpy(np.ascontiguousarray(case["batch"], np.int32)).to(dev))
        o.d_batch = keep[-1].data_ptr()
    if C:
        keep.append(torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(dev))
        o.d_values = keep[-1].data_ptr()
    o.voxel, o.num_batches, o.channels, o.capacity = case["voxel"], B, C, cap
    for axis in range(3):
        o.origin[axis] = case["origin"][axis]
    shapes = {name: ((cap, w) if w > 1 else (cap,), dt) for name, (w, dt) in PER_VOXEL.items()}
    if C:
        shapes["d_value_mean"] = ((cap, C), np.float32)
    shapes["d_offsets"] = ((B + 1,), np.int64)
    shapes["d_map"] = ((n,), np.int32)
    bufs = {}
    for name, (shape, dt) in shapes.items():
        if outputs is not None and name not in outputs:
            continue
        t = empty(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev)
        if fill is not None:
            t.view(torch.uint8).fill_(fill)
        bufs[name] = t
        setattr(o, name, t.data_ptr() if t.numel() else spare.data_ptr())
    info = _voxel_lib.VoxelGridInfo()
    with torch.cuda.device(dev):
        rc = _voxel_lib.load().tknnVoxelGrid(eng._h, ctypes.byref(o), ctypes.byref(info), eng._stream())
    torch.cuda.synchronize()
    assert (spare == 0).all()
    return rc, {name: t.cpu().numpy() for name, t in bufs.items()}, info.as_dict()


EXACT = ("d_cell", "d_count", "d_first", "d_voxel_label", "d_offsets", "d_map")
COUNTERS = ("voxels", "rows_in_grid", "bad_rows", "bad_labels", "out_of_grid", "max_count")


def check(case, got, info, want, capacity=None):
    """Everything the module's docstring says, of one call's outputs; the tails behind V where the capacity is larger."""
    V = want["V"]
    P = np.ascontiguousarray(case["P"], np.float32).reshape(-1, 3)
    cap = len(P) if capacity is None else capacity
    assert info["voxels"] == V and [info[k] for k in COUNTERS[1:]] == [want[k] for k in ("rows_in_grid", "bad_rows", "bad_labels", "out_of_grid", "max_count")]
    assert np.array_equal(got["d_cell"][:V], want["cells"]) and np.array_equal(got["d_count"][:V], want["counts"])
    assert np.array_equal(got["d_first"][:V], want["first"]) and np.array_equal(got["d_voxel_label"][:V], want["labels"])
    assert np.array_equal(got["d_offsets"], want["offsets"]) and np.array_equal(got["d_map"], want["map"])
    pairs = [("d_centroid", "centroid")] + ([("d_value_mean", "means")] if "d_value_mean" in got else [])
    for name, key in pairs:
        d = vs.ulps_apart(got[name][:V], want[key])
        print("%s: %d entries, %d one fp32 value from the spec's, largest distance %d" % (name, d.size, int((d == 1).sum()), int(d.max()) if d.size else 0))
        assert np.array_equal(np.isnan(got[name][:V]), np.isnan(want[key]))
        assert (d <= 1).all(), name
        assert d.size == 0 or (d == 0).mean() >= 0.99, name
    assert np.array_equal(got["d_nearest"][:V], vs.nearest(P, want["members"], got["d_centroid"][:V]))
    # the tails
    assert (got["d_count"][V:] == 0).all() and (got["d_cell"][V:] == -1).all() and (got["d_voxel_label"][V:] == -1).all()
    assert (got["d_first"][V:] == -1).all() and (got["d_nearest"][V:] == -1).all() and np.isnan(got["d_centroid"][V:]).all()
    assert "d_value_mean" not in got or np.isnan(got["d_value_mean"][V:]).all()
    assert len(got["d_count"]) == cap


def bits(got):
    return {name: a.view(np.int32) if a.dtype == np.float32 else a for name, a in got.items()}


def same(a, b, names=None):
    a, b = bits(a), bits(b)
    assert a.keys() == b.keys()
    return [name for name in (a if names is None else names) if not np.array_equal(a[name], b[name])]


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_spec(eng, name):
    rc, got, info = raw(eng, CASES[name], fill=0x5A)
    assert rc == 0
    check(CASES[name], got, info, spec(name))
    rc, again, info2 = raw(eng, CASES[name], fill=0xA5)
    assert rc == 0 and same(got, again) == [], "the same call twice: every output bit for bit"
    assert [info[k] for k in COUNTERS] == [info2[k] for k in COUNTERS]


@pytest.mark.parametrize("name", ["u1025_one_per_voxel", "u1025_128_per_voxel", "u1025_one_voxel", "left_out", "c16"])
def test_the_wave_kernel_alone(eng, name):
    want = spec(name)
    rc, got, info = raw(eng, CASES[name])
    assert rc == 0
    if name.startswith("u1025"):
        assert info["wave_voxels"] == int((want["counts"] > LANE_ROWS).sum()), "voxels of more than TKNN_VOXEL_LANE_ROWS rows take the wave kernel"
        assert (info["wave_voxels"] > 0) == (name != "u1025_one_per_voxel")
    with forced(True):
        rc, wave, winfo = raw(eng, CASES[name])
    assert rc == 0 and winfo["wave_voxels"] == want["V"], "every voxel"
    check(CASES[name], wave, winfo, want)
    assert same(got, wave, EXACT) == [], "the exact outputs do not depend on the path"
    assert [info[k] for k in COUNTERS] == [winfo[k] for k in COUNTERS]
    with forced(True):
        assert same(wave, raw(eng, CASES[name])[1]) == []


@pytest.mark.parametrize("name", ["u1025_128_per_voxel", "u1025_one_voxel", "c16_one_voxel"])
def test_the_workgroup_kernel(eng, name):
    """A voxel of more than TKNN_VOXEL_WAVE_ROWS rows is summed by a workgroup of 1 024 lanes: the threshold moved down to 100 rows
    sends the runs of about 128 rows, the run of 1 025 (a second stride for lane 0) and the 16 channels there; with the threshold
    in place the run of 1 025 is a wave's."""
    want = spec(name)
    rc, got, info = raw(eng, CASES[name])
    assert rc == 0 and info["block_voxels"] == 0
    with forced(True, "TKNN_VOXEL_WAVE_ROWS", "100"):
        rc, block, binfo = raw(eng, CASES[name])
        assert rc == 0 and same(block, raw(eng, CASES[name])[1]) == []
    assert binfo["block_voxels"] == int((want["counts"] > 100).sum()) > 0
    assert binfo["wave_voxels"] == int(((want["counts"] > LANE_ROWS) & (want["counts"] <= 100)).sum())
    check(CASES[name], block, binfo, want)
    assert same(got, block, EXACT) == [] and [info[k] for k in COUNTERS] == [binfo[k] for k in COUNTERS]


def test_three_clouds_share_no_voxel(eng):
    want = spec("three_clouds")
    rc, got, info = raw(eng, CASES["three_clouds"])
    V = want["V"]
    assert rc == 0 and info["voxels"] == V and V % 3 == 0
    third = V // 3
    assert got["d_offsets"].tolist() == [0, third, 2 * third, V]
    for b in range(3):
        assert (got["d_voxel_label"][b * third:(b + 1) * third] == b).all()
        assert np.array_equal(got["d_cell"][b * third:(b + 1) * third], got["d_cell"][:third])
        assert np.array_equal(got["d_centroid"][b * third:(b + 1) * third].view(np.int32), got["d_centroid"][:third].view(np.int32))
    assert np.array_equal(got["d_voxel_label"][got["d_map"]], CASES["three_clouds"]["batch"]), "every row in a voxel of its own cloud"


def test_a_permutation_of_the_rows(eng):
    case = CASES["left_out"]
    perm = np.random.default_rng(21).permutation(len(case["P"]))
    moved = dict(case, P=case["P"][perm], batch=case["batch"][perm], values=case["values"][perm])
    _, a, ia = raw(eng, case)
    rc, b, ib = raw(eng, moved)
    V = ia["voxels"]
    assert rc == 0 and [ia[k] for k in COUNTERS] == [ib[k] for k in COUNTERS]
    assert same(a, b, ("d_cell", "d_count", "d_voxel_label", "d_offsets")) == []
    assert np.array_equal(b["d_map"], a["d_map"][perm]), "the map follows the rows"
    inverse = np.argsort(perm)
    members = vs.spec_of(case)["members"]
    assert np.array_equal(b["d_first"][:V], [inverse[m].min() for m in members]), "first: the smallest row in the new numbering"
    for name in ("d_centroid", "d_value_mean"):
        assert (vs.ulps_apart(a[name][:V], b[name][:V]) <= 1).all(), name
    check(moved, b, ib, vs.spec_of(moved))


def test_count_pass_then_fill_and_the_capacity(eng):
    case = CASES["c3"]
    want = spec("c3")
    V = want["V"]
    rc, counted, info = raw(eng, case, outputs=("d_map", "d_offsets"), fill=0x5A)
    assert rc == 0 and info["voxels"] == V and info["max_count"] == want["max_count"]
    assert np.array_equal(counted["d_map"], want["map"]) and np.array_equal(counted["d_offsets"], want["offsets"])
    rc, none, info = raw(eng, case, outputs=())
    assert rc == 0 and info["voxels"] == V
    rc, got, info = raw(eng, case, capacity=V, fill=0x5A)
    assert rc == 0
    check(case, got, info, want, capacity=V)
    # one entry short: refused, nothing written
    rc, short, _ = raw(eng, case, capacity=V - 1, fill=0x5A)
    from owlraytracing_amd import _lib

    assert rc == ARG and "capacity" in _lib.load().tknnLastError().decode()
    for name, a in short.items():
        assert (a.view(np.uint8) == 0x5A).all(), name
    # 300 entries more: the tails
    rc, more, info = raw(eng, case, capacity=V + 300, fill=0x5A)
    assert rc == 0
    check(case, more, info, want, capacity=V + 300)
    assert same({k: v[:V] for k, v in more.items() if k in PER_VOXEL}, {k: v[:V] for k, v in got.items() if k in PER_VOXEL}) == []
    # an output asked alone gives the same bits
    for name in ("d_nearest", "d_centroid", "d_value_mean", "d_count"):
        rc, alone, _ = raw(eng, case, capacity=V, outputs=(name,), fill=0x5A)
        assert rc == 0 and same(alone, {name: got[name]}) == [], name


def test_poisoned_scratch_and_a_fresh_engine(eng):
    """tests/test_engine_state_gpu.py's rule for the new call: no word of scratch is read before the call has written it."""
    from owlraytracing_amd import _debug_lib
    from owlraytracing_amd.trueknn import TrueKNN

    for name in ("left_out", "u1025_128_per_voxel"):
        for variable, value in ((None, None), (FORCE_WAVE, "1"), ("TKNN_VOXEL_WAVE_ROWS", "100")):
            with forced(variable is not None, variable or FORCE_WAVE, value):
                _, want, winfo = raw(eng, CASES[name])
                fresh = TrueKNN(device=0)
                try:
                    _, first, finfo = raw(fresh, CASES[name])
                    assert same(want, first) == [] and [winfo[k] for k in COUNTERS] == [finfo[k] for k in COUNTERS]
                    for byte in (0xFF, 0x5A):
                        assert _debug_lib.poison(fresh, _debug_lib.POISON_ALL, byte, 4 << 20) >= 4 << 20
                        _, got, info = raw(fresh, CASES[name])
                        assert same(want, got) == [], "after poison 0x%02X" % byte
                        assert [winfo[k] for k in COUNTERS + ("wave_voxels", "block_voxels")] == [info[k] for k in COUNTERS + ("wave_voxels", "block_voxels")]
                finally:
                    fresh.close()


def test_on_a_side_stream(eng):
    """The call on a stream of its own, its inputs made on that stream, poison on the same stream directly before it: a sort, a scan
    or a copy issued on another stream than the caller's is ordered only by accident on the null stream."""
    import torch

    from owlraytracing_amd import _debug_lib

    _, want, winfo = raw(eng, CASES["three_clouds"])
    stream = torch.cuda.Stream(device=0)
    with torch.cuda.stream(stream):
        assert _debug_lib.poison(eng, _debug_lib.POISON_ALL, 0x5A, 4 << 20) >= 4 << 20
        rc, got, info = raw(eng, CASES["three_clouds"])
    assert rc == 0 and same(want, got) == [] and [winfo[k] for k in COUNTERS] == [info[k] for k in COUNTERS]


def test_a_built_tree_is_left_alone(eng):
    from owlraytracing_amd.trueknn import TrueKNN

    P = vs.uniform(3000, 2)
    e = TrueKNN(device=0)
    try:
        e.build(P)
        before = e.knn(P[:200], k=4)
        _, got, info = raw(e, CASES["c3"])
        check(CASES["c3"], got, info, spec("c3"))
        after = e.knn(P[:200], k=4)
        assert np.array_equal(before["idx"].cpu().numpy(), after["idx"].cpu().numpy()) and e.n == 3000
    finally:
        e.close()


@pytest.mark.parametrize("byte", [0x5A, 0xC3])
def test_guarded_outputs(eng, byte):
    """No stray write around any output and no stale word in one (tests/test_output_bounds_gpu.py's a. and b.), on both paths, with a
    capacity beyond V."""
    import torch

    import guarded_outputs as go

    case, want = CASES["left_out"], spec("left_out")
    for wave in (False, True):
        g = go.Guarded(torch, byte)
        with forced(wave):
            rc, got, info = raw(eng, case, capacity=want["V"] + 77, empty=g.empty)
        assert rc == 0 and g.stray() == [], g.stray()
        check(case, got, info, want, capacity=want["V"] + 77)
        for r in g.records:
            assert not g.as_filled(r.name).any(), "%s holds a word the call did not write" % r


@pytest.mark.parametrize("reduce", ["mean", "nearest", "center"])
def test_the_wrapper_under_the_guard(reduce):
    """TrueKNN.voxel_down_sample with the engine's torch handle replaced by the guard, as tests/test_output_bounds_gpu.py runs the
    other wrappers: sized by n, every output is written whole -- the tails behind V included -- under three fills, nothing is
    written around one, and the spare is left alone."""
    import torch

    import guarded_outputs as go
    from owlraytracing_amd.trueknn import TrueKNN

    case, stale, account = CASES["left_out"], None, None
    for byte in (0x00, 0xFF, 0x5A):
        e = TrueKNN(device=0)
        g = go.Guarded(torch, byte)
        e._torch = g
        try:
            r = e.voxel_down_sample(case["P"], case["voxel"], batch=case["batch"], num_batches=3, values=case["values"], origin=case["origin"], reduce=reduce,
                                    want_map=True, want_cells=True)
            torch.cuda.synchronize()
            assert r["info"]["voxels"] == spec("left_out")["V"] and g.stray() == [], g.stray()
            assert [x.spare for x in g.records].count(True) == 1 and all(g.as_filled(x.name).all() for x in g.records if x.spare)
            filled = {x.name: g.as_filled(x.name).cpu().numpy() for x in g.records if not x.spare}
            records = [(x.name, x.shape, str(x.dtype)) for x in g.records]
        finally:
            e.close()
        assert account is None or account == records
        account = records
        stale = filled if stale is None else {name: stale[name] & filled[name] for name in stale}
    assert len(stale) >= 6 and [name for name, left in stale.items() if left.any()] == [], "an output holds a word that no fill changed: never written"


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def test_the_four_reduce_modes_the_default_origin_and_the_map(eng):
    rng = np.random.default_rng(31)
    P = (rng.random((1500, 3), dtype=np.float32) * np.float32(2.0) - np.float32(0.7)).astype(np.float32)
    P[11] = np.nan
    values = rng.random((1500, 4), dtype=np.float32)
    voxel = 0.3
    finite = np.isfinite(P).all(axis=1)
    origin = P[finite].min(axis=0) - np.float32(voxel) / np.float32(2)  # Open3D's
    want = vs.grid(P, voxel, origin, values=values)
    V = want["V"]
    r = eng.voxel_down_sample(P, voxel, values=values, want_map=True, want_cells=True)
    assert r["info"]["voxels"] == V and r["info"]["bad_rows"] == 1 and tuple(r["points"].shape) == (V, 3)
    assert np.array_equal(r["cells"].cpu().numpy(), want["cells"]) and np.array_equal(r["counts"].cpu().numpy(), want["counts"])
    assert np.array_equal(r["map"].cpu().numpy(), want["map"]) and r["offsets"].tolist() == [0, V] and "rows" not in r and "batch" not in r
    centroid = r["points"].cpu().numpy()
    assert (vs.ulps_apart(centroid, want["centroid"]) <= 1).all() and (vs.ulps_apart(r["values"].cpu().numpy(), want["means"]) <= 1).all()
    first = eng.voxel_down_sample(P, voxel, values=values, reduce="first")
    assert np.array_equal(first["rows"].cpu().numpy(), want["first"]) and np.array_equal(first["points"].cpu().numpy(), P[want["first"]])
    assert np.array_equal(first["values"].cpu().numpy(), values[want["first"]])
    near = eng.voxel_down_sample(P, voxel, reduce="nearest")
    rows = vs.nearest(P, want["members"], centroid)
    assert np.array_equal(near["rows"].cpu().numpy(), rows) and np.array_equal(near["points"].cpu().numpy(), P[rows]) and "values" not in near
    center = eng.voxel_down_sample(P, voxel, values=values, reduce="center")
    expect = (origin[None, :] + (want["cells"].astype(np.float32) + np.float32(0.5)) * np.float32(voxel)).astype(np.float32)
    assert np.array_equal(center["points"].cpu().numpy(), expect) and np.array_equal(center["values"].cpu().numpy(), r["values"].cpu().numpy())
    # labels, an explicit origin, a capacity, a tensor in, and the one-shot with numpy out
    import torch

    import owlraytracing_amd

    batch = (np.arange(1500) % 3).astype(np.int32)
    wb = vs.grid(P, voxel, (-1, -1, -1), batch=batch, B=3)
    rb = eng.voxel_down_sample(torch.from_numpy(P).to(eng.device), voxel, batch=batch, origin=(-1, -1, -1), max_voxels=wb["V"] + 5)
    assert np.array_equal(rb["batch"].cpu().numpy(), wb["labels"]) and rb["offsets"].tolist() == wb["offsets"].tolist() and len(rb["counts"]) == wb["V"]
    with pytest.raises(RuntimeError):
        eng.voxel_down_sample(P, voxel, max_voxels=V - 1)
    one = owlraytracing_amd.voxel_down_sample(P[:, :2], voxel, reduce="first")
    assert isinstance(one["points"], np.ndarray) and one["points"].shape[1] == 3 and (one["points"][:, 2] == 0).all() and one["info"]["bad_rows"] == 1


def test_global_registration_on_a_voxel_grid():
    """tests/test_ransac_gpu.py's two views, sampled eight times as densely, through global_registration(voxel_size=...): the grid
    leaves about 2 000 points per view, normals, FPFH, matching and RANSAC run on those, ICP and the evaluations on the full clouds;
    the planted motion is recovered to within max_dist, the existing test's tolerance."""
    import global_spec as gs
    from owlraytracing_amd.trueknn import global_registration

    v = gs.two_views(count=16000)
    max_dist = gs.VIEW_MAX_DIST
    r = global_registration(v["P"], v["S"], feature_radius=0.15, max_dist=max_dist, seed=3, target_viewpoint=v["view_p"], source_viewpoint=v["view_s"],
                            voxel_size=0.03)
    print("points left: target %d of %d, source %d of %d; pairs %d, ransac inliers %d" % (r["target_down"], len(v["P"]), r["source_down"], len(v["S"]),
                                                                                       len(r["pairs"]), r["ransac"]["inliers"]))
    assert 1500 <= r["target_down"] <= 3000 and 1500 <= r["source_down"] <= 3000, "about 2 000 points"
    assert r["pairs"][:, 0].max() < r["source_down"] and r["pairs"][:, 1].max() < r["target_down"], "the pairs name the reduced clouds' rows"
    assert r["ransac"]["best_trial"] >= 0 and len(r["pairs"]) >= 10
    clean = (v["Q"] - v["T0"][:3, 3]) @ v["T0"][:3, :3]  # the source before its noise
    T = r["transform"].numpy()
    moved = clean @ T[:3, :3].T + T[:3, 3]
    assert np.linalg.norm(moved - v["Q"], axis=1).max() < max_dist, "the motion is recovered to within max_dist"
    assert np.array_equal(T, r["icp"]["transform"].numpy())
    assert r["icp_eval"]["fitness"] >= r["ransac_eval"]["fitness"], "the evaluations are of the full clouds"
    assert r["icp_eval"]["fitness"] >= v["shared"] / len(v["S"]), "every shared point of the full source finds its twin"
