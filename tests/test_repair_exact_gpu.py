"""tknnRepairExact (TrueKNN.repair_exact) against brute force: after solve + repair, every finished row is the exact kNN of
the engine's points (own and halo) in (dist, index) order -- distances bit for bit, indices (ids on id-built trees)
identical.  tests/test_repair_expectations.py checks on the CPU that the tie sets and per-query radii used here tell that
contract from the rule the pass used to follow (walk only rows with d_k > r_q)."""
import ctypes

import numpy as np
import pytest

import oracle
import tile_sets
from conftest import load_golden
from owlraytracing_amd import _lib, datasets

pytestmark = pytest.mark.gpu

KERNELS = {"lane": _lib.KERNEL_LANE, "wave": _lib.KERNEL_WAVE, "team": _lib.KERNEL_TEAM}
REGISTER_KS = [1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 16, 17, 24, 25, 32, 33, 64]
TKNN_E_ARG, TKNN_E_STATE = -1, -3


def _engine():
    from owlraytracing_amd.trueknn import TrueKNN
    return TrueKNN()


def _bruteforce(xyz, k, ids=None, queries=None):
    """oracle.bruteforce_knn with ties ordered by id: the points are put in ascending id order first, and positions
    mapped back to ids.  ``queries``: positions in xyz (default all)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    queries = np.arange(len(xyz)) if queries is None else np.asarray(queries)
    if ids is None:
        return oracle.bruteforce_knn(xyz, k, query_ids=queries)
    ids = np.asarray(ids, np.int32)
    order = np.argsort(ids, kind="stable")
    where = np.empty_like(order)
    where[order] = np.arange(len(order))
    bi, bd = oracle.bruteforce_knn(xyz[order], k, query_ids=where[queries])
    return ids[order][bi], bd


def _repair(eng, r, k, r0):
    """Repair in place; returns (count, rows before) for _check_count."""
    before = r["idx"].clone(), r["dist"].clone()
    return eng.repair_exact(r, k, r0), before


def _bits(t):
    import torch
    return t.view(dtype=torch.int32)


def _check_count(eng, r, k, r0, fixed, before):
    """The count equals the rows whose idx or dist changed, and a second call changes nothing."""
    changed = (before[0] != r["idx"]).any(dim=1) | (_bits(before[1]) != _bits(r["dist"])).any(dim=1)
    assert fixed == int(changed.sum()), "the pass reports %d rows repaired, %d changed" % (fixed, int(changed.sum()))
    once_i, once_d = r["idx"].clone(), r["dist"].clone()
    assert eng.repair_exact(r, k, r0) == 0
    assert bool((once_i == r["idx"]).all()) and bool((_bits(once_d) == _bits(r["dist"])).all())


def _check(r, bi, bd, what, rows=None):
    """Finished rows (of ``rows``, default all) equal brute force bit for bit."""
    idx, dist, lv = r["idx"].cpu().numpy(), r["dist"].cpu().numpy(), r["levels"].cpu().numpy()
    if rows is not None:
        idx, dist, lv = idx[rows], dist[rows], lv[rows]
    fin = lv >= 0
    bad_d = (dist[fin].view(np.int32) != bd[fin].view(np.int32)).any(axis=1)
    bad_i = (idx[fin] != bi[fin]).any(axis=1)
    assert not bad_d.any(), "%s: %d finished rows differ from brute force in their distances (first %d)" % (
        what, bad_d.sum(), np.nonzero(fin)[0][np.argmax(bad_d)])
    assert not bad_i.any(), "%s: %d finished rows differ from brute force in their indices (first %d)" % (
        what, bad_i.sum(), np.nonzero(fin)[0][np.argmax(bad_i)])


def _solve_repair_check(eng, xyz, k, r0, what, ids=None, **kw):
    r = eng.solve(k, r0, want_levels=True, **kw)
    fixed, before = _repair(eng, r, k, r0)
    bi, bd = _bruteforce(xyz, k, ids)
    _check(r, bi, bd, what)
    _check_count(eng, r, k, r0, fixed, before)
    return r


@pytest.fixture(scope="module")
def uniform():
    xyz = datasets.uniform3d(6000, seed=71)
    eng = _engine()
    eng.build(xyz)
    yield xyz, eng
    eng.close()


@pytest.mark.parametrize("k", REGISTER_KS)
def test_every_register_capacity(uniform, k):
    """Each repair_kernel<K>: at K = k and at k just above the next smaller capacity."""
    xyz, eng = uniform
    r0 = datasets.start_radius(len(xyz), k)
    r = _solve_repair_check(eng, xyz, k, r0, "uniform k=%d" % k)
    assert (r["levels"] >= 0).all()


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("k", [3, 10, 33])
def test_each_kernels_levels(uniform, kernel, k):
    xyz, eng = uniform
    r0 = datasets.start_radius(len(xyz), k)
    _solve_repair_check(eng, xyz, k, r0, "uniform k=%d %s" % (k, kernel), kernel=KERNELS[kernel])


def _tie_case(name):
    if name == "crossgolden":
        return load_golden("crossroundties_n400_k2")["xyz"], 1.0
    if name == "boundary":
        xyz, r0, _ = tile_sets.repair_boundary_case()
        return xyz, r0
    return tile_sets.tie_set(name)


@pytest.mark.parametrize("name,k", [("crossgolden", 2), ("crossgolden", 3), ("crossgolden", 5), ("boundary", 2),
                                    ("lattice", 6), ("duplicates", 4), ("quantised", 5), ("quantised", 16)])
@pytest.mark.parametrize("kernel", ["lane", "team"])
def test_tie_sets(name, k, kernel):
    """Rows whose replay order of bit-identical distances (first level seen, then index) is not (dist, index) order,
    including rows with d_k <= r_q and no tie inside the row (the hand-built 'boundary' case)."""
    xyz, r0 = _tie_case(name)
    eng = _engine()
    eng.build(xyz)
    r = _solve_repair_check(eng, xyz, k, r0, "%s k=%d %s" % (name, k, kernel), kernel=KERNELS[kernel])
    if name == "boundary":
        assert r["idx"][0].tolist() == [3, 1]
    eng.close()


def test_planar():
    """z = 0 for every point: the boxes are flat."""
    xyz = datasets.uniform3d(5000, seed=72)
    xyz[:, 2] = 0
    eng = _engine()
    eng.build(xyz)
    for k in (5, 12):
        _solve_repair_check(eng, xyz, k, datasets.start_radius(len(xyz), k) * 2, "planar k=%d" % k)
    lat = tile_sets.lattice(60, 2, 5)
    eng.build(lat)
    _solve_repair_check(eng, lat, 7, 0.02, "planar lattice k=7")
    eng.close()


def test_offset_coordinates():
    """Points near 1e4 whose spacing is a few fp32 ulps there (ulp = 2**-10): box faces c +- r round, and distances tie."""
    rng = np.random.default_rng(73)
    ulp = np.float32(2.0 ** -10)
    xyz = (np.float32(1e4) + rng.integers(0, 40, (5000, 3)).astype(np.float32) * ulp).astype(np.float32)
    xyz = np.unique(xyz, axis=0)[rng.permutation(len(np.unique(xyz, axis=0)))]
    eng = _engine()
    eng.build(xyz)
    for k, r0 in ((4, float(ulp) * 0.7), (10, float(ulp) * 1.5)):
        _solve_repair_check(eng, xyz, k, r0, "offset k=%d" % k)
    eng.close()


@pytest.mark.parametrize("scale", [1.0, 1e-6, 1e-12, 1e-15, 1e-18, 1e-21, 1e-24])
def test_magnitudes(scale):
    """Uniform points scaled down until squared offsets are subnormal (1e-21) and vanish (1e-24): the walk's half-width
    d_k * 1.000001 + 2**-74 keeps every point of computed distance <= d_k in the box."""
    xyz = (datasets.uniform3d(3000, seed=74) * np.float32(scale)).astype(np.float32)
    k = 6
    r0 = float(np.float32(datasets.start_radius(len(xyz), k) * scale))
    eng = _engine()
    eng.build(xyz)
    _solve_repair_check(eng, xyz, k, r0, "scale %g" % scale)
    eng.close()


@pytest.mark.parametrize("name,k", [("quantised", 5), ("crossgolden", 3), ("uniform", 10)])
@pytest.mark.parametrize("base", [0, 1 << 30])
def test_id_built_tree(name, k, base):
    """Permuted ids below n, and the same from 2**30 up: rows list ids, ties order by id."""
    if name == "uniform":
        xyz, r0 = datasets.uniform3d(5000, seed=75), datasets.start_radius(5000, k)
    else:
        xyz, r0 = _tie_case(name)
    ids = (tile_sets.relabel(len(xyz), seed=3) + np.int32(base)).astype(np.int32)
    eng = _engine()
    eng.build(xyz, ids=ids)
    _solve_repair_check(eng, xyz, k, r0, "%s k=%d ids from %d" % (name, k, base), ids=ids)
    eng.close()


@pytest.mark.parametrize("name,k", [("quantised", 5), ("cross", 2), ("lattice", 16)])
def test_halo_tile(name, k):
    """A tile with a halo (tknnSetHalo): own rows against brute force over own + halo, ids = positions in G.
    Phase 0 with the whole complement as halo; then phases 1 and 2 of the sharded driver with the halo of its first
    exchange (unfinished rows are left as they are)."""
    xyz, r0 = _tie_case(name)
    own, rest = tile_sets.split(xyz)
    eng = _engine()
    eng.build(xyz[own], ids=own)
    eng.set_halo(xyz[rest], rest)
    both = np.concatenate([own, rest])
    r = eng.solve(k, r0, want_levels=True)
    fixed, before = _repair(eng, r, k, r0)
    bi, bd = _bruteforce(xyz[both], k, ids=both, queries=np.arange(len(own)))
    assert (r["levels"] >= 0).all()
    _check(r, bi, bd, "%s k=%d phase 0" % (name, k))
    _check_count(eng, r, k, r0, fixed, before)
    # phases 1 -> 2
    from oracle.trueknn_numpy import trueknn_numpy
    cap = tile_sets.phase_cap(trueknn_numpy(xyz, k, r0)["level"])
    lay = tile_sets.phases(xyz, own, rest, r0, cap)
    near = lay["near"]
    eng.set_halo(None, None)
    eng.halo_select(lay["peer_box"][None, :], [1], 2)  # the count pass marks the boundary queries
    eng.set_halo(xyz[near], near)
    kw = dict(kernel=_lib.KERNEL_TEAM, max_rounds=cap + 1, allow_unfinished=True, want_levels=True)
    r = eng.solve(k, r0, phase=1, **kw)
    r = eng.solve(k, r0, out={f: r[f] for f in ("idx", "dist", "intersections", "levels")}, phase=2, **kw)
    lv = r["levels"].cpu().numpy()
    assert (lv >= 0).any() and (lv < 0).any()
    left_i, left_d = r["idx"].cpu().numpy()[lv < 0], r["dist"].cpu().numpy()[lv < 0]
    fixed, before = _repair(eng, r, k, r0)
    assert np.array_equal(r["idx"].cpu().numpy()[lv < 0], left_i)
    assert np.array_equal(r["dist"].cpu().numpy()[lv < 0].view(np.int32), left_d.view(np.int32))
    both = np.concatenate([own, near])
    bi, bd = _bruteforce(xyz[both], k, ids=both, queries=np.arange(len(own)))
    _check(r, bi, bd, "%s k=%d phases 1, 2" % (name, k))
    _check_count(eng, r, k, r0, fixed, before)
    eng.close()


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_per_query_start_radii(kind):
    """After a solve with d_start_radii the levels count doublings of each row's own radius; the repair is called with a
    placeholder start radius (1.0) and must still give exact rows."""
    import torch

    n, k = 20_000, 8
    rng = np.random.default_rng(76)
    xyz = datasets.uniform3d(n, seed=77) if kind == "uniform" else datasets.gaussian_mixture3d(n, components=7, sigma=0.03, seed=78)
    radii = rng.choice(np.float32([0.004, 0.01, 0.03]), n).astype(np.float32)
    eng = _engine()
    eng.build(xyz)
    r = eng.solve(k, 1.0, start_radii=torch.from_numpy(radii), kernel=_lib.KERNEL_TEAM, want_levels=True)
    fixed, before = _repair(eng, r, k, 1.0)
    bi, bd = _bruteforce(xyz, k)
    _check(r, bi, bd, "%s per-query radii" % kind)
    _check_count(eng, r, k, 1.0, fixed, before)
    assert fixed > n // 50
    eng.close()


@pytest.mark.parametrize("kernel", ["lane", "team"])
def test_unfinished_rows(uniform, kernel):
    """allow_unfinished with few rounds: rows with level -1 (never written: a sentinel here) come back bit-identical,
    the others are exact."""
    import torch

    xyz, eng = uniform
    n, k = len(xyz), 10
    r0 = datasets.start_radius(n, k)
    out = {"idx": torch.full((n, k), -7, dtype=torch.int32, device=eng.device),
           "dist": torch.full((n, k), -2.5, dtype=torch.float32, device=eng.device)}
    r = eng.solve(k, r0, out=out, kernel=KERNELS[kernel], max_rounds=2, allow_unfinished=True, want_levels=True)
    lv = r["levels"].cpu().numpy()
    assert (lv < 0).any() and (lv >= 0).any()
    fixed, before = _repair(eng, r, k, r0)
    assert (r["idx"].cpu().numpy()[lv < 0] == -7).all() and (r["dist"].cpu().numpy()[lv < 0] == -2.5).all()
    bi, bd = _bruteforce(xyz, k)
    _check(r, bi, bd, "unfinished %s" % kernel)
    _check_count(eng, r, k, r0, fixed, before)


def test_errors(uniform):
    """k = 0 and k = 65: TKNN_E_ARG; before tknnBuild: TKNN_E_STATE; the wrapper refuses mismatched results before any
    launch."""
    import torch

    xyz, eng = uniform
    n, k = len(xyz), 10
    r = eng.solve(k, datasets.start_radius(n, k), want_levels=True)
    ptrs = [ctypes.c_void_p(r[f].data_ptr()) for f in ("levels", "idx", "dist")]
    for bad_k in (0, 65):
        with pytest.raises(_lib.TknnError) as e:
            _lib.check(eng._lib.tknnRepairExact(eng._h, bad_k, ctypes.c_float(0.01), *ptrs, None, eng._stream()))
        assert e.value.code == TKNN_E_ARG, bad_k
    fresh = _engine()
    try:
        with pytest.raises(_lib.TknnError) as e:
            _lib.check(fresh._lib.tknnRepairExact(fresh._h, k, ctypes.c_float(0.01), *ptrs, None, fresh._stream()))
        assert e.value.code == TKNN_E_STATE
    finally:
        fresh.close()
    keep_i, keep_d = r["idx"].clone(), r["dist"].clone()
    bad = [
        ("no levels", {f: r[f] for f in ("idx", "dist")}),
        ("levels None", dict(r, levels=None)),
        ("idx shape", dict(r, idx=r["idx"][:, :5].contiguous())),
        ("dist rows", dict(r, dist=r["dist"][: n - 1])),
        ("levels shape", dict(r, levels=r["levels"][:-1])),
        ("idx dtype", dict(r, idx=r["idx"].to(torch.int64))),
        ("dist dtype", dict(r, dist=r["dist"].double())),
        ("levels dtype", dict(r, levels=r["levels"].to(torch.int16))),
        ("dist on host", dict(r, dist=r["dist"].cpu())),
        ("levels on host", dict(r, levels=r["levels"].cpu())),
        ("idx not contiguous", dict(r, idx=torch.empty((k, n), dtype=torch.int32, device=eng.device).t())),
        ("dist not contiguous", dict(r, dist=torch.empty((n, 2 * k), dtype=torch.float32, device=eng.device)[:, ::2])),
    ]
    for what, res in bad:
        with pytest.raises(ValueError):
            eng.repair_exact(res, k, 0.01)
        assert bool((keep_i == r["idx"]).all()) and bool((keep_d == r["dist"]).all()), what
    with pytest.raises(ValueError):
        eng.repair_exact(r, k + 1, 0.01)  # k does not match the rows
