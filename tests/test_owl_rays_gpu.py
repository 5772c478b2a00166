"""The ray path of include/owl/device_runtime.h on the GPU against the brute-force reference of tests/ray_spec.py:
real rays (every octant, zero direction components, tmin / tmax) against boxes and spheres in two geometry groups under
six instances (identity, translation, reflection x power-of-two scale, scale, rotation x shear, a child set afterwards),
any-hit modes, optixTerminateRay, a second ray type, the ray flags, 2-D and one-thread launches, LaunchDesc::order, refit.

One `owl_host_driver rays` process per scene runs every pass (tests/owl_programs/ray_programs.cu); the tests share its
output.  Rays that stay clear of the general-matrix instance are compared bit for bit with the float32 restatement, rays
that touch it with the float64 restatement inside the band ray_spec.py derives."""
import os
import subprocess

import numpy as np
import pytest

import ray_spec as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build", "owl_tests")
DRIVER = os.path.join(BUILD, "owl_host_driver")
RAY_HSACO = os.path.join(BUILD, "ray_programs.hsaco")
F4, U4 = np.float32, np.uint32

BIG_PASSES = ["count", "closest", "ignore_odd", "ignore_near", "terminate", "types", "flag_disable_anyhit", "flag_enforce_anyhit",
              "flag_terminate_first", "flag_disable_closesthit", "flag_disable_anyhit_terminate_first", "launch2d", "launch_one",
              "refit"]
SMALL_PASSES = ["count", "closest", "ignore_odd", "ignore_near", "terminate", "types"]


def _run(tmp, name, passes, n1d, dx, dy, env=None):
    """One driver process: scene + rays in, {pass: (records, calls, idsum)} out."""
    if not (os.path.exists(DRIVER) and os.path.exists(RAY_HSACO)):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "owl_programs", "build.sh")])
    case = rs.case(name)
    scene_file, ray_file, out_file = (str(tmp / (name + ext)) for ext in (".scene", ".rays", ".out"))
    with open(scene_file, "wb") as f:
        f.write(rs.scene_bytes(case["scene"]))
    with open(ray_file, "wb") as f:
        f.write(rs.ray_bytes(case["rays"]))
    r = subprocess.run([DRIVER, "rays", RAY_HSACO, scene_file, ray_file, out_file, ",".join(passes), str(n1d), str(dx), str(dy)],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out_file, "rb") as f:
        return _parse(f.read(), case, passes)


def _parse(raw, case, passes):
    n, ni = len(case["rays"]), len(case["scene"]["instances"])
    per_pass = n * rs.HIT_DTYPE.itemsize + 2 * n * ni * 4
    assert len(raw) == per_pass * len(passes)
    out = {}
    for k, p in enumerate(passes):
        base = k * per_pass
        rec = np.frombuffer(raw, rs.HIT_DTYPE, n, base)
        calls = np.frombuffer(raw, U4, n * ni, base + n * rs.HIT_DTYPE.itemsize).reshape(n, ni)
        idsum = np.frombuffer(raw, U4, n * ni, base + n * rs.HIT_DTYPE.itemsize + n * ni * 4).reshape(n, ni)
        out[p] = (rec, calls, idsum)
    return out


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("rays_big"), "big", BIG_PASSES, rs.N_RAYS, *rs.LAUNCH_2D)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    n = len(rs.case("small")["rays"])
    return _run(tmp_path_factory.mktemp("rays_small"), "small", SMALL_PASSES, n, n, 1)


# ---- comparisons -------------------------------------------------------------------------------------------------------
def _bits(t):
    return np.asarray(t, F4).view(U4)


def _lookup(c, ray, inst, geom, prim, kind):
    """Index into the (sorted) candidates of the one with this identity, -1 if the reference has no such candidate."""
    keys = rs.key_of(c["ray"], c["inst"], c["geom"], c["prim"], c["kind"])
    want = rs.key_of(ray, inst, geom, prim, kind)
    at = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    return np.where(keys[at] == want, at, -1)


def _untouched(rec):
    return (rec["prim"] == -2) & (rec["status"] == rs.UNTOUCHED) & (rec["inst_index"] == -2) & (rec["kind"] == -2) & (rec["geom"] == -2)


def check_hits(case, ev, rec, which, ok, closest=True):
    """Records of the rays `which` against the float32 restatement `ev`, whose candidates `ok` the pass can accept.
    closest: the record is the nearest of them (any of those with bit-equal t); otherwise any one of them (a ray that
    terminates at the first accepted candidate: which comes first is the walk's to choose)."""
    c, n = ev["cands"], len(rec)
    ids = np.array([i["id"] for i in case["scene"]["instances"]], np.int64)
    has = np.bincount(c["ray"][ok], minlength=n).astype(bool)
    miss = which & ~has
    assert np.all(rec["status"][miss] == rs.MISS0_RAN) and np.all(rec["prim"][miss] == -1)
    assert np.all(rec["kind"][miss] == -2) and np.all(rec["geom"][miss] == -2)  # ... and closest-hit did not run
    hit = np.flatnonzero(which & has)
    got = rec[hit]
    assert np.all(got["status"] == rs.CLOSEST_HIT_RAN), np.unique(got["status"], return_counts=True)
    assert np.all((got["inst_index"] >= 0) & (got["inst_index"] < len(ids)))
    assert np.array_equal(got["inst_id"], ids[got["inst_index"]])
    assert np.array_equal(got["attr0"], got["prim"].astype(U4))
    at = _lookup(c, hit, got["inst_index"], got["geom"], got["prim"], got["kind"])
    assert np.all(at >= 0), "a reported hit the reference does not have: rays %s" % hit[at < 0][:10]
    assert np.all(ok[at]), "a reported hit the pass cannot accept: rays %s" % hit[~ok[at]][:10]
    assert np.array_equal(_bits(got["t"]), _bits(c["t"][at])), "t differs in bits: rays %s" % hit[_bits(got["t"]) != _bits(c["t"][at])][:10]
    if closest:
        best = rs.best_t(c, ok, n)[hit]
        assert np.array_equal(c["t"][at], best), "not the closest candidate: rays %s" % hit[c["t"][at] != best][:10]
    return len(hit), int(miss.sum())


def check_general(case, ev64, rec, which):
    """Records of rays that touch the general-matrix instance against the float64 restatement, undecided rays skipped."""
    rays = case["rays"]
    c = ev64["cands"]
    sel = which & case["touch"] & ~rs.undecided(ev64, rays)
    best = rs.best_candidate(c, rs.eligible(c, rays), len(rays))
    miss, hit = sel & (best < 0), np.flatnonzero(sel & (best >= 0))
    assert np.all(rec["status"][miss] == rs.MISS0_RAN)
    got, want = rec[hit], c[best[hit]]
    assert np.all(got["status"] == rs.CLOSEST_HIT_RAN)
    for col_got, col_want in (("inst_index", "inst"), ("geom", "geom"), ("prim", "prim"), ("kind", "kind")):
        assert np.array_equal(got[col_got], want[col_want]), col_got
    gap = rs.t_gap(got["t"].astype(np.float64), want["t"], rs.t_slack(rays)[hit])
    print("general-matrix instance: %d hits, %d misses, largest gap in t %.3g (band %.3g)" % (len(hit), miss.sum(), gap.max(), rs.GENERAL_BAND))
    assert np.all(gap <= rs.GENERAL_BAND)
    return len(hit)


def _exact(case, n):
    which = ~case["touch"].copy()
    which[n:] = False
    return which


def check_count(case, ev, calls, idsum, n):
    is_exact = np.array([i["exact"] for i in case["scene"]["instances"]])
    assert is_exact.sum() >= 5
    assert np.array_equal(calls[:n][:, is_exact].astype(np.int64), ev["calls"][:n][:, is_exact])
    assert np.array_equal(idsum[:n][:, is_exact].astype(np.int64), ev["idsum"][:n][:, is_exact])
    assert np.all(calls[n:] == 0)
    assert ev["calls"][:n][:, is_exact].sum() > 4 * n or n < 1000


# ---- the big scene -----------------------------------------------------------------------------------------------------
def test_count_pass_calls_exactly_the_leaf_boxes_of_the_slab_test(big):
    """Pass 1: per (ray, instance) the intersection-program calls and the sum of the primitives called equal the float32
    slab test over every leaf box -- no band, no exclusions (every instance but the general-matrix one)."""
    case = rs.case("big")
    check_count(case, case["f32"], big["count"][1], big["count"][2], rs.N_RAYS)


def test_closest_hit_is_bit_equal(big):
    """Pass 2: primitive, geometry, instance id and index, hit kind, attribute and t (in bits) of the closest hit."""
    case = rs.case("big")
    c = case["f32"]["cands"]
    hits, misses = check_hits(case, case["f32"], big["closest"][0], _exact(case, rs.N_RAYS), rs.eligible(c, case["rays"]))
    assert hits > 2000 and misses > 300
    assert np.all(big["closest"][0]["prim"][rs.N_RAYS:] == -9)  # the launch had N_RAYS indices: nothing wrote past them


@pytest.mark.parametrize("name,modes", [("ignore_odd", (1, 1)), ("ignore_near", (1, 2))])
def test_ignored_candidates_leave_the_accepted_hit_alone(big, name, modes):
    """Pass 3: any-hit ignores odd primitives / near roots (owlGeomSet1i + owlBuildSBT): the closest of the rest, with ITS
    t, kind and attribute although nearer candidates were reported and ignored after it was accepted."""
    case = rs.case("big")
    c = case["f32"]["cands"]
    hits, _ = check_hits(case, case["f32"], big[name][0], _exact(case, rs.N_RAYS), rs.eligible(c, case["rays"], *modes))
    assert hits > 1500
    assert not np.array_equal(big[name][0], big["closest"][0])


def test_terminate_ray_ends_at_an_acceptable_candidate(big):
    """Pass 4: any-hit accepts and calls optixTerminateRay: one of the candidates inside (tmin, tmax), closest-hit ran
    with its t, kind and attribute; without candidates the miss program ran."""
    case = rs.case("big")
    c = case["f32"]["cands"]
    ok = rs.eligible(c, case["rays"])
    hits, misses = check_hits(case, case["f32"], big["terminate"][0], _exact(case, rs.N_RAYS), ok, closest=False)
    assert hits > 2000 and misses > 300
    # the walk did stop early: some rays ended on a candidate that is not the closest
    rec, which = big["terminate"][0], _exact(case, rs.N_RAYS)
    assert (which & (rec["status"] == 1) & (rec["t"] != big["closest"][0]["t"])).sum() > 100


def test_second_ray_type(big):
    """Pass 5: rays of type 1 (every third) use the spheres' far-root program of that type, no closest-hit program and the
    second miss program; boxes have no program of that type.  Type-0 rays of the same launch are unchanged."""
    case = rs.case("big")
    rays, c = case["rays"], case["f32"]["cands"]
    rec, n = big["types"][0], rs.N_RAYS
    type0 = rays["type"] == 0
    type0[n:] = False
    assert np.array_equal(rec[type0], big["closest"][0][type0])
    which = _exact(case, n) & (rays["type"] == 1)
    ok = rs.eligible(c, rays, far_only=True)
    has = np.bincount(c["ray"][ok], minlength=len(rays)).astype(bool)
    miss = which & ~has
    assert miss.sum() > 100 and np.all(rec["status"][miss] == rs.MISS1_RAN) and np.all(rec["prim"][miss] == -7)
    assert np.all(rec["far_prim"][miss] == -2)
    hit = np.flatnonzero(which & has)
    got = rec[hit]
    assert len(hit) > 500 and np.all(_untouched(got))  # no closest-hit record, no miss program
    ids = [i["id"] for i in case["scene"]["instances"]]
    inst = np.array([ids.index(v) if v in ids else -1 for v in got["far_inst_id"].tolist()])
    assert np.all(inst >= 0)
    at = _lookup(c, hit, inst, got["far_geom"], got["far_prim"], 1)
    assert np.all(at >= 0) and np.all(ok[at])
    assert np.array_equal(_bits(got["far_t"]), _bits(c["t"][at]))
    assert np.array_equal(c["t"][at], rs.best_t(c, ok, len(rays))[hit])


def test_ray_flags(big):
    """Pass 6: every geometry's any-hit program ignores odd primitives; each OPTIX_RAY_FLAG_* on top of that."""
    case = rs.case("big")
    rays, c, n = case["rays"], case["f32"]["cands"], rs.N_RAYS
    which = _exact(case, n)
    with_anyhit, without = rs.eligible(c, rays, 1, 1), rs.eligible(c, rays, anyhit=False)
    # DISABLE_ANYHIT: no any-hit call, every candidate in range is accepted
    check_hits(case, case["f32"], big["flag_disable_anyhit"][0], which, without)
    assert np.array_equal(big["flag_disable_anyhit"][0][:n], big["closest"][0][:n])
    # ENFORCE_ANYHIT: nothing to override
    check_hits(case, case["f32"], big["flag_enforce_anyhit"][0], which, with_anyhit)
    assert np.array_equal(big["flag_enforce_anyhit"][0][:n], big["ignore_odd"][0][:n])
    # TERMINATE_ON_FIRST_HIT: the first ACCEPTED candidate ends the walk, closest-hit still runs
    rec = big["flag_terminate_first"][0]
    check_hits(case, case["f32"], rec, which, with_anyhit, closest=False)
    assert (which & (rec["status"] == 1) & (rec["t"] != big["ignore_odd"][0]["t"])).sum() > 100
    # DISABLE_CLOSESTHIT: no closest-hit call on a hit, the miss program on a miss
    rec = big["flag_disable_closesthit"][0]
    has = np.bincount(c["ray"][with_anyhit], minlength=len(rays)).astype(bool)
    assert (which & has).sum() > 1500 and np.all(_untouched(rec[which & has]))
    assert np.all(rec["status"][which & ~has] == rs.MISS0_RAN)
    # DISABLE_ANYHIT | TERMINATE_ON_FIRST_HIT
    rec = big["flag_disable_anyhit_terminate_first"][0]
    check_hits(case, case["f32"], rec, which, without, closest=False)
    odd = which & (rec["status"] == 1) & (rec["prim"] % 2 == 1)
    assert odd.sum() > 100  # (odd primitives are accepted again)


def test_general_matrix_instance_against_float64(big):
    """Pass 7: rays that touch the rotation x shear instance, closest hit against the float64 restatement."""
    case = rs.case("big")
    which = np.arange(len(case["rays"])) < rs.N_RAYS
    assert check_general(case, case["f64"], big["closest"][0], which) > 400


def test_launch_shapes(big):
    """Pass 8: the same rays as a 37 x 111 launch (4107 indices over 17 workgroups, the last 11 rays miss) give the same
    records by i = x + y * dims.x; a launch of one index writes one record."""
    case = rs.case("big")
    n, total = rs.N_RAYS, rs.LAUNCH_2D[0] * rs.LAUNCH_2D[1]
    assert total == len(case["rays"]) == 4107 and total % 256 != 0
    rec = big["launch2d"][0]
    assert np.array_equal(rec[:n], big["closest"][0][:n])
    assert np.all(rec["status"][n:] == rs.MISS0_RAN) and np.all(rec["prim"][n:] == -1)
    check_hits(case, case["f32"], rec, _exact(case, total), rs.eligible(case["f32"]["cands"], case["rays"]))
    one = big["launch_one"][0]
    assert np.array_equal(one[:1], big["closest"][0][:1]) and one["status"][0] != -9
    assert np.all(one["prim"][1:] == -9)


def test_refit_then_real_rays(big):
    """Pass 9: a third of the centres moved, a fifth of the half-widths changed, owlGroupRefitAccel on the groups and on
    the instance group: the closest hits of the new scene."""
    case = rs.case("big")
    ev = case["f32_refit"]
    hits, _ = check_hits(case, ev, big["refit"][0], _exact(case, rs.N_RAYS), rs.eligible(ev["cands"], case["rays"]))
    assert hits > 2000
    changed = (_bits(big["refit"][0]["t"]) != _bits(big["closest"][0]["t"]))[:rs.N_RAYS]
    assert changed.sum() > 500


# ---- trees of 1, 2 and 65 primitives -----------------------------------------------------------------------------------
def test_small_trees(small):
    case = rs.case("small")
    rays, c, n = case["rays"], case["f32"]["cands"], len(case["rays"])
    assert sorted(sum(len(g["half"]) for g in grp) for grp in case["scene"]["groups"]) == [1, 2, 65]
    which = _exact(case, n)
    check_count(case, case["f32"], small["count"][1], small["count"][2], n)
    hits, misses = check_hits(case, case["f32"], small["closest"][0], which, rs.eligible(c, rays))
    assert hits > 150 and misses > 50
    check_hits(case, case["f32"], small["ignore_odd"][0], which, rs.eligible(c, rays, 1, 1))
    check_hits(case, case["f32"], small["ignore_near"][0], which, rs.eligible(c, rays, 1, 2))
    check_hits(case, case["f32"], small["terminate"][0], which, rs.eligible(c, rays), closest=False)
    check_general(case, case["f64"], small["closest"][0], np.ones(n, bool))
    type0 = rays["type"] == 0
    assert np.array_equal(small["types"][0][type0], small["closest"][0][type0])


# ---- LaunchDesc::order ---------------------------------------------------------------------------------------------------
def test_launch_order_permutation_with_real_rays(tmp_path):
    """One built user group and as many rays as it has primitives: the launch hands the group's curve order to the
    threads (LaunchDesc::order).  Records are equal by ray index with the permutation and, OWL_LAUNCH_ORDER=0, without."""
    case = rs.case("single")
    rays, c, n = case["rays"], case["f32"]["cands"], len(case["rays"])
    assert n % 256 != 0 and n > 256
    env = dict(os.environ)
    env.pop("OWL_LAUNCH_ORDER", None)
    runs = [_run(tmp_path, "single", ["count", "closest"], n, n, 1, env=e) for e in (env, dict(env, OWL_LAUNCH_ORDER="0"))]
    for run in runs:
        check_count(case, case["f32"], run["count"][1], run["count"][2], n)
        hits, _ = check_hits(case, case["f32"], run["closest"][0], _exact(case, n), rs.eligible(c, rays))
        assert hits > 200
        check_general(case, case["f64"], run["closest"][0], np.ones(n, bool))
    assert np.array_equal(runs[0]["closest"][0]["t"].view(U4), runs[1]["closest"][0]["t"].view(U4))
