"""The brute-force ray reference (tests/ray_spec.py) judged on the CPU, before tests/test_owl_rays_gpu.py compares the GPU
with it: its float32 and float64 restatements agree, every category of ray the GPU tests claim to cover is there in
numbers, and the rays skipped as undecided at the general-matrix instance stay under the cap."""
import numpy as np

import ray_spec as rs

F4 = np.float32


def _closest(ev, rays, **kw):
    c = ev["cands"]
    ok = rs.eligible(c, rays, **kw)
    return c, ok, rs.best_candidate(c, ok, len(rays))


def test_inverse_of_an_exact_instance_is_exact():
    for inst in rs.make_scene("small")["instances"]:
        if inst["exact"]:
            o2w, w2o = inst["o2w"].astype(np.float64), inst["w2o"].astype(np.float64)
            assert np.array_equal(w2o[:, :3] @ o2w[:, :3], np.eye(3)), inst["kind"]
            assert np.array_equal(w2o[:, :3] @ o2w[:, 3] + w2o[:, 3], np.zeros(3)), inst["kind"]
            assert np.count_nonzero(w2o[:, :3]) == 3


def test_float32_and_float64_restatements_agree_on_the_exact_instances():
    worst = 0.0
    for name in ("big", "small", "single"):
        case = rs.case(name)
        rays, exact = case["rays"], ~case["touch"]
        is_exact = np.array([i["exact"] for i in case["scene"]["instances"]])
        # (ray, box) pairs: the slab test passes for the same leaf boxes
        assert np.array_equal(case["f32"]["calls"][:, is_exact], case["f64"]["calls"][:, is_exact]), name
        assert np.array_equal(case["f32"]["idsum"][:, is_exact], case["f64"]["idsum"][:, is_exact]), name
        for kw in (dict(), dict(mode_boxes=1, mode_spheres=1), dict(mode_boxes=1, mode_spheres=2), dict(far_only=True)):
            c32, _, b32 = _closest(case["f32"], rays, **kw)
            c64, _, b64 = _closest(case["f64"], rays, **kw)
            assert np.array_equal((b32 >= 0)[exact], (b64 >= 0)[exact]), (name, kw)
            hit = exact & (b32 >= 0)
            for col in ("inst", "geom", "prim", "kind"):
                assert np.array_equal(c32[col][b32[hit]], c64[col][b64[hit]]), (name, kw, col)
            t32, t64 = c32["t"][b32[hit]], c64["t"][b64[hit]]
            worst = max(worst, float(np.max(rs.t_gap(t32, t64, rs.t_slack(rays)[hit]))))
    print("largest difference in t between the restatements (rs.t_gap), exact instances: %.3g" % worst)
    # Not a tolerance of the GPU tests (those compare bits) but a check of the float32 restatement: the programs do a
    # dozen float32 operations on coordinates of the size rs.t_slack measures, so the two agree to a few units of 2^-24
    # = 6e-8 in that measure, while a wrong formula is off by O(1).  64 units:
    assert worst < 64 * 2.0 ** -24


def test_spheres_lie_inside_the_boxes_the_walk_must_reach():
    """The premise of the hit passes: a sphere root inside the ray's interval belongs to a leaf box that passes the slab
    test (radius 0.75 half: a quarter of the half-width of margin), so culling never legitimately loses a hit."""
    for name in ("big", "small", "single"):
        case = rs.case(name)
        for key in ("f32", "f64", "f32_refit"):
            if key in case:
                assert case[key]["sphere_outside_box"] == 0, (name, key)


def test_every_category_of_ray_is_populated():
    case = rs.case("big")
    scene, n = case["scene"], rs.N_RAYS
    rays, ev = case["rays"][:n], case["f32"]
    exact = ~case["touch"][:n]
    d, o = rays["dir"], rays["org"]
    zeros = (d == 0).sum(1)
    neg_zero, pos_zero = ((d == 0) & np.signbit(d)).any(1), ((d == 0) & ~np.signbit(d)).any(1)
    count = {}
    count["one zero direction component"] = int((zeros == 1).sum())
    count["two zero direction components"] = int((zeros == 2).sum())
    count["a +0.0 component"], count["a -0.0 component"] = int(pos_zero.sum()), int(neg_zero.sum())
    octant = (d[:, 0] < 0) * 4 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0)
    for k in range(8):
        count["octant %d" % k] = int(((octant == k) & (zeros == 0) & exact).sum())
    length = np.sqrt((d.astype(np.float64) ** 2).sum(1))
    count["unnormalised direction"] = int((np.abs(length - 1) > 0.05).sum())

    c = ev["cands"]
    c = c[c["ray"] < n]
    tmin, tmax = rays["tmin"][c["ray"]].astype(np.float64), rays["tmax"][c["ray"]].astype(np.float64)
    inside_sphere = c["sphere"] & (c["kind"] == 1) & (c["t"] > 0)  # far root ahead ...
    near_behind = np.zeros(len(c), bool)
    near_behind[1:] = (c["kind"][:-1] == 0) & (c["t"][:-1] < 0) & c["sphere"][:-1]  # ... and near root behind (sorted: near, far)
    count["origin inside a sphere"] = len(np.unique(c["ray"][inside_sphere & near_behind & exact[c["ray"]]]))
    # a box candidate passed the slab test from tmin on; entered before t = 0 with tmin = 0: the origin is in the box
    count["origin inside a box"] = len(np.unique(c["ray"][~c["sphere"] & (c["t"] < 0) & (tmin == 0) & exact[c["ray"]]]))
    on_face = np.zeros(n, bool)
    for g in scene["groups"][scene["instances"][0]["child"]]:  # the identity instance: world = object space
        lo, hi = g["centers"] - g["half"][:, None], g["centers"] + g["half"][:, None]
        for s in range(0, n, 256):
            oo = o[s:s + 256, None, :]
            within = ((lo[None] <= oo) & (oo <= hi[None])).all(2)
            on_face[s:s + 256] |= (within & ((oo == lo[None]) | (oo == hi[None])).any(2)).any(1)
    count["origin exactly on a box face"] = int(on_face.sum())
    count["on a face, zero direction in that axis"] = int((on_face & (zeros >= 1)).sum())

    ok0 = rs.eligible(c, rays)
    b0 = rs.best_t(c, ok0, n)
    no_tmin = rays.copy()
    no_tmin["tmin"] = 0
    count["tmin > 0 cuts off a nearer hit"] = int(((rs.best_t(c, rs.eligible(c, no_tmin), n) < b0) & exact).sum())
    no_tmax = rays.copy()
    no_tmax["tmax"] = F4(1e30)
    count["finite tmax cuts off the only hit"] = int((np.isinf(b0) & np.isfinite(rs.best_t(c, rs.eligible(c, no_tmax), n)) & exact).sum())
    count["misses everything"] = int((np.isinf(b0) & exact).sum())
    count["meets no leaf box at all"] = int((ev["calls"][:n].sum(1) == 0).sum())
    best = rs.best_candidate(c, ok0, n)
    hit = (best >= 0) & exact
    for i, inst in enumerate(scene["instances"]):
        if inst["exact"]:
            for g in scene["groups"][inst["child"]]:
                sel = hit & (c["inst"][best] == i) & (c["geom"][best] == g["tag"])
                count["closest hit in instance %d (%s), geometry %d" % (i, inst["kind"], g["tag"])] = int(sel.sum())
    count["closest hit is a far root (kind 1)"] = int((hit & (c["kind"][best] == 1)).sum())
    b1 = rs.best_t(c, rs.eligible(c, rays, 1, 1), n)
    count["ignored odd primitive nearer than the accepted hit"] = int(((b0 < b1) & np.isfinite(b1) & exact).sum())
    b2 = rs.best_t(c, rs.eligible(c, rays, 1, 2), n)
    best2 = rs.best_candidate(c, rs.eligible(c, rays, 1, 2), n)
    count["ignored near root nearer than the accepted hit"] = int(((b0 < b2) & np.isfinite(b2) & (c["kind"][best2] == 1) & exact).sum())
    per_ray = np.bincount(c["ray"][ok0], minlength=n)
    count["two or more candidates"] = int(((per_ray >= 2) & exact).sum())
    type1 = rays["type"] == 1
    bf = rs.best_t(c, rs.eligible(c, rays, far_only=True), n)
    count["type-1 ray with a hit"] = int((type1 & np.isfinite(bf) & exact).sum())
    count["type-1 ray without"] = int((type1 & np.isinf(bf) & exact).sum())
    count["type-1 ray whose far root is not the type-0 answer"] = int((type1 & np.isfinite(bf) & (bf != b0) & exact).sum())
    # the general-matrix instance
    gi = [i for i, inst in enumerate(scene["instances"]) if not inst["exact"]][0]
    c64 = case["f64"]["cands"]
    b64 = rs.best_candidate(c64, rs.eligible(c64, case["rays"]), len(case["rays"]))[:n]
    count["closest hit in the general-matrix instance"] = int(((b64 >= 0) & (c64["inst"][b64] == gi)).sum())
    for k, v in count.items():
        print("%6d  %s" % (v, k))
    for k, v in count.items():
        assert v >= 20, (k, v)
    # the padding rays of the 2-D launch miss everything
    assert np.all(case["f32"]["calls"][n:] == 0) and np.all(case["f64"]["calls"][n:] == 0)


def test_small_scenes_reach_every_instance_and_geometry():
    for name in ("small", "single"):
        case = rs.case(name)
        c, ok, best = _closest(case["f32"], case["rays"])
        hit = (best >= 0) & ~case["touch"]
        for i, inst in enumerate(case["scene"]["instances"]):
            if inst["exact"]:
                for g in case["scene"]["groups"][inst["child"]]:
                    assert (hit & (c["inst"][best] == i) & (c["geom"][best] == g["tag"])).sum() >= 3, (name, i, g["tag"])
    single = rs.case("single")
    assert len(single["scene"]["groups"]) == 1
    assert len(single["rays"]) == sum(len(g["half"]) for g in single["scene"]["groups"][0])  # what hands out LaunchDesc::order


def test_general_instance_gap_and_undecided_cap():
    """The band of the general-matrix comparison: 4x the largest relative gap between the two restatements on the rays that
    touch that instance (rs.GENERAL_MEASURED_REL_GAP is that measurement, rounded up), and at most 2 % of them undecided."""
    for name in ("big", "small", "single"):
        case = rs.case(name)
        rays, touch = case["rays"], case["touch"]
        und = rs.undecided(case["f64"], rays)
        share = (und & touch).sum() / max(1, touch.sum())
        c32, ok32, b32 = _closest(case["f32"], rays)
        c64, ok64, b64 = _closest(case["f64"], rays)
        sel = touch & ~und
        assert np.array_equal((b32 >= 0)[sel], (b64 >= 0)[sel]), name
        hit = sel & (b64 >= 0)
        for col in ("inst", "geom", "prim", "kind"):
            assert np.array_equal(c32[col][b32[hit]], c64[col][b64[hit]]), (name, col)
        t32, t64 = c32["t"][b32[hit]], c64["t"][b64[hit]]
        gap = float(np.max(rs.t_gap(t32, t64, rs.t_slack(rays)[hit]))) if hit.any() else 0.0
        print("%s: %d rays touch the general instance, %d undecided (%.2f %%), %d hits, largest gap in t (rs.t_gap) %.3g"
              % (name, touch.sum(), (und & touch).sum(), 100 * share, hit.sum(), gap))
        gi = [i for i, inst in enumerate(case["scene"]["instances"]) if not inst["exact"]][0]
        e32, e64 = (case[k]["events"] for k in ("f32", "f64"))
        e32, e64 = (e[(e["inst"] == gi) & touch[e["ray"]]] for e in (e32, e64))
        _, i32, i64 = np.intersect1d(rs.key_of(e32["ray"], gi, e32["geom"], e32["prim"], 0),
                                     rs.key_of(e64["ray"], gi, e64["geom"], e64["prim"], 0), return_indices=True)
        decision_gap = float(np.max(np.abs(e32["rel"][i32] - e64["rel"][i64])))
        print("%s: largest gap in a discriminant or a slab interval, relative: %.3g over %d" % (name, decision_gap, len(i32)))
        assert share <= rs.UNDECIDED_CAP, name
        assert gap <= rs.GENERAL_MEASURED_REL_GAP, name
        assert decision_gap <= rs.GENERAL_MEASURED_DECISION_GAP, name
        if name == "big":
            assert touch.sum() >= 400 and hit.sum() >= 200
