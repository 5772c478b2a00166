"""Brute-force reference for the ray path of include/owl/device_runtime.h, as driven by tests/owl_programs/ray_programs.cu
through `owl_host_driver rays`.  numpy only; no tree: every (ray, instance, primitive) is evaluated.

The programs are restated twice by the same code, run on two number types:

* float32, operation for operation (the device programs switch contraction off, and tools/owl_embed.py compiles device
  code with -ffp-contract=off): this restatement decides equality.  For the EXACT instances -- identity, translation,
  signed axis permutation x power-of-two scale -- the object-space ray is derivable bit for bit whatever the compiler
  does with `xfm_point`: each row has one non-zero product, that product is exact, so the row is fl(+-2^k x + t) with or
  without an FMA, and `invert_3x4` (double precision on the host) inverts such a matrix exactly.
* float64 on the same float32 inputs: for the general-matrix instance (rotation x shear), where a compiler that is
  allowed to contract `xfm_point` may round differently, and to judge the float32 restatement itself.

The slab test is monotone under rounding (subtracting the same origin and dividing by the same direction component
preserve order, fmin / fmax are exact), so the interval of a parent box always contains its children's: a correct tree
walk calls the intersection program for EXACTLY the leaf boxes that pass the float32 slab test with the ray's initial
interval, as long as no hit shortens the ray (the COUNT pass reports none).
"""
import functools
import struct

import numpy as np

F4, U4, I4 = np.float32, np.uint32, np.int32
RAY_DTYPE = np.dtype([("org", F4, 3), ("dir", F4, 3), ("tmin", F4), ("tmax", F4), ("type", U4), ("flags", U4)])
HIT_DTYPE = np.dtype([("prim", I4), ("inst_id", U4), ("inst_index", I4), ("kind", I4), ("attr0", U4), ("t", F4),
                      ("geom", I4), ("status", I4), ("far_prim", I4), ("far_inst_id", U4), ("far_geom", I4), ("far_t", F4)])
assert RAY_DTYPE.itemsize == 40 and HIT_DTYPE.itemsize == 48
SCENE_MAGIC = 0x52415953
BOXES, SPHERES = 0, 1
# status column of a record (ray_programs.cu)
UNTOUCHED, CLOSEST_HIT_RAN, MISS0_RAN, MISS1_RAN = 0, 1, 2, 3

# ---- general-matrix instance: how far float32 may lie from float64 ---------------------------------------------------
# Largest difference in the closest hit's t between the float32 and the float64 restatement, in the measure of t_gap()
# below (relative to |t| + |org| / |dir|), over the decided rays of the big scene that touch the general-matrix
# instance; measured on the CPU by tests/test_ray_expectations.py::test_general_instance_gap_and_undecided_cap, which
# asserts that the measurement stays below this constant.  Measured: 4.2e-7.
GENERAL_MEASURED_REL_GAP = 4.5e-7
# A compiler that contracts the header's xfm_point to FMAs changes each object-space coordinate by at most one rounding,
# the same size of perturbation that separates the two restatements; 4x the measured gap is the margin granted for it.
GENERAL_MARGIN_FACTOR = 4.0
GENERAL_BAND = GENERAL_MARGIN_FACTOR * GENERAL_MEASURED_REL_GAP
# The same for the two yes/no decisions of the programs, each a quantity compared with zero: a sphere's discriminant
# relative to the terms that cancel in it, (r*r - l*l) / max(r*r, l*l), and a box's clipped slab interval relative to
# its ends, (t1 - t0) / max(|t0|, |t1|).  Largest difference between the restatements over every such quantity below
# 1e-3 on the same rays, same test.  Measured: 1.35e-5 (a sphere of radius 0.03 seen from 1.5 away).
GENERAL_MEASURED_DECISION_GAP = 1.4e-5
GENERAL_DECISION_BAND = GENERAL_MARGIN_FACTOR * GENERAL_MEASURED_DECISION_GAP
UNDECIDED_CAP = 0.02  # at most this share of the general-instance rays may be skipped as undecided


# ---- scenes ----------------------------------------------------------------------------------------------------------
def invert_3x4(m):
    """owl_runtime.cpp's invert_3x4 restated: double arithmetic on the float32 matrix, rounded to float32 at the end."""
    m = np.asarray(m, F4).astype(np.float64).reshape(12)
    a, b, c, d, e, f, g, h, i = m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    idet = 1.0 / det if det != 0.0 else 0.0
    r = [(e * i - f * h) * idet, (c * h - b * i) * idet, (b * f - c * e) * idet,
         (f * g - d * i) * idet, (a * i - c * g) * idet, (c * d - a * f) * idet,
         (d * h - e * g) * idet, (b * g - a * h) * idet, (a * e - b * d) * idet]
    inv = np.zeros(12, F4)
    for row in range(3):
        for col in range(3):
            inv[4 * row + col] = F4(r[3 * row + col])
        inv[4 * row + 3] = F4(-(r[3 * row] * m[3] + r[3 * row + 1] * m[7] + r[3 * row + 2] * m[11]))
    return inv.reshape(3, 4)


def _instances(children):
    """The six transforms (row-major 3x4 object-to-world), their kinds, ids above 2^16 and how the driver sets them."""
    ang = 0.7
    rot = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.4), -np.sin(0.4)], [0, np.sin(0.4), np.cos(0.4)]])
    shear = np.array([[1, 0.3, 0], [0, 1, -0.2], [0, 0, 1.25]])
    mats = [
        ("identity", np.eye(3), (0, 0, 0)),
        ("translation", np.eye(3), (3.0, 0.5, -0.25)),
        # x' = -2 y, y' = 0.5 z, z' = 4 x: a signed permutation with power-of-two scales, determinant -4
        ("reflection", np.array([[0, -2, 0], [0, 0, 0.5], [4, 0, 0]]), (-4.0, 2.0, 1.5)),
        ("scale", np.diag([2.0, 0.5, 4.0]), (0.25, -3.0, 2.0)),
        ("general", rot @ shear, (-3.0, -3.0, -3.0)),
        # x' = -y, y' = x: a quarter turn, determinant +1; this slot's child is set with owlInstanceGroupSetChild
        ("set_child", np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), (2.5, 3.0, 0.0)),
    ]
    out = []
    for n, (kind, lin, tr) in enumerate(mats):
        o2w = np.concatenate([np.asarray(lin, np.float64), np.asarray(tr, np.float64)[:, None]], axis=1).astype(F4)
        how = (1 if n in (1, 2, 4) else 0) | (2 if kind == "set_child" else 0)
        out.append(dict(kind=kind, o2w=o2w, w2o=invert_3x4(o2w), id=70001 + 1000 * n, how=how, child=children[n],
                        exact=kind != "general"))
    assert np.linalg.det(out[2]["o2w"][:, :3].astype(np.float64)) < 0
    return out


def _geom(rng, gtype, n, half_lo, half_hi, second):
    g = dict(type=gtype, centers=rng.random((n, 3)).astype(F4), half=(half_lo + (half_hi - half_lo) * rng.random(n)).astype(F4))
    if second:  # the refit pass: a third of the centres move, every fifth half-width changes
        c2, h2 = g["centers"].copy(), g["half"].copy()
        moved = np.arange(n) % 3 == 1
        c2[moved] = (c2[moved] + (0.2 * rng.random((int(moved.sum()), 3)) - 0.1)).astype(F4)
        resized = np.arange(n) % 5 == 2
        h2[resized] = (h2[resized] * (0.5 + rng.random(int(resized.sum())))).astype(F4)
        g["centers2"], g["half2"] = c2, h2
    return g


def make_scene(name):
    """big: group A = boxes + spheres, group B = spheres, about 2000 primitives each, half-widths over a factor of six.
    small: groups of 1, 2 and 65 primitives.  single: ONE group (the launch-order case)."""
    rng = np.random.default_rng({"big": 20240611, "small": 7, "single": 11}[name])
    if name == "big":
        groups = [[_geom(rng, BOXES, 2000, 0.01, 0.06, True), _geom(rng, SPHERES, 1987, 0.01, 0.06, True)],
                  [_geom(rng, SPHERES, 2003, 0.01, 0.06, True)]]
        children = [0, 1, 0, 1, 0, 1]
    elif name == "small":
        groups = [[_geom(rng, BOXES, 1, 0.2, 0.4, False)],
                  [_geom(rng, SPHERES, 1, 0.2, 0.4, False), _geom(rng, BOXES, 1, 0.2, 0.4, False)],
                  [_geom(rng, SPHERES, 65, 0.05, 0.3, False)]]
        children = [0, 1, 2, 0, 1, 2]
    else:
        groups = [[_geom(rng, BOXES, 300, 0.02, 0.12, False), _geom(rng, SPHERES, 213, 0.02, 0.12, False)]]
        children = [0] * 6
    tag = 0
    for grp in groups:
        for g in grp:
            g["tag"] = tag
            tag += 1
    return dict(name=name, groups=groups, instances=_instances(children))


def scene_bytes(scene):
    has_second = int("centers2" in scene["groups"][0][0])
    out = [struct.pack("<4i", SCENE_MAGIC, len(scene["groups"]), len(scene["instances"]), has_second)]
    for grp in scene["groups"]:
        out.append(struct.pack("<i", len(grp)))
        for g in grp:
            out.append(struct.pack("<2i", g["type"], len(g["half"])))
            out += [g["centers"].tobytes(), g["half"].tobytes()]
            if has_second:
                out += [g["centers2"].tobytes(), g["half2"].tobytes()]
    for inst in scene["instances"]:
        out.append(struct.pack("<3i", inst["child"], inst["id"], inst["how"]))
        out.append(np.ascontiguousarray(inst["o2w"].T).astype(F4).tobytes())  # OWL format: vx, vy, vz, translation
    return b"".join(out)


def ray_bytes(rays):
    return struct.pack("<i", len(rays)) + rays.tobytes()


# ---- rays ------------------------------------------------------------------------------------------------------------
def _to_world(inst, p):
    m = inst["o2w"].astype(np.float64)
    return p @ m[:, :3].T + m[:, 3]


def make_rays(scene, n, n_pad, seed):
    """n rays aimed at the instances of `scene` plus n_pad rays that miss everything.  Besides random rays: axis-parallel
    ones (one or two zero direction components, +0.0 and -0.0), origins inside boxes and spheres and exactly on box faces,
    unnormalised directions, tmin > 0, finite tmax, and rays that point away from everything."""
    rng = np.random.default_rng(seed)
    insts = scene["instances"]
    rays = np.zeros(n + n_pad, RAY_DTYPE)
    rays["tmax"] = F4(1e30)
    rays["type"] = (np.arange(n + n_pad) % 3 == 1).astype(U4)  # used by the `types` pass only
    pick = rng.integers(0, len(insts), n)
    general = [k for k, i in enumerate(insts) if not i["exact"]]
    pick[rng.random(n) < 0.15] = general[0]
    exact_ids = np.array([k for k, i in enumerate(insts) if i["exact"]])
    for k in range(n):
        inst = insts[pick[k]]
        target = _to_world(inst, rng.random(3))
        style = k % 16
        if style < 9:  # from outside (or just inside) the instance's cube towards a point in it, any length of direction
            origin = _to_world(inst, rng.random(3) * 3.0 - 1.0)
            d = (target - origin) * (0.25 + 3.75 * rng.random())
        elif style == 9:  # between instances: may cross several
            origin = _to_world(insts[rng.integers(0, len(insts))], rng.random(3))
            d = (target - origin) * (0.5 + rng.random())
        elif style == 10:  # points away from everything (every instance lies within 20 of the world origin)
            origin = 40.0 + rng.random(3)
            d = rng.random(3) + 0.1
        else:  # axis-parallel in world space through an EXACT instance: zero components stay zero in object space
            inst = insts[0] if style == 15 else insts[exact_ids[rng.integers(0, len(exact_ids))]]
            grp = scene["groups"][inst["child"]]
            g = grp[rng.integers(0, len(grp))]
            j = rng.integers(0, len(g["half"]))
            c, h = g["centers"][j].astype(np.float64), float(g["half"][j])
            axes = rng.permutation(3)
            zero = axes[:2] if style in (11, 12) else axes[:1]
            d_obj = rng.choice([-1.0, 1.0], 3) * (0.3 + 2.0 * rng.random(3))
            d_obj[zero] = 0.0
            if style == 13:  # origin inside the primitive (box and sphere: within 0.5 h of the centre per axis)
                o_obj = c + (rng.random(3) - 0.5) * h
            else:  # through the primitive's box, or just past it in the zero-direction axes
                o_obj = c + (rng.random(3) * 2.2 - 1.1) * h - d_obj * 1.5 * h
            lin = inst["o2w"][:, :3].astype(np.float64)
            origin, d = _to_world(inst, o_obj), lin @ d_obj
            d = np.where(d == 0, rng.choice([0.0, -0.0], 3), d)
            if style == 15:
                # the identity instance: origin exactly on a face plane of the primitive's box, in the zero-direction axis
                # (the closed `lo <= o <= hi` test decides) or in a non-zero one (a slab distance of exactly zero)
                a = zero[0] if (k // 16) % 2 else axes[2]
                face = g["centers"][j][a] - g["half"][j] if (k // 32) % 2 else g["centers"][j][a] + g["half"][j]
                origin[a] = float(F4(face))
        rays["org"][k] = origin.astype(F4)
        rays["dir"][k] = d.astype(F4)
        u = rng.random()
        if style not in (10,) and u < 0.2:
            rays["tmin"][k] = F4(0.6 * rng.random())
        elif u < 0.4:
            rays["tmax"][k] = F4(0.2 + 1.2 * rng.random())
    rays["org"][n:] = F4(50.0)
    rays["dir"][n:] = F4(1.0)
    return rays


# ---- the programs, on any number type --------------------------------------------------------------------------------
def object_rays(inst, rays, T):
    """xfm_point / xfm_vector with w2o, left to right as written in the header."""
    m = inst["w2o"].astype(T)
    o, d = rays["org"].astype(T), rays["dir"].astype(T)
    oo = np.stack([((m[r, 0] * o[:, 0] + m[r, 1] * o[:, 1]) + m[r, 2] * o[:, 2]) + m[r, 3] for r in range(3)], axis=1)
    od = np.stack([(m[r, 0] * d[:, 0] + m[r, 1] * d[:, 1]) + m[r, 2] * d[:, 2] for r in range(3)], axis=1)
    if inst["kind"] == "identity":  # the header skips the transform (same values; signed zeros aside)
        oo, od = o, d
    assert oo.dtype == T and od.dtype == T
    return oo, od


def slab(lo, hi, o, d, t0, t1):
    """ray_hits_box for rays (R) x boxes (P): whether the segment meets the closed box, the entry parameter (max over the
    non-zero axes of the near slab plane: what the Boxes program reports), and how far from touch-and-go the decision
    was: t1 - t0 of the clipped interval relative to its ends (for the undecided band)."""
    T = o.dtype
    R, P = len(o), len(lo)
    T0, T1 = np.repeat(t0[:, None], P, 1), np.repeat(t1[:, None], P, 1)
    entry = np.full((R, P), -np.inf, T)
    ok = np.ones((R, P), bool)
    for a in range(3):
        da, oa = d[:, a][:, None], o[:, a][:, None]
        la, ha = lo[:, a][None, :], hi[:, a][None, :]
        zero = np.flatnonzero(da[:, 0] == 0)  # the d == 0 branch is taken by whole rows: computed apart, below
        keep = (T0[zero].copy(), T1[zero].copy(), entry[zero].copy())
        da = np.where(da == 0, T.type(1), da)
        ta, tb = (la - oa) / da, (ha - oa) / da
        tn, tf = np.fmin(ta, tb), np.fmax(ta, tb)
        np.fmax(T0, tn, out=T0)
        np.fmin(T1, tf, out=T1)
        np.fmax(entry, tn, out=entry)
        passed = T0 <= T1
        if len(zero):
            T0[zero], T1[zero], entry[zero] = keep
            passed[zero] = (la <= oa[zero]) & (oa[zero] <= ha)
        ok &= passed
    assert entry.dtype == T
    with np.errstate(invalid="ignore", divide="ignore"):
        graze = (T1 - T0) / np.maximum(np.abs(T0), np.abs(T1))
    return ok, entry, graze


def sphere_roots(c, r, o, d):
    """The quadratic of ray_programs.cu in its order of operations: real (R, P), near and far root."""
    x, y, z = (o[:, k][:, None] - c[:, k][None, :] for k in range(3))
    dx, dy, dz = (d[:, k][:, None] for k in range(3))
    a = ((dx * dx) + (dy * dy)) + (dz * dz)
    s = -(((x * dx) + (y * dy)) + (z * dz)) / a
    lx, ly, lz = x + (s * dx), y + (s * dy), z + (s * dz)
    rr, ll = (r * r)[None, :], ((lx * lx) + (ly * ly)) + (lz * lz)
    disc = rr - ll
    real = disc >= 0
    with np.errstate(invalid="ignore"):
        h = np.sqrt(disc / a)
    near, far = s - h, s + h
    assert near.dtype == o.dtype
    # how close to tangent, relative to the terms that cancel, and where along the ray (for the undecided band)
    return real, near, far, disc / np.maximum(rr, ll), s


CAND_DTYPE = np.dtype([("ray", I4), ("inst", I4), ("geom", I4), ("prim", I4), ("kind", I4), ("sphere", bool), ("t", np.float64)])


def evaluate(scene, rays, T, second=False, chunk=64):
    """Every candidate the intersection programs can report, in number type T: for boxes that pass the slab test with the
    ray's initial interval the entry point (kind 0), for spheres with real roots both roots (kind 0 near, 1 far), whatever
    their t.  Also per (ray, instance): the number of leaf boxes that pass the slab test and the sum of (tag << 12) + prim
    over them; and `events`: (ray, instance, geometry, primitive, t, rel) of every decision that was touch-and-go within a relative 1e-3 -- a sphere's
    discriminant against zero, a box's clipped slab interval against empty -- for the band of the general instance."""
    R, NI = len(rays), len(scene["instances"])
    calls, idsum = np.zeros((R, NI), np.int64), np.zeros((R, NI), np.int64)
    sphere_outside_box = 0
    cands, events = [], []
    for n, inst in enumerate(scene["instances"]):
        oo, od = object_rays(inst, rays, T)
        t0, t1 = rays["tmin"].astype(T), rays["tmax"].astype(T)
        for g in scene["groups"][inst["child"]]:
            c32, h32 = (g["centers2"], g["half2"]) if second else (g["centers"], g["half"])
            lo, hi = (c32 - h32[:, None]).astype(T), (c32 + h32[:, None]).astype(T)  # the bounds program, in float32
            r = (F4(0.75) * h32).astype(T)
            prim = np.arange(len(h32))
            for s in range(0, R, chunk):
                sl = slice(s, min(R, s + chunk))
                ok, entry, graze = slab(lo, hi, oo[sl], od[sl], t0[sl], t1[sl])
                calls[sl, n] += ok.sum(1)
                idsum[sl, n] += (ok * ((g["tag"] << 12) + prim)[None, :]).sum(1)
                if g["type"] == BOXES:
                    ri, pi = np.nonzero(ok)
                    cands.append(_cands(ri + s, n, g, pi, 0, entry[ri, pi]))
                    ri, pi = np.nonzero(np.abs(graze) < 1e-3)
                    events.append(_events(ri + s, n, g, pi, entry[ri, pi], graze[ri, pi]))
                else:
                    real, near, far, rel, mid = sphere_roots(c32.astype(T), r, oo[sl], od[sl])
                    ri, pi = np.nonzero(np.abs(rel) < 1e-3)
                    events.append(_events(ri + s, n, g, pi, mid[ri, pi], rel[ri, pi]))
                    ri, pi = np.nonzero(real)
                    cands.append(_cands(ri + s, n, g, pi, 0, near[ri, pi]))
                    cands.append(_cands(ri + s, n, g, pi, 1, far[ri, pi]))
                    # a root inside the ray's interval lies in a box the walk must reach: count the exceptions
                    nr, fr, lo_t, hi_t = near[ri, pi], far[ri, pi], t0[ri + s], t1[ri + s]
                    inr = ((nr > lo_t) & (nr < hi_t)) | ((fr > lo_t) & (fr < hi_t))
                    sphere_outside_box += int((inr & ~ok[ri, pi]).sum())
    c = np.concatenate(cands)
    c = c[np.lexsort((c["kind"], c["prim"], c["geom"], c["inst"], c["ray"]))]
    return dict(cands=c, calls=calls, idsum=idsum, events=np.concatenate(events), sphere_outside_box=sphere_outside_box, T=T)


EVENT_DTYPE = np.dtype([("ray", I4), ("inst", I4), ("geom", I4), ("prim", I4), ("t", np.float64), ("rel", np.float64)])


def _events(ray, inst, g, prim, t, rel):
    e = np.zeros(len(ray), EVENT_DTYPE)
    e["ray"], e["inst"], e["geom"], e["prim"], e["t"], e["rel"] = ray, inst, g["tag"], prim, t, rel
    return e


def _cands(ray, inst, g, prim, kind, t):
    c = np.zeros(len(ray), CAND_DTYPE)
    c["ray"], c["inst"], c["geom"], c["prim"], c["kind"], c["sphere"], c["t"] = ray, inst, g["tag"], prim, kind, g["type"] == SPHERES, t
    return c


def key_of(ray, inst, geom, prim, kind):
    return ((((np.asarray(ray, np.int64) * 8 + inst) * 8 + geom) * 8192 + prim) * 2) + kind


def eligible(c, rays, mode_boxes=0, mode_spheres=0, anyhit=True, far_only=False):
    """Which candidates optixReportIntersection accepts at some tmax >= t: inside the ray's open interval, not ignored by
    the any-hit program of the geometry's mode, and -- the far root of a sphere -- only if the near root was not
    accepted (the program reports the far root only then).  far_only: ray type 1 (far roots of spheres, no any-hit)."""
    t = c["t"]
    ok = (t > rays["tmin"][c["ray"]].astype(np.float64)) & (t < rays["tmax"][c["ray"]].astype(np.float64))
    if far_only:
        return ok & c["sphere"] & (c["kind"] == 1)
    if anyhit:
        mode = np.where(c["sphere"], mode_spheres, mode_boxes)
        ok &= ~(((mode == 1) & (c["prim"] % 2 == 1)) | ((mode == 2) & (c["kind"] == 0)))
    # candidates are sorted so that a sphere's far root directly follows its near root
    near_ok = np.zeros(len(c), bool)
    same = (c["kind"][1:] == 1) & (c["kind"][:-1] == 0) & c["sphere"][1:] & \
        (key_of(c["ray"], c["inst"], c["geom"], c["prim"], 0)[1:] == key_of(c["ray"], c["inst"], c["geom"], c["prim"], 0)[:-1])
    near_ok[1:] = same & ok[:-1]
    return ok & ~near_ok


def best_t(c, ok, n_rays):
    """Per ray the smallest t among the candidates `ok` (inf: none)."""
    best = np.full(n_rays, np.inf)
    np.minimum.at(best, c["ray"][ok], c["t"][ok])
    return best


def general_touch(scene, rays, band=GENERAL_BAND):
    """Rays that come near the general-matrix instance: the float64 slab test against its boxes grown by the band's
    share of the box size and position.  Their records are compared with the float64 restatement."""
    touch = np.zeros(len(rays), bool)
    for inst in scene["instances"]:
        if inst["exact"]:
            continue
        oo, od = object_rays(inst, rays, np.float64)
        for g in scene["groups"][inst["child"]]:
            for c32, h32 in [(g["centers"], g["half"])] + ([(g["centers2"], g["half2"])] if "centers2" in g else []):
                grow = 64 * band * (np.abs(c32).max(1) + h32).astype(np.float64)[:, None] + 1e-4
                lo, hi = c32.astype(np.float64) - h32[:, None] - grow, c32.astype(np.float64) + h32[:, None] + grow
                for s in range(0, len(rays), 64):
                    sl = slice(s, s + 64)
                    ok, _, _ = slab(lo, hi, oo[sl], od[sl], rays["tmin"][sl].astype(np.float64), rays["tmax"][sl].astype(np.float64))
                    touch[sl] |= ok.any(1)
    return touch


def t_slack(rays):
    """Per ray, the parameter length of the origin's distance from the world origin, |org| / |dir|.  The float32 rounding of
    coordinates of size |org| moves every surface by about 2^-24 |org| / |dir| along the ray whatever t is, so a hit just
    in front of the origin is not known to 2^-24 of its own small t: every band on t is relative to |t| + this."""
    org, d = rays["org"].astype(np.float64), rays["dir"].astype(np.float64)
    return np.sqrt((org * org).sum(1)) / np.sqrt((d * d).sum(1))


def t_gap(ta, tb, slack):
    """|ta - tb| in the measure of every band on t: relative to the size of t plus the ray's t_slack."""
    return np.abs(ta - tb) / (np.maximum(np.abs(ta), np.abs(tb)) + slack)


def undecided(ev64, rays, band=GENERAL_BAND, decision_band=GENERAL_DECISION_BAND):
    """Rays whose closest hit float64 cannot call for a float32 evaluation.  Only what lies at or before the closest hit
    (plus the band) can change it: there, a discriminant within the band of zero, a root within the band of tmin or
    tmax, a box whose clipped slab interval is within the band of empty (its entry point appears or vanishes like a
    tangent root); and the two nearest accepted candidates closer to each other than the band."""
    c = ev64["cands"]
    R = len(rays)
    ok = eligible(c, rays)
    slack = t_slack(rays)
    lo, hi = rays["tmin"].astype(np.float64), rays["tmax"].astype(np.float64)
    widen = lambda t: band * (np.abs(t) + slack)  # noqa: E731
    reach = best_t(c, ok, R)
    reach = reach + widen(reach)
    und = np.zeros(R, bool)
    ev = ev64["events"]
    r, t, rel = ev["ray"], ev["t"], np.abs(ev["rel"])
    und[r[(rel < decision_band) & (t <= reach[r]) & (t >= (lo - widen(lo))[r]) & (t <= (hi + widen(hi))[r])]] = True
    for edge in (lo, hi):
        near_edge = (t_gap(c["t"], edge[c["ray"]], slack[c["ray"]]) <= band) & (c["t"] <= reach[c["ray"]])
        und[c["ray"][near_edge]] = True
    order = np.lexsort((c["t"][ok], c["ray"][ok]))
    r, t = c["ray"][ok][order], c["t"][ok][order]
    first = np.r_[True, r[1:] != r[:-1]]
    second = np.r_[False, first[:-1]] & ~first  # the second candidate of a ray that has two
    close = np.zeros(len(r), bool)
    close[1:] = second[1:] & (t_gap(t[1:], t[:-1], slack[r[1:]]) <= band)
    und[r[close]] = True
    return und


# ---- shared, computed once per process -------------------------------------------------------------------------------
N_RAYS, LAUNCH_2D = 4096, (37, 111)


@functools.lru_cache(maxsize=None)
def case(name):
    """Scene, rays and both restatements of one of the three scenes; computed once, shared by every test, never changed."""
    scene = make_scene(name)
    if name == "big":
        rays = make_rays(scene, N_RAYS, LAUNCH_2D[0] * LAUNCH_2D[1] - N_RAYS, seed=5)
    elif name == "small":
        rays = make_rays(scene, 600, 0, seed=6)
    else:
        rays = make_rays(scene, sum(len(g["half"]) for g in scene["groups"][0]), 0, seed=8)
    out = dict(scene=scene, rays=rays, f32=evaluate(scene, rays, F4), f64=evaluate(scene, rays, np.float64),
               touch=general_touch(scene, rays))
    if name == "big":
        out["f32_refit"] = evaluate(scene, rays, F4, second=True)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def best_candidate(c, ok, n_rays):
    """Per ray the index into `c` of a candidate with the smallest t among `ok` (-1: none)."""
    idx = np.flatnonzero(ok)
    order = idx[np.lexsort((c["t"][idx], c["ray"][idx]))]
    first = np.r_[True, c["ray"][order][1:] != c["ray"][order][:-1]] if len(order) else np.zeros(0, bool)
    out = np.full(n_rays, -1, np.int64)
    out[c["ray"][order][first]] = order[first]
    return out
