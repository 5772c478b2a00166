#!/usr/bin/env python3
"""Times of tknnIcp (rigid registration by iterated closest points, the loop inside the library) on one MI355X, written to
profiles/icp_measurements.json.

The target: --points uniform points of the unit cube, built once, with normals from TrueKNN.normals(k=16).  The sources: --queries
(1 M and 100 k) of its points moved by half a degree and a quarter of the mean spacing.  Per source both methods and two max_dist,
about 2 x and 50 x the mean spacing n^(-1/3).  The loop runs --steps steps with both thresholds 0, so it never stops by itself; a
time per iteration is the call's time over its searches.  Per configuration the variants alternate inside every repetition, --reps
of them after 1 warm-up, in one process on one tree; median, minimum and maximum of each:
  icp               the call as built: per iteration all of it, its searches (transform, order, seed bounds, walks) and its moments;
  prev_bound=0/1 x reuse_order=0/1   the two measured choices of DESIGN 3.4n through TKNN_ICP_PREV_BOUND and TKNN_ICP_REUSE_ORDER:
                    the previous partner's distance as a walk bound from the second search on, and the first search's curve order
                    kept.  The results of the four are compared bit for bit before anything is timed;
  knn_floor         tknnKnn at k = 1 on the transformed points of the call's last search: what a search cannot go below;
  recipe            what a user has without the call, per iteration on the same device: the transform in torch, TrueKNN.knn at
                    k = 1, a mask by max_dist, gathers, the sums and torch.linalg.svd (point-to-point) or torch.linalg.solve
                    (point-to-plane), fitness and rmse read on the host.

    python scripts/icp_measurements.py [--reps 3] [--steps 10] [--out profiles/icp_measurements.json]
"""
import argparse
import contextlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from radius_measurements import stats  # noqa: E402


@contextlib.contextmanager
def choices(prev_bound, reuse_order):
    names = {"TKNN_ICP_PREV_BOUND": prev_bound, "TKNN_ICP_REUSE_ORDER": reuse_order}
    before = {k: os.environ.pop(k, None) for k in names}
    for k, v in names.items():
        if v is not None:
            os.environ[k] = "1" if v else "0"
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--queries", default="1000000,100000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    n = a.points
    spacing = n ** (-1.0 / 3.0)
    rec = {"device": torch.cuda.get_device_name(0), "warmups": 1, "points": n, "steps": a.steps, "mean_spacing": spacing,
           "source_fingerprint": _lib.source_fingerprint(), "cases": []}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every configuration: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    P = torch.from_numpy(datasets.uniform3d(n, seed=0)).to(dev)
    eng = TrueKNN(device=0)
    eng.build(P)
    normals = eng.normals(k=16)["normals"]
    ang = np.deg2rad(0.5)
    R0 = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    rng = np.random.default_rng(5)
    for m in (int(x) for x in a.queries.split(",")):
        rows = torch.from_numpy(rng.choice(n, m, replace=False)).to(dev)
        mid = np.full(3, 0.5)
        S = ((P[rows].double() - torch.tensor(mid, device=dev)) @ torch.tensor(R0.T, device=dev) + torch.tensor(mid + 0.25 * spacing, device=dev)).float().contiguous()
        for method in ("point_to_point", "point_to_plane"):
            for factor in (2.0, 50.0):
                max_dist = factor * spacing
                kw = dict(method=method, target_normals=normals if method == "point_to_plane" else None, max_iterations=a.steps, rel_fitness=0.0, rel_rmse=0.0)
                case = {"queries": m, "method": method, "max_dist": max_dist, "max_dist_over_spacing": factor}
                variants = {"icp": (None, None), "prev_bound=0,reuse_order=0": (False, False), "prev_bound=1,reuse_order=0": (True, False),
                            "prev_bound=0,reuse_order=1": (False, True), "prev_bound=1,reuse_order=1": (True, True)}
                # the choices change no result
                first = None
                for name, (pb, ro) in variants.items():
                    with choices(pb, ro):
                        r = eng.icp(S, max_dist, want_correspondences=True, want_aligned=True, **kw)
                    bits = (r["transform"].numpy().tobytes(), r["corr"].cpu().numpy().tobytes(), r["inlier_rmse"], r["fitness"])
                    first = first or bits
                    assert bits == first, "%s changes the result" % name
                    last = r
                case.update(searches=last["searches"], fitness=last["fitness"], inlier_rmse=last["inlier_rmse"], lane_rows=last["lane_rows"])
                aligned = last["aligned"]
                Rm = torch.tensor(last["transform"][:3, :3].numpy(), dtype=torch.float32, device=dev)
                tv = torch.tensor(last["transform"][:3, 3].numpy(), dtype=torch.float32, device=dev)

                def recipe_iteration():
                    X = S @ Rm.T + tv
                    k = eng.knn(X, k=1)
                    ok = k["dist"][:, 0] <= max_dist
                    idx = k["idx"][:, 0][ok].long()
                    x, p = X[ok], P[idx]
                    d2 = ((x - p) ** 2).sum(1)
                    if method == "point_to_point":
                        mu_s, mu_p = x.mean(0), p.mean(0)
                        H = (x - mu_s).T @ (p - mu_p)
                        U, _, Vt = torch.linalg.svd(H)
                        D = torch.eye(3, device=dev)
                        D[2, 2] = torch.sign(torch.linalg.det(Vt.T @ U.T))
                        step = Vt.T @ D @ U.T
                    else:
                        nn = normals[idx]
                        r = ((x - p) * nn).sum(1)
                        J = torch.cat([torch.linalg.cross(x, nn), nn], dim=1)
                        step = torch.linalg.solve(J.T @ J, -(J.T @ r))
                    return float(ok.float().mean()), float(d2.mean().sqrt()), step.cpu()

                t = {name: {"per_iteration_ms": [], "search_ms": [], "moment_ms": []} for name in variants}
                t["knn_floor"], t["recipe"] = {"ms": [], "walk_ms": []}, {"per_iteration_ms": []}
                for rep in range(a.reps + 1):
                    for name, (pb, ro) in variants.items():
                        with choices(pb, ro):
                            r = eng.icp(S, max_dist, **kw)
                        if rep:
                            t[name]["per_iteration_ms"].append(r["solve_ms"] / r["searches"])
                            t[name]["search_ms"].append(r["search_ms"] / r["searches"])
                            t[name]["moment_ms"].append(r["moment_ms"] / r["searches"])
                    ms, k = timed(lambda: eng.knn(aligned, k=1))
                    ms_r, _ = timed(lambda: [recipe_iteration() for _ in range(3)])
                    if rep:
                        t["knn_floor"]["ms"].append(ms)
                        t["knn_floor"]["walk_ms"].append(k["info"]["solve_ms"])
                        t["recipe"]["per_iteration_ms"].append(ms_r / 3)
                case["times"] = {name: {f: stats(v) for f, v in fields.items()} for name, fields in t.items()}
                med = lambda name, f: case["times"][name][f]["median"]  # noqa: E731
                case["ratios"] = {"recipe_over_icp": med("recipe", "per_iteration_ms") / med("icp", "per_iteration_ms"),
                                  "icp_search_over_knn_floor": med("icp", "search_ms") / med("knn_floor", "ms"),
                                  "prev_bound_1_over_0": med("prev_bound=1,reuse_order=0", "per_iteration_ms") / med("prev_bound=0,reuse_order=0", "per_iteration_ms"),
                                  "reuse_order_1_over_0": med("prev_bound=0,reuse_order=1", "per_iteration_ms") / med("prev_bound=0,reuse_order=0", "per_iteration_ms"),
                                  "both_over_neither": med("prev_bound=1,reuse_order=1", "per_iteration_ms") / med("prev_bound=0,reuse_order=0", "per_iteration_ms")}
                rec["cases"].append(case)
                save()
                print("m %d %s max_dist %.0fx: icp %.3f ms/it (search %.3f, moments %.3f), knn floor %.3f, recipe %.3f; ratios %s"
                      % (m, method, factor, med("icp", "per_iteration_ms"), med("icp", "search_ms"), med("icp", "moment_ms"), med("knn_floor", "ms"),
                         med("recipe", "per_iteration_ms"), json.dumps({k: round(v, 3) for k, v in case["ratios"].items()})), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
