#!/usr/bin/env python3
"""Times of tknnLocalPca (neighbourhood covariance, normals and curvature, no lists) on one MI355X, written to
profiles/pca_measurements.json.

The cases:
  uniform_own   10 M uniform points of the unit cube, the set's own points as queries;
  plane_own     10 M points of a noisy tilted plane over the unit square (sigma 0.002), own points;
  uniform_ext   1 M external uniform queries against the uniform 10 M.
Per case three neighbourhoods: a radius with about 10 and with about 50 points within it, and k = 16.  Per neighbourhood the
variants alternate inside every repetition, --reps of them after 1 warm-up, in one process on one tree; median, minimum and maximum
of the HIP events around each and of the call's own info (bound_ms, order_ms, walk_ms, finish_ms):
  pca            the call with every output;
  normals        the call asking for normals, curvature and counts;
  moments        the call asking for counts, centroid and covariance (no eigen-solve);
  recipe         what a user has without it: radius_query(sort=False) or knn, a torch gather, index_add_ of the nine moments of
                 the offsets, torch.linalg.eigh.  Not run where the lists would hold more than --recipe-pairs pairs;
  reduce_count   tknnRadiusReduce's count pass at the same radius: the floor of a walk that hands out one query per team (radius
                 neighbourhoods);
  knn            tknnKnn alone at the same k (k neighbourhoods): bound_ms + walk_ms against it is what the second walk costs.
Before anything is timed the call's counts are held to the lists' lengths exactly and its covariance to the float64 covariance of
the lists inside the bound of tests/pca_spec.py.

    python scripts/pca_measurements.py [--reps 5] [--cases uniform_own,plane_own,uniform_ext] [--out profiles/pca_measurements.json]
A case replaces the record of the same name in an existing --out file, so the cases can be run one process each.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from radius_measurements import stats  # noqa: E402

U = 2.0 ** -24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--cases", default="uniform_own,plane_own,uniform_ext")
    ap.add_argument("--recipe-pairs", type=float, default=2.5e8, help="the recipe runs where the lists hold at most so many pairs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "warmups": 1, "points": a.points, "queries": a.queries, "cases": []}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            rec["cases"] = json.load(fh).get("cases", [])
    rec["source_fingerprint"] = _lib.source_fingerprint()

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every neighbourhood: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    n, m = a.points, a.queries
    eng = TrueKNN(device=0)
    for name in a.cases.split(","):
        plane = name.startswith("plane")
        own = name.endswith("_own")
        if plane:
            rng = np.random.default_rng(11)
            xy = rng.random((n, 2))
            pts = np.column_stack([xy, 0.3 * xy[:, 0] + 0.2 * xy[:, 1] + 0.1 + 0.002 * rng.standard_normal(n)]).astype(np.float32)
        else:
            pts = np.ascontiguousarray(datasets.uniform3d(n, seed=0), np.float32)
        P = torch.from_numpy(pts).to(dev)
        Q = None if own else torch.from_numpy(np.random.default_rng(7).random((m, 3), dtype=np.float32)).to(dev)
        q_dev, rows_n = (P, n) if own else (Q, m)
        eng.build(P)

        def radius_for(within):
            return float(np.float32(np.sqrt(within / (np.pi * n)) if plane else (within / (n * 4.1887902)) ** (1.0 / 3.0)))

        case = {"case": name, "rows": rows_n, "neighbourhoods": {}}
        for label, radius, k, about in (("within10", radius_for(10), None, 10), ("within50", radius_for(50), None, 50), ("k16", None, 16, 16)):
            with_recipe = float(rows_n) * about <= a.recipe_pairs
            print("%s %s: %d rows, radius %s, k %s" % (name, label, rows_n, radius, k), flush=True)

            def lists():
                """(src, idx): the pairs of the neighbourhoods, as the list calls give them."""
                if k is None:
                    rows = eng.radius_query(q_dev, radius, sort=False, want_dist=False)
                    lens = rows["offsets"][1:] - rows["offsets"][:-1]
                    return torch.repeat_interleave(torch.arange(rows_n, device=dev), lens), rows["idx"].long()
                kk = k - 1 if own else k  # (the own points: k counts the point itself)
                idx = eng.knn(queries=None if own else Q, k=kk, want_dist=False)["idx"].long()
                if own:
                    idx = torch.cat([torch.arange(rows_n, device=dev)[:, None], idx], dim=1)
                return torch.arange(rows_n, device=dev).repeat_interleave(idx.shape[1]), idx.reshape(-1)

            def recipe(dtype=torch.float32):
                src, idx = lists()
                d = (P[idx] - q_dev[src]).to(dtype)
                mom = torch.cat([torch.ones_like(d[:, :1]), d, d[:, :1] * d, d[:, 1:2] * d[:, 1:], d[:, 2:] * d[:, 2:]], dim=1)
                S = torch.zeros((rows_n, 10), dtype=dtype, device=dev).index_add_(0, src, mom)
                ln = S[:, :1].clamp(min=1)
                mean = S[:, 1:4] / ln
                mm = torch.cat([mean[:, :1] * mean, mean[:, 1:2] * mean[:, 1:], mean[:, 2:] * mean[:, 2:]], dim=1)
                cov = S[:, 4:] / ln - mm
                C = cov[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
                lam, vec = torch.linalg.eigh(C)
                return {"counts": S[:, 0], "cov": cov, "eigenvalues": lam, "normals": vec[:, :, 0], "d": d, "src": src}

            hood = {"radius": radius, "k": k, "about_within": about, "recipe_measured": with_recipe, "variants": {}}
            if with_recipe:  # the call against the lists, before anything is timed
                got = eng.local_pca(radius=radius, k=k, queries=Q, want=("counts", "cov"))
                ref = recipe(torch.float64)
                R2 = torch.zeros(rows_n, dtype=torch.float64, device=dev).index_reduce_(0, ref["src"], (ref["d"] * ref["d"]).sum(dim=1), "amax", include_self=True)
                tol = 2.0 * U * (3.0 * ref["counts"] + 12.0) * R2 + 1e-37
                share = float(((got["cov"].double() - ref["cov"]).abs().max(dim=1).values / tol).max())
                ok = bool(torch.equal(got["counts"].long(), ref["counts"].long())) and share <= 1.0
                hood["verified"] = {"inside_the_bound": ok, "worst_share_of_the_bound": share}
                print("  verified: %s, worst share of the covariance bound %.3f" % ("ok" if ok else "OUTSIDE THE BOUND", share), flush=True)
                del got, ref, R2, tol
                torch.cuda.empty_cache()
                if not ok:
                    case["neighbourhoods"][label] = hood
                    rec["cases"] = [c for c in rec["cases"] if c["case"] != name] + [case]
                    save()
                    sys.exit(1)

            variants = {
                "pca": lambda: eng.local_pca(radius=radius, k=k, queries=Q)["info"],
                "normals": lambda: eng.normals(radius=radius, k=k, queries=Q)["info"],
                "moments": lambda: eng.local_pca(radius=radius, k=k, queries=Q, want=("counts", "centroid", "cov"))["info"],
            }
            if with_recipe:
                variants["recipe"] = lambda: recipe() and {}
            if k is None:
                variants["reduce_count"] = lambda: eng.radius_reduce(radius, queries=Q, want_wsum=False)["info"]
            else:
                variants["knn"] = lambda: eng.knn(queries=Q, k=k - 1 if own else k, want_dist=True)["info"]
            wall, infos = {v: [] for v in variants}, {}
            for rep in range(a.reps + 1):
                for v, f in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    res = f()
                    e1.record()
                    e1.synchronize()
                    if rep:  # (rep 0: the warm-up)
                        wall[v].append(e0.elapsed_time(e1))
                        infos.setdefault(v, []).append(res)
                    del res
                torch.cuda.empty_cache()
            for v in variants:
                entry = {"events_ms": stats(wall[v])}
                for field in ("solve_ms", "bound_ms", "order_ms", "walk_ms", "finish_ms", "seed_ms", "total", "max_row", "degenerate_rows", "fallback_items",
                              "point_tests", "node_tests"):
                    vals = [i[field] for i in infos[v] if field in i]
                    if vals:
                        entry[field] = stats(vals) if isinstance(vals[0], float) else vals[0]
                hood["variants"][v] = entry
                e = entry["events_ms"]
                parts = "  ".join("%s %.3f" % (f[:-3], entry[f]["median"]) for f in ("bound_ms", "order_ms", "walk_ms", "finish_ms") if f in entry)
                print("  %-14s events %.3f ms (%.3f .. %.3f)  %s" % (v, e["median"], e["min"], e["max"], parts), flush=True)
            mine = hood["variants"]["pca"]["events_ms"]["median"]
            hood["ratios"] = {other + "_over_pca": hood["variants"][other]["events_ms"]["median"] / mine for other in ("recipe", "reduce_count", "knn")
                              if other in hood["variants"]}
            case["neighbourhoods"][label] = hood
            rec["cases"] = [c for c in rec["cases"] if c["case"] != name] + [case]
            save()
        del P, Q
        torch.cuda.empty_cache()
    eng.close()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
