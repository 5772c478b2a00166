#!/usr/bin/env python3
"""Times of TrueKNN.dbscan_query (cluster labels for points that are not in the tree) on BASELINE config 3's set -- 10 M
points of a 64-component Gaussian mixture, eps 0.01, minPts 4, clustered once -- beside the two walks of the in-set calls
that bracket it, on one MI355X, written to profiles/dbscan_query_measurements.json.

Query sets: 10 M and 1 M points drawn from the same mixture with another seed, and Q = P.  Each with and without counts:
3 warm-up calls, then REPS timed ones; the times are the HIP-event times the call reports (solve_ms: the whole call with the
ordering of the queries; label_ms: the traversal kernel alone).  Yardsticks, same process: tknnDbscanAssign's label_ms (the
same label walk for the points of the set that are not core) and tknnDbscan(want_counts)'s core_ms (the same counted walk).
Before anything is timed, Q = P must give tknnDbscan's labels and counts for every row, and 64 seeded foreign queries are
checked against the numpy spec (tests/dbscan_query_spec.py).

    python scripts/dbscan_query_measurements.py [--points 10000000] [--reps 20] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "p10": float(np.percentile(v, 10)),
            "p90": float(np.percentile(v, 90)), "reps": int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_query_measurements.json"))
    a = ap.parse_args()

    import torch

    import dbscan_query_spec as ds
    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    n, eps, min_pts = a.points, float(np.float32(0.01)), 4
    mix = dict(components=64, sigma=0.02, seed=1)
    dev = torch.device("cuda", 0)
    P = datasets.gaussian_mixture3d(n, **mix)
    Q = ds.mixture_draw(n, mix["components"], mix["sigma"], mix["seed"], 1234)
    eng = TrueKNN(device=0)
    eng.build(P)
    p_dev, q_dev = torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev)
    q_1m = q_dev[: n // 10].contiguous()

    full = eng.dbscan(eps, min_pts, want_counts=True)
    core_label = torch.where(full["core"], full["labels"], torch.full_like(full["labels"], -1)).contiguous()
    print("clustered: %d clusters, %d core points of %d" % (full["info"]["clusters"], int(full["core"].sum()), n), flush=True)

    r = eng.dbscan_query(p_dev, eps, core_label, want_counts=True)
    same = bool(torch.equal(r["labels"], full["labels"]) and torch.equal(r["counts"], full["counts"]))
    print("Q = P against tknnDbscan, every row:", "ok" if same else "MISMATCH", flush=True)
    rows = np.sort(np.random.default_rng(79).choice(n, 64, replace=False))
    r = eng.dbscan_query(q_dev, eps, core_label, want_counts=True)
    want_labels, want_counts = ds.query_labels(P, core_label.cpu().numpy(), eps, Q[rows], block=4)
    pick = torch.from_numpy(rows).to(dev)
    spot = bool(np.array_equal(r["labels"][pick].cpu().numpy(), want_labels) and np.array_equal(r["counts"][pick].cpu().numpy(), want_counts))
    print("spot check of 64 foreign queries against the numpy spec:", "ok" if spot else "MISMATCH", flush=True)
    if not (same and spot):
        sys.exit(1)

    # the in-set yardsticks through the C-ABI (the Python front end of the assign step returns no info)
    lib = eng._lib
    assign_out = torch.empty((n,), dtype=torch.int32, device=dev)

    def assign():
        info = _lib.DbscanInfo()
        _lib.check(lib.tknnDbscanAssign(eng._h, ctypes.c_float(eps), ctypes.c_void_p(core_label.data_ptr()), ctypes.c_void_p(assign_out.data_ptr()),
                                        ctypes.byref(info), eng._stream()))
        return info.as_dict()

    variants = {
        "assign": assign,
        "dbscan_counts": lambda: eng.dbscan(eps, min_pts, want_counts=True)["info"],
        "query_10m": lambda: eng.dbscan_query(q_dev, eps, core_label)["info"],
        "query_10m_counts": lambda: eng.dbscan_query(q_dev, eps, core_label, want_counts=True)["info"],
        "query_1m": lambda: eng.dbscan_query(q_1m, eps, core_label)["info"],
        "query_1m_counts": lambda: eng.dbscan_query(q_1m, eps, core_label, want_counts=True)["info"],
        "query_set": lambda: eng.dbscan_query(p_dev, eps, core_label)["info"],
        "query_set_counts": lambda: eng.dbscan_query(p_dev, eps, core_label, want_counts=True)["info"],
    }
    keys = ("solve_ms", "label_ms", "core_ms")
    rec = {"device": torch.cuda.get_device_name(0), "points": n, "eps": eps, "min_pts": min_pts, "mixture": mix, "reps": a.reps, "warmups": 3,
           "clusters": full["info"]["clusters"], "core_points": int(full["core"].sum()), "checks": "ok",
           "source_fingerprint": _lib.source_fingerprint(), "variants": {}}
    for name, f in variants.items():
        for _ in range(3):
            info = f()
        torch.cuda.synchronize()
        times = {key: [] for key in keys}
        for _ in range(a.reps):
            info = f()
            for key in keys:
                times[key].append(info[key])
        v = {key: stats(times[key]) for key in keys if name == "dbscan_counts" or key != "core_ms"}
        v["node_tests"], v["point_tests"] = int(info["node_tests"]), int(info["point_tests"])
        if name == "dbscan_counts":
            v["core_point_tests"] = int(info["core_point_tests"])
        rec["variants"][name] = v
        print("%-18s solve %.3f ms  label %.3f ms%s  node tests %d  point tests %d" % (
            name, v["solve_ms"]["median"], v["label_ms"]["median"], "  core %.3f ms" % v["core_ms"]["median"] if "core_ms" in v else "",
            v["node_tests"], v["point_tests"]), flush=True)
    V = rec["variants"]
    med = lambda name, key: V[name][key]["median"]  # noqa: E731
    rec["ratios"] = {
        # the same tree work as assign's walk for every point of the set (assign walks for the points that are not core only)
        "query_set_label_over_assign_label": med("query_set", "label_ms") / med("assign", "label_ms"),
        "query_set_solve_over_assign_solve": med("query_set", "solve_ms") / med("assign", "solve_ms"),
        "query_set_order_ms": med("query_set", "solve_ms") - med("query_set", "label_ms"),
        "query_set_node_tests_over_assign": V["query_set"]["node_tests"] / max(1, V["assign"]["node_tests"]),
        "query_set_point_tests_over_assign": V["query_set"]["point_tests"] / max(1, V["assign"]["point_tests"]),
        "counted_walk_ms_set": med("query_set_counts", "label_ms") - med("query_set", "label_ms"),
        "counted_walk_over_dbscan_core_ms": (med("query_set_counts", "label_ms") - med("query_set", "label_ms")) / med("dbscan_counts", "core_ms"),
    }
    for key, val in rec["ratios"].items():
        print("%-40s %.3f" % (key, val))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
