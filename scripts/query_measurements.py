#!/usr/bin/env python3
"""Times of TrueKNN.query (queries that are not in the tree) beside the two self-solve kernels that bracket it, on one
MI355X, written to profiles/query_measurements.json.

One process, every shape warmed up first, then REPS repetitions in which the variants alternate; per variant the
median and the spread of (a) HIP events around the call and (b) the device time the call reports in info["solve_ms"],
and for queries the split: order (code + sort) = solve_ms - dominant_kernel_ms - tie_ms, traversal =
dominant_kernel_ms, lane pass = tie_ms.  1 000 seeded rows of the flagship query shape are checked against the numpy
spec (tests/query_spec.py) before anything is timed.

    python scripts/query_measurements.py [--points 10000000] [--reps 20]
"""
import argparse
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_measurements.json"))
    a = ap.parse_args()

    import torch

    import query_spec as qs
    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    n, k = a.points, 10
    r0 = datasets.start_radius(n, k)
    dev = torch.device("cuda", 0)
    P = datasets.uniform3d(n, seed=0)
    Q = np.random.default_rng(77).random((n, 3), dtype=np.float32)  # fresh points in the same cube
    eng = TrueKNN(device=0)
    eng.build(P)
    q_all = torch.from_numpy(Q).to(dev)
    q_1m = q_all[: n // 10].contiguous()

    clustered = datasets.gaussian_mixture3d(n, components=64, sigma=0.02, seed=1)
    lo, hi = clustered.min(0), clustered.max(0)
    Qc = (lo + np.random.default_rng(78).random((n, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    eng_c = TrueKNN(device=0)
    eng_c.build(clustered)
    q_c = torch.from_numpy(Qc).to(dev)
    r0_c = 0.004

    outs = {}

    def buffers(key, m, kk):
        if key not in outs:
            outs[key] = {"idx": torch.empty((m, kk), dtype=torch.int32, device=dev), "dist": torch.empty((m, kk), dtype=torch.float32, device=dev),
                         "intersections": torch.empty((m,), dtype=torch.int64, device=dev)}
        return dict(outs[key])

    variants = {
        "solve_team": lambda: eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, out=buffers("self", n, k)),
        "solve_lane": lambda: eng.solve(k, r0, kernel=_lib.KERNEL_LANE, out=buffers("self", n, k)),
        "query": lambda: eng.query(q_all, k, r0, out=buffers("q", n, k)),
        "query_exact": lambda: eng.query(q_all, k, r0, exact=True, out=buffers("q", n, k)),
        "query_1m": lambda: eng.query(q_1m, k, r0, out=buffers("q1", len(q_1m), k)),
        "query_k32": lambda: eng.query(q_all, 32, datasets.start_radius(n, 32), out=buffers("q32", n, 32)),
        "query_clustered": lambda: eng_c.query(q_c, k, r0_c, out=buffers("q", n, k)),
    }

    # spot check of the flagship query shape against the numpy spec, as bench.py --full does for its line
    r = variants["query"]()
    rows = np.sort(np.random.default_rng(79).choice(n, 1000, replace=False))
    spec = qs.query_rows(P, Q[rows], (k,), r0)[k]
    got_idx, got_dist = r["idx"][torch.from_numpy(rows).to(dev)].cpu().numpy(), r["dist"][torch.from_numpy(rows).to(dev)].cpu().numpy()
    got_isect = r["intersections"][torch.from_numpy(rows).to(dev)].cpu().numpy()
    ok = bool(np.array_equal(got_idx, spec["idx"]) and np.array_equal(got_dist.view(np.int32), spec["dist"].view(np.int32))
              and np.array_equal(got_isect, spec["intersections"]))
    print("spot check of 1000 rows against the numpy spec:", "ok" if ok else "MISMATCH", flush=True)
    if not ok:
        sys.exit(1)

    infos = {}
    for name, f in variants.items():  # warm-up of every shape
        for _ in range(2):
            infos[name] = f()["info"]
        torch.cuda.synchronize()
        print("warm", name, "%.3f ms" % infos[name]["solve_ms"], flush=True)
    wall = {name: [] for name in variants}
    device = {name: [] for name in variants}
    split = {name: {"order_ms": [], "traversal_ms": [], "lane_ms": []} for name in variants if name.startswith("query")}
    for rep in range(a.reps):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            info = f()["info"]
            e1.record()
            e1.synchronize()
            wall[name].append(e0.elapsed_time(e1))
            device[name].append(info["solve_ms"])
            if name in split:
                split[name]["traversal_ms"].append(info["dominant_kernel_ms"])
                split[name]["lane_ms"].append(info["tie_ms"])
                split[name]["order_ms"].append(info["solve_ms"] - info["dominant_kernel_ms"] - info["tie_ms"])
    rec = {"device": torch.cuda.get_device_name(0), "points": n, "k": k, "start_radius": r0, "reps": a.reps, "spot_check_rows": 1000,
           "spot_check": "ok", "source_fingerprint": _lib.source_fingerprint(), "variants": {}}
    for name in variants:
        v = {"events_ms": stats(wall[name]), "device_ms": stats(device[name]),
             "info": {key: infos[name][key] for key in ("rounds", "unfinished", "tie_rows", "node_tests", "point_tests", "total_intersections")}}
        if name in split:
            v["split"] = {key: stats(val) for key, val in split[name].items()}
            if name == "query_exact":
                v["split_note"] = "order_ms here also holds the exact pass"
        rec["variants"][name] = v
        print("%-16s events %.3f ms (%.3f .. %.3f)  device %.3f ms" % (name, v["events_ms"]["median"], v["events_ms"]["min"], v["events_ms"]["max"],
                                                                      v["device_ms"]["median"]), flush=True)
    med = {name: rec["variants"][name]["device_ms"]["median"] for name in variants}
    rec["ratios"] = {"query_over_solve_team": med["query"] / med["solve_team"], "query_over_solve_lane": med["query"] / med["solve_lane"]}
    print("query / solve_team = %.2f   query / solve_lane = %.2f" % (rec["ratios"]["query_over_solve_team"], rec["ratios"]["query_over_solve_lane"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
