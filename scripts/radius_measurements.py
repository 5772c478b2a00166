#!/usr/bin/env python3
"""Times of tknnRadiusQuery (fixed-radius neighbour lists) beside the two calls that bracket it, on one MI355X, written to
profiles/radius_measurements.json.

The 10 M uniform set and r = 0.0062 (about ten neighbours per point), for Q = P and for 1 M external queries: the count pass,
the fill pass with sort = 0 and the fill pass with sort = 1, and in the same run tknnDbscanQuery with counts on the same queries
and eps (its counted walk answers the count pass's question; no point is core, so its label walk does not run) and tknnQuery
at k = 10.  Per variant 2 warm-ups, then the median and the spread of REPS timed calls: (a) HIP events around the call and (b)
the device time the call reports.  2 000 seeded rows are checked against the numpy spec (tests/radius_spec.py, the candidates
of a row proposed by a grid of cells wider than r) before anything is timed.

    python scripts/radius_measurements.py [--points 10000000] [--reps 5]
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
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "reps": int(len(v))}


def spot_rows(P, Q, rows, r):
    """The spec's rows of the queries Q[rows]: radius_rows over the points of the 27 grid cells around each query."""
    import radius_spec as rs

    cell = max(2.0 * float(r), 0.01)
    g = int(np.ceil(1.0 / cell)) + 2
    ijk = np.clip(np.floor(P / cell).astype(np.int64) + 1, 0, g - 1)
    key = (ijk[:, 0] * g + ijk[:, 1]) * g + ijk[:, 2]
    order = np.argsort(key, kind="stable")
    key = key[order]
    out = []
    for j in rows:
        c = np.clip(np.floor(Q[j] / cell).astype(np.int64) + 1, 0, g - 1)
        cand = []
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                lo = ((c[0] + dx) * g + c[1] + dy) * g + c[2] - 1
                a, b = np.searchsorted(key, lo), np.searchsorted(key, lo + 3)
                cand.append(order[a:b])
        cand = np.sort(np.concatenate(cand))
        out.append(rs.radius_rows(P[cand], Q[j:j + 1], r, ids=cand))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--radius", type=float, default=0.0062)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    n, r, k = a.points, float(np.float32(a.radius)), 10
    dev = torch.device("cuda", 0)
    P = datasets.uniform3d(n, seed=0)
    Qx = np.random.default_rng(77).random((n // 10, 3), dtype=np.float32)  # fresh points in the same cube
    eng = TrueKNN(device=0)
    eng.build(P)
    lib, stream = eng._lib, None
    queries = {"self": torch.from_numpy(P).to(dev), "ext": torch.from_numpy(Qx).to(dev)}
    no_core = torch.full((n,), -1, dtype=torch.int32, device=dev)

    # spot check: 1 000 rows of each query set against the spec
    rng = np.random.default_rng(79)
    for name, host in (("self", P), ("ext", Qx)):
        got = eng.radius_query(queries[name], r)
        off, idx, dist = got["offsets"].cpu().numpy(), got["idx"].cpu().numpy(), got["dist"].cpu().numpy()
        rows = np.sort(rng.choice(len(host), 1000, replace=False))
        ok = True
        for j, want in zip(rows, spot_rows(P, host, rows, r)):
            ok &= bool(np.array_equal(idx[off[j]:off[j + 1]], want["idx"]) and np.array_equal(dist[off[j]:off[j + 1]].view(np.int32), want["dist"].view(np.int32)))
        print("spot check of 1000 rows (%s) against the numpy spec:" % name, "ok" if ok else "MISMATCH", flush=True)
        if not ok:
            sys.exit(1)
        del got, off, idx, dist

    state = {}
    for name, q in queries.items():
        m = int(q.shape[0])
        offsets = torch.empty((m + 1,), dtype=torch.int64, device=dev)
        o, info = _lib.RadiusOptions(), _lib.RadiusInfo()
        o.d_queries, o.m, o.radius, o.sort, o.d_offsets = q.data_ptr(), m, r, 1, offsets.data_ptr()
        _lib.check(lib.tknnRadiusQuery(eng._h, ctypes.byref(o), ctypes.byref(info), stream))
        total = int(info.total)
        state[name] = {"m": m, "offsets": offsets, "total": total, "max_row": int(info.max_row),
                       "idx": torch.empty((total,), dtype=torch.int32, device=dev), "dist": torch.empty((total,), dtype=torch.float32, device=dev)}

    def radius_call(name, fill, sort):
        st = state[name]
        o, info = _lib.RadiusOptions(), _lib.RadiusInfo()
        o.d_queries, o.m, o.radius, o.sort, o.d_offsets = queries[name].data_ptr(), st["m"], r, int(sort), st["offsets"].data_ptr()
        if fill:
            o.d_idx, o.d_dist, o.capacity = st["idx"].data_ptr(), st["dist"].data_ptr(), st["total"]
        _lib.check(lib.tknnRadiusQuery(eng._h, ctypes.byref(o), ctypes.byref(info), stream))
        return info.as_dict()

    outs = {}

    def knn_out(name):
        m = state[name]["m"]
        if name not in outs:
            outs[name] = {"idx": torch.empty((m, k), dtype=torch.int32, device=dev), "dist": torch.empty((m, k), dtype=torch.float32, device=dev),
                          "intersections": torch.empty((m,), dtype=torch.int64, device=dev)}
        return dict(outs[name])

    variants = {}
    for name in queries:
        variants[name + "/count"] = lambda name=name: radius_call(name, False, 1)
        variants[name + "/fill_unsorted"] = lambda name=name: radius_call(name, True, 0)
        variants[name + "/fill_sorted"] = lambda name=name: radius_call(name, True, 1)
        variants[name + "/dbscan_query_counts"] = lambda name=name: eng.dbscan_query(queries[name], r, no_core, want_counts=True)["info"]
        variants[name + "/query_k10"] = lambda name=name: eng.query(queries[name], k, datasets.start_radius(n, k), out=knn_out(name))["info"]

    infos, wall, device = {}, {v: [] for v in variants}, {v: [] for v in variants}
    for v, f in variants.items():
        for _ in range(2):
            infos[v] = f()
        torch.cuda.synchronize()
        print("warm", v, "%.3f ms" % infos[v]["solve_ms"], flush=True)
    for rep in range(a.reps):
        for v, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            info = f()
            e1.record()
            e1.synchronize()
            wall[v].append(e0.elapsed_time(e1))
            device[v].append(info["solve_ms"])
    rec = {"device": torch.cuda.get_device_name(0), "points": n, "radius": r, "k": k, "reps": a.reps, "warmups": 2, "spot_check_rows": 2000,
           "spot_check": "ok", "source_fingerprint": _lib.source_fingerprint(),
           "rows": {name: {"m": st["m"], "total": st["total"], "max_row": st["max_row"], "mean_row": st["total"] / st["m"]} for name, st in state.items()},
           "variants": {}}
    for v in variants:
        keep = ("node_tests", "point_tests", "order_ms", "walk_ms", "sort_ms", "label_ms", "dominant_kernel_ms")
        rec["variants"][v] = {"events_ms": stats(wall[v]), "device_ms": stats(device[v]), "info": {key: infos[v][key] for key in keep if key in infos[v]}}
        e = rec["variants"][v]["events_ms"]
        print("%-28s events %.3f ms (%.3f .. %.3f)  device %.3f ms" % (v, e["median"], e["min"], e["max"], rec["variants"][v]["device_ms"]["median"]), flush=True)
    rec["count_over_dbscan_query"] = {}
    for name in queries:
        c, d = rec["variants"][name + "/count"]["events_ms"], rec["variants"][name + "/dbscan_query_counts"]["events_ms"]
        rec["count_over_dbscan_query"][name] = {"ratio": c["median"] / d["median"], "count_ms": c["median"], "dbscan_query_ms": d["median"],
                                                "spread_ms": max(c["max"] - c["min"], d["max"] - d["min"])}
        print("%s: count pass / tknnDbscanQuery with counts = %.2f" % (name, c["median"] / d["median"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
