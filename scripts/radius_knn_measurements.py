#!/usr/bin/env python3
"""Times of tknnRadiusKnn (at most k nearest within a radius) beside the two workarounds it replaces, on one MI355X, written to
profiles/radius_knn_measurements.json.

The 10 M uniform set, 1 M and 10 M external queries, k = 10 and 32, and per k three radii: mean row length about k / 2, 4 k and
100 k.  Per (queries, k, radius), in the same run:
  radius_knn        tknnRadiusKnn: solve_ms and walk_ms, point tests per query, lane_rows
  radius_query      tknnRadiusQuery, count pass + fill pass with sort = 1 (the rows would then be truncated to k); left out, and
                    said so, where the rows do not fit one call (2^31 entries) or --max-entries
  query_exact       tknnQuery with exact = 1, started at that radius (its rows would then be cut at r)
Per variant 1 warm-up, then the median and the spread of --reps timed calls, by HIP events around the call and by the device time
the call reports.  Before anything is timed, 200 seeded rows of each tknnRadiusKnn result are checked against brute force over the
grid cells around the query (tests/radius_knn_spec.py).  Also recorded: the point-test ratio of the everything-in-reach case of
tests/test_radius_knn_gpu.py.

    python scripts/radius_knn_measurements.py [--points 10000000] [--queries 1000000,10000000] [--reps 3]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from radius_measurements import spot_rows, stats  # noqa: E402


def radius_for(mean_row, n):
    """The radius at which a query inside the unit cube has `mean_row` of n uniform points in reach on average."""
    return float(np.float32((mean_row / (n * 4.0 / 3.0 * np.pi)) ** (1.0 / 3.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--queries", default="1000000,10000000")
    ap.add_argument("--ks", default="10,32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-entries", type=int, default=1_500_000_000, help="largest tknnRadiusQuery result timed (its keys are sorted out of place)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_knn_measurements.json"))
    a = ap.parse_args()

    import torch

    import radius_knn_spec as ks
    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    n = a.points
    dev = torch.device("cuda", 0)
    P = datasets.uniform3d(n, seed=0)
    eng = TrueKNN(device=0)
    eng.build(P)
    lib = eng._lib
    rec = {"device": torch.cuda.get_device_name(0), "points": n, "reps": a.reps, "warmups": 1, "spot_check_rows": 200, "spot_check": "ok",
           "source_fingerprint": _lib.source_fingerprint(), "cases": []}

    # the point-test ratio of the everything-in-reach test (4 096 points, 256 queries, r = 4, k = 10)
    small = TrueKNN(device=0)
    sp, sq = ks.uniform_case()
    small.build(sp)
    mine, fill = small.radius_knn(sq, 10, radius=4.0)["info"], small.radius_query(sq, 4.0)["info"]
    rec["everything_in_reach"] = {"radius_knn_point_tests": mine["point_tests"], "radius_query_fill_point_tests": fill["point_tests"],
                                  "ratio": mine["point_tests"] / fill["point_tests"]}
    print("everything in reach: point tests %d against %d" % (mine["point_tests"], fill["point_tests"]), flush=True)
    small.close()

    rng = np.random.default_rng(81)
    for m in [int(v) for v in a.queries.split(",")]:
        Qh = np.random.default_rng(77).random((m, 3), dtype=np.float32)  # fresh points in the same cube
        q = torch.from_numpy(Qh).to(dev)
        for k in [int(v) for v in a.ks.split(",")]:
            idx = torch.empty((m, k), dtype=torch.int32, device=dev)
            dist = torch.empty((m, k), dtype=torch.float32, device=dev)
            counts = torch.empty((m,), dtype=torch.int32, device=dev)
            for label, mean_row in (("k/2", k / 2), ("4k", 4 * k), ("100k", 100 * k)):
                r = radius_for(mean_row, n)

                def knn_call():
                    o, info = _lib.RadiusKnnOptions(), _lib.RadiusKnnInfo()
                    o.d_queries, o.m, o.k, o.radius = q.data_ptr(), m, k, r
                    o.d_idx, o.d_dist, o.d_counts = idx.data_ptr(), dist.data_ptr(), counts.data_ptr()
                    _lib.check(lib.tknnRadiusKnn(eng._h, ctypes.byref(o), ctypes.byref(info), None))
                    return info.as_dict()

                info = knn_call()
                rows = np.sort(rng.choice(m, 200, replace=False))
                hi, hd, hc = idx[rows].cpu().numpy(), dist[rows].cpu().numpy(), counts[rows].cpu().numpy()
                ok = True
                for t, full in enumerate(spot_rows(P, Qh, rows, r)):
                    want = ks.cut_rows(full, k)
                    ok &= bool(np.array_equal(hi[t], want["idx"][0]) and np.array_equal(hd[t].view(np.int32), want["dist"][0].view(np.int32)) and hc[t] == want["counts"][0])
                print("m=%d k=%d r=%s (%.5f): spot check of 200 rows %s" % (m, k, label, r, "ok" if ok else "MISMATCH"), flush=True)
                if not ok:
                    sys.exit(1)
                case = {"m": m, "k": k, "radius_label": label, "radius": r, "mean_row_wanted": mean_row, "mean_count": info["total"] / m,
                        "full_rows": info["full_rows"], "lane_rows": info["lane_rows"], "point_tests_per_query": info["point_tests"] / m,
                        "node_tests_per_query": info["node_tests"] / m, "variants": {}}
                variants = {"radius_knn": knn_call}

                # workaround 1: count + fill with sort = 1
                offsets = torch.empty((m + 1,), dtype=torch.int64, device=dev)
                o, cinfo = _lib.RadiusOptions(), _lib.RadiusInfo()
                o.d_queries, o.m, o.radius, o.sort, o.d_offsets = q.data_ptr(), m, r, 1, offsets.data_ptr()
                rc = lib.tknnRadiusQuery(eng._h, ctypes.byref(o), ctypes.byref(cinfo), None)
                total = int(cinfo.total)
                case["radius_query_total"] = total
                case["radius_query_point_tests_per_query_count_pass"] = cinfo.point_tests / m
                if rc != 0 or total > a.max_entries:
                    case["radius_query_left_out"] = "2^31 or more entries: not served in one call" if rc != 0 else "more than --max-entries entries"
                else:
                    fidx = torch.empty((total,), dtype=torch.int32, device=dev)
                    fdist = torch.empty((total,), dtype=torch.float32, device=dev)

                    def radius_query_call():
                        o, ci, fi = _lib.RadiusOptions(), _lib.RadiusInfo(), _lib.RadiusInfo()
                        o.d_queries, o.m, o.radius, o.sort, o.d_offsets = q.data_ptr(), m, r, 1, offsets.data_ptr()
                        _lib.check(lib.tknnRadiusQuery(eng._h, ctypes.byref(o), ctypes.byref(ci), None))
                        o.d_idx, o.d_dist, o.capacity = fidx.data_ptr(), fdist.data_ptr(), total
                        _lib.check(lib.tknnRadiusQuery(eng._h, ctypes.byref(o), ctypes.byref(fi), None))
                        return {"solve_ms": ci.solve_ms + fi.solve_ms, "walk_ms": ci.walk_ms + fi.walk_ms, "sort_ms": fi.sort_ms,
                                "point_tests": ci.point_tests + fi.point_tests}

                    variants["radius_query_count_fill_sort"] = radius_query_call

                # workaround 2: the exact k nearest, the doubling started at r
                kout = {"idx": torch.empty((m, k), dtype=torch.int32, device=dev), "dist": torch.empty((m, k), dtype=torch.float32, device=dev)}
                variants["query_exact"] = lambda: eng.query(q, k, r, exact=True, out=dict(kout))["info"]

                for v, f in variants.items():
                    last = f()
                    wall, device = [], []
                    for _ in range(a.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        last = f()
                        e1.record()
                        e1.synchronize()
                        wall.append(e0.elapsed_time(e1))
                        device.append(last["solve_ms"])
                    keep = ("walk_ms", "order_ms", "sort_ms", "point_tests", "node_tests", "dominant_kernel_ms")
                    case["variants"][v] = {"events_ms": stats(wall), "device_ms": stats(device), "info": {key: last[key] for key in keep if key in last}}
                    print("  %-30s events %.3f ms (%.3f .. %.3f)  device %.3f ms" % (v, np.median(wall), min(wall), max(wall), np.median(device)), flush=True)
                rec["cases"].append(case)
                del variants
                if "fidx" in locals():
                    del fidx, fdist
                torch.cuda.empty_cache()
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
                    json.dump(rec, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
