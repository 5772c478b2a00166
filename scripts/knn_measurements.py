#!/usr/bin/env python3
"""Times of tknnKnn (exact k nearest, no radius from the caller) beside the existing spellings of the same question, on one MI355X,
written to profiles/knn_measurements.json.

The 10 M uniform set, 1 M external queries and the 10 M rows of the set's own points, k = 10 and 32.  Per (mode, k), in one run:
  knn               tknnKnn: solve_ms, order_ms, seed_ms, walk_ms, point tests per query (walk and seeds), tightened rows, lane rows
  radius_knn_cover  (a) tknnRadiusKnn at radius 2, which covers the unit cube: the only radius-free spelling before tknnKnn
                    (own points: the set as its own queries, every point skipped in its own row)
  query_exact       (b) external queries: tknnQuery with exact = 1 from bench.py's start radius
  solve_repair      (c) own points: solve(TEAM) + repair_exact from bench.py's start radius
Per variant 1 warm-up, then --reps timed calls, the variants alternating call by call; median, minimum and maximum of the time
between two HIP events around the call, and of the device time the call reports where it reports one.  Before anything is timed,
200 seeded rows of each tknnKnn result are checked against brute force (tests/knn_spec.py over the grid cells around the query,
which hold the row: the check asserts that the k-th distance stays inside them), and the other variants' rows are compared with
tknnKnn's on the device.  `faster_than_radius_knn_by_more_than_the_spread`: tknnKnn's slowest call is faster than (a)'s fastest.

    python scripts/knn_measurements.py [--points 10000000] [--queries 1000000] [--reps 3]
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

CELL = 0.02  # 10 M uniform points: some 2 000 points in the 27 cells around a query


class Cells:
    """The points of the unit cube by grid cell, for brute force over a query's neighbourhood."""

    def __init__(self, P):
        self.P = P
        self.g = int(np.ceil(1.0 / CELL)) + 2
        ijk = np.clip(np.floor(P / CELL).astype(np.int64) + 1, 0, self.g - 1)
        key = (ijk[:, 0] * self.g + ijk[:, 1]) * self.g + ijk[:, 2]
        self.order = np.argsort(key, kind="stable")
        self.key = key[self.order]

    def around(self, q):
        c = np.clip(np.floor(q / CELL).astype(np.int64) + 1, 0, self.g - 1)
        cand = []
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                lo = ((c[0] + dx) * self.g + c[1] + dy) * self.g + c[2] - 1
                a, b = np.searchsorted(self.key, lo), np.searchsorted(self.key, lo + 3)
                cand.append(self.order[a:b])
        return np.sort(np.concatenate(cand))


def spot_check(cells, Q, rows, k, skip, idx, dist, counts):
    """Rows `rows` of a result against brute force over the cells around each query; every point outside them is farther than CELL."""
    import knn_spec as kn

    for t, j in enumerate(rows):
        cand = cells.around(Q[j])
        want = kn.knn_rows(cells.P[cand], Q[j:j + 1], k, skip=None if skip is None else [skip[j]], ids=cand)
        assert want["counts"][0] == k and want["dist"][0, k - 1] < CELL, "the neighbourhood does not hold the row"
        if not (np.array_equal(idx[t], want["idx"][0]) and np.array_equal(dist[t].view(np.int32), want["dist"][0].view(np.int32)) and counts[t] == k):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--ks", default="10,32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    n, m_ext = a.points, a.queries
    dev = torch.device("cuda", 0)
    P = datasets.uniform3d(n, seed=0)
    Qh = np.random.default_rng(77).random((m_ext, 3), dtype=np.float32)  # fresh points in the same cube
    cells = Cells(P)
    eng = TrueKNN(device=0)
    eng.build(P)
    p_dev, q_dev = torch.from_numpy(P).to(dev), torch.from_numpy(Qh).to(dev)
    own_ids = torch.arange(n, dtype=torch.int32, device=dev)
    rec = {"device": torch.cuda.get_device_name(0), "points": n, "reps": a.reps, "warmups": 1, "spot_check_rows": 200, "spot_check": "ok",
           "cover_radius": 2.0, "source_fingerprint": _lib.source_fingerprint(), "cases": []}
    rng = np.random.default_rng(81)

    for mode, m, Q in (("external", m_ext, Qh), ("own points", n, P)):
        for k in [int(v) for v in a.ks.split(",")]:
            r0 = datasets.start_radius(n, k)
            if mode == "external":
                variants = {"knn": lambda: eng.knn(q_dev, k),
                            "radius_knn_cover": lambda: eng.radius_knn(q_dev, k, radius=2.0),
                            "query_exact": lambda: eng.query(q_dev, k, r0, exact=True)}
            else:
                def solve_repair():
                    res = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, want_levels=True)
                    res["repaired"] = eng.repair_exact(res, k, r0)
                    return res

                variants = {"knn": lambda: eng.knn(k=k),
                            "radius_knn_cover": lambda: eng.radius_knn(p_dev, k, radius=2.0, skip_ids=own_ids),
                            "solve_repair": solve_repair}
            # warm-up: the results are checked
            first = {v: f() for v, f in variants.items()}
            got = first["knn"]
            rows = np.sort(rng.choice(m, 200, replace=False))
            sel = torch.from_numpy(rows).to(dev)
            ok = spot_check(cells, Q, rows, k, None if mode == "external" else np.arange(n), got["idx"][sel].cpu().numpy(),
                            got["dist"][sel].cpu().numpy(), got["counts"][sel].cpu().numpy())
            print("%s m=%d k=%d: spot check of 200 rows %s" % (mode, m, k, "ok" if ok else "MISMATCH"), flush=True)
            if not ok:
                rec["spot_check"] = "MISMATCH"
                sys.exit(1)
            info = got["info"]
            case = {"mode": mode, "m": m, "k": k, "start_radius": r0, "full_rows": info["full_rows"], "lane_rows": info["lane_rows"],
                    "tightened_rows": info["tightened_rows"], "tightened_share": info["tightened_rows"] / m,
                    "point_tests_per_query": {"knn_walk": info["point_tests"] / m, "knn_seeds": info["seed_point_tests"] / m},
                    "node_tests_per_query": {"knn": info["node_tests"] / m}, "rows_equal_to_knn": {}, "variants": {}}
            for v, res in first.items():
                if v != "knn":
                    same = (res["idx"] == got["idx"]).all(dim=1) & (res["dist"].view(torch.int32) == got["dist"].view(torch.int32)).all(dim=1)
                    case["rows_equal_to_knn"][v] = float(same.float().mean())
                    case["point_tests_per_query"][v] = res["info"]["point_tests"] / m
                    case["node_tests_per_query"][v] = res["info"]["node_tests"] / m
            del first, got, res
            torch.cuda.empty_cache()
            wall, device, last = {v: [] for v in variants}, {v: [] for v in variants}, {}
            for _ in range(a.reps):
                for v, f in variants.items():  # alternating
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    res = f()
                    e1.record()
                    e1.synchronize()
                    wall[v].append(e0.elapsed_time(e1))
                    device[v].append(res["info"]["solve_ms"])
                    last[v] = dict(res["info"], **({"repaired": res["repaired"]} if "repaired" in res else {}))
                    del res
            keep = ("walk_ms", "order_ms", "seed_ms", "dominant_kernel_ms", "rounds", "repaired", "lane_rows")
            for v in variants:
                case["variants"][v] = {"events_ms": stats(wall[v]), "info": {key: last[v][key] for key in keep if key in last[v]}}
                if v != "solve_repair":  # (tknnRepairExact reports no time: the pair is timed by the events alone)
                    case["variants"][v]["device_ms"] = stats(device[v])
                print("  %-18s events %.3f ms (%.3f .. %.3f)  device %.3f ms" % (v, np.median(wall[v]), min(wall[v]), max(wall[v]), np.median(device[v])), flush=True)
            mine = case["variants"]["knn"]["events_ms"]
            for v in variants:
                if v != "knn":
                    case["variants"][v]["ratio_to_knn"] = case["variants"][v]["events_ms"]["median"] / mine["median"]
            case["faster_than_radius_knn_by_more_than_the_spread"] = bool(mine["max"] < case["variants"]["radius_knn_cover"]["events_ms"]["min"])
            rec["cases"].append(case)
            del variants
            torch.cuda.empty_cache()
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
                json.dump(rec, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
