#!/usr/bin/env python3
"""Times of tknnPeriodicKnn (k nearest in a periodic cell) on one MI355X, written to profiles/periodic_knn_measurements.json.

Uniform points in the unit cell, all three axes periodic, external queries, no radius.
  (a) 10 M points, 1 M queries, k = 10 and 32: tknnPeriodicKnn beside the unchanged tknnKnn on the same inputs.  tknnKnn answers
      the OPEN question, so it is the cost floor: the ratio and the extra node tests and point tests per query are recorded, there
      is no threshold.
  (b) 1 M points, 1 M queries, k = 10: tknnPeriodicKnn beside the workaround it replaces -- a tknnBuild over the 27 shifted copies
      of the set and tknnKnn on that tree (indices taken modulo n) --, the query alone and build + query.  The condition:
      tknnPeriodicKnn's slowest timed call is faster than the fastest build + query of the workaround
      (`faster_than_build_plus_query_by_more_than_the_spread`); the query alone is recorded without a condition.
One process, the variants alternating call by call, 1 warm-up and --reps timed calls, the time between two HIP events around
the call: median with minimum and maximum.  Before anything is timed, 200 seeded rows of every tknnPeriodicKnn result are checked
against tests/periodic_spec.py over the 27 grid cells around the query, the cells across the faces included (the check asserts
that the k-th distance stays inside them).

    python scripts/periodic_knn_measurements.py [--points 10000000] [--queries 1000000] [--copies-points 1000000] [--reps 3]
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

LO, PERIOD = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


class PeriodicCells:
    """The points of the unit cell by grid cell, for brute force over a query's neighbourhood, around the faces too."""

    def __init__(self, P, cell):
        self.P, self.g = P, int(round(1.0 / cell))
        self.cell = 1.0 / self.g
        ijk = np.clip(np.floor(P / self.cell).astype(np.int64), 0, self.g - 1)
        key = (ijk[:, 0] * self.g + ijk[:, 1]) * self.g + ijk[:, 2]
        self.order = np.argsort(key, kind="stable")
        self.key = key[self.order]

    def around(self, q):
        c = np.clip(np.floor(q / self.cell).astype(np.int64), 0, self.g - 1)
        cand = []
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    key = (((c[0] + dx) % self.g) * self.g + (c[1] + dy) % self.g) * self.g + (c[2] + dz) % self.g
                    a, b = np.searchsorted(self.key, key), np.searchsorted(self.key, key + 1)
                    cand.append(self.order[a:b])
        return np.sort(np.concatenate(cand))


def spot_check(cells, Q, rows, k, idx, dist, counts):
    """Rows `rows` of a result against the spec over the cells around each query; every point outside them is farther than a cell."""
    import periodic_spec as ps

    for t, j in enumerate(rows):
        cand = cells.around(Q[j])
        want = ps.knn_rows(cells.P[cand], Q[j:j + 1], k, LO, PERIOD, ids=cand)
        assert want["counts"][0] == k and want["dist"][0, k - 1] < cells.cell, "the neighbourhood does not hold the row"
        if not (np.array_equal(idx[t], want["idx"][0]) and np.array_equal(dist[t].view(np.int32), want["dist"][0].view(np.int32)) and counts[t] == k):
            return False
    return True


def timed(variants, reps):
    """{variant: [ms per call]}: the variants alternating call by call, HIP events around each call; and the last info of each."""
    import torch

    wall, last = {v: [] for v in variants}, {}
    for _ in range(reps):
        for v, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = f()
            e1.record()
            e1.synchronize()
            wall[v].append(e0.elapsed_time(e1))
            last[v] = res["info"]
            del res
    return wall, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--copies-points", type=int, default=1_000_000)
    ap.add_argument("--ks", default="10,32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic_knn_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    m = a.queries
    Qh = np.random.default_rng(77).random((m, 3), dtype=np.float32)
    q_dev = torch.from_numpy(Qh).to(dev)
    rec = {"device": torch.cuda.get_device_name(0), "queries": m, "reps": a.reps, "warmups": 1, "spot_check_rows": 200, "spot_check": "ok",
           "cell": {"lo": LO, "period": PERIOD}, "source_fingerprint": _lib.source_fingerprint(), "cases": []}
    rng = np.random.default_rng(81)

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    def checked(cells, got, k, what):
        rows = np.sort(rng.choice(m, 200, replace=False))
        sel = torch.from_numpy(rows).to(dev)
        ok = spot_check(cells, Qh, rows, k, got["idx"][sel].cpu().numpy(), got["dist"][sel].cpu().numpy(), got["counts"][sel].cpu().numpy())
        print("%s k=%d: spot check of 200 rows %s" % (what, k, "ok" if ok else "MISMATCH"), flush=True)
        if not ok:
            rec["spot_check"] = "MISMATCH"
            save()
            sys.exit(1)

    def summary(wall, last, variants):
        out = {}
        for v in variants:
            keep = ("solve_ms", "walk_ms", "order_ms", "seed_ms", "lane_rows", "build_ms")
            out[v] = {"events_ms": stats(wall[v]), "info": {key: last[v][key] for key in keep if key in last[v]}}
            print("  %-20s events %.3f ms (%.3f .. %.3f)" % (v, np.median(wall[v]), min(wall[v]), max(wall[v])), flush=True)
        return out

    # ---- (a) beside tknnKnn, the open question ----
    n = a.points
    P = datasets.uniform3d(n, seed=0)
    cells = PeriodicCells(P, 0.02 if n >= 5_000_000 else 0.04)
    eng = TrueKNN(device=0)
    eng.build(P)
    for k in [int(v) for v in a.ks.split(",")]:
        variants = {"periodic_knn": lambda: eng.periodic_knn(q_dev, k, lo=LO, period=PERIOD), "knn": lambda: eng.knn(q_dev, k)}
        first = {v: f() for v, f in variants.items()}
        got, open_rows = first["periodic_knn"], first["knn"]
        checked(cells, got, k, "(a) n=%d m=%d" % (n, m))
        same = (open_rows["idx"] == got["idx"]).all(dim=1) & (open_rows["dist"].view(torch.int32) == got["dist"].view(torch.int32)).all(dim=1)
        pi, oi = got["info"], open_rows["info"]
        case = {"setup": "a", "points": n, "m": m, "k": k, "full_rows": pi["full_rows"], "lane_rows": pi["lane_rows"],
                "tightened_share": pi["tightened_rows"] / m, "rows_equal_to_the_open_rows": float(same.float().mean()),
                "point_tests_per_query": {"periodic_knn": pi["point_tests"] / m, "knn": oi["point_tests"] / m,
                                          "extra": (pi["point_tests"] - oi["point_tests"]) / m, "seeds": pi["seed_point_tests"] / m},
                "node_tests_per_query": {"periodic_knn": pi["node_tests"] / m, "knn": oi["node_tests"] / m, "extra": (pi["node_tests"] - oi["node_tests"]) / m}}
        del first, got, open_rows, same
        torch.cuda.empty_cache()
        wall, last = timed(variants, a.reps)
        case["variants"] = summary(wall, last, variants)
        case["ratio_to_knn"] = case["variants"]["periodic_knn"]["events_ms"]["median"] / case["variants"]["knn"]["events_ms"]["median"]
        rec["cases"].append(case)
        save()
    eng.close()
    del eng, cells, P
    torch.cuda.empty_cache()

    # ---- (b) beside the tree over 27 shifted copies ----
    n, k = a.copies_points, 10
    P = datasets.uniform3d(n, seed=1)
    cells = PeriodicCells(P, 0.04)
    shifts = np.float32([[x, y, z] for x in (0, -1, 1) for y in (0, -1, 1) for z in (0, -1, 1)])
    copies_dev = torch.from_numpy(np.concatenate([P + s for s in shifts]).astype(np.float32)).to(dev)  # copy c of point i: row c * n + i
    eng, eng27 = TrueKNN(device=0), TrueKNN(device=0)
    eng.build(P)
    eng27.build(copies_dev)

    def build_and_query():
        eng27.build(copies_dev)
        res = eng27.knn(q_dev, k)
        res["info"] = dict(res["info"], build_ms=eng27.build_info["build_ms"])
        return res

    variants = {"periodic_knn": lambda: eng.periodic_knn(q_dev, k, lo=LO, period=PERIOD), "copies_query": lambda: eng27.knn(q_dev, k),
                "copies_build_query": build_and_query}
    first = {v: f() for v, f in variants.items()}
    got = first["periodic_knn"]
    checked(cells, got, k, "(b) n=%d m=%d" % (n, m))
    same = (first["copies_query"]["idx"] % n == got["idx"]).all(dim=1)  # (the copies' distances round differently: indices only)
    case = {"setup": "b", "points": n, "copies_points": 27 * n, "m": m, "k": k, "lane_rows": got["info"]["lane_rows"],
            "rows_with_the_copies_indices": float(same.float().mean()),
            "point_tests_per_query": {"periodic_knn": got["info"]["point_tests"] / m, "copies_query": first["copies_query"]["info"]["point_tests"] / m}}
    del first, got, same
    torch.cuda.empty_cache()
    wall, last = timed(variants, a.reps)
    case["variants"] = summary(wall, last, variants)
    mine = case["variants"]["periodic_knn"]["events_ms"]
    for v in ("copies_query", "copies_build_query"):
        case["variants"][v]["ratio_to_periodic_knn"] = case["variants"][v]["events_ms"]["median"] / mine["median"]
    case["faster_than_build_plus_query_by_more_than_the_spread"] = bool(mine["max"] < case["variants"]["copies_build_query"]["events_ms"]["min"])
    case["faster_than_the_query_alone_by_more_than_the_spread"] = bool(mine["max"] < case["variants"]["copies_query"]["events_ms"]["min"])
    rec["cases"].append(case)
    save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
