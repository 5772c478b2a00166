#!/usr/bin/env python3
"""Times of tknnRadiusReduce (weighted neighbour sums within a radius, no lists) on one MI355X, written to
profiles/reduce_measurements.json.

The cases, all on 10 M uniform points of the unit cube with 16 value columns:
  within10, within100, within1000   1 M external uniform queries at radii with about 10, 100 and 1 000 points within r;
  own10                             the set's own 10 M points as queries, about 10 within r, with and without skip_self.
Per case the call is timed for the weights one and gauss and C = 0, 1, 3, 16 channels: --reps whole calls after 1 warm-up; median,
minimum and maximum of the HIP events around the call and of the call's own info (order_ms, stage_ms, walk_ms).  The comparison
partners run in the same process on the same tree, alternating with the call inside every repetition:
  (a) radius_query's count pass over the same queries: the floor for C = 0;
  (b) what a user has today -- radius_query with sort = 0 (count + fill), then torch: the weights from the distances, index_add_
      of w and of w * values[idx] into the rows.  Not run where the CSR would hold more than --recipe-pairs pairs.
Before anything is timed the call's outputs and the recipe's are held to the tolerance of tests/reduce_spec.py against float64 sums
over the recipe's CSR rows (the fp32 squared distances recomputed from the coordinates, the weights and the sums in float64 on the
device), and the counts to the rows' lengths, exactly.

    python scripts/reduce_measurements.py [--reps 5] [--cases within10,within100,within1000,own10] [--out profiles/reduce_measurements.json]
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

WEIGHTS = ("one", "gauss")
CHANNELS = (0, 1, 3, 16)


def radius_for(n, within):
    """The radius of a ball that holds `within` of n uniform points of the unit cube."""
    return float(np.float32((within / (n * 4.1887902)) ** (1.0 / 3.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--cases", default="within10,within100,within1000,own10")
    ap.add_argument("--recipe-pairs", type=float, default=2.5e8, help="the recipe runs where the CSR holds at most so many pairs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_measurements.json"))
    a = ap.parse_args()

    import torch

    import reduce_spec as rd
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
        with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    n, m = a.points, a.queries
    P = torch.from_numpy(np.ascontiguousarray(datasets.uniform3d(n, seed=0), np.float32)).to(dev)
    Q = torch.from_numpy(np.random.default_rng(7).random((m, 3), dtype=np.float32)).to(dev)
    V = torch.from_numpy(rd.values_for(n, seed=3)).to(dev)
    eng = TrueKNN(device=0)
    eng.build(P)

    def weights_of(weight, d2, r, h, dtype):
        if weight == "one":
            return torch.ones_like(d2, dtype=dtype)
        return torch.exp(d2.to(dtype) * float(rd.constants("gauss", r, h)))

    def recipe(queries, r, h, weight, C):
        """radius_query + torch: dict(counts, wsum, out) as the call gives them."""
        rows = eng.radius_query(queries, r, sort=False, want_dist=weight != "one")
        lens = rows["offsets"][1:] - rows["offsets"][:-1]
        src = torch.repeat_interleave(torch.arange(len(lens), device=dev), lens)
        idx = rows["idx"].long()
        w = weights_of(weight, rows["dist"] * rows["dist"], r, h, torch.float32) if weight != "one" else None
        wsum = lens.float() if w is None else torch.zeros(len(lens), device=dev).index_add_(0, src, w)
        out = None
        if C:
            v = V[:, :C][idx]
            out = torch.zeros((len(lens), C), device=dev).index_add_(0, src, v if w is None else v * w[:, None])
        return {"counts": lens.int(), "wsum": wsum, "out": out}

    def verify(queries, r, h, weight, C, got, skip_self):
        """The call's and the recipe's outputs against float64 sums over the CSR rows, inside reduce_spec's bound; (ok, worst share
        of the bound the call uses, the recipe's)."""
        q = P if queries is None else queries
        rows = eng.radius_query(q, r, sort=False, want_dist=False)
        lens = rows["offsets"][1:] - rows["offsets"][:-1]
        src = torch.repeat_interleave(torch.arange(len(lens), device=dev), lens)
        idx = rows["idx"].long()
        if skip_self:
            keep = idx != src
            src, idx = src[keep], idx[keep]
            lens = torch.zeros(len(lens), dtype=torch.int64, device=dev).index_add_(0, src, torch.ones_like(src))
        diff = P[idx] - q[src]
        x, y, z = diff[:, 0], diff[:, 1], diff[:, 2]
        d2 = ((x * x) + (y * y)) + (z * z)
        w = weights_of(weight, d2, r, h, torch.float64)
        ck, ln = rd.c_k(weight, r, h), lens.double()
        W = torch.zeros(len(lens), dtype=torch.float64, device=dev).index_add_(0, src, w)
        ok = bool(torch.equal(got["counts"].long(), lens))
        shares = {}
        for who, res in (("call", got), ("recipe", None if skip_self else recipe(queries if queries is not None else P, r, h, weight, C))):
            if res is None:
                continue
            worst = float(((res["wsum"].double() - W).abs() / (2.0 * rd.U * ((ln + 2.0) * W + ck * ln) + 1e-37)).max())
            if C:
                v = V[:, :C][idx].double()
                S = torch.zeros((len(lens), C), dtype=torch.float64, device=dev).index_add_(0, src, v * w[:, None])
                A = torch.zeros((len(lens), C), dtype=torch.float64, device=dev).index_add_(0, src, (v * w[:, None]).abs())
                Vs = torch.zeros((len(lens), C), dtype=torch.float64, device=dev).index_add_(0, src, v.abs())
                worst = max(worst, float(((res["out"].double() - S).abs() / (2.0 * rd.U * ((ln[:, None] + 2.0) * A + ck * Vs) + 1e-37)).max()))
            shares[who] = worst
            ok &= worst <= 1.0
        return ok, shares

    shapes = {"within10": (10, False), "within100": (100, False), "within1000": (1000, False), "own10": (10, True)}
    for name in a.cases.split(","):
        within, own = shapes[name]
        r = radius_for(n, within)
        h = float(rd.bandwidth(r))
        queries, rows_n = (None, n) if own else (Q, m)
        pairs = float(rows_n) * within
        with_recipe = pairs <= a.recipe_pairs
        case = {"case": name, "rows": rows_n, "radius": r, "bandwidth": h, "about_within": within, "recipe_measured": with_recipe, "verified": {}, "variants": {}}
        print("%s: %d rows, r %.5f" % (name, rows_n, r), flush=True)

        def call(weight, C, skip_self=False):
            return eng.radius_reduce(r, queries=queries, values=V[:, :C].contiguous() if C else None, weight=weight, bandwidth=h, skip_self=skip_self)

        if with_recipe:  # (the verification builds the CSR too)
            for weight in WEIGHTS:
                for C in ((3, 16) if pairs <= 2e7 else (3,)):
                    ok, shares = verify(queries, r, h, weight, C, call(weight, C), False)
                    case["verified"]["%s_c%d" % (weight, C)] = {"inside_the_bound": ok, "worst_share_of_the_bound": shares}
                    print("  verified %s C %d: %s %s" % (weight, C, "ok" if ok else "OUTSIDE THE BOUND", shares), flush=True)
                    if not ok:
                        rec["cases"] = [c for c in rec["cases"] if c["case"] != name] + [case]
                        save()
                        sys.exit(1)
            if own:
                ok, shares = verify(None, r, h, "gauss", 3, call("gauss", 3, True), True)
                case["verified"]["gauss_c3_skip_self"] = {"inside_the_bound": ok, "worst_share_of_the_bound": shares}
                if not ok:
                    sys.exit(1)
            torch.cuda.empty_cache()

        values_c = {C: (V[:, :C].contiguous() if C else None) for C in CHANNELS}
        variants = {}
        for weight in WEIGHTS:
            for C in CHANNELS:
                variants["reduce_%s_c%d" % (weight, C)] = (lambda w=weight, c=C: eng.radius_reduce(r, queries=queries, values=values_c[c], weight=w, bandwidth=h)["info"])
                if with_recipe and C in (0, 3, 16):
                    variants["recipe_%s_c%d" % (weight, C)] = (lambda w=weight, c=C: recipe(queries if queries is not None else P, r, h, w, c) and {})
        if own:
            variants["reduce_gauss_c3_skip_self"] = lambda: eng.radius_reduce(r, values=values_c[3], weight="gauss", bandwidth=h, skip_self=True)["info"]
        q_dev = P if own else Q
        offsets = torch.empty((rows_n + 1,), dtype=torch.int64, device=dev)

        def count_pass():
            import ctypes

            o, ri = _lib.RadiusOptions(), _lib.RadiusInfo()
            o.d_queries, o.m, o.radius, o.sort, o.d_offsets = q_dev.data_ptr(), rows_n, r, 0, offsets.data_ptr()
            _lib.check(eng._lib.tknnRadiusQuery(eng._h, ctypes.byref(o), ctypes.byref(ri), None))
            return ri.as_dict()

        variants["radius_query_count"] = count_pass
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
            for field in ("solve_ms", "order_ms", "stage_ms", "walk_ms", "total", "max_row", "fallback_items", "point_tests", "node_tests"):
                vals = [i[field] for i in infos[v] if field in i]
                if vals:
                    entry[field] = stats(vals) if isinstance(vals[0], float) else vals[0]
            case["variants"][v] = entry
            e = entry["events_ms"]
            print("  %-28s events %.3f ms (%.3f .. %.3f)%s" % (v, e["median"], e["min"], e["max"],
                                                             "  walk %.3f stage %.3f" % (entry["walk_ms"]["median"], entry["stage_ms"]["median"]) if "stage_ms" in entry else ""), flush=True)
        ratios = {}
        count = case["variants"]["radius_query_count"]
        for weight in WEIGHTS:
            for C in CHANNELS:
                mine = case["variants"]["reduce_%s_c%d" % (weight, C)]
                entry = {"walk_over_count_walk": mine["walk_ms"]["median"] / count["walk_ms"]["median"],
                         "call_over_count_call": mine["events_ms"]["median"] / count["events_ms"]["median"]}
                other = case["variants"].get("recipe_%s_c%d" % (weight, C))
                if other:
                    entry["recipe_over_call"] = other["events_ms"]["median"] / mine["events_ms"]["median"]
                ratios["%s_c%d" % (weight, C)] = entry
        case["ratios"] = ratios
        rec["cases"] = [c for c in rec["cases"] if c["case"] != name] + [case]
        save()
    eng.close()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
