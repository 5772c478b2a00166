#!/usr/bin/env python3
"""Times of tknnRadiusNms (greedy suppression within a radius, per cloud) on one MI355X, written to
profiles/nms_measurements.json.

The sets:
  uniform     10 M uniform points at radii with about 2, 10 and 50 points within r, keys hashed and from random scores;
  mixture     10 M points of the 64-component mixture, the radius of "about 10" above, hashed;
  clouds      1 024 clouds of 1 024 uniform points in one batched tree, about 10 points within r, hashed;
  smooth      1 M uniform points, the score a point's x coordinate: the long-chain case.
Per set: rounds, rounds_ms, cover_ms, init_ms of --reps whole calls (1 warm-up; median, minimum, maximum of the HIP events around the
call and of the call's own info), and the course of the rounds: calls cut short by max_rounds = 1, 2, 3, 4, 6, 8, 12, ... report the
points still undecided and the time of the rounds so far, so the items and the time of a round follow from two neighbours.
Yardsticks, same process, same points, same radius, alternating with the call:
  (a) radius_query's count pass over the set's own points (not for the batched set: it would count across clouds);
  (b) --recipe sets only: what a user has today -- radius_query with sort = 0 (count + fill), then the same rounds as torch ops on the
      CSR (edges towards better keys, scatter_add of the neighbours' states); its kept set must equal the call's.
Before anything is timed --spot rows of every set are checked against the definition with tests/radius_spec.py's rows: a kept point
has no kept neighbour with a better key, a dropped one has, and its cover is the nearest kept neighbour by (distance bits, name).

    python scripts/nms_measurements.py [--reps 5] [--sets uniform2,uniform10,...] [--out profiles/nms_measurements.json]
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


def radius_for(n, within):
    """The radius of a ball that holds `within` of n uniform points of the unit cube."""
    return float(np.float32((within / (n * 4.1887902)) ** (1.0 / 3.0)))


def spot_check(P, r, keep, cover, key, rows, batch=None):
    """The definition on the points `rows`: True if every one of them has the state and the cover its neighbours demand."""
    ok = True
    for p, near in zip(rows, spot_rows(P, P, rows, r)):
        q, d = near["idx"].astype(np.int64), near["dist"]
        sel = q != p
        if batch is not None:
            sel &= batch[q] == batch[p]
        q, d = q[sel], d[sel]
        kept_better = keep[q] & (key[q] > key[p])
        ok &= bool(keep[p] == (not kept_better.any()))
        if keep[p]:
            ok &= bool(cover[p] == p)
        else:
            c = np.flatnonzero(keep[q])
            ok &= bool(len(c) > 0 and cover[p] == q[c[np.lexsort((q[c], d[c].view(np.uint32)))[0]]])
    return ok


def torch_rounds(n, offsets, idx, rank):
    """The recipe on CSR rows: (keep, rounds).  rank: int64 per point, the larger the better key."""
    import torch

    lens = offsets[1:] - offsets[:-1]
    src = torch.repeat_interleave(torch.arange(n, device=idx.device), lens)
    dst = idx.long()
    dom = rank[dst] > rank[src]
    src, dst = src[dom], dst[dom]
    state = torch.zeros(n, dtype=torch.int32, device=idx.device)  # 0 undecided, 1 kept, 2 dropped
    rounds = 0
    while True:
        st = state[dst]
        kept_near = torch.zeros(n, dtype=torch.int32, device=idx.device).scatter_add_(0, src, (st == 1).int()) > 0
        open_near = torch.zeros(n, dtype=torch.int32, device=idx.device).scatter_add_(0, src, (st == 0).int()) > 0
        und = state == 0
        state = torch.where(und & kept_near, 2, torch.where(und & ~open_near, 1, state)).int()
        rounds += 1
        if not bool((state == 0).any()):  # the recipe's one host read per round
            return state == 1, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spot", type=int, default=300)
    ap.add_argument("--sets", default="uniform2,uniform10,uniform50,uniform2_scored,uniform10_scored,uniform50_scored,mixture,clouds,smooth")
    ap.add_argument("--recipe", default="uniform2,uniform10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nms_measurements.json"))
    a = ap.parse_args()

    import torch

    import nms_spec as ns
    from owlraytracing_amd import _lib, _nms_lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    lib = _nms_lib.load()
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmups": 1, "spot_rows": a.spot, "spot_check": "ok",
           "source_fingerprint": _lib.source_fingerprint(), "cases": []}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    big, small = 10_000_000, 1_000_000
    sets = {}
    for within in (2, 10, 50):
        sets["uniform%d" % within] = dict(kind="uniform", n=big, r=radius_for(big, within), scored=False)
        sets["uniform%d_scored" % within] = dict(kind="uniform", n=big, r=radius_for(big, within), scored=True)
    sets["mixture"] = dict(kind="mixture", n=big, r=radius_for(big, 10), scored=False)
    sets["clouds"] = dict(kind="clouds", n=1024 * 1024, r=radius_for(1024, 10), scored=False)
    sets["smooth"] = dict(kind="smooth", n=small, r=radius_for(small, 10), scored=True)
    made = {}

    for name in a.sets.split(","):
        sh = sets[name]
        n, r = sh["n"], sh["r"]
        if sh["kind"] not in made:
            made.clear()
            if sh["kind"] == "mixture":
                P = datasets.gaussian_mixture3d(n, components=64, sigma=0.02, seed=1)
            else:
                P = datasets.uniform3d(n, seed=0 if sh["kind"] == "uniform" else 3)
            made[sh["kind"]] = np.ascontiguousarray(P, np.float32)
        P = made[sh["kind"]]
        batch = np.repeat(np.arange(1024, dtype=np.int32), 1024) if sh["kind"] == "clouds" else None
        scores = None
        if sh["kind"] == "smooth":
            scores = P[:, 0].copy()
        elif sh["scored"]:
            scores = np.random.default_rng(11).standard_normal(n).astype(np.float32)
        p_dev = torch.from_numpy(P).to(dev)
        s_dev = None if scores is None else torch.from_numpy(scores).to(dev)
        eng = TrueKNN(device=0)
        if batch is None:
            eng.build(p_dev)
        else:
            eng.build(p_dev, batch=torch.from_numpy(batch).to(dev), num_batches=1024)
        got = eng.radius_nms(r, scores=s_dev)
        keep, cover, info = got["keep"].cpu().numpy(), got["cover"].cpu().numpy(), got["info"]
        key = ns.keys(np.arange(n), scores)
        rows = np.sort(np.random.default_rng(79).choice(n, a.spot, replace=False))
        ok = spot_check(P, r, keep, cover, key, rows, batch)
        print("%s: n %d r %.5f kept %d rounds %d, spot check of %d points %s" % (name, n, r, info["kept"], info["rounds"], a.spot, "ok" if ok else "MISMATCH"), flush=True)
        if not ok:
            rec["spot_check"] = "MISMATCH"
            save()
            sys.exit(1)
        case = {"set": name, "points": n, "radius": r, "keys": "scores" if scores is not None else "hash", "kept": info["kept"], "eligible": info["eligible"],
                "fallback_items": info["fallback_items"], "variants": {}}
        del got

        # the course of the rounds: calls cut short
        keep_t = torch.empty((n,), dtype=torch.uint8, device=dev)
        course, t, last = [], 1, None
        while True:
            o, ci = _nms_lib.RadiusNmsOptions(), _nms_lib.RadiusNmsInfo()
            o.radius, o.max_rounds, o.d_keep = r, t, keep_t.data_ptr()
            o.d_scores = None if s_dev is None else s_dev.data_ptr()
            rc = lib.tknnRadiusNms(eng._h, ctypes.byref(o), ctypes.byref(ci), None)
            course.append({"max_rounds": t, "rounds": int(ci.rounds), "undecided": int(ci.undecided), "rounds_ms": float(ci.rounds_ms)})
            if rc == 0 or len(course) >= 40:
                break
            t = t + 1 if t < 4 else t + t // 2
        for i, c in enumerate(course):  # between two neighbours: the items that entered the later one's first new round, the time per round
            prev = course[i - 1] if i else {"rounds": 0, "undecided": info["eligible"], "rounds_ms": 0.0}
            steps = max(c["rounds"] - prev["rounds"], 1)
            c["items_at_start"] = prev["undecided"]
            c["ms_per_round"] = (c["rounds_ms"] - prev["rounds_ms"]) / steps
        case["course"] = course
        print("  course:", ", ".join("%d: %d left, %.3f ms" % (c["rounds"], c["undecided"], c["rounds_ms"]) for c in course[:12]), flush=True)

        # the timed variants, alternating
        def whole(cover_too):
            return lambda: eng.radius_nms(r, scores=s_dev, want_cover=cover_too)["info"]

        def first_round():
            o, ci = _nms_lib.RadiusNmsOptions(), _nms_lib.RadiusNmsInfo()
            o.radius, o.max_rounds, o.d_keep = r, 1, keep_t.data_ptr()
            o.d_scores = None if s_dev is None else s_dev.data_ptr()
            lib.tknnRadiusNms(eng._h, ctypes.byref(o), ctypes.byref(ci), None)
            return ci.as_dict()

        variants = {"radius_nms": whole(True), "radius_nms_no_cover": whole(False), "first_round": first_round}
        if batch is None:
            offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev)

            def count_pass():
                o, ri = _lib.RadiusOptions(), _lib.RadiusInfo()
                o.d_queries, o.m, o.radius, o.sort, o.d_offsets = p_dev.data_ptr(), n, r, 0, offsets.data_ptr()
                _lib.check(eng._lib.tknnRadiusQuery(eng._h, ctypes.byref(o), ctypes.byref(ri), None))
                return ri.as_dict()

            try:  # (a dense set has 2^31 or more neighbours in one call at this radius: the count pass refuses it)
                count_pass()
                variants["radius_query_count"] = count_pass
            except _lib.TknnError as err:
                case["radius_query_count_refused"] = str(err)
        if name in a.recipe.split(","):
            rank = torch.from_numpy(np.argsort(np.argsort(key)).astype(np.int64)).to(dev)

            def recipe():
                rows_ = eng.radius_query(p_dev, r, sort=False, want_dist=False)
                k_, rounds_ = torch_rounds(n, rows_["offsets"], rows_["idx"], rank)
                return {"rounds": rounds_, "kept": int(k_.sum()), "equal": bool(torch.equal(k_.cpu(), torch.from_numpy(keep)))}

            variants["recipe_radius_query_torch"] = recipe
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
        for v in variants:
            entry = {"events_ms": stats(wall[v])}
            for field in ("rounds", "rounds_ms", "cover_ms", "init_ms", "solve_ms", "walk_ms", "point_tests", "node_tests", "kept", "equal"):
                vals = [i[field] for i in infos[v] if field in i]
                if vals:
                    entry[field] = stats(vals) if isinstance(vals[0], float) else vals
            case["variants"][v] = entry
            e = entry["events_ms"]
            print("  %-26s events %.3f ms (%.3f .. %.3f)" % (v, e["median"], e["min"], e["max"]), flush=True)
        if "radius_query_count" in variants:
            f1, cnt = case["variants"]["first_round"]["rounds_ms"], case["variants"]["radius_query_count"]["walk_ms"]
            case["first_round_vs_count_walk"] = {"first_round_rounds_ms": f1["median"], "count_walk_ms": cnt["median"], "ratio": f1["median"] / cnt["median"],
                                                 "slower_by_more_than_the_spread": bool(f1["min"] > cnt["max"])}
        if "recipe_radius_query_torch" in variants:
            case["recipe_over_radius_nms"] = case["variants"]["recipe_radius_query_torch"]["events_ms"]["median"] / case["variants"]["radius_nms_no_cover"]["events_ms"]["median"]
        rec["cases"].append(case)
        save()
        eng.close()
        del eng, p_dev, s_dev, keep_t
        torch.cuda.empty_cache()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
