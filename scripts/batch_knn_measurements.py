#!/usr/bin/env python3
"""Times of the batched build and of tknnBatchKnn (k nearest inside the query's own cloud) on one MI355X, written to
profiles/batch_knn_measurements.json.

Uniform points, every cloud in the same unit cube, no radius.
  (a) the set's own points, k = 16, 32 clouds of 4 096 points (a DGCNN batch);
  (b) the set's own points, k = 16, 1 024 clouds of 1 024 points;
  (c) 1 M external queries against 10 M points in 64 clouds, k = 10.
Beside tknnBatchKnn, what the library offered before it:
  * `per_cloud_loop`: tknnBuild + tknnKnn per cloud on one reused engine, the clouds being slices of the same device buffers
    (the same rows, local indices);
  * `union_knn`: tknnKnn on a plain tree over all points, labels ignored -- ANOTHER answer (the k nearest of all clouds); it
    is the floor of the walk's work, recorded without a condition;
  * `build_batched` beside `build_plain` on the same points.
One process, the variants alternating call by call, 1 warm-up and --reps timed calls, the time between two HIP events around
the call: median with minimum and maximum.  Before anything is timed, 100 seeded rows of every tknnBatchKnn result are checked
against tests/batch_spec.py by brute force over the row's own cloud.

    python scripts/batch_knn_measurements.py [--reps 5] [--out profiles/batch_knn_measurements.json]
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

SPOT_ROWS = 100


def spot_check(P, batch, Q, batch_q, rows, k, idx, dist, counts, own):
    """Rows `rows` of a result against the spec over each row's own cloud (clouds are slices: batch is sorted)."""
    import batch_spec as bs

    starts = np.searchsorted(batch, np.arange(int(batch.max()) + 2))
    for t, j in enumerate(rows):
        b = int(batch_q[j])
        members = np.arange(starts[b], starts[b + 1])
        zeros = np.zeros(len(members), np.int32)
        want = bs.knn_rows(P[members], zeros, Q[j:j + 1], zeros[:1], k, ids=members, skip=[j] if own else None)
        if not (np.array_equal(idx[t], want["idx"][0]) and np.array_equal(dist[t].view(np.int32), want["dist"][0].view(np.int32))
                and counts[t] == want["counts"][0]):
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
            last[v] = res
            del res
    return wall, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_knn_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmups": 1, "spot_check_rows": SPOT_ROWS, "spot_check": "ok",
           "source_fingerprint": _lib.source_fingerprint(), "cases": []}
    rng = np.random.default_rng(91)

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    shapes = {"a": dict(clouds=32, per_cloud=4096, queries=None, k=16), "b": dict(clouds=1024, per_cloud=1024, queries=None, k=16),
              "c": dict(clouds=64, per_cloud=156_250, queries=1_000_000, k=10)}
    for name in a.shapes.split(","):
        sh = shapes[name]
        B, per, k = sh["clouds"], sh["per_cloud"], sh["k"]
        n = B * per
        own = sh["queries"] is None
        P = np.random.default_rng(7).random((n, 3), dtype=np.float32)
        batch = np.repeat(np.arange(B, dtype=np.int32), per)  # sorted: cloud b is a slice, which the per-cloud loop needs
        p_dev, b_dev = torch.from_numpy(P).to(dev), torch.from_numpy(batch).to(dev)
        if own:
            m, Q, bq, q_dev, bq_dev = n, P, batch, None, None
        else:
            m = sh["queries"]
            Q = np.random.default_rng(8).random((m, 3), dtype=np.float32)
            bq = np.repeat(np.arange(B, dtype=np.int32), m // B)
            assert len(bq) == m
            q_dev, bq_dev = torch.from_numpy(Q).to(dev), torch.from_numpy(bq).to(dev)
        eng, plain, loop_eng = TrueKNN(device=0), TrueKNN(device=0), TrueKNN(device=0)
        eng.build(p_dev, batch=b_dev, num_batches=B)
        plain.build(p_dev)

        def batch_call():
            return eng.batch_knn(q_dev, k, batch=bq_dev)["info"]

        def union_call():
            return plain.knn(q_dev, k)["info"]

        def loop_call():
            build_ms = solve_ms = 0.0
            for b in range(B):
                loop_eng.build(p_dev[b * per:(b + 1) * per])
                build_ms += loop_eng.build_info["build_ms"]
                part = None if own else q_dev[b * (m // B):(b + 1) * (m // B)]
                solve_ms += loop_eng.knn(part, k)["info"]["solve_ms"]
            return {"build_ms": build_ms, "solve_ms": solve_ms}

        def build_batched():
            return dict(eng.build(p_dev, batch=b_dev, num_batches=B))

        def build_plain():
            return dict(plain.build(p_dev))

        got = eng.batch_knn(q_dev, k, batch=bq_dev)
        rows = np.sort(rng.choice(m, SPOT_ROWS, replace=False))
        sel = torch.from_numpy(rows).to(dev)
        ok = spot_check(P, batch, Q, bq, rows, k, got["idx"][sel].cpu().numpy(), got["dist"][sel].cpu().numpy(), got["counts"][sel].cpu().numpy(), own)
        print("(%s) %d clouds of %d, m=%d, k=%d: spot check of %d rows %s" % (name, B, per, m, k, SPOT_ROWS, "ok" if ok else "MISMATCH"), flush=True)
        if not ok:
            rec["spot_check"] = "MISMATCH"
            save()
            sys.exit(1)
        bi, ui = got["info"], plain.knn(q_dev, k)["info"]
        case = {"setup": name, "clouds": B, "points_per_cloud": per, "points": n, "m": m, "k": k, "own_points": own, "key_bits": eng.batch_layout()["key_bits"],
                "full_rows": bi["full_rows"], "lane_rows": bi["lane_rows"],
                "point_tests_per_query": {"batch_knn": bi["point_tests"] / m, "union_knn": ui["point_tests"] / m, "seeds": bi["seed_point_tests"] / m},
                "node_tests_per_query": {"batch_knn": bi["node_tests"] / m, "union_knn": ui["node_tests"] / m}}
        del got
        torch.cuda.empty_cache()
        loop_call()  # the warm-up of the loop's engine (its buffers are sized by the first cloud)
        variants = {"batch_knn": batch_call, "union_knn": union_call, "per_cloud_loop": loop_call}
        wall, last = timed(variants, a.reps)
        builds = {"build_batched": build_batched, "build_plain": build_plain}
        bwall, blast = timed(builds, a.reps + 1)
        bwall = {v: w[1:] for v, w in bwall.items()}  # (the first: the warm-up)
        wall.update(bwall), last.update(blast)
        keep = ("solve_ms", "walk_ms", "order_ms", "seed_ms", "lane_rows", "build_ms")
        case["variants"] = {}
        for v in list(variants) + list(builds):
            case["variants"][v] = {"events_ms": stats(wall[v]), "info": {key: last[v][key] for key in keep if key in last[v]}}
            print("  %-16s events %.3f ms (%.3f .. %.3f)" % (v, np.median(wall[v]), min(wall[v]), max(wall[v])), flush=True)
        mine = case["variants"]["batch_knn"]["events_ms"]
        for v in ("union_knn", "per_cloud_loop"):
            case["variants"][v]["ratio_to_batch_knn"] = case["variants"][v]["events_ms"]["median"] / mine["median"]
        case["build_batched_over_build_plain"] = case["variants"]["build_batched"]["events_ms"]["median"] / case["variants"]["build_plain"]["events_ms"]["median"]
        both = case["variants"]["build_batched"]["events_ms"]["median"] + mine["median"]
        case["build_plus_query_ms"] = both
        case["per_cloud_loop_over_build_plus_query"] = case["variants"]["per_cloud_loop"]["events_ms"]["median"] / both
        case["faster_than_the_loop_by_more_than_the_spread"] = bool(
            case["variants"]["build_batched"]["events_ms"]["max"] + mine["max"] < case["variants"]["per_cloud_loop"]["events_ms"]["min"])
        rec["cases"].append(case)
        save()
        eng.close(), plain.close(), loop_eng.close()
        del eng, plain, loop_eng, p_dev, b_dev, q_dev, bq_dev
        torch.cuda.empty_cache()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
