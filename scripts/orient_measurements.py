#!/usr/bin/env python3
"""Times of tknnOrientNormals (consistent normal orientation along a minimum spanning tree) on one MI355X, written to
profiles/orient_measurements.json.

Sets: 1 M and 10 M points of a unit sphere with noisy radial normals of random sign, and of the 64-component mixture with random
normals; k = 16.  Per case 1 warm-up and --reps timed calls: the time between two HIP events around the call and the device times
the call reports (solve, knn, emst, sort, forest, apply), the rounds, tree edges, components and flips.  On the same engine in the
same run the own-points tknnKnn(k = 16) and tknnEmst alone: the floor the call cannot beat, since it runs both.  `forest_over_emst`
= forest_ms / emst_ms and `rounds_over_inner` = forest_ms / (knn_ms + emst_ms), medians.
Checks before anything is timed: on the sphere the oriented normals of 1 000 seeded rows point outward (dot with the position > 0)
-- noise of this size does not turn a normal past 90 degrees --; on both sets a second call on the output flips nothing.
At 1 M points the host recipe on the same edges, if scipy is present: scipy.sparse.csgraph.minimum_spanning_tree over the kNN and
EMST edges weighted 1 - |n_i . n_j| and breadth_first_order from the top point (the flips along it are one more vectorised pass and
are left out); if scipy is absent the record says so.

    python scripts/orient_measurements.py [--sets sphere:1000000,mixture:1000000,sphere:10000000,mixture:10000000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from emst_measurements import timed  # noqa: E402
from radius_measurements import stats  # noqa: E402

K = 16
HOST_N = 1000000


def make(kind, n):
    from owlraytracing_amd import datasets

    rng = np.random.default_rng(17)
    g = rng.standard_normal((n, 3)).astype(np.float32)
    U = g / np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32)
    if kind == "sphere":
        P = U
        N = U + rng.standard_normal((n, 3)).astype(np.float32) * np.float32(0.2)
        N /= np.linalg.norm(N, axis=1, keepdims=True).astype(np.float32)
    else:
        P = datasets.gaussian_mixture3d(n, components=64, sigma=0.02, seed=1)
        N = U
    N = np.where((rng.random(n) < 0.5)[:, None], -N, N)
    return np.ascontiguousarray(P, np.float32), np.ascontiguousarray(N, np.float32)


def host_recipe(eng, P, N):
    """Seconds of scipy's spanning tree and breadth-first order on the call's own edges, or why not."""
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import breadth_first_order, minimum_spanning_tree
    except ImportError:
        return {"scipy": "not installed on this machine: the host recipe was not run"}
    n = eng.n
    idx = eng.knn(k=K, want_dist=False)["idx"].cpu().numpy()
    f = eng.emst()
    i = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), K), f["u"].cpu().numpy().astype(np.int64)])
    j = np.concatenate([idx.reshape(-1).astype(np.int64), f["v"].cpu().numpy().astype(np.int64)])
    keep = j >= 0
    i, j = i[keep], j[keep]
    t0 = time.perf_counter()
    w = np.maximum(1.0 - np.abs((N[i] * N[j]).sum(axis=1, dtype=np.float64)), 0.0) + 1e-12  # (scipy drops explicit zeros)
    G = sp.coo_matrix((w, (i, j)), shape=(n, n)).tocsr()
    t1 = time.perf_counter()
    T = minimum_spanning_tree(G)
    t2 = time.perf_counter()
    T = T + T.T
    breadth_first_order(T, int(np.argmax(P[:, 2])), directed=False)
    t3 = time.perf_counter()
    return {"scipy": "present", "edges": int(len(i)), "graph_s": t1 - t0, "minimum_spanning_tree_s": t2 - t1, "breadth_first_order_s": t3 - t2, "total_s": t3 - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="sphere:1000000,mixture:1000000,sphere:10000000,mixture:10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "k": K, "reps": a.reps, "warmups": 1, "checks": "ok", "source_fingerprint": _lib.source_fingerprint(), "cases": []}
    for spec in a.sets.split(","):
        kind, n = spec.split(":")
        n = int(n)
        P, N = make(kind, n)
        eng = TrueKNN(device=0)
        eng.build(P)
        Nd = torch.from_numpy(N).to(dev)
        got = eng.orient_normals(Nd, k=K)  # warm-up: the result is checked
        again = eng.orient_normals(got["normals"], k=K, want="flip")
        ok = again["info"]["flipped"] == 0
        if kind == "sphere":
            rows = torch.from_numpy(np.sort(np.random.default_rng(18).choice(n, 1000, replace=False))).to(dev)
            ok = ok and bool(((got["normals"][rows] * torch.from_numpy(P).to(dev)[rows]).sum(dim=1) > 0).all())
        print("%s n=%d: checks %s" % (kind, n, "ok" if ok else "MISMATCH"), flush=True)
        if not ok:
            rec["checks"] = "MISMATCH"
            sys.exit(1)
        del got, again
        wall, infos = timed(lambda: eng.orient_normals(Nd, k=K), a.reps)
        eng.knn(k=K, want_dist=False)
        knn_wall, knn_infos = timed(lambda: eng.knn(k=K, want_dist=False), a.reps)
        emst_wall, emst_infos = timed(lambda: eng.emst(), a.reps)
        last = infos[-1]
        case = {"set": kind, "n": n, "rounds": last["rounds"], "round_bound": int(np.ceil(np.log2(n))) + 1, "candidates": last["candidates"],
                "tree_edges": last["tree_edges"], "components": last["components"], "flipped": last["flipped"], "events_ms": stats(wall),
                "device_ms": {key: stats([i[key] for i in infos]) for key in ("solve_ms", "knn_ms", "emst_ms", "sort_ms", "forest_ms", "apply_ms")},
                "knn16_alone_events_ms": stats(knn_wall), "emst_alone_events_ms": stats(emst_wall)}
        d = case["device_ms"]
        case["forest_over_emst"] = d["forest_ms"]["median"] / d["emst_ms"]["median"]
        case["rounds_over_inner"] = d["forest_ms"]["median"] / (d["knn_ms"]["median"] + d["emst_ms"]["median"])
        case["call_over_floor"] = case["events_ms"]["median"] / (case["knn16_alone_events_ms"]["median"] + case["emst_alone_events_ms"]["median"])
        print("  orient %.2f ms (%.2f .. %.2f): knn %.2f emst %.2f sort %.2f forest %.2f apply %.2f; %d rounds; alone: knn(k=16) %.2f ms, emst %.2f ms; forest/emst %.3f, call/floor %.3f"
              % (case["events_ms"]["median"], case["events_ms"]["min"], case["events_ms"]["max"], d["knn_ms"]["median"], d["emst_ms"]["median"], d["sort_ms"]["median"],
                 d["forest_ms"]["median"], d["apply_ms"]["median"], last["rounds"], case["knn16_alone_events_ms"]["median"], case["emst_alone_events_ms"]["median"],
                 case["forest_over_emst"], case["call_over_floor"]), flush=True)
        if n == HOST_N:
            case["host_recipe"] = host_recipe(eng, P, N)
            print("  host recipe:", case["host_recipe"], flush=True)
        rec["cases"].append(case)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)
        eng.close()
        del Nd
        torch.cuda.empty_cache()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
