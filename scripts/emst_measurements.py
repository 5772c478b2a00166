#!/usr/bin/env python3
"""Times of tknnEmst (minimum spanning tree, Euclidean and under mutual reachability) on one MI355X, written to
profiles/emst_measurements.json.

Sets: 1 M and 10 M uniform points, 10 M points of a 64-component mixture; each plain and with min_samples = 5 (core distance =
the 4th column of tknnKnn over the set's own points).  Per case 1 warm-up and --reps timed calls: the time between two HIP events
around the call and the device times the call reports (solve, walk, merge, sort), rounds, node and point tests per point and
the subtrees stepped over.  Per round: the call is repeated with max_rounds = 1, 2, ... (it then ends with TKNN_E_ROUNDS, writes
nothing and reports the work so far), and a round's walk and merge times are the differences of consecutive reports.
The yardstick is the own-points tknnKnn(k = 1) on the same engine in the same run -- Boruvka's first round asks exactly that
question, later rounds skip ever larger subtrees: `ratio_to_rounds_times_knn1` = emst / (rounds x knn1), medians of the events.
Checks before anything is timed: edges = n - 1; plain: the nearest-neighbour edge of 200 seeded points (tknnKnn, k = 1) is in the
tree (the cut property); mutual reachability: the weights of 200 seeded records recomputed on the host from the points and the
core distances, bit for bit.

    python scripts/emst_measurements.py [--sets uniform:1000000,uniform:10000000,mixture:10000000] [--reps 3]
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

from radius_measurements import stats  # noqa: E402

MIN_SAMPLES = 5
E_ROUNDS = -4


def timed(f, reps):
    import torch

    wall, infos = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = f()
        e1.record()
        e1.synchronize()
        wall.append(e0.elapsed_time(e1))
        infos.append(res["info"])
        del res
    return wall, infos


def rounds_report(eng, core, rounds):
    """Cumulative (walk_ms, merge_ms, edges) after 1 .. rounds rounds, through the C ABI: a call cut short reports in its info."""
    import torch

    from owlraytracing_amd import _emst_lib

    lib = _emst_lib.load()
    n = eng.n
    u = torch.empty(n - 1, dtype=torch.int32, device=eng.device)
    v = torch.empty(n - 1, dtype=torch.int32, device=eng.device)
    out = []
    for r in range(1, rounds + 1):
        o, info = _emst_lib.EmstOptions(), _emst_lib.EmstInfo()
        o.d_u, o.d_v, o.max_rounds = u.data_ptr(), v.data_ptr(), r
        o.d_core_dist = None if core is None else core.data_ptr()
        rc = lib.tknnEmst(eng._h, ctypes.byref(o), ctypes.byref(info), eng._stream())
        assert rc in (0, E_ROUNDS) and info.rounds == r, (rc, info.rounds, r)
        out.append((info.walk_ms, info.merge_ms, info.edges))
    per_round = []
    for r, (walk, merge, edges) in enumerate(out):
        pw, pm, pe = out[r - 1] if r else (0.0, 0.0, 0)
        per_round.append({"round": r + 1, "walk_ms": walk - pw, "merge_ms": merge - pm, "edges_added": edges - pe})
    return per_round


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="uniform:1000000,uniform:10000000,mixture:10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emst_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmups": 1, "checked_points": 200, "checks": "ok",
           "source_fingerprint": _lib.source_fingerprint(), "cases": []}
    rng = np.random.default_rng(91)
    for spec in a.sets.split(","):
        kind, n = spec.split(":")
        n = int(n)
        P = datasets.uniform3d(n, seed=0) if kind == "uniform" else datasets.gaussian_mixture3d(n, components=64, sigma=0.02, seed=1)
        P = np.ascontiguousarray(P, np.float32)
        eng = TrueKNN(device=0)
        eng.build(P)
        eng.knn(k=1)  # warm-up
        knn_wall, knn_infos = timed(lambda: eng.knn(k=1, want_dist=False), a.reps)
        nn = eng.knn(k=1)["idx"][:, 0]
        for min_samples in (1, MIN_SAMPLES):
            core = None if min_samples == 1 else eng.knn(k=min_samples - 1)["dist"][:, -1].contiguous()
            got = eng.emst(core_dist=core)  # warm-up: the result is checked
            info = got["info"]
            assert got["edges"] == n - 1 and info["components"] == 1, info
            rows = np.sort(rng.choice(n, 200, replace=False))
            if core is None:
                sel = torch.from_numpy(rows).to(dev)
                a_, b_ = sel.to(torch.int64), nn[sel].to(torch.int64)
                want = (torch.minimum(a_, b_) << 32) | torch.maximum(a_, b_)
                have = (got["u"].to(torch.int64) << 32) | got["v"].to(torch.int64)
                ok = bool(torch.isin(want, have).all())
            else:
                sel = torch.from_numpy(np.sort(rng.choice(n - 1, 200, replace=False))).to(dev)
                u, v, w = got["u"][sel].cpu().numpy(), got["v"][sel].cpu().numpy(), got["w"][sel].cpu().numpy()
                c = core.cpu().numpy()
                d = P[u] - P[v]
                dist = np.sqrt(((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2]), dtype=np.float32)
                ok = np.array_equal(np.maximum(np.maximum(dist, c[u]), c[v]).view(np.uint32), w.view(np.uint32))
            print("%s n=%d min_samples=%d: check of 200 %s" % (kind, n, min_samples, "ok" if ok else "MISMATCH"), flush=True)
            if not ok:
                rec["checks"] = "MISMATCH"
                sys.exit(1)
            del got
            wall, infos = timed(lambda: eng.emst(core_dist=core), a.reps)
            last = infos[-1]
            case = {"set": kind, "n": n, "min_samples": min_samples, "rounds": last["rounds"], "round_bound": int(np.ceil(np.log2(n))) + 1,
                    "events_ms": stats(wall), "device_ms": {key: stats([i[key] for i in infos]) for key in ("solve_ms", "walk_ms", "merge_ms", "sort_ms")},
                    "point_tests_per_point": last["point_tests"] / n, "node_tests_per_point": last["node_tests"] / n,
                    "skipped_subtrees_per_point": last["skipped_subtrees"] / n,
                    "knn1_events_ms": stats(knn_wall), "knn1_device_ms": stats([i["solve_ms"] for i in knn_infos]),
                    "per_round": rounds_report(eng, core, last["rounds"])}
            case["ratio_to_rounds_times_knn1"] = case["events_ms"]["median"] / (last["rounds"] * case["knn1_events_ms"]["median"])
            print("  emst %.2f ms (%.2f .. %.2f), %d rounds, walk %.2f merge %.2f sort %.2f; knn(k=1) %.2f ms; ratio %.3f; %.1f point tests per point"
                  % (case["events_ms"]["median"], case["events_ms"]["min"], case["events_ms"]["max"], last["rounds"], last["walk_ms"], last["merge_ms"],
                     last["sort_ms"], case["knn1_events_ms"]["median"], case["ratio_to_rounds_times_knn1"], case["point_tests_per_point"]), flush=True)
            for r in case["per_round"]:
                print("    round %d: walk %.2f ms, merge %.2f ms, %d edges" % (r["round"], r["walk_ms"], r["merge_ms"], r["edges_added"]), flush=True)
            rec["cases"].append(case)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
                json.dump(rec, fh, indent=1)
            del core
            torch.cuda.empty_cache()
        eng.close()
        del nn
    print("wrote", a.out)


if __name__ == "__main__":
    main()
