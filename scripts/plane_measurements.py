#!/usr/bin/env python3
"""Times of tknnSegmentPlane (RANSAC plane segmentation scored through the box pyramid) on one MI355X, written to
profiles/plane_measurements.json.

Sets: 1 M and 10 M points of datasets.room3d (a floor with 40 % of the points, two walls, uniform clutter) and the 10 M uniform cube.
Per set the threshold is 1 and 5 mean point spacings (the floor's 1 / sqrt(0.4 n) in the room, n^(-1/3) in the cube); per threshold
1 024 and 10 240 trials with confidence = 1 and 10 240 trials with the default confidence (0.999), refit_rounds = 1.  Per setting, on
one engine in one run, alternating: the call as it is (the walk) and the call with TKNN_PLANE_FORCE_FALLBACK=1 (every trial against
every row), 1 warm-up and --reps timed calls each: the time between two HIP events around the call and the device times the call
reports; the two must agree in plane, inliers and best trial or the script stops.  `tested_share` = point_tests / (c * scored trials)
of the walk, `walk_over_fallback` = the walk's score_ms over the fallback's, medians.  The floor of the walk's score kernel:
bytes = 16 B per row tested + 24 B per box tested over the measured copy bandwidth (6.29 TB/s), lane operations = 10 per row tested
+ 40 per box tested over 256 CUs * 128 lanes * 2.4 GHz; `score_over_floor` = score_ms over the larger of the two, which is named.
The torch recipe on the same device, confidence = 1 settings only: the planes of the same trials (tests/global_spec.py's sampler, all
rows active) as a (T, 4) matrix, |planes[:, :3] @ points.T + planes[:, 3]| <= thr summed per plane in chunks of --chunk planes, and
the argmax over the samples the call's DEGENERATE rule keeps; its best count is recorded beside the call's (fp32 matmul arithmetic is not the call's: they may differ by a few rows).

    python scripts/plane_measurements.py [--sets room:1000000,room:10000000,uniform:10000000] [--reps 3]
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

from emst_measurements import timed  # noqa: E402
from radius_measurements import stats  # noqa: E402

ENV = "TKNN_PLANE_FORCE_FALLBACK"
COPY_BYTES_PER_S = 6.29e12
LANE_OPS_PER_S = 256 * 128 * 2.4e9
SEED = 7


def make(kind, n):
    from owlraytracing_amd import datasets

    if kind == "room":
        return datasets.room3d(n), 1.0 / np.sqrt(0.4 * n)
    return datasets.uniform3d(n, seed=0), float(n) ** (-1.0 / 3.0)


def call(eng, thr, trials, confidence, fallback):
    os.environ.pop(ENV, None)
    if fallback:
        os.environ[ENV] = "1"
    try:
        return eng.segment_plane(thr, num_iterations=trials, confidence=confidence, seed=SEED, refit_rounds=1, return_info=True)
    finally:
        os.environ.pop(ENV, None)


def torch_recipe(torch, Pd, P, thr, trials, chunk, reps):
    """(events ms of --reps runs, best count): planes of the call's own trials, scored by a chunked matmul."""
    import global_spec

    idx, ok = global_spec.samples(SEED, np.arange(trials), 3, len(P))
    idx = torch.from_numpy(idx[ok]).to(Pd.device)

    def run():
        p0, p1, p2 = Pd[idx[:, 0]], Pd[idx[:, 1]], Pd[idx[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        nrm = torch.linalg.cross(e1, e2)
        good = (nrm * nrm).sum(dim=1) > 2.0 ** -40 * (e1 * e1).sum(dim=1) * (e2 * e2).sum(dim=1)  # the call's DEGENERATE rule: such a plane is not ranked
        nrm = nrm / nrm.norm(dim=1, keepdim=True)
        d = -(nrm * p0).sum(dim=1)
        counts = torch.empty((len(idx),), dtype=torch.int64, device=Pd.device)
        for lo in range(0, len(idx), chunk):
            counts[lo:lo + chunk] = ((nrm[lo:lo + chunk] @ Pd.T + d[lo:lo + chunk, None]).abs() <= thr).sum(dim=1)
        counts[~good] = -1
        best = torch.argmax(counts)
        return {"info": {"best": int(counts[best])}}

    run()
    wall, infos = timed(run, reps)
    return wall, infos[-1]["best"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="room:1000000,room:10000000,uniform:10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmups": 1, "refit_rounds": 1, "seed": SEED, "torch_chunk_planes": a.chunk, "checks": "ok",
           "copy_bytes_per_s": COPY_BYTES_PER_S, "lane_ops_per_s": LANE_OPS_PER_S, "source_fingerprint": _lib.source_fingerprint(), "cases": []}
    for spec in a.sets.split(","):
        kind, n = spec.split(":")
        n = int(n)
        P, spacing = make(kind, n)
        eng = TrueKNN(device=0)
        eng.build(P)
        Pd = torch.from_numpy(P).to(dev)
        for spacings in (1, 5):
            thr = float(np.float32(spacings * spacing))
            for trials, confidence in ((1024, 1.0), (10240, 1.0), (10240, 0.999)):
                walk, sweep = call(eng, thr, trials, confidence, False), call(eng, thr, trials, confidence, True)  # warm-up: the results are checked
                ok = (walk["plane"].tolist() == sweep["plane"].tolist() and walk["info"]["inliers"] == sweep["info"]["inliers"] and walk["info"]["best_trial"] == sweep["info"]["best_trial"]
                      and walk["info"]["status_counts"] == sweep["info"]["status_counts"] and torch.equal(walk["rows"], sweep["rows"]))
                print("%s n=%d thr=%.3g (%d spacings) trials=%d confidence=%g: checks %s" % (kind, n, thr, spacings, trials, confidence, "ok" if ok else "MISMATCH"), flush=True)
                if not ok:
                    rec["checks"] = "MISMATCH"
                    sys.exit(1)
                del walk, sweep
                wall, infos, wall_s, infos_s = [], [], [], []
                for _ in range(a.reps):  # alternating: other people's work shares the machine
                    w, i = timed(lambda: call(eng, thr, trials, confidence, False), 1)
                    wall += w
                    infos += i
                    w, i = timed(lambda: call(eng, thr, trials, confidence, True), 1)
                    wall_s += w
                    infos_s += i
                last = infos[-1]
                scored, c = last["status_counts"]["ok"], last["active"]
                case = {"set": kind, "n": n, "threshold": thr, "spacings": spacings, "max_trials": trials, "confidence": confidence, "trials_run": last["trials_run"], "batches": last["batches"],
                        "scored_trials": scored, "active": c, "inliers": last["inliers"], "fitness": last["fitness"], "inlier_rmse": last["inlier_rmse"], "refits_kept": last["refits_kept"],
                        "plane": last["plane"], "node_tests": last["node_tests"], "point_tests": last["point_tests"], "boxes_counted": last["boxes_counted"],
                        "tested_share": last["point_tests"] / max(c * scored, 1), "walk_events_ms": stats(wall), "fallback_events_ms": stats(wall_s),
                        "walk_device_ms": {k: stats([i[k] for i in infos]) for k in ("solve_ms", "sample_ms", "score_ms", "refit_ms")},
                        "fallback_device_ms": {k: stats([i[k] for i in infos_s]) for k in ("solve_ms", "sample_ms", "score_ms", "refit_ms")}}
                score, score_s = case["walk_device_ms"]["score_ms"]["median"], case["fallback_device_ms"]["score_ms"]["median"]
                case["walk_over_fallback"] = score / score_s
                case["call_walk_over_fallback"] = case["walk_events_ms"]["median"] / case["fallback_events_ms"]["median"]
                floors = {"bytes": (16.0 * last["point_tests"] + 24.0 * last["node_tests"]) / COPY_BYTES_PER_S * 1e3,
                          "lane_operations": (10.0 * last["point_tests"] + 40.0 * last["node_tests"]) / LANE_OPS_PER_S * 1e3}
                bound = max(floors, key=floors.get)
                case["score_floor_ms"], case["score_floor_bound"], case["score_over_floor"] = floors, bound, score / max(floors[bound], 1e-9)
                fall_floor = max(16.0 * c * scored / COPY_BYTES_PER_S, 10.0 * c * scored / LANE_OPS_PER_S) * 1e3
                case["fallback_score_over_floor"] = score_s / max(fall_floor, 1e-9)
                if confidence == 1.0:
                    tw, tbest = torch_recipe(torch, Pd, P, thr, trials, a.chunk, a.reps)
                    case["torch_events_ms"], case["torch_best_count"] = stats(tw), tbest
                    case["walk_over_torch"] = case["walk_events_ms"]["median"] / case["torch_events_ms"]["median"]
                print("  walk %.2f ms (score %.2f) fallback %.2f ms (score %.2f): score ratio %.3f, tested share %.4f, %d trials run, %d inliers; score/floor %.1f (%s)%s"
                      % (case["walk_events_ms"]["median"], score, case["fallback_events_ms"]["median"], score_s, case["walk_over_fallback"], case["tested_share"], last["trials_run"],
                         last["inliers"], case["score_over_floor"], bound, "; torch %.2f ms" % case["torch_events_ms"]["median"] if confidence == 1.0 else ""), flush=True)
                rec["cases"].append(case)
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
                    json.dump(rec, fh, indent=1)
        eng.close()
        del Pd
        torch.cuda.empty_cache()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
