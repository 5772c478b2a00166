#!/usr/bin/env python3
"""Times of tknnFps (farthest point sampling per cloud, pruned by the tree) on one MI355X, written to
profiles/fps_measurements.json.

Uniform points, every cloud in the same unit cube, the default start.
  (a) 32 clouds of 4 096 points, 1 024 samples each (a PointNet++ batch);
  (b) 1 024 clouds of 1 024 points, 256 samples each;
  (c) one cloud of 1 M points, 10 000 samples;
  (d) one cloud of 10 M points, 100 000 samples -- ONE call, no warm-up, no repetition.
Beside tknnFps:
  * `torch_loop`: what a user runs today, a dense loop in torch on the same device over the padded (B, N, 3) tensor -- per sample
    the distances to the last one, a `minimum` and an `argmax`.  It is the yardstick, not the code under test.  In (d) it runs
    --d-torch-samples samples only and the record says so (its cost per sample does not depend on the sample);
  * `no_prune`: tknnFps with TKNN_FPS_NO_PRUNE, a side figure, in (a) and (b) only (one wave would read a whole large cloud
    for every sample).
One process, the variants alternating call by call, 1 warm-up and --reps timed calls, the time between two HIP events around the
call: median with minimum and maximum.  Before anything is timed the rows of three seeded clouds equal tests/fps_spec.py's brute
force; of the large single clouds the first --prefix samples do (a row's head is the row of a smaller S), and the whole row is
compared with the torch loop's (recorded, uniform random points have no ties).

    python scripts/fps_measurements.py [--reps 5] [--shapes a,b,c,d] [--out profiles/fps_measurements.json]
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

from batch_knn_measurements import timed  # noqa: E402
from radius_measurements import stats  # noqa: E402


def torch_loop(X, S):
    """The dense loop over X (B, N, 3): (B, S) rows, the first sample row 0 of each cloud."""
    import torch

    B, N, _ = X.shape
    D = torch.full((B, N), float("inf"), device=X.device)
    cur = torch.zeros(B, dtype=torch.long, device=X.device)
    out = torch.empty((B, S), dtype=torch.long, device=X.device)
    clouds = torch.arange(B, device=X.device)
    for t in range(S):
        out[:, t] = cur
        d = X - X[clouds, cur][:, None, :]
        x, y, z = d[..., 0], d[..., 1], d[..., 2]
        D = torch.minimum(D, (x * x + y * y) + z * z)
        cur = D.argmax(dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--prefix", type=int, default=200)
    ap.add_argument("--d-torch-samples", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_measurements.json"))
    a = ap.parse_args()

    import torch

    import fps_spec as fs
    from owlraytracing_amd import _lib
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmups": 1, "spec_check": "ok",
           "source_fingerprint": _lib.source_fingerprint(), "cases": []}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    shapes = {"a": dict(clouds=32, per_cloud=4096, S=1024), "b": dict(clouds=1024, per_cloud=1024, S=256),
              "c": dict(clouds=1, per_cloud=1_000_000, S=10_000), "d": dict(clouds=1, per_cloud=10_000_000, S=100_000)}
    for name in a.shapes.split(","):
        sh = shapes[name]
        B, per, S = sh["clouds"], sh["per_cloud"], sh["S"]
        n, once = B * per, name == "d"
        P = np.random.default_rng(7).random((n, 3), dtype=np.float32)
        batch = np.repeat(np.arange(B, dtype=np.int32), per)
        p_dev = torch.from_numpy(P).to(dev)
        X = p_dev.view(B, per, 3)
        eng = TrueKNN(device=0)
        if B > 1:
            eng.build(p_dev, batch=torch.from_numpy(batch).to(dev), num_batches=B)
        else:
            eng.build(p_dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = eng.fps(num_samples=S)
        e1.record()
        e1.synchronize()
        first_call_ms = e0.elapsed_time(e1)
        idx, info = got["idx"].cpu().numpy(), got["info"]
        # the spec, before anything is timed
        if B > 1:
            seeded = sorted(int(b) for b in np.random.default_rng(92).choice(B, 3, replace=False))
            want = fs.brute(P, S, batch=batch, num_batches=B, clouds=seeded)
            ok = np.array_equal(idx[seeded], want["idx"][seeded]) and np.array_equal(got["dist"].cpu().numpy()[seeded].view(np.int32), want["dist"][seeded].view(np.int32))
            checked = {"clouds": seeded, "samples": S}
        else:
            head = max(min(a.prefix, 2 * 10**8 // n), 2)  # (the numpy loop reads the whole cloud per sample)
            want = fs.brute(P, head)
            ok = np.array_equal(idx[0, :head], want["idx"][0]) and np.array_equal(got["dist"].cpu().numpy()[0, :head].view(np.int32), want["dist"][0].view(np.int32))
            checked = {"clouds": [0], "samples": head}
        print("(%s) %d clouds of %d, S=%d: spec check %s, first call %.1f ms" % (name, B, per, S, "ok" if ok else "MISMATCH", first_call_ms), flush=True)
        if not ok:
            rec["spec_check"] = "MISMATCH"
            save()
            sys.exit(1)
        torch_S = min(S, a.d_torch_samples) if once else S
        rows = torch_loop(X, torch_S).cpu().numpy()
        local = idx - (np.arange(B, dtype=np.int64) * per)[:, None]
        case = {"setup": name, "clouds": B, "points_per_cloud": per, "points": n, "samples_per_cloud": S, "spec_checked": checked,
                "torch_loop_rows_equal": bool(np.array_equal(rows, local[:, :torch_S])), "first_call_ms": first_call_ms,
                "point_tests": info["point_tests"], "node_tests": info["node_tests"], "brute_force_point_updates": n * S,
                "point_tests_over_brute_force": info["point_tests"] / float(n * S), "variants": {}}
        del got
        if once:
            e0.record()
            torch_loop(X, torch_S)
            e1.record()
            e1.synchronize()
            t_ms = e0.elapsed_time(e1)
            case["variants"]["tknn_fps"] = {"events_ms": stats([first_call_ms]), "info": {k: info[k] for k in ("solve_ms", "init_ms", "walk_ms")},
                                            "note": "one call, no warm-up", "exceeds_a_few_seconds": bool(first_call_ms > 5000.0)}
            case["variants"]["torch_loop"] = {"events_ms": stats([t_ms]), "samples_run": torch_S, "extrapolated_ms": t_ms * S / torch_S}
            case["torch_loop_over_tknn_fps"] = t_ms * S / torch_S / first_call_ms
            print("  tknn_fps %.1f ms once; torch_loop %.1f ms for %d samples (%.1f ms for all)" % (first_call_ms, t_ms, torch_S, t_ms * S / torch_S), flush=True)
        else:
            variants = {"tknn_fps": lambda: eng.fps(num_samples=S)["info"], "torch_loop": lambda: {"rows": int(torch_loop(X, S).shape[0])}}
            if B > 1:
                variants["no_prune"] = lambda: eng.fps(num_samples=S, prune=False)["info"]
            timed(variants, 1)  # the warm-up
            wall, last = timed(variants, a.reps)
            for v in variants:
                case["variants"][v] = {"events_ms": stats(wall[v]), "info": {k: last[v][k] for k in ("solve_ms", "init_ms", "walk_ms", "point_tests") if k in last[v]}}
                print("  %-12s events %.3f ms (%.3f .. %.3f)" % (v, np.median(wall[v]), min(wall[v]), max(wall[v])), flush=True)
            mine, theirs = case["variants"]["tknn_fps"]["events_ms"], case["variants"]["torch_loop"]["events_ms"]
            case["torch_loop_over_tknn_fps"] = theirs["median"] / mine["median"]
            case["faster_than_the_torch_loop_by_more_than_the_spread"] = bool(mine["max"] < theirs["min"])
            case["slower_than_the_torch_loop_by_more_than_the_spread"] = bool(mine["min"] > theirs["max"])
            case["us_per_sample"] = 1000.0 * mine["median"] / S
        rec["cases"].append(case)
        save()
        eng.close()
        del eng, p_dev, X
        torch.cuda.empty_cache()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
