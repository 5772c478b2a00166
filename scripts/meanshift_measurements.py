#!/usr/bin/env python3
"""Times of tknnMeanShift (mean-shift trajectories, the loop on the device) on one MI355X, written to
profiles/meanshift_measurements.json.

The workloads: 10 M uniform points of the unit cube and 10 M points of the 64-component mixture; as seeds 1 M external points (uniform
for the uniform set, points of the mixture jittered by r for the mixture) at radii with about 10 and about 100 points within r -- for
the mixture at a component's centre, fewer elsewhere --, and the seeds of bin_seeds(points, r) at the larger radius; the flat kernel
(bandwidth r) and the Gauss kernel (bandwidth r / 3, truncated at r).  Per workload, in one process on one tree, the variants alternating inside every repetition, 1 warm-up, the median
of --reps:
  pass        the call with tol = 0 and max_iterations = --passes: no seed stops but those without neighbours; HIP events around the
              call and the call's own walk_ms, per pass;
  recipe_pass what a user has without the call, on the same engine: per pass radius_reduce(queries = x, values = P, normalize) plus
              the torch shift, mask and index compaction, the same number of passes with a negative tol: every seed that has
              neighbours stays, as in the call (the recipe's shift is a difference of absolute coordinates and rounds to exactly 0
              for seeds whose offset sums do not; at tol = 0 it would walk fewer seeds than the call);
  call        the whole call at tol = 1e-3 bandwidth and at most --max-iterations: info.walks against m * passes, compact_ms,
              order_ms, the seeds per status;
  recipe      the recipe's loop at the same tol and cap;
  reorder_R   the call with TKNN_MEANSHIFT_REORDER=R (R = 1, 3), after its arrays were compared with the plain call's bit for bit.
Before anything is timed one step of the call is compared with one step of the recipe.  The recipe sums absolute coordinates, so the
comparison is under ITS bound, reduce_spec's with |p| <= B = |x| + r for every neighbour: dS <= 2 u ((len + 2) W + c_K len) B per axis,
dW the same without B, so the quotient errs by at most 2 (2 u (len + 2 + c_K len / W) B) + u B; the call's own bound is the same with
r for B and is added (B + r in place of B).  The counts are compared exactly.

    python scripts/meanshift_measurements.py [--reps 3] [--cases uniform_ext10,...] [--out profiles/meanshift_measurements.json]
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
from reduce_measurements import radius_for  # noqa: E402

KERNELS = ("flat", "gauss")
CASES = ("uniform_ext10", "uniform_ext100", "uniform_bins100", "mixture_ext10", "mixture_ext100", "mixture_bins100")
ARRAYS = ("modes", "counts", "wsum", "shift", "iterations", "status")
REORDER = "TKNN_MEANSHIFT_REORDER"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--seeds", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=40)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meanshift_measurements.json"))
    a = ap.parse_args()

    import torch

    import reduce_spec as rd
    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN, bin_seeds

    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "warmups": 1, "points": a.points, "seeds": a.seeds, "passes": a.passes,
           "max_iterations": a.max_iterations, "cases": []}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            rec["cases"] = json.load(fh).get("cases", [])
    rec["source_fingerprint"] = _lib.source_fingerprint()

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    n, m = a.points, a.seeds
    eng = TrueKNN(device=0)
    built = None
    for name in a.cases.split(","):
        data, kind = name.split("_")
        within = int(kind.lstrip("extbins"))
        # points per unit volume: n for the uniform set; for the mixture at a component's centre, n / (64 (2 pi)^1.5 sigma^3)
        density = n if data == "uniform" else n / (64 * (2.0 * np.pi) ** 1.5 * 0.02 ** 3)
        r = radius_for(density, within)
        if built != data:
            pts = datasets.uniform3d(n, seed=0) if data == "uniform" else datasets.gaussian_mixture3d(n)
            P = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
            eng.build(P)
            built = data
        if kind.startswith("bins"):
            X = bin_seeds(P, r)
        elif data == "uniform":
            X = torch.from_numpy(np.random.default_rng(7).random((m, 3), dtype=np.float32)).to(dev)
        else:
            rng = np.random.default_rng(8)
            X = (P[torch.from_numpy(rng.integers(0, n, m)).to(dev)] + torch.from_numpy(rng.normal(0, r, (m, 3)).astype(np.float32)).to(dev)).contiguous()
        rows = int(X.shape[0])
        case = {"case": name, "seeds": rows, "radius": r, "about_within": within, "kernels": {}}
        print("%s: %d seeds, r %.5f" % (name, rows, r), flush=True)
        for kernel in KERNELS:
            bw = r if kernel == "flat" else r / 3.0
            weight = "one" if kernel == "flat" else "gauss"
            tol = 1e-3 * bw

            def call(tol_, iters):
                return eng.mean_shift_modes(bw, seeds=X, kernel=kernel, radius=r, tol=tol_, max_iterations=iters)

            def recipe(tol_, iters):
                """The loop in torch around radius_reduce; (positions, passes, walks)."""
                x, alive = X.clone(), torch.arange(rows, device=dev)
                passes = walks = 0
                while passes < iters and alive.numel():
                    q = x[alive].contiguous()
                    res = eng.radius_reduce(r, queries=q, values=P, weight=weight, bandwidth=bw, normalize=True, want_wsum=False)
                    passes += 1
                    walks += int(alive.numel())
                    has = res["counts"] > 0
                    new = torch.where(has[:, None], res["out"], q)
                    shift = torch.linalg.vector_norm(new - q, dim=1)
                    x[alive] = new
                    alive = alive[has & (shift > tol_)]
                return x, passes, walks

            # ---- one step of each against the other, under the recipe's bound ----
            one = call(0.0, 1)
            x1, _, _ = recipe(0.0, 1)
            ln, W = one["counts"].double(), one["wsum"].double().clamp_min(1e-300)
            B = X.abs().double().amax(dim=1) + r
            ck = rd.c_k(weight, r, bw)
            bound = 2.0 * (2.0 * rd.U * (ln + 2.0 + ck * ln / W) * (B + r)) + rd.U * B + 1e-37
            has = one["counts"] > 0
            err = (one["modes"].double() - x1.double()).abs().amax(dim=1)
            share = float((err[has] / bound[has]).max()) if bool(has.any()) else 0.0
            counts_ok = bool(torch.equal(one["counts"], eng.radius_reduce(r, queries=X, want_wsum=False)["counts"]))
            print("  %s: one step, call against recipe: worst share of the recipe's bound %.3g, counts %s" % (kernel, share, "equal" if counts_ok else "DIFFER"), flush=True)
            entry = {"bandwidth": bw, "tol": tol, "verified": {"worst_share_of_the_recipes_bound": share, "counts_equal": counts_ok, "seeds_with_neighbours": int(has.sum())}}
            if not (share <= 1.0 and counts_ok):
                case["kernels"][kernel] = entry
                rec["cases"] = [c for c in rec["cases"] if c["case"] != name] + [case]
                save()
                sys.exit(1)
            # ---- reordering changes no bit ----
            plain = call(tol, a.max_iterations)
            same = {}
            for R in (1, 3):
                os.environ[REORDER] = str(R)
                other = call(tol, a.max_iterations)
                os.environ.pop(REORDER)
                same[R] = all(torch.equal(plain[k].view(torch.int32) if plain[k].dtype == torch.float32 else plain[k],
                                          other[k].view(torch.int32) if other[k].dtype == torch.float32 else other[k]) for k in ARRAYS)
                same[R] = same[R] and other["info"]["walks"] == plain["info"]["walks"]
            entry["reorder_bit_for_bit"] = {str(R): ok for R, ok in same.items()}
            print("  %s: reorder 1, 3 against none, bit for bit: %s" % (kernel, same), flush=True)
            del plain, other, one, x1
            if not all(same.values()):
                case["kernels"][kernel] = entry
                rec["cases"] = [c for c in rec["cases"] if c["case"] != name] + [case]
                save()
                sys.exit(1)

            def reordered(R):
                os.environ[REORDER] = str(R)
                try:
                    return call(tol, a.max_iterations)["info"]
                finally:
                    os.environ.pop(REORDER)

            variants = {"pass": lambda: call(0.0, a.passes)["info"], "recipe_pass": lambda: dict(zip(("x", "iterations", "walks"), recipe(-1.0, a.passes))),
                        "call": lambda: call(tol, a.max_iterations)["info"], "recipe": lambda: dict(zip(("x", "iterations", "walks"), recipe(tol, a.max_iterations))),
                        "reorder_1": lambda: reordered(1), "reorder_3": lambda: reordered(3)}
            wall, infos = {v: [] for v in variants}, {}
            for rep in range(a.reps + 1):
                for v, f in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    res = f()
                    e1.record()
                    e1.synchronize()
                    res.pop("x", None)
                    if rep:  # (rep 0: the warm-up)
                        wall[v].append(e0.elapsed_time(e1))
                        infos.setdefault(v, []).append(res)
                torch.cuda.empty_cache()
            out = {}
            for v in variants:
                e = {"events_ms": stats(wall[v])}
                for field in ("solve_ms", "order_ms", "walk_ms", "compact_ms", "iterations", "walks", "converged", "empty", "running", "invalid", "fallback_items",
                              "point_tests", "node_tests"):
                    vals = [i[field] for i in infos[v] if field in i]
                    if vals:
                        e[field] = stats(vals) if isinstance(vals[0], float) else vals[0]
                e["events_ms_per_pass"] = e["events_ms"]["median"] / max(1, e["iterations"])
                e["events_ms_per_million_walks"] = e["events_ms"]["median"] / max(1, e["walks"]) * 1e6
                out[v] = e
                print("  %s %-12s events %.3f ms (%.3f .. %.3f), %d passes, %d walks of %d: %.3f ms per pass, %.3f ms per 1 M walks%s" % (
                    kernel, v, e["events_ms"]["median"], e["events_ms"]["min"], e["events_ms"]["max"], e["iterations"], e["walks"], rows * e["iterations"],
                    e["events_ms_per_pass"], e["events_ms_per_million_walks"],
                    "  walk %.3f compact %.3f order %.3f" % (e["walk_ms"]["median"], e["compact_ms"]["median"], e["order_ms"]["median"]) if "walk_ms" in e else ""), flush=True)
            entry["variants"] = out
            entry["ratios"] = {"recipe_pass_over_pass": out["recipe_pass"]["events_ms"]["median"] / out["pass"]["events_ms"]["median"],
                               "recipe_over_call": out["recipe"]["events_ms"]["median"] / out["call"]["events_ms"]["median"],
                               "reorder_1_over_call": out["reorder_1"]["events_ms"]["median"] / out["call"]["events_ms"]["median"],
                               "reorder_3_over_call": out["reorder_3"]["events_ms"]["median"] / out["call"]["events_ms"]["median"],
                               "walks_over_m_passes": out["call"]["walks"] / float(rows * out["call"]["iterations"])}
            case["kernels"][kernel] = entry
        rec["cases"] = [c for c in rec["cases"] if c["case"] != name] + [case]
        save()
    eng.close()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
