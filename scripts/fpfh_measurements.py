#!/usr/bin/env python3
"""Times of tknnFpfh (33-bin point-feature histograms, no lists) on one MI355X, written to profiles/fpfh_measurements.json.

The cases: uniform points of the unit cube and the 64-component Gaussian mixture, --sizes points each, normals from
normals(k=16).  Per case two radii, with about 25 and about 50 points within them on average (found by bisection on
tknnRadiusReduce's counts).  Per radius the variants alternate inside every repetition, --reps of them after 1 warm-up, in one process
on one tree; median, minimum and maximum of the HIP events around each and of the call's own info (stage_ms, spfh_ms, fpfh_ms):
  fpfh           the call asking for d_fpfh alone;
  spfh           the call asking for d_spfh alone (pass 1 and its rows kernel, no second pass);
  recipe         what a user has without it: radius_query(sort=False), torch gathers of points and normals, the pair features in
                 torch, bincount for the SPFH and one index_add_ of the 33 weighted columns.  Not run where the lists would hold more
                 than --recipe-pairs pairs;
  reduce_c0      tknnRadiusReduce on the own points at the same radius, skip_self, no values: the floor of pass 1's walk;
  reduce_c16     the same with 16 channels: the value traffic of one 64-byte row per pair; pass 2 moves a 144-byte row.
tknnRadiusReduce's code is the parent commit's, unchanged by tknnFpfh, so the two floors are the parent's in the same session.
Before anything is timed the recipe's integer histograms are compared with the call's (the share of pairs that sit in another bin,
torch's atan2 and contractions being its own: at most 1 %) and the recipe's blend, fed the call's counts, with the call's FPFH (inside
twice the relative bound of tests/fpfh_spec.py); outside either, the script stops.  A case replaces the record of the same name and
size in an existing --out file, so the sizes can be run one process each.

    python scripts/fpfh_measurements.py [--reps 5] [--sizes 1000000,10000000] [--cases uniform,mixture] [--out profiles/fpfh_measurements.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from radius_measurements import stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--cases", default="uniform,mixture")
    ap.add_argument("--recipe-pairs", type=float, default=6e7, help="the recipe runs where the lists hold at most so many pairs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "warmups": 1, "reps": a.reps, "cases": []}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            rec["cases"] = json.load(fh).get("cases", [])
    rec["source_fingerprint"] = _lib.source_fingerprint()

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every radius: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    eng = TrueKNN(device=0)
    for name in a.cases.split(","):
        for n in (int(s) for s in a.sizes.split(",")):
            pts = datasets.uniform3d(n, seed=0) if name == "uniform" else datasets.gaussian_mixture3d(n)
            P = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
            eng.build(P)
            normals = eng.normals(k=16)["normals"].contiguous()

            def mean_count(r):
                return float(eng.radius_reduce(r, skip_self=True, want_wsum=False)["info"]["total"]) / n

            def radius_for(within):
                lo, hi = 0.0, 0.5
                for _ in range(18):
                    mid = 0.5 * (lo + hi)
                    lo, hi = (mid, hi) if mean_count(mid) < within else (lo, mid)
                return float(np.float32(hi))

            case = {"case": name, "points": n, "radii": {}}
            for about in (25, 50):
                radius = radius_for(about)
                pairs = mean_count(radius) * n
                with_recipe = pairs <= a.recipe_pairs
                print("%s n=%d about %d within: radius %.6f, %.0f pairs, recipe %s" % (name, n, about, radius, pairs, with_recipe), flush=True)

                def recipe():
                    rows = eng.radius_query(P, radius, sort=False, want_dist=False)
                    lens = rows["offsets"][1:] - rows["offsets"][:-1]
                    src, dst = torch.repeat_interleave(torch.arange(n, device=dev), lens), rows["idx"].long()
                    keep = src != dst
                    src, dst = src[keep], dst[keep]
                    dp, ni, nj = P[dst] - P[src], normals[src], normals[dst]
                    d2 = (dp * dp).sum(dim=1)
                    f4 = d2.sqrt()
                    a1, a2 = (ni * dp).sum(dim=1) / f4, (nj * dp).sum(dim=1) / f4
                    sw = (a1.abs() < a2.abs())[:, None]
                    n1, n2, dq = torch.where(sw, nj, ni), torch.where(sw, ni, nj), torch.where(sw, -dp, dp)
                    f3 = torch.where(sw[:, 0], -a2, a1)
                    v = torch.linalg.cross(dq, n1)
                    vn = v.norm(dim=1)
                    v = v / vn[:, None]
                    w = torch.linalg.cross(n1, v)
                    f2 = (v * n2).sum(dim=1)
                    f1 = torch.atan2((w * n2).sum(dim=1), (n1 * n2).sum(dim=1))
                    ok = (d2 > 0) & (vn > 0) & torch.isfinite(f1) & torch.isfinite(f2) & torch.isfinite(f3)
                    src, dst, d2 = src[ok], dst[ok], d2[ok]
                    bins = [(11 * (f1[ok] + np.pi) / (2 * np.pi)).floor().clamp(0, 10).long(), (11 * (f2[ok] + 1) * 0.5).floor().clamp(0, 10).long() + 11,
                            (11 * (f3[ok] + 1) * 0.5).floor().clamp(0, 10).long() + 22]
                    counts = torch.stack([torch.bincount(src * 33 + b, minlength=n * 33) for b in bins]).sum(dim=0).reshape(n, 33)
                    return {"counts": counts, "fpfh": blend_of(counts, src, dst, d2)}

                def blend_of(counts, src, dst, d2):
                    valid = counts[:, :11].sum(dim=1, keepdim=True)
                    spfh = torch.where(valid > 0, counts.float() * (100.0 / valid.clamp(min=1).float()), torch.zeros((), device=dev))
                    A = torch.zeros((n, 33), dtype=torch.float32, device=dev).index_add_(0, src, spfh[dst] / d2[:, None])
                    S = A.reshape(n, 3, 11).sum(dim=2, keepdim=True)
                    blend = torch.where(S > 0, A.reshape(n, 3, 11) * (100.0 / S.clamp(min=1e-30)), torch.zeros((), device=dev)).reshape(n, 33)
                    return blend + spfh

                entry = {"radius": radius, "about_within": about, "pairs": pairs, "recipe_measured": with_recipe, "variants": {}}
                if with_recipe:
                    got = eng.fpfh(radius, normals=normals, want_spfh=True)
                    ref = recipe()
                    moved = float((got["spfh_counts"].long() - ref["counts"]).abs().sum()) / 2 / max(pairs, 1)
                    # the floats: the recipe's blend FED the call's counts, both sides fp32 sums of non-negative terms: twice the
                    # relative bound of tests/fpfh_spec.py at the longest row
                    rows = eng.radius_query(P, radius, sort=False, want_dist=False)
                    lens = rows["offsets"][1:] - rows["offsets"][:-1]
                    src, dst = torch.repeat_interleave(torch.arange(n, device=dev), lens), rows["idx"].long()
                    keep = src != dst
                    src, dst = src[keep], dst[keep]
                    dq = P[dst] - P[src]
                    d2 = (dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1]) + dq[:, 2] * dq[:, 2]
                    fed = blend_of(got["spfh_counts"].long(), src[d2 > 0], dst[d2 > 0], d2[d2 > 0])
                    k = 2.0 * float(lens.max()) + 20.0
                    bound = 2.0 * k * 2.0 ** -24 / (1.0 - k * 2.0 ** -24)
                    share = float(((got["fpfh"] - fed).abs() / (bound * fed).clamp(min=1e-30)).max())
                    ok = moved <= 0.01 and share <= 1.0
                    entry["recipe_against_the_call"] = {"share_of_pairs_in_another_bin": moved, "fpfh_worst_share_of_the_bound": share, "inside": ok}
                    print("  recipe against the call: %.2e of the pairs in another bin; fed the call's counts, FPFH at %.3f of the bound: %s"
                          % (moved, share, "ok" if ok else "OUTSIDE"), flush=True)
                    del got, ref, rows, src, dst, dq, d2, fed
                    torch.cuda.empty_cache()
                    if not ok:
                        case["radii"]["within%d" % about] = entry
                        rec["cases"] = [c for c in rec["cases"] if (c["case"], c["points"]) != (name, n)] + [case]
                        save()
                        sys.exit(1)
                values = torch.ones((n, 16), dtype=torch.float32, device=dev)
                variants = {
                    "fpfh": lambda: eng.fpfh(radius, normals=normals)["info"],
                    "spfh": lambda: spfh_only(eng, radius, normals),
                    "reduce_c0": lambda: eng.radius_reduce(radius, skip_self=True, want_wsum=False)["info"],
                    "reduce_c16": lambda: eng.radius_reduce(radius, values=values, skip_self=True, want_wsum=False)["info"],
                }
                if with_recipe:
                    variants["recipe"] = lambda: recipe() and {}
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
                    e = {"events_ms": stats(wall[v])}
                    for field in ("solve_ms", "stage_ms", "spfh_ms", "fpfh_ms", "finish_ms", "walk_ms", "total", "max_row", "skipped_pairs", "fallback_items",
                                  "point_tests", "node_tests"):
                        vals = [i[field] for i in infos[v] if field in i]
                        if vals:
                            e[field] = stats(vals) if isinstance(vals[0], float) else vals[0]
                    entry["variants"][v] = e
                    parts = "  ".join("%s %.3f" % (f[:-3], e[f]["median"]) for f in ("stage_ms", "spfh_ms", "fpfh_ms", "walk_ms") if f in e)
                    print("  %-11s events %.3f ms (%.3f .. %.3f)  %s" % (v, e["events_ms"]["median"], e["events_ms"]["min"], e["events_ms"]["max"], parts), flush=True)
                f = entry["variants"]["fpfh"]
                entry["ratios"] = {"spfh_ms_over_reduce_c0": f["spfh_ms"]["median"] / entry["variants"]["reduce_c0"]["events_ms"]["median"],
                                   "fpfh_ms_over_reduce_c16": f["fpfh_ms"]["median"] / entry["variants"]["reduce_c16"]["events_ms"]["median"]}
                if with_recipe:
                    entry["ratios"]["recipe_over_fpfh"] = entry["variants"]["recipe"]["events_ms"]["median"] / f["events_ms"]["median"]
                print("  ratios: %s" % json.dumps(entry["ratios"]), flush=True)
                case["radii"]["within%d" % about] = entry
                rec["cases"] = [c for c in rec["cases"] if (c["case"], c["points"]) != (name, n)] + [case]
                save()
                del values
            del P, normals
            torch.cuda.empty_cache()
    eng.close()
    print("wrote", a.out)


def spfh_only(eng, radius, normals):
    """The call asking for d_spfh alone, through the C ABI (the wrapper always asks for d_fpfh)."""
    import ctypes

    import torch

    from owlraytracing_amd import _fpfh_lib, _lib

    out = torch.empty((eng.n, 33), dtype=torch.float32, device=eng.device)
    opt, info = _fpfh_lib.FpfhOptions(), _fpfh_lib.FpfhInfo()
    opt.radius, opt.d_normals, opt.d_spfh = float(radius), normals.data_ptr(), out.data_ptr()
    _lib.check(_fpfh_lib.load().tknnFpfh(eng._h, ctypes.byref(opt), ctypes.byref(info), eng._stream()))
    return info.as_dict()


if __name__ == "__main__":
    main()
