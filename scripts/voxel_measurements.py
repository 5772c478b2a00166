#!/usr/bin/env python3
"""Times of tknnVoxelGrid (voxel-grid downsampling per cloud) on one MI355X, written to profiles/voxel_measurements.json.

The sets:
  uniform1m, uniform10m   1 M and 10 M uniform points of the unit cube;
  mixture10m              10 M points of the 64-component mixture;
  clouds                  1 024 clouds of 1 024 uniform points, labelled, one call;
each at voxel sizes with about 1, 8, 64 and 1 000 rows per voxel (of a uniform set of that size; the mixture's voxels are fuller)
and with C = 0, 3 and 6 value columns; and one voxel that holds every row of uniform1m and uniform10m.
Per case --reps whole calls through TrueKNN.voxel_down_sample (1 warm-up; median, minimum, maximum of the HIP events around the call
and of the call's own key_ms, sort_ms, reduce_ms), alternating in the same process with
  (a) the torch recipe on the same device: bin_seeds' packed int64 key of floor((p - origin) / voxel), torch.unique(return_inverse,
      return_counts) and index_add_ of the fp64 rows for the sums -- its counts must equal the call's, its means lie within one fp32
      value of them;
  (b) torch.sort of the same packed keys alone, the floor of sort_ms: rocPRIM's radix sort as the call's hipcub one is, but of
      (int64 key, int64 index) pairs, 16 bytes a pair where the call sorts 12;
and against (c) a byte floor of the reduce: 4 bytes of row index and 12 + 4 C bytes read per row plus the outputs written, over the
8 TB/s of HBM that the project's shares are taken of (profiles/hbm_traffic.json).
The threshold between the lane and the wave (TKNN_VOXEL_LANE_ROWS) is swept on --sweep sets; the pipeline is global_registration on
two views of --pipeline-size points with a voxel_size that leaves about 20 k points of each.

    python scripts/voxel_measurements.py [--reps 5] [--sets uniform1m,...] [--out profiles/voxel_measurements.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "reps": int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", default="uniform1m,uniform10m,mixture10m,clouds")
    ap.add_argument("--per-voxel", default="1,8,64,1000")
    ap.add_argument("--channels", default="0,3,6")
    ap.add_argument("--sweep", default="uniform10m")
    ap.add_argument("--sweep-rows", default="1,4,8,16,24,32,48,64,128")
    ap.add_argument("--pipeline-size", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_measurements.json"))
    a = ap.parse_args()

    import torch

    import voxel_spec as vs
    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN, global_registration

    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmups": 1, "checks": "ok", "source_fingerprint": _lib.source_fingerprint(),
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "cases": [], "sweep": [], "one_voxel": [], "pipeline": []}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), res

    def packed_key(P, voxel, origin):
        c = torch.floor((P - origin) / voxel).to(torch.int64)
        span = (c.max(dim=0).values + 1).tolist()  # (bin_seeds' one host read)
        return (c[:, 0] * span[1] + c[:, 1]) * span[2] + c[:, 2]

    def recipe(P, values, voxel, origin, batch):
        key = packed_key(P, voxel, origin)
        if batch is not None:
            key = batch.to(torch.int64) * (int(key.max()) + 1) + key
        uniq, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
        rows = P if values is None else torch.cat([P, values], dim=1)
        sums = torch.zeros((uniq.shape[0], rows.shape[1]), dtype=torch.float64, device=P.device).index_add_(0, inverse, rows.double())
        return counts, (sums / counts[:, None].double()).float()

    eng = TrueKNN(device=0)
    sizes = {"uniform1m": 1_000_000, "uniform10m": 10_000_000, "mixture10m": 10_000_000, "clouds": 1024 * 1024}
    for name in [s for s in a.sets.split(",") if s]:
        n = sizes[name]
        if name == "mixture10m":
            P_host, lo = datasets.gaussian_mixture3d(n, components=64, sigma=0.02, seed=1), -0.5
        else:
            P_host, lo = datasets.uniform3d(n, seed=0 if name != "clouds" else 3), 0.0
        P = torch.from_numpy(np.ascontiguousarray(P_host, np.float32)).to(dev)
        batch = torch.arange(1024, dtype=torch.int32, device=dev).repeat_interleave(1024) if name == "clouds" else None
        clouds = 1024 if batch is not None else 1
        origin_t = torch.full((3,), lo, dtype=torch.float32, device=dev)
        all_values = torch.from_numpy(np.random.default_rng(7).random((n, 6), dtype=np.float32)).to(dev)
        for per in [int(x) for x in a.per_voxel.split(",")]:
            if per * 2 > n // clouds:
                continue
            voxel = float(np.float32((per * clouds / n) ** (1.0 / 3.0)))
            voxel_t = torch.tensor(voxel, dtype=torch.float32, device=dev)
            for C in [int(x) for x in a.channels.split(",")]:
                values = None if C == 0 else all_values[:, :C].contiguous()
                kw = dict(values=values, origin=(lo, lo, lo), batch=batch, num_batches=None if batch is None else clouds)
                got = eng.voxel_down_sample(P, voxel, **kw)
                counts, means = recipe(P, values, voxel_t, origin_t, batch)
                info = got["info"]
                mine = got["points"] if C == 0 else torch.cat([got["points"], got["values"]], dim=1)
                ok = bool(torch.equal(counts.to(torch.int32), got["counts"]))
                ulps = int(np.max(vs.ulps_apart(mine[::97].cpu().numpy(), means[::97].cpu().numpy()))) if ok else -1
                if not ok or ulps > 1:
                    rec["checks"] = "MISMATCH at %s per %d C %d (counts equal %s, largest distance %d)" % (name, per, C, ok, ulps)
                    save()
                    sys.exit(rec["checks"])
                V = int(info["voxels"])
                case = {"set": name, "points": n, "clouds": clouds, "rows_per_voxel_aimed": per, "voxel": voxel, "channels": C, "voxels": V, "max_count": info["max_count"],
                        "wave_voxels": info["wave_voxels"], "block_voxels": info["block_voxels"], "means_within_ulps_of_recipe": ulps, "variants": {}}
                del got, counts, means, mine
                key = packed_key(P, voxel_t, origin_t)
                variants = {"voxel_down_sample": lambda: eng.voxel_down_sample(P, voxel, **kw)["info"],
                            "torch_recipe": lambda: recipe(P, values, voxel_t, origin_t, batch) and {},
                            "torch_sort_keys": lambda: torch.sort(key) and {}}
                wall, infos = {v: [] for v in variants}, {v: [] for v in variants}
                for rep in range(a.reps + 1):
                    for v, f in variants.items():
                        ms, res = timed(f)
                        if rep:  # (rep 0: the warm-up)
                            wall[v].append(ms)
                            infos[v].append(res)
                        del res
                for v in variants:
                    entry = {"events_ms": stats(wall[v])}
                    for field in ("key_ms", "sort_ms", "reduce_ms", "solve_ms"):
                        vals = [i[field] for i in infos[v] if field in i]
                        if vals:
                            entry[field] = stats(vals)
                    case["variants"][v] = entry
                call = case["variants"]["voxel_down_sample"]
                floor_bytes = n * (4 + 12 + 4 * C) + V * (4 * (3 + C) + 4) + n * 4  # rows, points and values in; means, counts and the map out
                case["reduce_byte_floor_ms"] = 1e3 * floor_bytes / HBM_BYTES_PER_S
                case["reduce_over_byte_floor"] = call["reduce_ms"]["median"] / case["reduce_byte_floor_ms"]
                case["sort_over_torch_sort"] = call["sort_ms"]["median"] / case["variants"]["torch_sort_keys"]["events_ms"]["median"]
                case["recipe_over_call"] = case["variants"]["torch_recipe"]["events_ms"]["median"] / call["events_ms"]["median"]
                print("%s per %d C %d: V %d, call %.3f ms (key %.3f sort %.3f reduce %.3f), recipe %.3f ms (%.2f x), torch.sort %.3f ms, reduce %.1f x its byte floor"
                      % (name, per, C, V, call["events_ms"]["median"], call["key_ms"]["median"], call["sort_ms"]["median"], call["reduce_ms"]["median"],
                         case["variants"]["torch_recipe"]["events_ms"]["median"], case["recipe_over_call"], case["variants"]["torch_sort_keys"]["events_ms"]["median"],
                         case["reduce_over_byte_floor"]), flush=True)
                rec["cases"].append(case)
                save()
                del key
        # the threshold between a lane and a wave per voxel: reduce_ms at each, same inputs, alternating
        if name in a.sweep.split(","):
            thresholds = [int(x) for x in a.sweep_rows.split(",")]
            for per in (8, 32, 64):
                voxel = float(np.float32((per / n) ** (1.0 / 3.0)))
                for C in (0, 6):
                    values = None if C == 0 else all_values[:, :C].contiguous()
                    reduce_ms = {t: [] for t in thresholds}
                    for rep in range(a.reps + 1):
                        for t in thresholds:
                            os.environ["TKNN_VOXEL_LANE_ROWS"] = str(t)
                            info = eng.voxel_down_sample(P, voxel, values=values, origin=(lo, lo, lo))["info"]
                            if rep:
                                reduce_ms[t].append(info["reduce_ms"])
                            last = info
                    os.environ.pop("TKNN_VOXEL_LANE_ROWS", None)
                    row = {"set": name, "rows_per_voxel_aimed": per, "channels": C, "voxels": last["voxels"], "max_count": last["max_count"],
                           "reduce_ms_by_lane_rows": {str(t): stats(reduce_ms[t]) for t in thresholds}}
                    print("sweep %s per %d C %d:" % (name, per, C), ", ".join("%d: %.3f" % (t, row["reduce_ms_by_lane_rows"][str(t)]["median"]) for t in thresholds), flush=True)
                    rec["sweep"].append(row)
                    save()
        # one voxel for every row: a workgroup's run
        if name in ("uniform1m", "uniform10m"):
            ms, infos = [], []
            for rep in range(a.reps + 1):
                t, info = timed(lambda: eng.voxel_down_sample(P, 2.0, origin=(0, 0, 0))["info"])
                if rep:
                    ms.append(t)
                    infos.append(info)
            rec["one_voxel"].append({"set": name, "points": n, "voxels": infos[0]["voxels"], "block_voxels": infos[0]["block_voxels"], "events_ms": stats(ms),
                                     "reduce_ms": stats([i["reduce_ms"] for i in infos]), "sort_ms": stats([i["sort_ms"] for i in infos])})
            print("one voxel", name, rec["one_voxel"][-1], flush=True)
            save()
        del P, all_values, batch
        torch.cuda.empty_cache()
    eng.close()

    # ---- the pipeline: scripts/global_measurements.py's two views, through a voxel grid that leaves about 20 k points ----
    n = a.pipeline_size
    if n > 0:
        rng = np.random.default_rng(5)
        overlap = 0.7
        spacing = 1.0 / np.sqrt(n)
        wave_dir, wave_k, wave_phase = rng.uniform(0, 2 * np.pi, 24), 2 * np.pi / (spacing * rng.uniform(15, 60, 24)), rng.uniform(0, 2 * np.pi, 24)

        def view(lo):
            xy = rng.random((n, 2))
            x, y = lo + xy[:, 0], xy[:, 1]
            z = 0.15 * np.sin(7.0 * x) * np.cos(5.0 * y) + 0.08 * np.cos(11.0 * y)
            for d, k, ph in zip(wave_dir, wave_k, wave_phase):
                z = z + spacing * np.sin(k * (np.cos(d) * x + np.sin(d) * y) + ph)
            return np.stack([x, y, z], axis=1)

        Pn, Qn = view(0.0), view(1.0 - overlap)
        ang = 0.9
        R0 = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]) @ np.array([[np.cos(0.5), -np.sin(0.5), 0], [np.sin(0.5), np.cos(0.5), 0], [0, 0, 1.0]])
        t0 = np.array([0.2, -0.3, 0.15])
        Sn = (Qn - t0) @ R0
        P, S = torch.from_numpy(Pn.astype(np.float32)).to(dev), torch.from_numpy(Sn.astype(np.float32)).to(dev)
        view_p, view_s = (0.5, 0.5, 5.0), tuple((np.array([1.5 - overlap, 0.5, 5.0]) - t0) @ R0)
        voxel = 0.01  # the bumpy surface of unit area crosses about two cells per column of the grid: about 20 k occupied cells
        runs = []
        for it in range(1 + max(1, a.reps - 1)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = global_registration(P, S, feature_radius=6.0 * voxel, max_dist=1.5 * voxel, seed=1, target_viewpoint=view_p, source_viewpoint=view_s, voxel_size=voxel)
            torch.cuda.synchronize()
            wall = 1e3 * (time.perf_counter() - t)
            T = r["transform"].numpy()
            st = {"total_ms": wall, "target_down": r["target_down"], "source_down": r["source_down"], "pairs": int(len(r["pairs"])), "ransac_inliers": r["ransac"]["inliers"],
                  "ransac_trials": r["ransac"]["trials_run"], "ransac_eval_fitness": r["ransac_eval"]["fitness"], "icp_fitness": r["icp_eval"]["fitness"],
                  "icp_rmse": r["icp_eval"]["inlier_rmse"], "max_error_in_spacings": float(np.linalg.norm(Sn[::97] @ T[:3, :3].T + T[:3, 3] - Qn[::97], axis=1).max() / spacing)}
            if it > 0:
                runs.append(st)
            print("pipeline", it, st, flush=True)
        case = {"points": n, "overlap": overlap, "voxel_size": voxel, "feature_radius": 6.0 * voxel, "max_dist": 1.5 * voxel, "spacing": spacing,
                "without_voxel_size": "profiles/global_measurements.json: 4.07 s, 3 RANSAC inliers"}
        for key in runs[0]:
            case[key] = stats([x[key] for x in runs]) if key.endswith("_ms") else runs[0][key]
        rec["pipeline"].append(case)
        save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
