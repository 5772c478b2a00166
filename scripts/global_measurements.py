#!/usr/bin/env python3
"""Times of tknnFeatureMatch and tknnRansac (include/owlknn_global.h) and of the pipeline around them on one MI355X, written to
profiles/global_measurements.json.  Every variant of a case alternates inside every repetition, --reps of them after 1 warm-up, in
one process; median, minimum and maximum of a host clock around the call (each ends in a synchronise) and of the call's own info.

  matcher    --match-sizes rows on both sides, D = 33, rows like an FPFH.
             match          the call; its time over the VALU floor: 3 operations * m * n * D over the fp32 lane rate,
                            256 compute units * 4 SIMDs * 32 lanes * 2.4 GHz (MI355X_MICROARCH: 64 FLOP per clock and SIMD
                            counts a fused multiply-add as two; the distance has none, by definition);
             match_r4       the same with 4 source rows per lane (TKNN_MATCH_ROWS=4) instead of 2;
             match_1chunk   the same with one chunk over all targets (TKNN_MATCH_CHUNK=n): what the chunks buy at small m;
             recipe         chunked torch.cdist + topk(2, largest=False), at most 2^28 distances per chunk.  Above
                            --recipe-rows rows it runs once, without a warm-up of its own.
             Before anything is timed the share of rows on which the recipe names the same best row is recorded.
  ransac     --ransac-sizes pairs, 30 % true, 100 000 trials at confidence 1 and again at the default confidence.
             ransac         the call; survivors per batch from its status counts, sample_ms / score_ms / refit_ms from its info;
             ransac_tile    the same scored by survivors x record chunks, the records broadcast from LDS (TKNN_RANSAC_SCORE=tile)
                            instead of a wave per survivor with its lanes over the records;
             recipe         the same number of trials as batched torch: randint samples, the edge check, linalg.svd on the
                            survivors, scoring by a batched matmul.
  pipeline   global_registration's stages on two views of --pipeline-size points each, timed one by one.

    python scripts/global_measurements.py [--reps 3] [--out profiles/global_measurements.json]
"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANE_RATE = 256 * 4 * 32 * 2.4e9  # fp32 lane operations per second


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "reps": int(len(v))}


@contextlib.contextmanager
def env(**kw):
    before = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--match-sizes", default="10000,100000,1000000")
    ap.add_argument("--recipe-rows", type=int, default=100000)
    ap.add_argument("--ransac-sizes", default="10000,100000")
    ap.add_argument("--pipeline-size", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib
    from owlraytracing_amd.trueknn import TrueKNN

    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "warmups": 1, "reps": a.reps, "source_fingerprint": _lib.source_fingerprint(), "lane_rate": LANE_RATE,
           "matcher": [], "ransac": [], "pipeline": []}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
            json.dump(rec, fh, indent=1)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def alternate(variants, reps, warm=1):
        """variants: name -> (callable, reps or None); every one once per repetition, in turn.  name -> list of (ms, result)."""
        got = {name: [] for name in variants}
        for it in range(warm + reps):
            for name, (fn, own) in variants.items():
                if own is not None and it >= own:
                    continue
                ms, out = timed(fn)
                if it >= warm or own is not None:
                    got[name].append((ms, out))
        return got

    eng = TrueKNN(device=0)

    # ---- matcher ----
    def fpfh_like(rows, seed):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        w = torch.rand((rows, 3, 11), device=dev, generator=g) ** 4
        w[torch.rand((rows, 3, 11), device=dev, generator=g) < 0.5] = 0.0
        w[:, :, 0] += 1e-3
        return (100.0 * w / w.sum(dim=2, keepdim=True)).reshape(rows, 33).contiguous()

    def recipe_match(A, B):
        rows = max(1, (1 << 28) // B.shape[0])
        best = torch.empty((A.shape[0],), dtype=torch.int64, device=dev)
        d12 = torch.empty((A.shape[0], 2), dtype=torch.float32, device=dev)
        for lo in range(0, A.shape[0], rows):
            v, i = torch.topk(torch.cdist(A[lo:lo + rows], B), 2, dim=1, largest=False)
            best[lo:lo + rows], d12[lo:lo + rows] = i[:, 0], v
        return best, d12

    for m in (int(s) for s in a.match_sizes.split(",")):
        A, B = fpfh_like(m, 1), fpfh_like(m, 2)
        ours = eng.match_features(A, B)
        agree = float((recipe_match(A[:20000], B)[0] == ours["best"][:20000].long()).float().mean())
        variants = {"match": (lambda: eng.match_features(A, B)["info"], None)}

        def with_env(**kw):
            def run():
                with env(**kw):
                    return eng.match_features(A, B)["info"]
            return run

        variants["match_r4"] = (with_env(TKNN_MATCH_ROWS=4), None)
        variants["match_1chunk"] = (with_env(TKNN_MATCH_CHUNK=m), None)
        variants["recipe"] = (lambda: recipe_match(A, B) and None, None if m <= a.recipe_rows else 1)
        got = alternate(variants, a.reps)
        floor_ms = 3.0 * m * m * 33 / LANE_RATE * 1e3
        case = {"m": m, "n": m, "D": 33, "floor_ms": floor_ms, "recipe_agrees_on_best": agree, "chunks": ours["info"]["chunks"]}
        for name, runs in got.items():
            case[name] = {"ms": stats([ms for ms, _ in runs])}
            if name != "recipe":
                case[name]["match_ms"] = stats([info["match_ms"] for _, info in runs])
                case[name]["merge_ms"] = stats([info["merge_ms"] for _, info in runs])
                case[name]["chunks"] = runs[0][1]["chunks"]
                case[name]["match_over_floor"] = case[name]["match_ms"]["median"] / floor_ms
        rec["matcher"].append(case)
        save()
        print("matcher", m, {k: (v["ms"]["median"] if isinstance(v, dict) and "ms" in v else v) for k, v in case.items()}, flush=True)
        del A, B, ours

    # ---- ransac ----
    def scene(c, true_share=0.3, noise=1e-3, seed=0):
        rng = np.random.default_rng(seed)
        P = rng.random((c, 3)).astype(np.float32)
        ang = 1.1
        R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, np.cos(0.7), -np.sin(0.7)], [0, np.sin(0.7), np.cos(0.7)]])
        t = np.array([0.3, -0.2, 0.1])
        S = ((P.astype(np.float64) - t) @ R + rng.normal(scale=noise, size=(c, 3))).astype(np.float32)
        pairs = np.stack([np.arange(c), np.arange(c)], axis=1)
        wrong = rng.random(c) >= true_share
        pairs[wrong, 1] = rng.integers(0, c, size=int(wrong.sum()))
        return torch.from_numpy(S).to(dev), torch.from_numpy(P).to(dev), torch.from_numpy(pairs.astype(np.int32)).to(dev)

    def recipe_ransac(S, P, pairs, n, max_dist, sim, trials, batch=4096):
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        s_all, p_all = S[pairs[:, 0].long()], P[pairs[:, 1].long()]
        c = s_all.shape[0]
        best, survivors = 0, 0
        for lo in range(0, trials, batch):
            k = min(batch, trials - lo)
            idx = torch.randint(0, c, (k, n), device=dev, generator=g)
            s, p = s_all[idx], p_all[idx]
            ok = torch.ones((k,), dtype=torch.bool, device=dev)
            for i in range(n):
                for j in range(i + 1, n):
                    ds, dt = (s[:, i] - s[:, j]).norm(dim=1), (p[:, i] - p[:, j]).norm(dim=1)
                    ok &= (idx[:, i] != idx[:, j]) & (ds >= sim * dt) & (dt >= sim * ds)
            s, p = s[ok].double(), p[ok].double()
            if s.shape[0] == 0:
                continue
            mus, mup = s.mean(dim=1, keepdim=True), p.mean(dim=1, keepdim=True)
            U, _, Vh = torch.linalg.svd((s - mus).transpose(1, 2) @ (p - mup))
            V = Vh.transpose(1, 2)
            D = torch.eye(3, dtype=torch.float64, device=dev).repeat(s.shape[0], 1, 1)
            D[:, 2, 2] = torch.sign(torch.linalg.det(V @ U.transpose(1, 2)))
            R = V @ D @ U.transpose(1, 2)
            t = mup.squeeze(1) - (R @ mus.transpose(1, 2)).squeeze(2)
            Rf, tf = R.float(), t.float()
            d = (s.float() @ Rf.transpose(1, 2) + tf[:, None] - p.float()).norm(dim=2)
            keep = (d <= max_dist).all(dim=1)
            Rf, tf = Rf[keep], tf[keep]
            survivors += int(Rf.shape[0])
            if Rf.shape[0] == 0:
                continue
            moved = torch.matmul(Rf, s_all.T[None]) + tf[:, :, None]
            inl = ((moved - p_all.T[None]).norm(dim=1) <= max_dist).sum(dim=1)
            best = max(best, int(inl.max()))  # (the batch's synchronisation, as the call has one)
        return {"inliers": best, "survivors": survivors}

    for c in (int(s) for s in a.ransac_sizes.split(",")):
        S, P, pairs = scene(c)
        for confidence in (1.0, 0.999):
            kw = dict(max_dist=0.02, max_trials=100000, confidence=confidence, seed=1)

            def ours():
                return eng.ransac(S, P, pairs, **kw)

            def tile():
                with env(TKNN_RANSAC_SCORE="tile"):
                    return eng.ransac(S, P, pairs, **kw)

            first = ours()
            variants = {"ransac": (ours, None), "ransac_tile": (tile, None)}
            if confidence == 1.0:
                variants["recipe"] = (lambda: recipe_ransac(S, P, pairs, 3, 0.02, 0.9, 100000), None)
            got = alternate(variants, a.reps)
            case = {"pairs": c, "true_share": 0.3, "confidence": confidence, "trials_run": first["trials_run"], "batches": first["batches"],
                    "status_counts": first["status_counts"], "survivor_share": first["status_counts"]["ok"] / max(first["trials_run"], 1),
                    "inliers": first["inliers"], "fitness": first["fitness"], "refits_kept": first["refits_kept"]}
            for name, runs in got.items():
                case[name] = {"ms": stats([ms for ms, _ in runs])}
                if name == "recipe":
                    case[name]["inliers"], case[name]["survivors"] = runs[0][1]["inliers"], runs[0][1]["survivors"]
                else:
                    for part in ("solve_ms", "sample_ms", "score_ms", "refit_ms"):
                        case[name][part] = stats([r[part] for _, r in runs])
                    assert runs[0][1]["inliers"] == first["inliers"] and runs[0][1]["best_trial"] == first["best_trial"], "the mappings agree"
            rec["ransac"].append(case)
            save()
            print("ransac", c, confidence, {k: (v["ms"]["median"] if isinstance(v, dict) and "ms" in v else v) for k, v in case.items()}, flush=True)

    # ---- pipeline ----
    n = a.pipeline_size
    rng = np.random.default_rng(5)
    overlap = 0.7
    spacing = 1.0 / np.sqrt(n)  # the points' typical distance: the fine bumps are tens of it wide, the radii follow it
    # the fine structure: 24 waves of random direction, phase and length (15 .. 60 spacings), so that no patch repeats
    wave_dir = rng.uniform(0, 2 * np.pi, 24)
    wave_k = 2 * np.pi / (spacing * rng.uniform(15, 60, 24))
    wave_phase = rng.uniform(0, 2 * np.pi, 24)

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
    radius, max_dist = 6.0 * spacing, 3.0 * spacing
    et, es = TrueKNN(device=0), TrueKNN(device=0)
    runs = []
    for it in range(1 + max(1, a.reps - 1)):
        st = {}
        st["build_ms"], _ = timed(lambda: (et.build(P), es.build(S)))
        st["normals_ms"], nn = timed(lambda: (et.normals(k=16, viewpoint=view_p)["normals"], es.normals(k=16, viewpoint=view_s)["normals"]))
        st["fpfh_ms"], ff = timed(lambda: (et.fpfh(radius, normals=nn[0])["fpfh"], es.fpfh(radius, normals=nn[1])["fpfh"]))
        st["match_ms"], match = timed(lambda: es.match_features(ff[1], ff[0], mutual=True))
        st["ransac_ms"], rs = timed(lambda: es.ransac(S, P, match["pairs"], max_dist, seed=1))
        st["icp_ms"], ic = timed(lambda: et.icp(S, max_dist, init=rs["transform"]))
        st["total_ms"] = sum(st.values())
        T = ic["transform"].numpy()
        st.update(pairs=int(match["pairs"].shape[0]), ransac_trials=rs["trials_run"], ransac_fitness=rs["fitness"], ransac_inliers=rs["inliers"],
                  icp_fitness=ic["fitness"], icp_rmse=ic["inlier_rmse"], icp_iterations=ic["iterations"],
                  max_error_in_spacings=float(np.linalg.norm(Sn[::97] @ T[:3, :3].T + T[:3, 3] - Qn[::97], axis=1).max() / spacing))
        if it > 0:
            runs.append(st)
        print("pipeline", it, st, flush=True)
    case = {"points": n, "overlap": overlap, "feature_radius": radius, "max_dist": max_dist, "spacing": spacing}
    for name in runs[0]:
        case[name] = stats([r[name] for r in runs]) if name.endswith("_ms") else runs[0][name]
    rec["pipeline"].append(case)
    save()


if __name__ == "__main__":
    main()
