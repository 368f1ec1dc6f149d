#!/usr/bin/env python3
"""The fused 3-nearest-neighbour distances (casualhdrsplat_amd.knn_mean_dist2: six kernels around four radix passes, one
host read of the status word) against the host path a cloud on the GPU would otherwise take (device -> host copy of the
points, scipy's k-d tree in float64 with 16 workers, host -> device copy of the result), on the same points.

    python scripts/time_knn.py --out profiles/knn_timing.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_knn.py --gpu-only --sizes 1000000 --clouds sfm
    python scripts/time_knn.py --fold-kernel-stats DIR/*/*kernel_stats.csv --out profiles/knn_timing.json

Sizes 100 k and 1 M points, uniform-random and the reconstruction-like mixture of tests/knn_reference.sfm_like (thin noisy
surfaces of uneven density, 2 % sparse outliers).  GPU: device events around the call (which includes its one wait), the
median and p10 / p90 of --iters runs after a warm-up.  Host: a host clock around copy + tree + query + copy, the median of
--host-iters runs.  Once each, at 100 k points, two clouds on which the boxes prune little: a dense shell around a dense
core, and a cloud with ONE far outlier that stretches the bounding box until the 10-bit Morton grid no longer resolves it
(DESIGN.md section 4.19).  The per-kernel split comes from the separate kernel-trace run, folded in afterwards."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import knn_reference as R
from casualhdrsplat_amd import knn_mean_dist2


def shell_core(P, seed=0):
    """Half the points in a ball of radius 0.05, half on a sphere of radius 1 around it (noise 1e-3)."""
    g = np.random.default_rng(seed)
    d = g.normal(size=(P // 2, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    shell = d * (1.0 + g.normal(0, 1e-3, (len(d), 1)))
    core = g.normal(0, 0.05 / 3, (P - len(d), 3))
    x = np.concatenate([core, shell]).astype(np.float32)
    return x[g.permutation(P)]


def far_outlier(P, seed=0):
    """A uniform unit cube and one point 4000 cube sides away: the cube falls into a single Morton cell."""
    x = R.uniform(P, seed)
    x[0] = 4000.0
    return x


CLOUDS = {"uniform": lambda P: R.uniform(P, seed=1), "sfm": lambda P: R.sfm_like(P, seed=1)}
CLIFFS = {"shell_core": shell_core, "far_outlier": far_outlier}


def time_gpu(x, iters, warmup):
    ms = []
    for it in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = knn_mean_dist2(x)
        b.record()
        b.synchronize()
        if it >= warmup:
            ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": statistics.median(ms), "p10_ms": ms[len(ms) // 10], "p90_ms": ms[9 * len(ms) // 10]}, out


def time_host(x, iters):
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None, None
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = x.cpu().numpy().astype(np.float64)
        d, _ = cKDTree(h).query(h, k=4, workers=16)
        out = torch.from_numpy(np.mean(d[:, 1:] ** 2, axis=1).astype(np.float32)).to(x.device)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "runs": len(ms), "workers": 16}, out


def fold_kernel_stats(path, out):
    rows = list(csv.DictReader(open(path)))
    mine = [r for r in rows if "knn_" in r["Name"] or "radix_" in r["Name"]]
    total = sum(float(r["TotalDurationNs"]) for r in mine)
    split = {r["Name"].replace("hs::(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]: {
        "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "share": float(r["TotalDurationNs"]) / total} for r in mine}
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["kernel_split_1M_sfm"] = split
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(split, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--clouds", default="uniform,sfm")
    ap.add_argument("--cliff-points", type=int, default=100_000)
    ap.add_argument("--gpu-only", action="store_true", help="run only the GPU path of --sizes x --clouds (for the kernel-trace run)")
    ap.add_argument("--fold-kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a --gpu-only run: add the split to --out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.fold_kernel_stats:
        return fold_kernel_stats(a.fold_kernel_stats, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("time_knn.py measures on the GPU only")
    res = {"iters": a.iters, "device": torch.cuda.get_device_name(0), "cases": {}, "cliff": {}}
    if a.out and os.path.exists(a.out):                        # (keep a kernel split folded in earlier)
        res = {**json.load(open(a.out)), **res}
    for P in [int(s) for s in a.sizes.split(",")]:
        for name in a.clouds.split(","):
            x = torch.from_numpy(CLOUDS[name](P)).cuda()
            row = {"P": P, "cloud": name}
            row["gpu"], got = time_gpu(x, a.iters, a.warmup)
            if not a.gpu_only:
                row["host"], ref = time_host(x, a.host_iters)
                if row["host"]:
                    row["host_over_gpu"] = row["host"]["median_ms"] / row["gpu"]["median_ms"]
                    rel = ((got.double() - ref.double()).abs() / ref.double().clamp_min(1e-30)).max()
                    row["max_rel_difference"] = float(rel)     # fp32 distances against float64's, not a bit comparison
            res["cases"][f"{name}_{P}"] = row
            print(f"{name}_{P}", json.dumps(row), flush=True)
    if not a.gpu_only:
        for name, make in CLIFFS.items():
            x = torch.from_numpy(make(a.cliff_points)).cuda()
            row = {"P": a.cliff_points, "cloud": name}
            row["gpu"], _ = time_gpu(x, 3, 1)
            res["cliff"][name] = row
            print(name, json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
