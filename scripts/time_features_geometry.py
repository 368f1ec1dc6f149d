#!/usr/bin/env python3
"""The geometry gradients through the composited feature channels (features.composite_features(..., geometry=...),
featgeo.hip) next to what delivered them before -- ceil(C / 3) colors_precomp rasterizer passes, forward and backward -- and
next to the features-only backward, in one process, the forms alternated on the same frame, medians of device events:

    python scripts/time_features_geometry.py --out profiles/features_geometry_timing.json [--label shipped]

  1M_1080p     1 M Gaussians, 1920 x 1080, SH degree 3 (bench.py's c3 geometry, one pose, linear radiance)
  100k_800sq   100 k Gaussians, 800 x 800, SH degree 3
  C            3 and 16 channels

  fwd_bwd_geometry       composite_features(out, features, geometry=...) and its backward to the features and the four
                         geometry tensors (through autograd, the Python calls included)
  fwd_bwd_features_only  composite_features(out, features) and its backward to the features
  geometry_backward      the geometry half alone: the replay passes, the segmented sum, the projection
  baseline_fwd_bwd       ceil(C / 3) GaussianRasterizer forwards with colors_precomp = features[:, 3 j : 3 j + 3] and their
                         backwards to the colours AND the four geometry tensors (what the parent commit offers)
  abs_gradient           accumulate_abs_gradients on the same frame (absgrad.hip: replay + segmented sum + fold), for scale

The kernels alone (--kernels): a few calls of the geometry backward and of accumulate_abs_gradients, to be run under
`rocprofv3 --kernel-trace --stats`; --merge-kernel-stats FILE.csv then puts the average times of featgeo_replay_kernel and
absgrad_replay_kernel (and the other kernels of the two calls) into the output file.

A/B of the channels per pass: build a variant library (make -C casualhdrsplat_amd/csrc variant NAME=geo8 TUS=featgeo
DEFS=-DHS_TUNE_GEO_PASS=8), select it with HS_LIB_PATH, give the run a --label and --no-baseline: the rows of every label
are kept side by side in the output file.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import (GaussianRasterizationSettings, GaussianRasterizer, _lib as L, accumulate_abs_gradients,
                                composite_features, features as F, synthetic as S)

SIZES = {"1M_1080p": (1_000_000, 1920, 1080, 3), "100k_800sq": (100_000, 800, 800, 3)}
CHANNELS = (3, 16)
KEYS = ("means3D", "opacities", "scales", "rotations")
KERNELS = ("featgeo_replay_kernel", "featgeo_segsum_kernel", "preprocess_bwd_kernel", "absgrad_replay_kernel",
           "absgrad_segsum_kernel", "absgrad_fold_kernel")


def time_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(v):
    v = sorted(v)
    return {"median_ms": statistics.median(v), "p10_ms": v[len(v) // 10], "p90_ms": v[9 * len(v) // 10], "n": len(v)}


def alternate(forms, iters, warmup):
    times = {k: [] for k in forms}
    for it in range(warmup + iters):
        for k, fn in forms.items():          # alternated: every form sees the same clocks and the same neighbours
            ms = time_once(fn)
            if it >= warmup:
                times[k].append(ms)
    return {k: summary(v) for k, v in times.items()}


def frame(P, W, H, deg, dev):
    sc = S.make_scene(P, W, H, deg, seed=0)
    cam = sc.camera
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev), scale_modifier=1.0,
        viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev), sh_degree=deg, campos=cam.campos.to(dev),
        prefiltered=False, debug=False)
    geo = {k: getattr(sc, k).to(dev).contiguous().requires_grad_(True) for k in KEYS}
    means2D = torch.zeros(P, 3, device=dev)
    rast = GaussianRasterizer(rs)
    shs = sc.shs.to(dev).contiguous().requires_grad_(True)
    color = rast(geo["means3D"], means2D, geo["opacities"], shs=shs, scales=geo["scales"], rotations=geo["rotations"])[0]
    return rs, geo, means2D, rast, color


def time_size(name, P, W, H, deg, dev, iters, warmup, baseline, kernels_only):
    rs, geo, means2D, rast, color = frame(P, W, H, deg, dev)
    row = dict(P=P, W=W, H=H, sh_degree=deg, num_rendered=int(rast.check_overflow()))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    wrt = [geo[k] for k in KEYS]
    for C in CHANNELS:
        feat = torch.randn(P, C, device=dev, generator=g).requires_grad_(True)
        dL = torch.randn(1, C, H, W, device=dev, generator=g)
        dL3 = torch.randn(3, H, W, device=dev, generator=g)
        held = composite_features(color, feat, geometry=geo)
        node = held.grad_fn
        accum = torch.zeros(P, device=dev)
        geometry_backward = lambda: F._geometry_backward(node.st, node.geo, node.features, dL)
        abs_gradient = lambda: accumulate_abs_gradients(color, dL3, accum)
        if kernels_only:
            for _ in range(warmup + iters):
                geometry_backward()
                abs_gradient()
            torch.cuda.synchronize()
            continue

        def with_geometry():
            out = composite_features(color, feat, geometry=geo)
            torch.autograd.grad(out, [feat] + wrt, dL)

        def features_only():
            out = composite_features(color, feat)
            torch.autograd.grad(out, feat, dL)

        forms = {"fwd_bwd_geometry": with_geometry, "fwd_bwd_features_only": features_only,
                 "geometry_backward": geometry_backward, "abs_gradient": abs_gradient}
        if baseline:
            n = (C + 2) // 3
            cols = [torch.nn.functional.pad(feat.detach(), (0, 3 * n - C))[:, 3 * j:3 * j + 3].contiguous().requires_grad_(True)
                    for j in range(n)]
            brast = GaussianRasterizer(rs)

            def base():
                for c in cols:
                    o = brast(geo["means3D"], means2D, geo["opacities"], colors_precomp=c, scales=geo["scales"],
                              rotations=geo["rotations"])[0]
                    torch.autograd.grad(o, [c] + wrt, dL3)

            forms["baseline_fwd_bwd"] = base
        r = alternate(forms, iters, warmup)
        r["baseline_passes"] = (C + 2) // 3
        if baseline:
            r["speedup_over_baseline"] = r["baseline_fwd_bwd"]["median_ms"] / r["fwd_bwd_geometry"]["median_ms"]
        r["cost_over_features_only"] = r["fwd_bwd_geometry"]["median_ms"] / r["fwd_bwd_features_only"]["median_ms"]
        row[f"C{C}"] = r
        print(name, f"C={C}", json.dumps(r), flush=True)
    torch.cuda.synchronize()
    return row


def merge_kernel_stats(path):
    """{kernel: {calls, average_us}} of the kernels of the two calls, from a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "").replace("hs::(anonymous namespace)::", "").split("(")[0]   # (keeps the template arguments)
            if any(k in name for k in KERNELS):
                e = out.setdefault(name.replace("void ", ""), {"calls": 0, "total_us": 0.0})
                e["calls"] += int(r["Calls"])
                e["total_us"] += float(r["TotalDurationNs"]) / 1e3
    for e in out.values():
        e["average_us"] = e.pop("total_us") / max(e["calls"], 1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated subset of: " + ", ".join(SIZES))
    ap.add_argument("--label", default="shipped", help="the name of this library's rows in the output file")
    ap.add_argument("--no-baseline", action="store_true", help="skip the rasterizer passes")
    ap.add_argument("--kernels", action="store_true", help="only run the two calls (for a rocprofv3 kernel trace); writes nothing")
    ap.add_argument("--merge-kernel-stats", default="", help="a rocprofv3 kernel_stats.csv of a --kernels run: needs no GPU")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_geometry_timing.json"))
    a = ap.parse_args(argv)
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.merge_kernel_stats:
        res.setdefault("kernels", {})[a.label] = dict(
            note="rocprofv3 --kernel-trace --stats over a --kernels run: every size and C of the run together; "
                 "featgeo_replay_kernel runs once per pass of channels", only=a.only, kernels=merge_kernel_stats(a.merge_kernel_stats))
    else:
        if not torch.cuda.is_available():
            raise SystemExit("time_features_geometry.py measures on the GPU only")
        dev = torch.device("cuda", 0)
        only = set(filter(None, a.only.split(",")))
        res["device"] = torch.cuda.get_device_name(0)
        rows = {} if a.kernels else res.setdefault("variants", {}).setdefault(a.label, {})
        rows["iters"] = a.iters
        rows["library"] = os.path.basename(L.LIB_PATH)
        for k, (P, W, H, deg) in SIZES.items():
            if not only or k in only:
                rows[k] = time_size(k, P, W, H, deg, dev, a.iters, a.warmup, not a.no_baseline, a.kernels)
        if a.kernels:
            return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
