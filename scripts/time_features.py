#!/usr/bin/env python3
"""The per-Gaussian feature compositing (casualhdrsplat_amd.features, features.hip) next to what a user had before it and
next to the render forward it replays, in one process, the forms alternated on the same frame, medians of device events:

    python scripts/time_features.py --out profiles/features_timing.json [--label shipped]

  1M_1080p     1 M Gaussians, 1920 x 1080, SH degree 3 (bench.py's c3 geometry, one pose, linear radiance)
  100k_800sq   100 k Gaussians, 800 x 800, SH degree 3
  C            3 and 16 channels

  forward          one composite_features (one kernel; the Python call included)
  backward         its backward (three kernels per backward pass of channels; through autograd)
  baseline_fwd     ceil(C / 3) GaussianRasterizer forwards with colors_precomp = features[:, 3 j : 3 j + 3] under no_grad:
                   preprocess + binning + sorts + render each
  baseline_fwd_bwd the same forwards with grad and their backwards, colors_precomp the only leaf that asks for a gradient
  render_fwd       replay_forward(HS_STAGE_RENDER) of the same frame, for scale

The library picks the forward's channel group (4, 8 or 16) and the backward's record width (16 or 32 bytes) per call from C.
A/B of one fixed choice: build a variant library (make -C casualhdrsplat_amd/csrc variant NAME=featg16 TUS=features
DEFS=-DHS_TUNE_FEAT_GROUP=16; -DHS_TUNE_FEAT_REC=4 or 8 for 16- or 32-byte backward records in every pass), select it with
HS_LIB_PATH and give the run a --label: the rows of every label are kept side by side in the output file (--no-baseline
skips the rasterizer forms, which do not depend on the variant).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import (GaussianRasterizationSettings, GaussianRasterizer, _lib as L, composite_features,
                                synthetic as S)
from casualhdrsplat_amd.rasterizer import replay_forward

SIZES = {"1M_1080p": (1_000_000, 1920, 1080, 3), "100k_800sq": (100_000, 800, 800, 3)}
CHANNELS = (3, 16)


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


def time_size(name, P, W, H, deg, dev, iters, warmup, baseline):
    sc = S.make_scene(P, W, H, deg, seed=0)
    cam = sc.camera
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=sc.bg.to(dev), scale_modifier=1.0,
        viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev), sh_degree=deg, campos=cam.campos.to(dev),
        prefiltered=False, debug=False)
    geo = {k: getattr(sc, k).to(dev).contiguous() for k in ("means3D", "opacities", "scales", "rotations")}
    means2D = torch.zeros(P, 3, device=dev)
    rast = GaussianRasterizer(rs)
    shs = sc.shs.to(dev).contiguous().requires_grad_(True)
    color = rast(geo["means3D"], means2D, geo["opacities"], shs=shs, scales=geo["scales"], rotations=geo["rotations"])[0]
    row = dict(P=P, W=W, H=H, sh_degree=deg, num_rendered=int(rast.check_overflow()))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for C in CHANNELS:
        feat = torch.randn(P, C, device=dev, generator=g).requires_grad_(True)
        dL = torch.randn(1, C, H, W, device=dev, generator=g)
        held = composite_features(color, feat)
        forms = {"forward": lambda: composite_features(color, feat),
                 "backward": lambda: torch.autograd.grad(held, feat, dL, retain_graph=True),
                 "render_fwd": lambda: replay_forward(color, L.HS_STAGE_RENDER)}
        if baseline:
            n = (C + 2) // 3
            cols = [torch.nn.functional.pad(feat.detach(), (0, 3 * n - C))[:, 3 * j:3 * j + 3].contiguous().requires_grad_(True)
                    for j in range(n)]
            dL3 = torch.randn(3, H, W, device=dev, generator=g)
            brast = GaussianRasterizer(rs)

            def base(grad):
                with torch.enable_grad() if grad else torch.no_grad():
                    for c in cols:
                        o = brast(geo["means3D"], means2D, geo["opacities"], colors_precomp=c, scales=geo["scales"],
                                  rotations=geo["rotations"])[0]
                        if grad:
                            torch.autograd.grad(o, c, dL3)

            forms["baseline_fwd"] = lambda: base(False)
            forms["baseline_fwd_bwd"] = lambda: base(True)
        r = alternate(forms, iters, warmup)
        r["baseline_passes"] = (C + 2) // 3
        # the traffic that scales with C: out written / dL_dout read once, the feature rows of every staged entry read
        r["image_bytes"] = 4 * C * H * W
        if baseline:
            r["forward_speedup"] = r["baseline_fwd"]["median_ms"] / r["forward"]["median_ms"]
            r["forward_backward_speedup"] = r["baseline_fwd_bwd"]["median_ms"] / (r["forward"]["median_ms"] + r["backward"]["median_ms"])
        row[f"C{C}"] = r
        print(name, f"C={C}", json.dumps(r), flush=True)
    torch.cuda.synchronize()
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated subset of: " + ", ".join(SIZES))
    ap.add_argument("--label", default="shipped", help="the name of this library's rows in the output file")
    ap.add_argument("--no-baseline", action="store_true", help="skip the rasterizer forms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_timing.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_features.py measures on the GPU only")
    dev = torch.device("cuda", 0)
    only = set(filter(None, a.only.split(",")))
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    rows = res.setdefault("variants", {}).setdefault(a.label, {})
    rows["iters"] = a.iters
    rows["library"] = os.path.basename(L.LIB_PATH)
    for k, (P, W, H, deg) in SIZES.items():
        if not only or k in only:
            rows[k] = time_size(k, P, W, H, deg, dev, a.iters, a.warmup, not a.no_baseline)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
