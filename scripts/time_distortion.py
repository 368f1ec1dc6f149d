#!/usr/bin/env python3
"""The depth-distortion loss (distortion.distortion_loss, distort.hip) next to the feature compositing whose walks it
repeats, in one process, the forms alternated on the same frame, medians of device events:

    python scripts/time_distortion.py --out profiles/distortion_timing.json

  1M_1080p     1 M Gaussians, 1920 x 1080, SH degree 3 (bench.py's c3 geometry, one pose, linear radiance)
  100k_800sq   100 k Gaussians, 800 x 800, SH degree 3

  distortion_forward           hs_distortion: one front-to-back replay, two planes written
  features_forward_C4          hs_composite_features at C = 4 on the same frame: the same walk with four channels
  distortion_backward          hs_distortion_backward, the whole call: replay, segmented sum, projection
  features_geometry_backward_C4  hs_composite_features_geometry_backward at C = 4, the whole call
  render_fwd / render_bwd      replay_forward(HS_STAGE_RENDER) and hs_backward's render stage of that frame, for scale

and the byte model beside them: the forward writes 2 planes and reads at most pairs x 64 B of records (an instance's 48-byte
record once per tile it is staged in, plus its point_list word and pair_act byte); the backward writes and reads the 64-byte
pair records once, plus the flags.
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
                                distortion as D, distortion_loss, features as F, synthetic as S)
from casualhdrsplat_amd.rasterizer import replay_backward, replay_forward

SIZES = {"1M_1080p": (1_000_000, 1920, 1080, 3), "100k_800sq": (100_000, 800, 800, 3)}
KEYS = ("means3D", "opacities", "scales", "rotations")
FWD_ALLOWED, BWD_ALLOWED = 1.15, 1.25      # the margins the forward and the backward were given against the C = 4 compositing


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


def time_size(name, P, W, H, deg, dev, iters, warmup):
    sc = S.make_scene(P, W, H, deg, seed=0)
    cam = sc.camera
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev), scale_modifier=1.0,
        viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev), sh_degree=deg, campos=cam.campos.to(dev),
        prefiltered=False, debug=False)
    geo = {k: getattr(sc, k).to(dev).contiguous().requires_grad_(True) for k in KEYS}
    rast = GaussianRasterizer(rs)
    shs = sc.shs.to(dev).contiguous().requires_grad_(True)
    color = rast(geo["means3D"], torch.zeros(P, 3, device=dev), geo["opacities"], shs=shs, scales=geo["scales"],
                 rotations=geo["rotations"])[0]
    pairs = int(rast.check_overflow())
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    feat = torch.randn(P, 4, device=dev, generator=g)
    dL4 = torch.randn(1, 4, H, W, device=dev, generator=g)
    dL3 = torch.randn(3, H, W, device=dev, generator=g)
    gamma = torch.randn(1, H, W, device=dev, generator=g)
    fnode = composite_features(color, feat, geometry=geo).grad_fn
    dnode = distortion_loss(color, geo).grad_fn
    st = dnode.st
    forms = {
        "distortion_forward": lambda: D._distortion_forward(st),
        "features_forward_C4": lambda: F._features_forward(st, feat),
        "distortion_backward": lambda: D._distortion_backward(st, dnode.geo, dnode.moment, gamma),
        "features_geometry_backward_C4": lambda: F._geometry_backward(st, fnode.geo, fnode.features, dL4),
        "render_fwd": lambda: replay_forward(color, L.HS_STAGE_RENDER),
        "render_bwd": lambda: replay_backward(color, dL3, L.HS_BWD_RENDER),
    }
    r = alternate(forms, iters, warmup)
    row = dict(P=P, W=W, H=H, sh_degree=deg, num_rendered=pairs, **r)
    row["forward_over_features_C4"] = r["distortion_forward"]["median_ms"] / r["features_forward_C4"]["median_ms"]
    row["backward_over_features_geometry_C4"] = r["distortion_backward"]["median_ms"] / r["features_geometry_backward_C4"]["median_ms"]
    row["forward_within_margin"] = row["forward_over_features_C4"] <= FWD_ALLOWED
    row["backward_within_margin"] = row["backward_over_features_geometry_C4"] <= BWD_ALLOWED
    row["byte_model"] = dict(
        forward_written=2 * 4 * H * W, forward_read_at_most=64 * pairs,
        backward_records_written_and_read_at_most=2 * 64 * pairs, backward_flags=2 * pairs,
        forward_GBps_at_most=(2 * 4 * H * W + 64 * pairs) / r["distortion_forward"]["median_ms"] / 1e6,
        backward_GBps_at_most=(2 * 64 * pairs + 2 * pairs + 64 * pairs) / r["distortion_backward"]["median_ms"] / 1e6)
    print(name, json.dumps(row), flush=True)
    torch.cuda.synchronize()
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated subset of: " + ", ".join(SIZES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_timing.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_distortion.py measures on the GPU only")
    dev = torch.device("cuda", 0)
    only = set(filter(None, a.only.split(",")))
    res = dict(device=torch.cuda.get_device_name(0), iters=a.iters, library=os.path.basename(L.LIB_PATH),
               margins=dict(forward=FWD_ALLOWED, backward=BWD_ALLOWED))
    for k, (P, W, H, deg) in SIZES.items():
        if not only or k in only:
            res[k] = time_size(k, P, W, H, deg, dev, a.iters, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
