#!/usr/bin/env python3
"""The absolute screen-gradient statistic (casualhdrsplat_amd.importance.accumulate_abs_gradients, absgrad.hip) next to the
render stage of the backward whose loop it walks again, in one process, the two alternated on the same frame under the same
upstream gradient, medians of device events:

    python scripts/absgrad_timing.py --out profiles/absgrad_timing.json

  1M_1080p     1 M Gaussians, 1920 x 1080, SH degree 3 (bench.py's c3 geometry, one pose, linear radiance)
  100k_800sq   100 k Gaussians, 800 x 800, SH degree 3

  abs_gradient   one accumulate_abs_gradients (three kernels: replay, per-instance sums, fold; the Python call included)
  render_bwd     replay_backward(HS_BWD_RENDER) of the same frame: hs_backward's render stage alone

The replay reduces two values per trip where the backward reduces nine; no time is fixed in advance, the two numbers and the
workspace bytes are recorded side by side.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import (DensifyStats, GaussianRasterizationSettings, GaussianRasterizer, _lib as L,
                                accumulate_abs_gradients, synthetic as S)
from casualhdrsplat_amd.importance import abs_gradient_workspace
from casualhdrsplat_amd.rasterizer import _state_of, replay_backward

SIZES = {"1M_1080p": (1_000_000, 1920, 1080, 3), "100k_800sq": (100_000, 800, 800, 3)}


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
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=sc.bg.to(dev), scale_modifier=1.0,
        viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev), sh_degree=deg, campos=cam.campos.to(dev),
        prefiltered=False, debug=False)
    leaf = {k: getattr(sc, k).to(dev).contiguous().requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    rast = GaussianRasterizer(rs)
    out = rast(leaf["means3D"], torch.zeros(P, 3, device=dev), leaf["opacities"], shs=leaf["shs"], scales=leaf["scales"],
               rotations=leaf["rotations"])
    color = out[0]
    stats = DensifyStats(P, dev, absgrad=True)
    dL = sc.dL_dimage.to(dev).contiguous()
    forms = {"abs_gradient": lambda: accumulate_abs_gradients(color, dL, stats),
             "render_bwd": lambda: replay_backward(color, dL, L.HS_BWD_RENDER)}
    row = alternate(forms, iters, warmup)
    torch.cuda.synchronize()
    row.update(P=P, W=W, H=H, sh_degree=deg, num_rendered=int(rast.check_overflow()),
               gaussians_reached=int((stats.abs_grad_accum > 0).sum()),
               workspace_bytes=int(abs_gradient_workspace(_state_of(color).dims, dev).numel()),
               abs_gradient_over_render_bwd=row["abs_gradient"]["median_ms"] / row["render_bwd"]["median_ms"])
    print(name, json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated subset of: " + ", ".join(SIZES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absgrad_timing.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("absgrad_timing.py measures on the GPU only")
    dev = torch.device("cuda", 0)
    only = set(filter(None, a.only.split(",")))
    res = {"iters": a.iters, "device": torch.cuda.get_device_name(0)}
    for k, (P, W, H, deg) in SIZES.items():
        if not only or k in only:
            res[k] = time_size(k, P, W, H, deg, dev, a.iters, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
