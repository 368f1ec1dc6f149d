#!/usr/bin/env python3
"""Fused L1 + D-SSIM loss (casualhdrsplat_amd.losses.photometric_loss) against the published torch formulation (five grouped
11 x 11 convolutions through MIOpen and the element-wise glue), forward + backward, both eager, alternated in one process.

    python scripts/time_loss.py --iters 300 --out profiles/photometric_loss_timing.json

Device events around each forward + backward; medians over --iters iterations after a warm-up that also runs MIOpen's
first-call tuning.  Sizes: 800 x 800 x 3 (BASELINE c2) and 1920 x 1080 x 3 (c3).  The per-kernel split comes from a separate
`rocprofv3 --kernel-trace --stats` run of this script (--fused-only)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

import loss_reference as R
from casualhdrsplat_amd import photometric_loss

SIZES = {"c2": (3, 800, 800), "c3": (3, 1080, 1920)}
LAMBDA = 0.2


def torch_step(x, y, win):
    import torch.nn.functional as F
    xx = x.unsqueeze(0)
    yy = y.unsqueeze(0)
    ch = x.shape[0]

    def conv(t):
        return F.conv2d(t, win, padding=R.WIN // 2, groups=ch)
    mu1, mu2 = conv(xx), conv(yy)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = conv(xx * xx) - mu1_sq
    s2 = conv(yy * yy) - mu2_sq
    s12 = conv(xx * yy) - mu1_mu2
    m = ((2 * mu1_mu2 + R.C1) * (2 * s12 + R.C2)) / ((mu1_sq + mu2_sq + R.C1) * (s1 + s2 + R.C2))
    loss = (1.0 - LAMBDA) * (x - y).abs().mean() + LAMBDA * (1.0 - m.mean())
    loss.backward()


def fused_step(x, y):
    photometric_loss(x, y, LAMBDA).backward()


def time_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--fused-only", action="store_true", help="run only the fused loss (for the kernel-trace run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"lambda_dssim": LAMBDA, "iters": a.iters, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for name, shape in SIZES.items():
        g = torch.Generator().manual_seed(0)
        x = torch.rand(shape, generator=g).cuda().requires_grad_(True)
        y = torch.rand(shape, generator=g).cuda()
        win = R.window_2d(shape[0], torch.float32).cuda()
        fns = {"fused": lambda: fused_step(x, y)}
        if not a.fused_only:
            fns["torch"] = lambda: torch_step(x, y, win)
        for _ in range(a.warmup):                 # (also MIOpen's first-call tuning of the grouped convolutions)
            for fn in fns.values():
                x.grad = None
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.iters):
            for k, fn in fns.items():            # alternated: both see the same clocks and neighbours
                x.grad = None
                t[k].append(time_once(fn))
        row = {k: {"median_ms": statistics.median(v), "p10_ms": sorted(v)[len(v) // 10], "p90_ms": sorted(v)[9 * len(v) // 10]}
               for k, v in t.items()}
        if "torch" in row:
            row["speedup"] = row["torch"]["median_ms"] / row["fused"]["median_ms"]
        plane = shape[1] * shape[2] * shape[0] * 4
        row["bytes_floor_mb"] = 11 * plane / 1e6      # forward reads 2 planes, writes 3; backward reads 5, writes 1
        res["sizes"][name] = {"shape": list(shape), **row}
        print(name, json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
