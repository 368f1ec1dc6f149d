#!/usr/bin/env python3
"""The fused Adam step (casualhdrsplat_amd.optim.GaussianAdam) against torch.optim.Adam on the same five cloud tensors,
alternated in one process.

    python scripts/time_adam.py --iters 300 --out profiles/adam_timing.json

Sizes: c3 (1 M Gaussians, SH degree 3) and c2 (100 k, SH degree 0).  Candidates: GaussianAdam dense; sparse at visible
fractions 1.0 / 0.5 / 0.1 with random rows (the worst case for locality) and with one contiguous block; torch.optim.Adam
fused=True, foreach=True and the default.  Device events around each step; medians and p10 / p90 over --iters iterations
after a warm-up.  Effective bytes = 28 B x touched elements + mask bytes.  The per-kernel split comes from a separate
`rocprofv3 --kernel-trace --stats` run of this script (--fused-only)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import GaussianAdam, cloud_param_groups

SIZES = {"c3": (1_000_000, 16), "c2": (100_000, 1)}
WIDTHS = lambda M: (3, 1, 3 * M, 3, 4)          # noqa: E731  means3D, opacities, shs, scales, rotations
PEAK, COPY = 8.0e12, 6.29e12


def make_cloud(P, M, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = ((P, 3), (P, 1), (P, M, 3), (P, 3), (P, 4))
    ts = [torch.randn(s, generator=g).cuda().requires_grad_(True) for s in shapes]
    flat = torch.randn(sum(t.numel() for t in ts), generator=g).cuda()      # gradients: views of one flat buffer
    off = 0
    for t in ts:
        t.grad = flat[off:off + t.numel()].view(t.shape)
        off += t.numel()
    return ts


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
    ap.add_argument("--fused-only", action="store_true", help="run only GaussianAdam (for the kernel-trace run)")
    ap.add_argument("--sizes", default="c3,c2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"iters": a.iters, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for name in a.sizes.split(","):
        P, M = SIZES[name]
        per_row = sum(WIDTHS(M))
        fns, touched = {}, {}

        def ours(vis=None):
            opt = GaussianAdam(cloud_param_groups(*make_cloud(P, M, 1)), eps=1e-15)
            return lambda: opt.step(visibility=vis)

        fns["fused_dense"], touched["fused_dense"] = ours(), (P, 0)
        g = torch.Generator().manual_seed(7)
        for frac in (1.0, 0.5, 0.1):
            rnd = (torch.rand(P, generator=g) < frac) if frac < 1.0 else torch.ones(P, dtype=torch.bool)
            blk = torch.arange(P) < int(frac * P)
            for kind, mask in (("random", rnd), ("block", blk)):
                radii = (mask.to(torch.int32) * 5).cuda()           # what the forward hands over: int32 radii
                key = f"fused_sparse_{frac}_{kind}"
                fns[key], touched[key] = ours(radii), (int(mask.sum()), 4 * P)
        if not a.fused_only:
            for key, kw in (("torch_fused", dict(fused=True)), ("torch_foreach", dict(foreach=True)), ("torch_default", {})):
                ts = make_cloud(P, M, 1)
                lrs = (0.00016, 0.05, 0.0025, 0.005, 0.001)
                opt = torch.optim.Adam([dict(params=[t], lr=lr) for t, lr in zip(ts, lrs)], eps=1e-15, **kw)
                fns[key], touched[key] = opt.step, (P, 0)
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.iters):
            for k, fn in fns.items():            # alternated: all see the same clocks and neighbours
                t[k].append(time_once(fn))
        row = {}
        for k, v in t.items():
            v = sorted(v)
            med = statistics.median(v)
            rows, mask_bytes = touched[k]
            nbytes = 28 * rows * per_row + mask_bytes
            row[k] = {"median_ms": med, "p10_ms": v[len(v) // 10], "p90_ms": v[9 * len(v) // 10], "effective_mb": nbytes / 1e6,
                      "frac_of_8TBps": nbytes / (med * 1e-3) / PEAK, "frac_of_copy_rate": nbytes / (med * 1e-3) / COPY}
        res["sizes"][name] = {"P": P, "M": M, "floats_per_gaussian": per_row, **row}
        for k, v in row.items():
            print(name, k, json.dumps(v), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
