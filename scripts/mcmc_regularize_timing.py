#!/usr/bin/env python3
"""The fused MCMC regularisers (casualhdrsplat_amd.regularize) against the torch formulation a trainer writes without them,

    (lambda_o * torch.sigmoid(raw_opacities).mean() + lambda_s * torch.exp(log_scales).mean()).backward()

onto leaves that already hold a gradient (the state after the rasterizer's backward: autograd ADDS), alternated in one
process on the same inputs.

    python scripts/mcmc_regularize_timing.py --iters 200 --out profiles/mcmc_regularize_timing.json

Sizes: 1 M and 100 k Gaussians.  Device events around each call on the current stream, medians and p10 / p90 over --iters
iterations after a warm-up.  Three fused forms are timed: with the two terms (two launches and the allocation of the [2]
result and the workspace), without (value=False: one launch), and the bare hs_mcmc_regularize call on preallocated buffers.
The kernel moves 48 bytes per Gaussian (opacity, three scales and their four gradients read, the four gradients written):
reported as a share of the 6.29 TB/s copy rate.  Both sides leave the gradient growing by the same term per iteration; the
values do not matter to the time."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import GaussianAdam, _lib as L, cloud_param_groups, regularize

SIZES = {"1M": 1_000_000, "100k": 100_000}
NAMES = ("means3D", "opacities", "shs", "scales", "rotations")
COPY = 6.29e12
LAMBDA_O = LAMBDA_S = 0.01


def make_cloud(P, seed):
    g = torch.Generator().manual_seed(seed)
    cloud = dict(means3D=torch.randn(P, 3, generator=g), opacities=1.0 + 2.0 * torch.randn(P, 1, generator=g),
                 shs=torch.randn(P, 1, 3, generator=g), scales=math.log(0.02) + 0.7 * torch.randn(P, 3, generator=g),
                 rotations=torch.randn(P, 4, generator=g))
    t = {k: v.cuda().requires_grad_(True) for k, v in cloud.items()}
    for k in ("opacities", "scales"):
        t[k].grad = 1e-4 * torch.randn_like(t[k])
    return t


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    q = statistics.quantiles(ms, n=10)
    return dict(median_ms=statistics.median(ms), p10_ms=q[0], p90_ms=q[-1])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4, help="the forms are alternated: --rounds blocks of --iters / --rounds each")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcmc_regularize_timing.json"))
    a = ap.parse_args(argv)
    lib = L.load()
    out = dict(iters=a.iters, device=torch.cuda.get_device_name(0), copy_rate_Bps=COPY, lambda_opacity=LAMBDA_O, lambda_scale=LAMBDA_S,
               sizes={})
    for name, P in SIZES.items():
        t = make_cloud(P, seed=1)
        opt = GaussianAdam(cloud_param_groups(*[t[k] for k in NAMES]), eps=1e-15)
        ptrs = (t["opacities"].grad.data_ptr(), t["scales"].grad.data_ptr())
        # the bare call: everything allocated once
        ws = torch.empty(max(int(lib.hs_mcmc_reg_workspace_bytes(P)), 16), dtype=torch.uint8, device="cuda")
        terms = torch.empty(2, dtype=torch.float32, device="cuda")
        args = L.hs_mcmc_reg_args()
        args.P, args.flags, args.lambda_opacity, args.lambda_scale = P, 3, LAMBDA_O, LAMBDA_S
        args.opacities, args.scales = t["opacities"].data_ptr(), t["scales"].data_ptr()
        args.dL_dopacities, args.dL_dscales = ptrs
        args.loss, args.workspace = terms.data_ptr(), ws.data_ptr()
        stream = torch.cuda.current_stream().cuda_stream

        def torch_form():
            (LAMBDA_O * torch.sigmoid(t["opacities"]).mean() + LAMBDA_S * torch.exp(t["scales"]).mean()).backward()

        forms = {"fused": lambda: regularize(opt, opacity_reg=LAMBDA_O, scale_reg=LAMBDA_S),
                 "fused_no_value": lambda: regularize(opt, opacity_reg=LAMBDA_O, scale_reg=LAMBDA_S, value=False),
                 "fused_abi": lambda: L.check(lib.hs_mcmc_regularize(C.byref(args), stream), "hs_mcmc_regularize"),
                 "torch": torch_form}
        ms = {k: [] for k in forms}
        per = max(a.iters // a.rounds, 1)
        for r in range(a.rounds):
            for k, fn in forms.items():
                ms[k] += timed(fn, per, a.warmup if r == 0 else 2)
        kept = (t["opacities"].grad.data_ptr(), t["scales"].grad.data_ptr()) == ptrs     # (plain leaf gradients: autograd adds in place)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(t["opacities"].grad).all()) and bool(torch.isfinite(t["scales"].grad).all())
        res = {k: stats(v) for k, v in ms.items()}
        mb = 48.0 * P / 1e6
        for k in ("fused", "fused_no_value", "fused_abi"):
            res[k].update(effective_mb=mb, frac_of_copy_rate=48.0 * P / (res[k]["median_ms"] * 1e-3) / COPY)
        res["ratio_torch_over_fused"] = res["torch"]["median_ms"] / res["fused"]["median_ms"]
        out["sizes"][name] = dict(P=P, gradients_kept_their_address=kept, **res)
        print(name, json.dumps(res), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
