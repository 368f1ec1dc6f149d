#!/usr/bin/env python3
"""The fused densify / prune (casualhdrsplat_amd.densify_and_prune: plan, one host read of P_out, allocation, one gather
launch over the five cloud tensors and both Adam moments) against the torch formulation a trainer writes without it
(upstream's sequence: boolean masks, index, cat and repeat on every parameter and both moments -- clone, split, drop the
split sources, prune), alternated in one process on the same inputs.

    python scripts/time_densify.py --iters 40 --out profiles/densify_timing.json

Sizes: c3 (1 M Gaussians, SH degree 3) and c2 (100 k, SH degree 0); statistics and thresholds placed so that about 10 % of
the rows are cloned, 5 % split and 5 % pruned.  Device events around each call (both formulations include their host
waits: the fused path's one read of P_out, torch's nonzero() behind every boolean index); medians and p10 / p90 over --iters
iterations after a warm-up.  Every iteration starts from fresh copies of the same cloud (made outside the timed window).
Effective bytes of the fused path = what the algorithm has to move once: the plan's inputs (28 B per source row), the row
map written and read (8 B per output row), every output row of the 15 matrices written (12 (11 + 3 M) B) and the source
rows behind them read (the moments of new rows are not read).  The per-kernel split comes from a separate
`rocprofv3 --kernel-trace --stats` run of this script (--fused-only)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import DensifyStats, GaussianAdam, cloud_param_groups, densify_and_prune

SIZES = {"c3": (1_000_000, 16), "c2": (100_000, 1)}
NAMES = ("means3D", "opacities", "shs", "scales", "rotations")
PEAK, COPY = 8.0e12, 6.29e12


def make_inputs(P, M, seed):
    g = torch.Generator().manual_seed(seed)
    cloud = dict(means3D=torch.randn(P, 3, generator=g), opacities=2.0 * torch.randn(P, 1, generator=g),
                 shs=torch.randn(P, M, 3, generator=g), scales=math.log(0.02) + 0.7 * torch.randn(P, 3, generator=g),
                 rotations=torch.randn(P, 4, generator=g))
    cloud = {k: v.cuda() for k, v in cloud.items()}
    moments = {k: (0.1 * torch.randn_like(v), 0.01 * torch.rand_like(v)) for k, v in cloud.items()}
    denom = torch.randint(1, 30, (P,), generator=g).float().cuda()
    grad = (denom * 2e-4 * torch.exp(torch.randn(P, generator=g).cuda()))
    radii = torch.randint(0, 100, (P,), generator=g).int().cuda()
    smax = torch.exp(cloud["scales"]).max(dim=1).values.cpu().double()
    extent = 10.0 * float(torch.quantile(smax[:1_000_000], 0.995))
    policy = dict(extent=extent, grad_threshold=float(torch.quantile((grad / denom).cpu()[:1_000_000], 0.85)),
                  percent_dense=float(torch.quantile(smax[:1_000_000], 0.667)) / extent,
                  min_opacity=float(torch.quantile(torch.sigmoid(cloud["opacities"].cpu()[:1_000_000, 0]), 0.04)), max_screen_size=98)
    noise = torch.randn(P, 2, 3, generator=g).cuda()
    return cloud, moments, (grad, denom, radii), policy, noise


def fused_setup(cloud, moments, stats3):
    t = {k: v.clone().requires_grad_(True) for k, v in cloud.items()}
    opt = GaussianAdam(cloud_param_groups(*[t[k] for k in NAMES]), eps=1e-15)
    opt.prepare()
    for k in NAMES:
        opt.state[t[k]]["exp_avg"].copy_(moments[k][0])
        opt.state[t[k]]["exp_avg_sq"].copy_(moments[k][1])
    stats = DensifyStats(stats3[0].shape[0])
    stats.grad_accum.copy_(stats3[0]); stats.denom.copy_(stats3[1]); stats.max_radii.copy_(stats3[2])
    return opt, stats


def torch_densify(t, mom, stats3, policy, noise):
    """Upstream's sequence on activated values, with the optimizer's part as cat / index on both moments."""
    grad, denom, radii = stats3
    P, N = grad.shape[0], 2
    g = grad / denom
    g[g.isnan()] = 0.0
    tau, pd, extent = policy["grad_threshold"], policy["percent_dense"], policy["extent"]

    rad = [radii]               # radii of the rows, carried through every cat / mask

    def extend(new, new_radii):
        for k in NAMES:
            t[k] = torch.cat([t[k], new[k]], dim=0)
            mom[k] = tuple(torch.cat([m, torch.zeros_like(new[k])], dim=0) for m in mom[k])
        rad[0] = torch.cat([rad[0], new_radii])

    def keep(valid):
        for k in NAMES:
            t[k] = t[k][valid]
            mom[k] = tuple(m[valid] for m in mom[k])
        rad[0] = rad[0][valid]

    scaling = torch.exp(t["scales"])
    sel = (g >= tau) & (scaling.max(dim=1).values <= pd * extent)
    extend({k: t[k][sel] for k in NAMES}, radii[sel])
    scaling = torch.exp(t["scales"])
    padded = torch.zeros(t["means3D"].shape[0], device=g.device)
    padded[:P] = g
    sel = (padded >= tau) & (scaling.max(dim=1).values > pd * extent)
    src = torch.arange(t["means3D"].shape[0], device=g.device)[sel]
    stds = scaling[sel].repeat(N, 1)
    samples = stds * torch.cat([noise[src, 0], noise[src, 1]], dim=0)
    q = torch.nn.functional.normalize(t["rotations"][sel])
    w, x, y, z = q.unbind(dim=1)
    rots = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3).repeat(N, 1, 1)
    new = {k: t[k][sel].repeat(N, *([1] * (t[k].dim() - 1))) for k in NAMES}
    new["means3D"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + new["means3D"]
    new["scales"] = torch.log(scaling[sel].repeat(N, 1) / (0.8 * N))
    extend(new, rad[0][sel].repeat(N))
    keep(~torch.cat([sel, torch.zeros(N * int(sel.sum()), dtype=torch.bool, device=g.device)]))
    prune = (torch.sigmoid(t["opacities"]) < policy["min_opacity"]).squeeze(-1)
    prune |= (rad[0] > policy["max_screen_size"]) | (torch.exp(t["scales"]).max(dim=1).values > 0.1 * extent)
    keep(~prune)
    return t["means3D"].shape[0]


def time_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true", help="run only the fused path (for the kernel-trace run)")
    ap.add_argument("--sizes", default="c3,c2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_densify.py measures on the GPU only")
    res = {"iters": a.iters, "device": torch.cuda.get_device_name(0), "copy_rate_Bps": COPY, "sizes": {}}
    for name in a.sizes.split(","):
        P, M = SIZES[name]
        cloud, moments, stats3, policy, noise = make_inputs(P, M, 1)
        per_row = 11 + 3 * M
        t = {"fused": [], "torch": []}
        counts = p_torch = None
        for it in range(a.warmup + a.iters):
            opt, stats = fused_setup(cloud, moments, stats3)
            torch.cuda.synchronize()
            ms, r = time_once(lambda: densify_and_prune(opt, stats, noise=noise, **policy))
            counts = r.counts
            del opt, stats, r
            if it >= a.warmup:
                t["fused"].append(ms)
            if a.fused_only:
                continue
            tt = {k: v.clone() for k, v in cloud.items()}
            mm = {k: (m.clone(), v.clone()) for k, (m, v) in moments.items()}
            s3 = tuple(x.clone() for x in stats3)
            torch.cuda.synchronize()
            ms, p_torch = time_once(lambda: torch_densify(tt, mm, s3, policy, noise))
            del tt, mm
            if it >= a.warmup:
                t["torch"].append(ms)
        if p_torch is not None and p_torch != counts["P_out"]:      # (thresholds compared as stored / as activated: borderline rows)
            print(f"note: P_out {counts['P_out']} (fused) against {p_torch} (torch)", flush=True)
        new_rows = counts["clones"] + counts["children"]
        nbytes = 28 * P + 8 * counts["P_out"] + 12 * per_row * counts["P_out"] + 4 * per_row * (counts["P_out"] + 2 * counts["survivors"])
        row = {}
        for k, v in t.items():
            if not v:
                continue
            v = sorted(v)
            med = statistics.median(v)
            row[k] = {"median_ms": med, "p10_ms": v[len(v) // 10], "p90_ms": v[9 * len(v) // 10]}
            if k == "fused":
                row[k].update(effective_mb=nbytes / 1e6, frac_of_8TBps=nbytes / (med * 1e-3) / PEAK,
                              frac_of_copy_rate=nbytes / (med * 1e-3) / COPY)
        res["sizes"][name] = {"P": P, "M": M, "floats_per_gaussian": per_row, "counts": counts, "new_rows": new_rows, "torch_P_out": p_torch, **row}
        for k, v in row.items():
            print(name, k, json.dumps(v), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
