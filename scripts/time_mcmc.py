#!/usr/bin/env python3
"""The fused MCMC refinement (casualhdrsplat_amd.inject_noise / relocate / grow) against the torch formulation a trainer writes
without it (the published inject_noise_to_position / relocate / sample_add: sigmoid, exp, normalise, quaternion -> matrix,
batched products and einsum for the noise; multinomial, bincount, the binomial sum and indexed writes or cat on the five
tensors and both Adam moments for the other two), alternated in one process on the same inputs.

    python scripts/time_mcmc.py --iters 40 --out profiles/mcmc_timing.json

Sizes: c3 (1 M Gaussians, SH degree 3) and c2 (100 k, SH degree 0); about 5 % of the rows dead (opacity below 0.005), growth
by 5 %.  Device events around each call, medians and p10 / p90 over --iters iterations after a warm-up; every iteration starts
from the same cloud (restored outside the timed window).  The torch relocation and growth include the host waits torch makes
(nonzero behind a boolean index, the largest ratio read for the binomial loop); the fused calls make none.
Effective bytes of the noise kernel = what it has to move once: the opacity of every row (4 B) and, for rows whose gate is
open, quaternion, scales, normals and the mean read and the mean written (64 B); reported as a share of the 6.29 TB/s copy
rate."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import GaussianAdam, cloud_param_groups, grow, inject_noise, relocate

SIZES = {"c3": (1_000_000, 16), "c2": (100_000, 1)}
NAMES = ("means3D", "opacities", "shs", "scales", "rotations")
COPY = 6.29e12
MIN_OPACITY, N_MAX = 0.005, 51


def make_inputs(P, M, seed):
    g = torch.Generator().manual_seed(seed)
    logit = (1.0 + 2.0 * torch.randn(P, 1, generator=g)).clamp(min=-5.0)
    logit[torch.rand(P, 1, generator=g) < 0.05] = -7.0
    cloud = dict(means3D=torch.randn(P, 3, generator=g), opacities=logit, shs=torch.randn(P, M, 3, generator=g),
                 scales=math.log(0.02) + 0.7 * torch.randn(P, 3, generator=g), rotations=torch.randn(P, 4, generator=g))
    cloud = {k: v.cuda() for k, v in cloud.items()}
    moments = {k: (0.1 * torch.randn_like(v), 0.01 * torch.rand_like(v)) for k, v in cloud.items()}
    return cloud, moments


def fused_setup(cloud, moments):
    t = {k: v.clone().requires_grad_(True) for k, v in cloud.items()}
    opt = GaussianAdam(cloud_param_groups(*[t[k] for k in NAMES]), eps=1e-15)
    opt.prepare()
    for k in NAMES:
        opt.state[t[k]]["exp_avg"].copy_(moments[k][0])
        opt.state[t[k]]["exp_avg_sq"].copy_(moments[k][1])
    return opt, t


def torch_noise(t, xi, scaler):
    opacities = torch.sigmoid(t["opacities"].flatten())
    scales = torch.exp(t["scales"])
    w, x, y, z = torch.nn.functional.normalize(t["rotations"], dim=-1).unbind(dim=-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    Mx = R * scales[:, None, :]
    covars = torch.bmm(Mx, Mx.transpose(1, 2))
    noise = xi * (1 / (1 + torch.exp(-100 * ((1 - opacities) - 0.995)))).unsqueeze(-1) * scaler
    t["means3D"].add_(torch.einsum("bij,bj->bi", covars, noise))


def binoms(dev):
    b = torch.zeros(N_MAX, N_MAX)
    for n in range(N_MAX):
        for k in range(n + 1):
            b[n, k] = math.comb(n, k)
    return b.to(dev)


def torch_compute_relocation(opacities, scales, ratios, table):
    ratios = ratios.clamp(min=1, max=N_MAX)
    new_opacities = 1.0 - torch.pow(1.0 - opacities, 1.0 / ratios.float())
    denom = torch.zeros_like(opacities)
    for i in range(1, int(ratios.max()) + 1):          # (the host reads the largest ratio: upstream's kernel loops per row)
        on = ratios >= i
        for k in range(i):
            term = table[i - 1, k] * ((-1.0) ** k / math.sqrt(k + 1)) * torch.pow(new_opacities, k + 1)
            denom = denom + torch.where(on, term, torch.zeros_like(term))
    return new_opacities, (opacities / denom)[:, None] * scales


def torch_relocate(t, mom, table, gen):
    opacities = torch.sigmoid(t["opacities"].flatten())
    dead = opacities <= MIN_OPACITY
    dead_idx, alive_idx = dead.nonzero(as_tuple=True)[0], (~dead).nonzero(as_tuple=True)[0]
    if dead_idx.numel() == 0:
        return 0
    sampled = alive_idx[torch.multinomial(opacities[alive_idx], dead_idx.numel(), replacement=True, generator=gen)]
    new_o, new_s = torch_compute_relocation(opacities[sampled], torch.exp(t["scales"])[sampled], torch.bincount(sampled)[sampled] + 1, table)
    new_o = torch.clamp(new_o, max=1.0 - torch.finfo(torch.float32).eps, min=MIN_OPACITY)
    t["opacities"][sampled] = torch.logit(new_o)[:, None]
    t["scales"][sampled] = torch.log(new_s)
    for k in NAMES:
        t[k][dead_idx] = t[k][sampled]
        for m in mom[k]:
            m[sampled] = 0
    return int(dead_idx.numel())


def torch_grow(t, mom, table, n_new, gen):
    opacities = torch.sigmoid(t["opacities"].flatten())
    sampled = torch.multinomial(opacities, n_new, replacement=True, generator=gen)
    new_o, new_s = torch_compute_relocation(opacities[sampled], torch.exp(t["scales"])[sampled], torch.bincount(sampled)[sampled] + 1, table)
    new_o = torch.clamp(new_o, max=1.0 - torch.finfo(torch.float32).eps, min=MIN_OPACITY)
    t["opacities"][sampled] = torch.logit(new_o)[:, None]
    t["scales"][sampled] = torch.log(new_s)
    for k in NAMES:
        t[k] = torch.cat([t[k], t[k][sampled]])
        mom[k] = tuple(torch.cat([m, torch.zeros((n_new, *m.shape[1:]), device=m.device)]) for m in mom[k])
    return t["means3D"].shape[0]


def time_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def summary(v):
    v = sorted(v)
    return {"median_ms": statistics.median(v), "p10_ms": v[len(v) // 10], "p90_ms": v[9 * len(v) // 10]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true", help="run only the fused paths (for a kernel-trace run)")
    ap.add_argument("--sizes", default="c3,c2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mcmc.py measures on the GPU only")
    res = {"iters": a.iters, "device": torch.cuda.get_device_name(0), "copy_rate_Bps": COPY, "sizes": {}}
    for name in a.sizes.split(","):
        P, M = SIZES[name]
        cloud, moments = make_inputs(P, M, 1)
        dev = cloud["means3D"].device
        table = binoms(dev)
        gen = torch.Generator(device=dev).manual_seed(3)
        n_new = int(1.05 * P) - P
        xi = torch.randn(P, 3, device=dev, generator=gen)
        u = torch.randint(-(1 << 63), (1 << 63) - 1, (P,), dtype=torch.int64, device=dev, generator=gen)
        lr = 1.6e-4
        o = torch.sigmoid(cloud["opacities"].flatten())
        open_rows = int((torch.exp(-100 * ((1 - o) - 0.995)) < 3.0e38).sum())
        n_dead = int((o <= MIN_OPACITY).sum())
        t = {k: {"fused": [], "torch": []} for k in ("noise", "relocate", "grow")}

        # --- noise and relocation: in place, on one optimizer whose tensors are restored before every call
        opt, ft = fused_setup(cloud, moments)
        tt = {k: v.clone() for k, v in cloud.items()}
        tm = {k: (m.clone(), v.clone()) for k, (m, v) in moments.items()}

        def restore():
            with torch.no_grad():
                for k in NAMES:
                    ft[k].copy_(cloud[k])
                    tt[k].copy_(cloud[k])
                    for j in range(2):
                        tm[k][j].copy_(moments[k][j])
                        opt.state[ft[k]]["exp_avg" if j == 0 else "exp_avg_sq"].copy_(moments[k][j])
            torch.cuda.synchronize()

        for it in range(a.warmup + a.iters):
            keep = it >= a.warmup
            restore()
            ms, _ = time_once(lambda: inject_noise(opt, noise_lr=5e5, lr=lr, xi=xi))
            if keep:
                t["noise"]["fused"].append(ms)
            restore()
            ms, r = time_once(lambda: relocate(opt, min_opacity=MIN_OPACITY, u=u))
            if keep:
                t["relocate"]["fused"].append(ms)
            if a.fused_only:
                continue
            restore()
            with torch.no_grad():
                ms, _ = time_once(lambda: torch_noise(tt, xi, lr * 5e5))
                if keep:
                    t["noise"]["torch"].append(ms)
                restore()
                ms, _ = time_once(lambda: torch_relocate(tt, tm, table, gen))
                if keep:
                    t["relocate"]["torch"].append(ms)
        counts = dict(zip(("P", "dead", "draws", "sources", "S_is_zero"), r.counts.cpu().tolist()))
        del opt, ft, tt, tm

        # --- growth: P changes, so every iteration starts from a fresh optimizer / fresh copies
        for it in range(a.warmup + a.iters):
            keep = it >= a.warmup
            opt, ft = fused_setup(cloud, moments)
            torch.cuda.synchronize()
            ms, g = time_once(lambda: grow(opt, cap_max=2 * P, min_opacity=MIN_OPACITY, u=u[:n_new]))
            assert g.n_new == n_new
            del opt, ft, g
            if keep:
                t["grow"]["fused"].append(ms)
            if a.fused_only:
                continue
            tt = {k: v.clone() for k, v in cloud.items()}
            tm = {k: (m.clone(), v.clone()) for k, (m, v) in moments.items()}
            torch.cuda.synchronize()
            with torch.no_grad():
                ms, p_out = time_once(lambda: torch_grow(tt, tm, table, n_new, gen))
            assert p_out == P + n_new
            del tt, tm
            if keep:
                t["grow"]["torch"].append(ms)

        noise_bytes = 4 * P + 64 * open_rows
        row = {"P": P, "M": M, "dead_rows": n_dead, "n_new": n_new, "gate_open_rows": open_rows, "relocate_counts": counts}
        for what, both in t.items():
            row[what] = {}
            for k, v in both.items():
                if not v:
                    continue
                row[what][k] = summary(v)
                if what == "noise" and k == "fused":
                    med = row[what][k]["median_ms"]
                    row[what][k].update(effective_mb=noise_bytes / 1e6, frac_of_copy_rate=noise_bytes / (med * 1e-3) / COPY)
                print(name, what, k, json.dumps(row[what][k]), flush=True)
        res["sizes"][name] = row
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
