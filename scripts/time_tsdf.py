#!/usr/bin/env python3
"""The fused TSDF integration (casualhdrsplat_amd.tsdf.TSDFVolume.integrate, ONE launch for all frames) against the torch
formulation of the same rule a trainer writes without it -- a loop over the frames, each projecting the whole volume, gathering
the nearest pixel and averaging under torch.where --, alternated in one process on the same inputs, and the mesh extraction.

    python scripts/time_tsdf.py --out profiles/tsdf_timing.json

Scene: a cube of side 4 around the origin, F cameras on a ring of radius 8 looking at its centre (half field of view 30 degrees
on the short side), depth maps of a sphere of radius 1.2 (pixels that miss it are invalid), alpha 1, colour random.  Every
camera sees the whole volume, so the brick cull drops nothing here: the figures are the walk's, not the cull's.  Sizes: 256^3 x 32 frames of 800 x 800 and 512^3 x 100 frames
of 1920 x 1080, with and without colour.
Figures: device events around ONE call, the median and the extremes over --iters calls (--torch-iters for the torch form at the
large size) after a warm-up, the two forms alternated in --rounds blocks.  Byte model of the fused form: 16 B per sample (tsdf
and weight read and written once), 40 B with colour, whatever F; model_GBps = that over the median, frac_of_copy = that over the
rate of a 1 GiB device copy (2 GiB moved) timed in the same run.  The torch form moves the volume tens of times per FRAME.
extract_mesh (plan, the host read of the sizes, emit) at 256^3 and 512^3 on the sphere as a filled volume: wall time around the
call ending in a synchronise, with V and T.
--example runs examples/train_synthetic.py --steps 300 --mcmc --distortion 0.1 --normal 0.05 --mesh and records what it prints
about the mesh: an observation, not a threshold."""
import argparse
import importlib.util
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import TSDFVolume

SIZES = {"256^3 x 32 x 800x800": (256, 32, 800, 800), "512^3 x 100 x 1920x1080": (512, 100, 1080, 1920)}
SIDE, RING, RADIUS = 4.0, 8.0, 1.2
COPY_BYTES = 1 << 30


def ring_views(F, dev):
    """[F, 4, 4] world-to-camera matrices in the transposed convention: cameras on a ring in the x-z plane, looking at the origin"""
    out = []
    for f in range(F):
        a = 2 * math.pi * f / F
        c = torch.tensor([RING * math.sin(a), 0.4 * math.sin(3 * a), -RING * math.cos(a)], dtype=torch.float64)
        z = -c / c.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), z)
        x = x / x.norm()
        y = torch.linalg.cross(z, x)
        R = torch.stack([x, y, z])                                  # rows: the camera's axes in world coordinates
        w2c = torch.eye(4, dtype=torch.float64)
        w2c[:3, :3], w2c[:3, 3] = R, -R @ c
        out.append(w2c.t())
    return torch.stack(out).to(dev, torch.float32).contiguous()


def sphere_frames(views, H, W, fx, fy):
    """invdepth [F, H, W]: 1 / z of the sphere of radius RADIUS around the origin, 0 where the ray misses it"""
    dev = views.device
    xh = (torch.arange(W, device=dev, dtype=torch.float32) + 0.5 - W / 2) / fx
    yh = (torch.arange(H, device=dev, dtype=torch.float32) + 0.5 - H / 2) / fy
    ray = torch.stack([xh[None, :].expand(H, W), yh[:, None].expand(H, W), torch.ones(H, W, device=dev)], dim=-1)   # z = 1
    out = []
    for V in views:
        o = V[3, :3]                                                # the world origin in camera coordinates
        b = (ray * o).sum(-1)
        a = (ray * ray).sum(-1)
        disc = b * b - a * ((o * o).sum() - RADIUS * RADIUS)
        t = (b - disc.clamp_min(0).sqrt()) / a
        out.append(torch.where(disc > 0, 1.0 / t, torch.zeros_like(t)))
    return torch.stack(out).contiguous()


def torch_integrate(tsdf, weight, color, grid, trunc, invdepth, views, fx, fy, alpha, frame_color, min_alpha=0.5):
    """the same rule, frame by frame on the whole volume: project, gather, where"""
    px, py, pz = grid
    F, H, W = invdepth.shape
    for f in range(F):
        V = views[f]
        xc = px * V[0, 0] + py * V[1, 0] + pz * V[2, 0] + V[3, 0]
        yc = px * V[0, 1] + py * V[1, 1] + pz * V[2, 1] + V[3, 1]
        zc = px * V[0, 2] + py * V[1, 2] + pz * V[2, 2] + V[3, 2]
        u = fx * (xc / zc) + W / 2
        v = fy * (yc / zc) + H / 2
        live = (zc > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        at = torch.where(live, v.to(torch.int64) * W + u.to(torch.int64), torch.zeros((), dtype=torch.int64, device=u.device))
        d, a = invdepth[f].reshape(-1)[at], alpha[f].reshape(-1)[at]
        live = live & torch.isfinite(d) & (d > 0) & torch.isfinite(a) & (a > 0) & (a >= min_alpha)
        sdf = a / d - zc
        live = live & ~(sdf < -trunc)
        t = (sdf / trunc).clamp_max(1.0)
        w1 = weight + 1
        tsdf = torch.where(live, (tsdf * weight + t) / w1, tsdf)
        if color is not None:
            got = frame_color[f].reshape(3, -1)[:, at]
            color = torch.where(live[None], (color * weight[None] + got) / w1[None], color)
        weight = torch.where(live, w1, weight)
    return tsdf, weight, color


def timed(fn, iters, warmup=1):
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
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), calls=len(ms))


def copy_rate(dev, iters=20):
    src = torch.empty(COPY_BYTES, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    ms = statistics.median(timed(lambda: dst.copy_(src), iters, warmup=3))
    return 2 * COPY_BYTES / (ms * 1e-3) / 1e9, ms


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sizes", nargs="*", default=list(SIZES))
    ap.add_argument("--mesh-sizes", nargs="*", type=int, default=[256, 512])
    ap.add_argument("--example", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_tsdf.py measures on an MI355X: no GPU here, nothing is measured")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), sizes={}, mesh={})
    gbps, copy_ms = copy_rate(dev)
    result["copy_1GiB"] = dict(median_ms=copy_ms, GBps=gbps)
    print(f"copy 1 GiB: {copy_ms:.3f} ms, {gbps:.0f} GB/s", flush=True)

    for name in a.sizes:
        n, F, H, W = SIZES[name]
        h = SIDE / (n - 1)
        fx = fy = 0.5 * W / math.tan(math.radians(30.0)) if W <= H else 0.5 * H / math.tan(math.radians(30.0))
        views = ring_views(F, dev)
        invdepth = sphere_frames(views, H, W, fx, fy)
        alpha = torch.ones_like(invdepth)
        frame_color = torch.rand((F, 3, H, W), device=dev)
        ax = [(-SIDE / 2 + h * torch.arange(n, device=dev, dtype=torch.float32)) for _ in range(3)]
        grid = (ax[0][None, None, :].expand(n, n, n).contiguous(), ax[1][None, :, None].expand(n, n, n).contiguous(),
                ax[2][:, None, None].expand(n, n, n).contiguous())
        for color in (False, True):
            vol = TSDFVolume((-SIDE / 2,) * 3, h, (n, n, n), color=color, device=dev)
            fused = lambda: vol.integrate(invdepth, views, fx, fy, alpha=alpha, color=frame_color if color else None)
            state = (vol.tsdf.clone(), vol.weight.clone(), vol.color.clone() if color else None)
            plain = lambda: torch_integrate(*state, grid, vol.trunc, invdepth, views, fx, fy, alpha, frame_color if color else None)
            # the two forms agree on one call from the empty volume (the torch form contracts and reorders: not bit for bit)
            fused()
            want = plain()
            seen = float((vol.weight > 0).float().mean())
            err = float((vol.tsdf - want[0]).abs().max())
            w_diff = int((vol.weight != want[1]).sum())
            ms = {"fused": [], "torch": []}
            t_iters = a.torch_iters if n > 256 else max(a.torch_iters, 5)
            for _ in range(a.rounds):
                ms["fused"] += timed(fused, max(a.iters // a.rounds, 1))
                ms["torch"] += timed(plain, max(t_iters // a.rounds, 1))
            model = (40 if color else 16) * n ** 3
            row = dict(samples=n ** 3, frames=F, H=H, W=W, color=color, fused=stats(ms["fused"]), torch=stats(ms["torch"]),
                       model_bytes=model, observed_share=seen, max_abs_tsdf_difference=err, samples_whose_weight_differs=w_diff)
            row["fused"]["model_GBps"] = model / (row["fused"]["median_ms"] * 1e-3) / 1e9
            row["fused"]["frac_of_copy"] = row["fused"]["model_GBps"] / gbps
            row["fused"]["ns_per_sample_and_frame"] = row["fused"]["median_ms"] * 1e6 / (n ** 3 * F)
            row["speedup"] = row["torch"]["median_ms"] / row["fused"]["median_ms"]
            result["sizes"][name + (" colour" if color else "")] = row
            print(name, "colour" if color else "plain", json.dumps(row), flush=True)
            del vol, state, want
        del grid, invdepth, alpha, frame_color
        torch.cuda.empty_cache()

    for n in a.mesh_sizes:
        h = SIDE / (n - 1)
        vol = TSDFVolume((-SIDE / 2,) * 3, h, (n, n, n), device=dev)
        axis = -SIDE / 2 + h * torch.arange(n, device=dev, dtype=torch.float32)
        dist = (axis[None, None, :] ** 2 + axis[None, :, None] ** 2 + axis[:, None, None] ** 2).sqrt()
        vol.tsdf.copy_(((dist - RADIUS) / vol.trunc).clamp(-1, 1))
        vol.weight.fill_(1.0)
        del dist
        v, f = vol.extract_mesh()
        torch.cuda.synchronize()
        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            v, f = vol.extract_mesh()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        result["mesh"][f"{n}^3"] = dict(samples=n ** 3, V=int(v.shape[0]), T=int(f.shape[0]), **stats(wall))
        print(f"extract_mesh {n}^3", json.dumps(result["mesh"][f"{n}^3"]), flush=True)
        del vol, v, f
        torch.cuda.empty_cache()

    if a.example:
        spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(ROOT, "examples", "train_synthetic.py"))
        ex = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ex)
        with tempfile.TemporaryDirectory() as tmp:
            r = ex.run(steps=300, mcmc=True, distortion=0.1, normal=0.05, mesh=os.path.join(tmp, "out.ply"), quiet=True)
            size = os.path.getsize(os.path.join(tmp, "out.ply"))
        m = {k: v for k, v in r["mesh"].items() if k != "path"}
        result["example"] = dict(command="examples/train_synthetic.py --steps 300 --mcmc --distortion 0.1 --normal 0.05 --mesh out.ply",
                                 psnr_db=r["last"]["psnr"], ply_bytes=size, **m)
        print("example", json.dumps(result["example"]), flush=True)

    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
