#!/usr/bin/env python3
"""The fused depth-normal consistency term and per-Gaussian normal (casualhdrsplat_amd.normals) against the torch formulation of
the same definition a trainer writes without them,

    z = alpha / invdepth;  P = z * ray;  c = cross(P[y+1] - P[y-1], P[x+1] - P[x-1]);  n = R (c / |c|)
    map = weight * (1 - <normals, n>) on the interior (the pixel and its four neighbours valid), 0 elsewhere
    normal_g = sign * column argmin(scales) of R(q / |q|),  sign from <column, campos - mean>

forward + backward under autograd, alternated in one process on the same inputs.

    python scripts/time_normals.py --iters 200 --out profiles/normal_consistency_timing.json

Shapes: 1080p and 800 x 800 (B = 1; alpha, weight and cam_to_world given), P = 1 M and 100 k.  Two kinds of figures:
  * fused / torch: forward + backward under autograd, device events around ONE call, medians and p10 / p90 over --iters calls
    after a warm-up, the forms alternated in --rounds blocks.  Both are bound by the host's launch cost at these sizes, and
    the calls of a block reuse the same tensors, which stay in the last-level cache: a comparison of the two forms, not a
    bandwidth figure.
  * abi_forward / abi_backward / copy_1GiB: the entry points on preallocated buffers, timed as a BATCH of launches between two
    events (a launch of ten microseconds is near the resolution of an event pair) that walks over `sets` distinct copies of
    the inputs and outputs -- enough that a pass moves at least 1 GiB (at most 40 sets), so no launch finds its data in the
    cache the launch before left (256 MB); per-launch time = batch time / launches.  The copy moves 2 GiB from and to HBM.
Byte model.  Term: forward 28 B per pixel (invdepth, alpha, weight 4 each and normals 12 read, the map written), backward 48 B
(the same 24 and dL_dout read, dL_dnormals 12, dL_dinvdepth and dL_dalpha 4 each written).  Per-Gaussian normal: forward 52 B
(rotations 16, scales 12, means 12 read, 12 written), backward 68 B (the same 40 and dL_dnormals 12 read, 16 written).
frac_of_copy = bytes of the model / median time / the measured copy rate.
--example-steps N > 0 also runs examples/train_synthetic.py --mcmc for N steps with --normal 0 and --normal 0.05 and records
the PSNR and the mean of the map."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import _lib as L, gaussian_normals, normal_consistency_loss

FRAMES = {"1080p": (1, 1080, 1920), "800x800": (1, 800, 800)}
CLOUDS = {"1M": 1_000_000, "100k": 100_000}
COPY_BYTES = 1 << 30


def torch_term(invd, N, alpha, weight, R, fx, fy):
    B, H, W = invd.shape
    valid = torch.isfinite(invd) & (invd > 0) & torch.isfinite(alpha) & (alpha > 0)
    z = torch.where(valid, alpha, torch.ones_like(alpha)) / torch.where(valid, invd, torch.ones_like(invd))
    xh = (torch.arange(W, device=invd.device, dtype=torch.float32) + 0.5 - W / 2) / fx
    yh = (torch.arange(H, device=invd.device, dtype=torch.float32) + 0.5 - H / 2) / fy
    ray = torch.stack([xh[None, :].expand(H, W), yh[:, None].expand(H, W), torch.ones(H, W, device=invd.device)], dim=-1)
    P = z[..., None] * ray[None]
    c = torch.linalg.cross(P[:, 2:, 1:-1] - P[:, :-2, 1:-1], P[:, 1:-1, 2:] - P[:, 1:-1, :-2], dim=-1)
    n = torch.einsum("bij,bhwj->bihw", R, c / c.norm(dim=-1, keepdim=True))
    inner = valid[:, 1:-1, 1:-1] & valid[:, 1:-1, :-2] & valid[:, 1:-1, 2:] & valid[:, :-2, 1:-1] & valid[:, 2:, 1:-1]
    core = weight[:, 1:-1, 1:-1] * (1.0 - (N[:, :, 1:-1, 1:-1] * n).sum(dim=1))
    return torch.nn.functional.pad(torch.where(inner, core, torch.zeros_like(core)), (1, 1, 1, 1))


def torch_gaussian_normals(q, scales, means, campos):
    w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(dim=1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    k = scales.argmin(dim=1)
    n0 = torch.gather(R, 2, k[:, None, None].expand(-1, 3, 1))[:, :, 0]
    sign = torch.where((n0.detach() * (campos[None] - means)).sum(dim=1) >= 0, 1.0, -1.0)
    return n0 * sign[:, None]


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


def timed_batch(fns, iters, warmup, passes=1):
    """ms PER LAUNCH: `passes` walks over the launches `fns` (one per buffer set) between two events, `iters` times"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(passes):
            for fn in fns:
                fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / (passes * len(fns)))
    return ms


def n_sets(bytes_per_launch):
    return int(min(40, max(2, -(-COPY_BYTES // int(bytes_per_launch)))))


def stats(ms):
    q = statistics.quantiles(ms, n=10)
    return dict(median_ms=statistics.median(ms), p10_ms=q[0], p90_ms=q[-1])


def run_forms(forms, a):
    """forms: name -> a callable (timed call by call) or a list of callables, one per buffer set (timed as batches)"""
    ms = {k: [] for k in forms}
    per = max(a.iters // a.rounds, 1)
    for r in range(a.rounds):
        for k, fn in forms.items():
            if isinstance(fn, list):
                ms[k] += timed_batch(fn, max(per // 5, 4), 2 if r == 0 else 1, passes=max(1, 20 // len(fn)))
            else:
                ms[k] += timed(fn, per, a.warmup if r == 0 else 2)
    res = {k: stats(v) for k, v in ms.items()}
    for k, fn in forms.items():
        if isinstance(fn, list):
            res[k]["sets"], res[k]["launches_per_event_pair"] = len(fn), max(1, 20 // len(fn)) * len(fn)
    return res


def example_runs(steps):
    spec = importlib.util.spec_from_file_location("train_synthetic_timing", os.path.join(ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for lam in (0.0, 0.05):
        r = mod.run(steps=steps, quiet=True, mcmc=True, normal=lam)
        out[f"lambda_{lam:g}"] = dict(first_psnr_db=r["first"]["psnr"], last_psnr_db=r["last"]["psnr"], first_loss=r["first"]["loss"],
                                      last_loss=r["last"]["loss"], first_mean_map=r["first"]["normal"], last_mean_map=r["last"]["normal"])
        print(f"lambda {lam:g}", json.dumps(out[f"lambda_{lam:g}"]), flush=True)
    return dict(steps=steps, mode="--mcmc", **out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4, help="the forms are alternated: --rounds blocks of --iters / --rounds each")
    ap.add_argument("--example-steps", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_consistency_timing.json"))
    a = ap.parse_args(argv)
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    src = torch.empty(COPY_BYTES, dtype=torch.uint8, device="cuda").zero_()
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)
    out = dict(iters=a.iters, device=torch.cuda.get_device_name(0), copy_bytes=COPY_BYTES, frames={}, clouds={})
    for name, (B, H, W) in FRAMES.items():
        gen = torch.Generator().manual_seed(1)
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        z = (4.0 + 1.6 * torch.sin(3.0 * xx / W) * torch.cos(2.0 * yy / H)) * (1.0 + 0.01 * torch.randn(H, W, generator=gen))
        alpha = (0.3 + 0.7 * torch.rand(B, H, W, generator=gen)).cuda().requires_grad_(True)
        invd = (alpha.detach().cpu() / z[None]).cuda().requires_grad_(True)
        N = torch.nn.functional.normalize(torch.randn(B, 3, H, W, generator=gen), dim=1).cuda().requires_grad_(True)
        weight = torch.rand(B, H, W, generator=gen).cuda()
        R = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen))[0].contiguous().cuda()
        d_out = torch.randn(B, H, W, generator=gen).cuda()
        fx, fy = 1.1 * W, 0.9 * W
        leaves = (invd, N, alpha)

        def fused():
            for t in leaves:
                t.grad = None
            normal_consistency_loss(invd, N, fx, fy, alpha=alpha, weight=weight, cam_to_world=R).backward(d_out)

        def torch_form():
            for t in leaves:
                t.grad = None
            torch_term(invd, N, alpha, weight, R, fx, fy).backward(d_out)

        px = B * H * W

        def abi_set():
            """one more copy of the inputs and outputs, and the argument struct over it"""
            ins = [t.detach().clone() for t in (invd, alpha, N, weight, R, d_out)]
            outs = [torch.empty_like(d_out), torch.empty_like(N.detach()), torch.empty_like(d_out), torch.empty_like(d_out)]
            s = L.hs_normal_consistency_args()
            s.B, s.H, s.W, s.fx, s.fy = B, H, W, fx, fy
            s.invdepth, s.alpha, s.normals, s.weight, s.cam_to_world, s.dL_dout = (t.data_ptr() for t in ins)
            s.out, s.dL_dnormals, s.dL_dinvdepth, s.dL_dalpha = (t.data_ptr() for t in outs)
            return s, ins, outs

        sets = [abi_set() for _ in range(n_sets(28 * px))]
        fwd = [(lambda s=s: L.check(lib.hs_normal_consistency(C.byref(s), stream), "forward")) for s, _, _ in sets]
        bwd = [(lambda s=s: L.check(lib.hs_normal_consistency_backward(C.byref(s), stream), "backward")) for s, _, _ in sets]
        forms = {"fused": fused, "torch": torch_form, "copy_1GiB": [copy], "abi_forward": fwd, "abi_backward": bwd}
        fused()
        g = [t.grad.clone() for t in leaves]
        torch_form()
        agree = {k: float((t.grad - g0).abs().max() / g0.abs().max()) for k, t, g0 in zip(("d_invdepth", "d_normals", "d_alpha"), leaves, g)}
        res = run_forms(forms, a)
        rate = 2.0 * COPY_BYTES / (res["copy_1GiB"]["median_ms"] * 1e-3)
        res["copy_rate_Bps"] = rate
        res["abi_forward"]["frac_of_copy"] = 28.0 * px / (res["abi_forward"]["median_ms"] * 1e-3) / rate
        res["abi_backward"]["frac_of_copy"] = 48.0 * px / (res["abi_backward"]["median_ms"] * 1e-3) / rate
        res["ratio_torch_over_fused"] = res["torch"]["median_ms"] / res["fused"]["median_ms"]
        out["frames"][name] = dict(B=B, H=H, W=W, workspace_bytes=int(lib.hs_normal_consistency_workspace_bytes(B, H, W)),
                                   max_rel_difference_to_torch=agree, **res)
        print(name, json.dumps(out["frames"][name]), flush=True)
    for name, P in CLOUDS.items():
        gen = torch.Generator().manual_seed(2)
        q = torch.randn(P, 4, generator=gen).cuda().requires_grad_(True)
        scales = torch.rand(P, 3, generator=gen).cuda()
        means = torch.randn(P, 3, generator=gen).cuda()
        campos = torch.tensor([0.3, -0.2, 4.0]).cuda()
        d_n = torch.randn(P, 3, generator=gen).cuda()

        def fused():
            q.grad = None
            gaussian_normals(q, scales, means, campos).backward(d_n)

        def torch_form():
            q.grad = None
            torch_gaussian_normals(q, scales, means, campos).backward(d_n)

        def abi_set():
            ins = [t.detach().clone() for t in (q, scales, means, d_n)]
            outs = [torch.empty_like(d_n), torch.empty_like(q.detach())]
            s = L.hs_gaussian_normals_args()
            s.P = P
            s.rotations, s.scales, s.means3D, s.dL_dnormals = (t.data_ptr() for t in ins)
            s.campos = campos.data_ptr()
            s.normals, s.dL_drotations = (t.data_ptr() for t in outs)
            return s, ins, outs

        sets = [abi_set() for _ in range(n_sets(52 * P))]
        fwd = [(lambda s=s: L.check(lib.hs_gaussian_normals(C.byref(s), stream), "forward")) for s, _, _ in sets]
        bwd = [(lambda s=s: L.check(lib.hs_gaussian_normals_backward(C.byref(s), stream), "backward")) for s, _, _ in sets]
        forms = {"fused": fused, "torch": torch_form, "copy_1GiB": [copy], "abi_forward": fwd, "abi_backward": bwd}
        fused()
        g0 = q.grad.clone()
        torch_form()
        agree = float((q.grad - g0).abs().max() / g0.abs().max())
        res = run_forms(forms, a)
        rate = 2.0 * COPY_BYTES / (res["copy_1GiB"]["median_ms"] * 1e-3)
        res["copy_rate_Bps"] = rate
        res["abi_forward"]["frac_of_copy"] = 52.0 * P / (res["abi_forward"]["median_ms"] * 1e-3) / rate
        res["abi_backward"]["frac_of_copy"] = 68.0 * P / (res["abi_backward"]["median_ms"] * 1e-3) / rate
        res["ratio_torch_over_fused"] = res["torch"]["median_ms"] / res["fused"]["median_ms"]
        out["clouds"][name] = dict(P=P, max_rel_difference_to_torch=agree, **res)
        print(name, json.dumps(out["clouds"][name]), flush=True)
    if a.example_steps > 0:
        out["example"] = example_runs(a.example_steps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
