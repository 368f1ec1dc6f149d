#!/usr/bin/env python3
"""The fused bilateral-grid correction (casualhdrsplat_amd.bilagrid) against the torch formulation a trainer writes without it,

    A = grid_sample(grids[ids], 2 (x, y, luma) - 1, bilinear, border, align_corners=True);  out = einsum(A, (r, g, b, 1))
    tv = sum over the lattice axes of mean(diff^2)

forward + backward of slice + 10 tv under autograd, alternated in one process on the same inputs.

    python scripts/time_bilagrid.py --iters 200 --out profiles/bilagrid_timing.json

Shapes: 1080p / F = 1, 800 x 800 / F = 1 and 320 x 208 / F = 4, grids 16 x 16 x 8.  Device events around each call on the current
stream, medians and p10 / p90 over --iters iterations after a warm-up, the forms alternated in --rounds blocks.  Beside the
whole step the entry points are timed one by one on preallocated buffers (each is one or two kernels): the slice, its backward
to the image alone, to the grids alone, the total variation and its backward.  Bytes floor: 24 B per pixel forward (image read,
out written), 36 B per pixel backward (image and dL_dout read, dL_dimage written), over the 6.29 TB/s copy rate.
--example-steps N > 0 also runs examples/train_synthetic.py for N steps on the distorted observations with and without
--bilagrid and records both PSNR."""
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
import torch.nn.functional as TF

from casualhdrsplat_amd import _lib as L, slice_image, tv_loss
from casualhdrsplat_amd.bilagrid import identity_grids

SHAPES = {"1080p": (1, 1080, 1920), "800x800": (1, 800, 800), "320x208x4": (4, 208, 320)}
GRID = (8, 16, 16)        # L, Y, X
COPY = 6.29e12
TV_WEIGHT = 10.0


def torch_slice(image, grids, ids):
    F, _, H, W = image.shape
    x = ((torch.arange(W, device=image.device, dtype=torch.float32) + 0.5) / W)[None, None, :].expand(F, H, W)
    y = ((torch.arange(H, device=image.device, dtype=torch.float32) + 0.5) / H)[None, :, None].expand(F, H, W)
    z = 0.299 * image[:, 0] + 0.587 * image[:, 1] + 0.114 * image[:, 2]
    at = 2.0 * torch.stack([x, y, z], dim=-1) - 1.0
    A = TF.grid_sample(grids[ids], at[:, None], mode="bilinear", padding_mode="border", align_corners=True)[:, :, 0]
    v = torch.cat([image, torch.ones_like(image[:, :1])], dim=1)
    return torch.einsum("fikhw,fkhw->fihw", A.reshape(F, 3, 4, H, W), v)


def torch_tv(g):
    return sum(((g.narrow(ax, 1, g.shape[ax] - 1) - g.narrow(ax, 0, g.shape[ax] - 1)) ** 2).mean() for ax in (2, 3, 4) if g.shape[ax] > 1)


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


def example_psnr(steps):
    spec = importlib.util.spec_from_file_location("train_synthetic_timing", os.path.join(ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for name, kw in (("distorted_without_bilagrid", dict(distort=True)), ("distorted_with_bilagrid", dict(bilagrid=True))):
        r = mod.run(steps=steps, quiet=True, **kw)
        out[name] = dict(first_psnr_db=r["first"]["psnr"], last_psnr_db=r["last"]["psnr"], first_loss=r["first"]["loss"],
                         last_loss=r["last"]["loss"])
        print(name, json.dumps(out[name]), flush=True)
    return dict(steps=steps, **out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4, help="the forms are alternated: --rounds blocks of --iters / --rounds each")
    ap.add_argument("--example-steps", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilagrid_timing.json"))
    a = ap.parse_args(argv)
    lib = L.load()
    out = dict(iters=a.iters, device=torch.cuda.get_device_name(0), copy_rate_Bps=COPY, grid_LYX=GRID, tv_weight=TV_WEIGHT, shapes={})
    for name, (F, H, W) in SHAPES.items():
        gen = torch.Generator().manual_seed(1)
        image = torch.rand(F, 3, H, W, generator=gen).cuda().requires_grad_(True)
        grids = (identity_grids(F, GRID[2], GRID[1], GRID[0]) + 0.1 * torch.randn(F, 12, *GRID, generator=gen)).cuda().requires_grad_(True)
        ids = torch.arange(F, dtype=torch.int32, device="cuda")
        ids64 = ids.long()
        d_out = torch.randn(F, 3, H, W, generator=gen).cuda()

        def fused():
            image.grad = grids.grad = None
            out_ = slice_image(image, grids, ids)
            torch.autograd.backward([out_, TV_WEIGHT * tv_loss(grids)], [d_out, None])

        def torch_form():
            image.grad = grids.grad = None
            torch.autograd.backward([torch_slice(image, grids, ids64), TV_WEIGHT * torch_tv(grids)], [d_out, None])

        # the entry points one by one, everything allocated once
        stream = torch.cuda.current_stream().cuda_stream
        s = L.hs_bilagrid_args()
        s.F, s.H, s.W, s.G, s.L, s.Y, s.X = F, H, W, F, *GRID
        nbytes = int(lib.hs_bilagrid_workspace_bytes(F, H, W, F, *GRID))
        bufs = dict(out=torch.empty_like(d_out), d_image=torch.empty_like(d_out), d_grids=torch.empty_like(grids.detach()),
                    ws=torch.empty(nbytes, dtype=torch.uint8, device="cuda"), tv=torch.empty(1, device="cuda"),
                    tvws=torch.empty(L.HS_BILAGRID_TV_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda"),
                    up=torch.ones(1, device="cuda"))
        s.image, s.grids, s.grid_ids = image.data_ptr(), grids.data_ptr(), ids.data_ptr()
        s.out, s.dL_dout = bufs["out"].data_ptr(), d_out.data_ptr()

        def variant(**kw):
            v = L.hs_bilagrid_args.from_buffer_copy(s)
            for k, val in kw.items():
                setattr(v, k, val)
            return v

        b_image = variant(dL_dimage=bufs["d_image"].data_ptr())
        b_grids = variant(dL_dgrids=bufs["d_grids"].data_ptr(), workspace=bufs["ws"].data_ptr())
        t = L.hs_bilagrid_tv_args()
        t.G, t.L, t.Y, t.X = F, *GRID
        t.grids, t.tv, t.workspace = grids.data_ptr(), bufs["tv"].data_ptr(), bufs["tvws"].data_ptr()
        t.dL_dtv, t.dL_dgrids = bufs["up"].data_ptr(), bufs["d_grids"].data_ptr()
        forms = {"fused": fused, "torch": torch_form,
                 "abi_slice": lambda: L.check(lib.hs_bilagrid_slice(C.byref(s), stream), "slice"),
                 "abi_backward_image": lambda: L.check(lib.hs_bilagrid_slice_backward(C.byref(b_image), stream), "backward image"),
                 "abi_backward_grids": lambda: L.check(lib.hs_bilagrid_slice_backward(C.byref(b_grids), stream), "backward grids"),
                 "abi_tv": lambda: L.check(lib.hs_bilagrid_tv(C.byref(t), stream), "tv"),
                 "abi_tv_backward": lambda: L.check(lib.hs_bilagrid_tv_backward(C.byref(t), stream), "tv backward")}
        # the two formulations compute the same thing (fp32 against fp32: to rounding)
        fused()
        gi, gg = image.grad.clone(), grids.grad.clone()
        torch_form()
        agree = dict(d_image_max_abs=float((image.grad - gi).abs().max()), d_grids_max_rel=float((grids.grad - gg).abs().max() / gg.abs().max()))
        ms = {k: [] for k in forms}
        per = max(a.iters // a.rounds, 1)
        for r in range(a.rounds):
            for k, fn in forms.items():
                ms[k] += timed(fn, per, a.warmup if r == 0 else 2)
        res = {k: stats(v) for k, v in ms.items()}
        px = F * H * W
        res["abi_slice"]["frac_of_bytes_floor"] = 24.0 * px / COPY / (res["abi_slice"]["median_ms"] * 1e-3)
        res["abi_backward_image"]["frac_of_bytes_floor"] = 36.0 * px / COPY / (res["abi_backward_image"]["median_ms"] * 1e-3)
        res["bytes_floor_ms"] = dict(forward=24.0 * px / COPY * 1e3, backward=36.0 * px / COPY * 1e3)
        res["abi_sum_ms"] = sum(res[k]["median_ms"] for k in forms if k.startswith("abi_"))
        res["ratio_torch_over_fused"] = res["torch"]["median_ms"] / res["fused"]["median_ms"]
        out["shapes"][name] = dict(F=F, H=H, W=W, workspace_bytes=nbytes, agreement_with_torch=agree, **res)
        print(name, json.dumps(out["shapes"][name]), flush=True)
    if a.example_steps > 0:
        out["example"] = example_psnr(a.example_steps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
