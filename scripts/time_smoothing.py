#!/usr/bin/env python3
"""The fused 3D smoothing filter (casualhdrsplat_amd.smoothing, smoothing.hip) against the torch formulation a trainer writes
without it, in one process, the forms alternated, medians of device events:

    python scripts/time_smoothing.py --out profiles/smoothing_timing.json

  filter    1 M Gaussians x 300 cameras and 100 k x 100: compute_filter_3D (allocations included) and the bare
            hs_smoothing_filter call against the published per-camera loop (Mip-Splatting's compute_3D_filter: a dozen [P]-sized
            kernels per camera and a boolean-mask update, which waits for the device once per camera) and against the same
            loop with torch.where in place of the masks (no wait).  ms and (Gaussian, camera) pairs per second.
  apply     forward + backward at 1 M rows: hs_smoothing_apply + hs_smoothing_apply_backward (88 bytes per row: 20 read and
            16 written forward, 36 read and 16 written backward) against exp, square, add, sqrt, prod, sigmoid, multiply and
            autograd.  Bytes over time as a fraction of the copy rate measured in the same loop (a 256 MiB device copy).
  one view  forward + backward at 1 M Gaussians / 1080p (bench.py's c3) through a "raw" rasterizer with and without filter_3D.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

import bench
from casualhdrsplat_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib as L, compute_filter_3D, synthetic as S

FILTER_SIZES = {"1M_x_300": (1_000_000, 300), "100k_x_100": (100_000, 100)}
APPLY_ROWS = 1_000_000
APPLY_BYTES = 88
W, H = 1920, 1080


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


def cameras(n, dev):
    """n poses around the default camera of make_scene (the cloud sits in front of it): small rotations and shifts."""
    base = S.make_camera(W, H)
    cams = S.perturbed_poses(base, n, seed=1, rot_step_deg=30.0 / n, step=1.0 / n)
    return torch.stack([c.viewmatrix for c in cams]).to(dev), W / (2 * base.tanfovx), H / (2 * base.tanfovy)


def published_filter(xyz, views, fx, fy, masked):
    """Mip-Splatting's compute_3D_filter, camera by camera (views: transposed convention, R = V[:3, :3], T = V[3, :3])."""
    P = xyz.shape[0]
    distance = torch.ones(P, device=xyz.device) * 100000.0
    valid_points = torch.zeros(P, device=xyz.device, dtype=torch.bool)
    focal = 0.0
    for V in views:
        xyz_cam = xyz @ V[:3, :3] + V[3, :3][None, :]
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * fx + W / 2.0
        y = y / z * fy + H / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * W, x <= W * 1.15), torch.logical_and(y >= -0.15 * H, y <= 1.15 * H))
        valid = torch.logical_and(valid_depth, in_screen)
        if masked:                           # as published: boolean-mask indexing (a nonzero and a host wait per camera)
            distance[valid] = torch.min(distance[valid], z[valid])
        else:
            distance = torch.where(valid, torch.min(distance, z), distance)
        valid_points = torch.logical_or(valid_points, valid)
        focal = max(focal, fx)
    if masked:
        distance[~valid_points] = distance[valid_points].max()
    else:
        distance = torch.where(valid_points, distance, (distance * valid_points).max())
    return distance / focal * (0.2 ** 0.5)


def time_filter(name, P, n_cams, dev, iters, warmup):
    lib = L.load()
    sc = S.make_scene(P, W, H, 0, seed=0)
    xyz = sc.means3D.to(dev).contiguous()
    views, fx, fy = cameras(n_cams, dev)
    ref = published_filter(xyz, views, fx, fy, masked=False)
    got, n_views = compute_filter_3D(xyz, views, fx, fy, W, H, return_views=True)
    seen = n_views > 0
    # (torch's matrix product rounds differently: a projection ON the margin may fall on the other side of it for one camera)
    differ = ((got - ref).abs() > 1e-5 * ref) & seen
    rel = float(differ.float().mean())
    assert rel < 1e-3 and int(seen.sum()) > P // 2, (rel, int(seen.sum()))
    intr = torch.tensor([[fx, fy, W, H]], dtype=torch.float32, device=dev).repeat(n_cams, 1).contiguous()
    flat = views.reshape(n_cams, 16).contiguous()
    out = torch.empty(P, device=dev)
    ws = torch.empty(int(lib.hs_smoothing_filter_workspace_bytes(P)), dtype=torch.uint8, device=dev)
    a = L.hs_smoothing_filter_args()
    a.P, a.C = P, n_cams
    a.xyz, a.viewmatrices, a.intrinsics = xyz.data_ptr(), flat.data_ptr(), intr.data_ptr()
    a.filter, a.workspace = out.data_ptr(), ws.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    forms = {"fused": lambda: compute_filter_3D(xyz, views, fx, fy, W, H),
             "fused_abi": lambda: L.check(lib.hs_smoothing_filter(C.byref(a), stream), "hs_smoothing_filter"),
             "torch_where": lambda: published_filter(xyz, views, fx, fy, masked=False),
             "torch_published": lambda: published_filter(xyz, views, fx, fy, masked=True)}
    row = alternate(forms, iters, warmup)
    pairs = P * n_cams
    for k in row:
        row[k]["pairs_per_s"] = pairs / (row[k]["median_ms"] * 1e-3)
    blocks = (P + 255) // 256
    row.update(P=P, cameras=n_cams, seen_fraction=float(seen.float().mean()), fraction_differing_from_torch=rel,
               workgroups=min(blocks, 2048), workgroups_per_cu=min(blocks, 2048) / 256.0,
               under_occupied=blocks < 2 * 256,     # fewer than two workgroups of 256 threads per compute unit
               ratio_torch_where_over_fused=row["torch_where"]["median_ms"] / row["fused"]["median_ms"],
               ratio_torch_published_over_fused=row["torch_published"]["median_ms"] / row["fused"]["median_ms"])
    print(name, json.dumps(row), flush=True)
    return row


def time_apply(dev, iters, warmup):
    lib = L.load()
    P = APPLY_ROWS
    g = torch.Generator().manual_seed(2)
    x = (3.0 * torch.randn(P, 1, generator=g)).to(dev)
    l = torch.empty(P, 3).uniform_(-9.0, 3.0, generator=g).to(dev)
    f = torch.exp(torch.empty(P).uniform_(-9.0, 1.0, generator=g)).to(dev)
    g_o, g_s = torch.randn(P, 1, generator=g).to(dev), torch.randn(P, 3, generator=g).to(dev)
    op, sc = torch.empty_like(x), torch.empty_like(l)
    d_o, d_s = g_o.clone(), g_s.clone()
    a = L.hs_smoothing_apply_args()
    a.P, a.g_begin, a.g_end = P, 0, P
    a.opacity_raw, a.scales_raw, a.filter = x.data_ptr(), l.data_ptr(), f.data_ptr()
    a.opacities, a.scales, a.dL_dopacities, a.dL_dscales = op.data_ptr(), sc.data_ptr(), d_o.data_ptr(), d_s.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    xt, lt = x.clone().requires_grad_(True), l.clone().requires_grad_(True)

    def fused():
        L.check(lib.hs_smoothing_apply(C.byref(a), stream), "hs_smoothing_apply")
        L.check(lib.hs_smoothing_apply_backward(C.byref(a), stream), "hs_smoothing_apply_backward")

    def torch_form():
        xt.grad = lt.grad = None
        scales = torch.exp(lt)
        scales_square = torch.square(scales)
        det1 = scales_square.prod(dim=1)
        scales_after_square = scales_square + torch.square(f)[:, None]
        det2 = scales_after_square.prod(dim=1)
        coef = torch.sqrt(det1 / det2)
        opacity = torch.sigmoid(xt) * coef[:, None]
        torch.autograd.backward([opacity, torch.sqrt(scales_after_square)], [g_o, g_s])

    # the two agree (the backward works in place: d_o / d_s hold the converted gradients after one call on fresh copies)
    fused()
    torch_form()
    torch.cuda.synchronize()
    err = max(float((d_s - lt.grad).abs().max() / lt.grad.abs().max()), float((d_o - xt.grad).abs().max() / xt.grad.abs().max()))
    assert err < 1e-4, err
    n = 64 * 1024 * 1024
    src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
    src.normal_()

    def refill():          # (in place: keep the gradients the backward converts in a sane range)
        d_o.copy_(g_o)
        d_s.copy_(g_s)

    times = {k: [] for k in ("fused", "torch", "copy_256MiB")}
    for it in range(warmup + iters):
        for k, fn in (("fused", fused), ("torch", torch_form), ("copy_256MiB", lambda: dst.copy_(src))):
            refill()
            ms = time_once(fn)
            if it >= warmup:
                times[k].append(ms)
    row = {k: summary(v) for k, v in times.items()}
    copy_rate = 2.0 * 4.0 * n / (row["copy_256MiB"]["median_ms"] * 1e-3)
    rate = APPLY_BYTES * P / (row["fused"]["median_ms"] * 1e-3)
    row.update(P=P, bytes_per_row=APPLY_BYTES, copy_rate_Bps=copy_rate, fused_Bps=rate, frac_of_copy_rate=rate / copy_rate,
               ratio_torch_over_fused=row["torch"]["median_ms"] / row["fused"]["median_ms"])
    print("apply", json.dumps(row), flush=True)
    return row


def time_view(dev, iters, warmup):
    P, Wv, Hv, deg, hdr, _ = bench.CONFIGS["c3"]
    sc = S.make_scene(P, Wv, Hv, deg, seed=0, hdr=hdr)
    cam = sc.camera
    kw = dict(exposure=sc.exposure.clone().to(dev), crf_table=sc.crf_table.clone().to(dev), crf_range=sc.crf_range) if hdr else {}
    rs = GaussianRasterizationSettings(
        image_height=Hv, image_width=Wv, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=sc.bg.to(dev), scale_modifier=1.0,
        viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev), sh_degree=deg, campos=cam.campos.to(dev),
        prefiltered=False, debug=False, **kw)
    stored = dict(means3D=sc.means3D, opacities=torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)), shs=sc.shs, scales=sc.scales.log(),
                  rotations=sc.rotations)
    stored = {k: v.to(dev).contiguous() for k, v in stored.items()}
    dL = sc.dL_dimage.to(dev)
    filt = compute_filter_3D(stored["means3D"], cam.viewmatrix.to(dev)[None], Wv / (2 * cam.tanfovx), Hv / (2 * cam.tanfovy), Wv, Hv)
    with torch.no_grad():
        probe = GaussianRasterizer(rs, parameterization="raw", filter_3D=filt)
        probe(stored["means3D"], torch.zeros(P, 3, device=dev), stored["opacities"], shs=stored["shs"], scales=stored["scales"],
              rotations=stored["rotations"])
        capacity = int(1.25 * probe.last_num_rendered) + 4096

    def make(filter_3D):
        leaf = {k: v.detach().clone().requires_grad_(True) for k, v in stored.items()}
        m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        rast = GaussianRasterizer(rs, capacity=capacity, parameterization="raw", filter_3D=filter_3D)

        def step():
            for t in list(leaf.values()) + [m2]:
                t.grad = None
            out = rast(leaf["means3D"], m2, leaf["opacities"], shs=leaf["shs"], scales=leaf["scales"], rotations=leaf["rotations"])
            torch.autograd.backward(out[0], grad_tensors=dL)

        return step, rast

    forms = {"raw": make(None), "raw_filter_3D": make(filt)}
    row = alternate({k: v[0] for k, v in forms.items()}, iters, warmup)
    pairs = {k: v[1].check_overflow() for k, v in forms.items()}
    row.update(P=P, W=Wv, H=Hv, sh_degree=deg, hdr=hdr, capacity=capacity, num_rendered=pairs, filter_median=float(filt.median()),
               filter_minus_plain_ms=row["raw_filter_3D"]["median_ms"] - row["raw"]["median_ms"])
    print("one_view", json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=5, help="iterations of the filter comparison (the torch loop takes a while)")
    ap.add_argument("--skip", default="", help="comma-separated: filter, apply, view")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smoothing_timing.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_smoothing.py measures on the GPU only")
    dev = torch.device("cuda", 0)
    skip = set(a.skip.split(","))
    res = {"iters": a.iters, "filter_iters": a.torch_iters, "device": torch.cuda.get_device_name(0)}
    if "filter" not in skip:
        res["filter"] = {k: time_filter(k, P, n, dev, a.torch_iters, 2) for k, (P, n) in FILTER_SIZES.items()}
    if "apply" not in skip:
        res["apply"] = time_apply(dev, a.iters, a.warmup)
    if "view" not in skip:
        res["one_view"] = time_view(dev, a.iters, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
