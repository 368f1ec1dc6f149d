#!/usr/bin/env python3
"""Forward + backward of one view from STORED parameters (logit opacities, log scales, unnormalised quaternions), three
ways, alternated in one process:

    torch_wiring   torch.sigmoid / torch.exp / F.normalize on the stored leaves in front of a default rasterizer
                   (the baseline: what a trainer wrote before parameterization="raw" existed)
    raw            GaussianRasterizer(..., parameterization="raw") on the stored leaves
    activated      the default rasterizer on pre-activated leaves: the floor, no activation at all

    python scripts/time_raw_parameters.py --iters 200 --out profiles/raw_parameters_timing.json

Sizes: bench.py's c3 (1 M Gaussians, 1920x1080, SH degree 3, HDR + CRF) and c2 (100 k, 800x800, degree 0).  Sync-free
rasterizers (fixed binning capacity 1.25 x the frame's pairs), device events around each step, medians and p10 / p90 over
--iters iterations after a warm-up.  Also the two kernels alone (hs_activate, hs_activate_backward through the C ABI) with
their algorithmic bytes -- forward 32 B read + 32 B written per Gaussian, backward 32 + 32 + 16 (the stored quaternion)
read and 32 written -- against the copy rate the project quotes."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

import bench
from casualhdrsplat_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib, synthetic as S

PEAK, COPY = 8.0e12, 6.29e12
FWD_BYTES, BWD_BYTES = 64, 112          # per Gaussian


def time_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(v):
    v = sorted(v)
    return {"median_ms": statistics.median(v), "p10_ms": v[len(v) // 10], "p90_ms": v[9 * len(v) // 10]}


def build(cfg, dev):
    P, W, H, deg, hdr, _ = cfg
    sc = S.make_scene(P, W, H, deg, seed=0, hdr=hdr)
    cam = sc.camera
    kw = {}
    if hdr:
        kw.update(exposure=sc.exposure.clone().to(dev).requires_grad_(True), crf_table=sc.crf_table.clone().to(dev).requires_grad_(True),
                  crf_range=sc.crf_range)
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=sc.bg.to(dev), scale_modifier=1.0,
        viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev), sh_degree=deg, campos=cam.campos.to(dev),
        prefiltered=False, debug=False, **kw)
    gen = torch.Generator().manual_seed(1)
    stored = dict(means3D=sc.means3D, opacities=torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)), shs=sc.shs, scales=sc.scales.log(),
                  rotations=sc.rotations * torch.exp(torch.empty(P, 1).uniform_(-2.0, 2.0, generator=gen)))
    stored = {k: v.to(dev).contiguous() for k, v in stored.items()}
    return sc, rs, stored


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="c3,c2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_raw_parameters.py measures on the GPU only")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    res = {"iters": a.iters, "device": torch.cuda.get_device_name(0), "copy_rate_Bps": COPY, "sizes": {}}
    for name in a.sizes.split(","):
        cfg = bench.CONFIGS[name]
        P = cfg[0]
        sc, rs, stored = build(cfg, dev)
        dL = sc.dL_dimage.to(dev)
        with torch.no_grad():
            activated = dict(stored, opacities=torch.sigmoid(stored["opacities"]), scales=torch.exp(stored["scales"]),
                             rotations=F.normalize(stored["rotations"]))
            probe = GaussianRasterizer(rs)
            probe(activated["means3D"], torch.zeros(P, 3, device=dev), activated["opacities"], shs=activated["shs"],
                  scales=activated["scales"], rotations=activated["rotations"])
            capacity = int(1.25 * probe.last_num_rendered) + 4096
        extra = [t for t in (rs.exposure, rs.crf_table) if t is not None]

        def make(how):
            src = activated if how == "activated" else stored
            leaf = {k: v.detach().clone().requires_grad_(True) for k, v in src.items()}
            m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
            rast = GaussianRasterizer(rs, capacity=capacity, parameterization="raw" if how == "raw" else "activated")

            def step():
                for t in list(leaf.values()) + [m2] + extra:
                    t.grad = None
                o, s, r = leaf["opacities"], leaf["scales"], leaf["rotations"]
                if how == "torch_wiring":
                    o, s, r = torch.sigmoid(o), torch.exp(s), F.normalize(r)
                out = rast(leaf["means3D"], m2, o, shs=leaf["shs"], scales=s, rotations=r)
                torch.autograd.backward(out[0], grad_tensors=dL)

            return step, rast

        forms = {k: make(k) for k in ("torch_wiring", "raw", "activated")}
        times = {k: [] for k in forms}
        for it in range(a.warmup + a.iters):
            for k, (step, _) in forms.items():          # alternated: every form sees the same clocks and the same neighbours
                ms = time_once(step)
                if it >= a.warmup:
                    times[k].append(ms)
        for _, rast in forms.values():
            rast.check_overflow()

        # the two kernels alone
        act = {k: torch.empty_like(stored[k]) for k in ("opacities", "scales", "rotations")}
        grads = {k: torch.randn_like(stored[k]) for k in act}
        b = _lib.hs_activate_args()
        b.P, b.g_begin, b.g_end = P, 0, P
        b.opacity_raw, b.scales_raw, b.rotations_raw = (stored[k].data_ptr() for k in ("opacities", "scales", "rotations"))
        b.opacities, b.scales, b.rotations = (act[k].data_ptr() for k in ("opacities", "scales", "rotations"))
        b.dL_dopacities, b.dL_dscales, b.dL_drotations = (grads[k].data_ptr() for k in ("opacities", "scales", "rotations"))
        stream = torch.cuda.current_stream().cuda_stream
        kern = {"hs_activate": [], "hs_activate_backward": []}
        for it in range(a.warmup + a.iters):
            for k in kern:
                for g in grads.values():                # (the backward works in place: keep its input in a sane range)
                    g.normal_()
                ms = time_once(lambda: _lib.check(getattr(lib, k)(C.byref(b), stream), k))
                if it >= a.warmup:
                    kern[k].append(ms)
        row = {k: summary(v) for k, v in times.items()}
        med = {k: v["median_ms"] for k, v in row.items()}
        row["torch_wiring_minus_raw_ms"] = med["torch_wiring"] - med["raw"]
        row["raw_minus_activated_ms"] = med["raw"] - med["activated"]
        for k, per in (("hs_activate", FWD_BYTES), ("hs_activate_backward", BWD_BYTES)):
            row[k] = summary(kern[k])
            nbytes = per * P
            row[k].update(effective_mb=nbytes / 1e6, frac_of_8TBps=nbytes / (row[k]["median_ms"] * 1e-3) / PEAK,
                          frac_of_copy_rate=nbytes / (row[k]["median_ms"] * 1e-3) / COPY)
        res["sizes"][name] = {"P": P, "W": cfg[1], "H": cfg[2], "sh_degree": cfg[3], "hdr": cfg[4], "capacity": capacity, **row}
        for k, v in row.items():
            print(name, k, json.dumps(v), flush=True)
        del forms, stored, activated, act, grads
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
