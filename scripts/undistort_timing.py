#!/usr/bin/env python3
"""The fused undistortion + downscale of captured frames (casualhdrsplat_amd.undistort: hs_undistort_remap) against the torch
formulation a trainer writes without it, on the same map,

    x = frames_u8.permute(0, 3, 1, 2).float()                                         # uint8 HWC -> fp32 NCHW
    y = grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False)
    y = avg_pool2d(y, S) / 255

alternated in one process.  Each size is a run of its own, under its own time limit:

    timeout -k 10 300 python scripts/undistort_timing.py --size 1080p_s1 --out profiles/undistort_timing.json && \\
    timeout -k 10 300 python scripts/undistort_timing.py --size 1080p_s2 --out profiles/undistort_timing.json && \\
    timeout -k 10 300 python scripts/undistort_timing.py --size 4k_s2 --out profiles/undistort_timing.json

(a run replaces its own size's entry of the file and keeps the others).  Sizes: 8 uint8 frames of 1920 x 1080 through an OPENCV
camera at S = 1 and S = 2, and of 3840 x 2160 at S = 2.  Device events around each call on the current stream, medians and
p10 / p90 over --iters iterations after a warm-up, the forms alternated in --rounds blocks; every buffer is allocated once.
The remap is set against its byte model F (3 H W + 12 H_out W_out) + 9 H' W' (every frame byte read once, every output
float written once, the map and its mask once) over the rate of a plain device-to-device copy of 1 GiB measured in the same
process (bytes read + bytes written over the median time)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as Fn

from casualhdrsplat_amd import _lib as L
from casualhdrsplat_amd import undistort as U
from casualhdrsplat_amd.scene_io import ColmapCamera

# name -> (W, H, S); the distortion is that of a phone's wide camera, in normalised coordinates
SIZES = {"1080p_s1": (1920, 1080, 1), "1080p_s2": (1920, 1080, 2), "4k_s2": (3840, 2160, 2)}
FRAMES = 8
DISTORTION = [-0.10, 0.03, 0.001, -0.0008]


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
    ap.add_argument("--size", choices=sorted(SIZES), required=True)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4, help="the forms are alternated: --rounds blocks of --iters / --rounds each")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_timing.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("undistort_timing.py measures on an MI355X: no GPU here")
    lib = L.load()
    W, H, S = SIZES[a.size]
    f = 0.78 * W
    cam = ColmapCamera(1, "OPENCV", W, H, np.array([f, f * 1.002, W / 2 + 7.3, H / 2 - 5.1] + DISTORTION))
    umap = U.undistort_map(cam, S)
    Hf, Wf = umap.map.shape[:2]
    Ho, Wo = Hf // S, Wf // S
    gen = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (FRAMES, H, W, 3), dtype=torch.uint8, generator=gen).cuda()
    out = torch.empty((FRAMES, 3, Ho, Wo), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    v = L.hs_undistort_args()
    v.W, v.H, v.Wf, v.Hf, v.F, v.factor, v.frames_u8 = W, H, Wf, Hf, FRAMES, S, 1
    v.map, v.frames, v.out = umap.map.data_ptr(), frames.data_ptr(), out.data_ptr()

    def abi_remap():
        L.check(lib.hs_undistort_remap(C.byref(v), stream), "hs_undistort_remap")

    def undistort_map_call():      # the whole Python call: the host's float64 size rule (Newton on the border) + the map kernel
        U.undistort_map(cam, S)

    # the same map in grid_sample's coordinates: pixel centre i + 0.5 of W is 2 (i + 0.5) / W - 1 without align_corners
    grid = torch.stack([umap.map[..., 0] * (2.0 / W) - 1.0, umap.map[..., 1] * (2.0 / H) - 1.0], dim=-1)[None].expand(FRAMES, Hf, Wf, 2)

    def torch_remap():
        x = frames.permute(0, 3, 1, 2).float()
        y = Fn.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False)
        if S > 1:
            y = Fn.avg_pool2d(y, S)
        return y / 255.0

    abi_remap()
    agree = float((out - torch_remap()).abs().max())       # the two formulations compute the same image, rounded differently

    big = torch.empty(1 << 28, device="cuda")              # 1 GiB
    dst = torch.empty_like(big)

    def copy():
        dst.copy_(big)

    forms = {"abi_remap": abi_remap, "torch_remap": torch_remap, "copy_1GiB": copy, "undistort_map_call": undistort_map_call}
    ms = {k: [] for k in forms}
    per = max(a.iters // a.rounds, 1)
    for r in range(a.rounds):
        for k, fn in forms.items():
            ms[k] += timed(fn, per, a.warmup if r == 0 else 1)
    res = {k: stats(t) for k, t in ms.items()}
    copy_rate = 2.0 * big.numel() * 4 / (res["copy_1GiB"]["median_ms"] * 1e-3)
    model_bytes = FRAMES * (3 * H * W + 12 * Ho * Wo) + 9 * Hf * Wf
    rate = model_bytes / (res["abi_remap"]["median_ms"] * 1e-3)
    res["abi_remap"].update(model_bytes=model_bytes, model_Bps=rate, frac_of_copy_rate=rate / copy_rate,
                            model_floor_ms=model_bytes / copy_rate * 1e3)
    res["ratio_torch_over_abi_remap"] = res["torch_remap"]["median_ms"] / res["abi_remap"]["median_ms"]
    entry = dict(W=W, H=H, factor=S, frames=FRAMES, grid=[Wf, Hf], out=[Wo, Ho], camera="OPENCV " + json.dumps(cam.params.tolist()),
                 iters=a.iters, device=torch.cuda.get_device_name(0), library=os.path.basename(L.LIB_PATH),
                 valid_share=float(umap.valid.float().mean()), copy_rate_Bps=copy_rate, max_abs_difference_to_torch=agree, **res)
    print(a.size, json.dumps(entry), flush=True)
    result = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            result = json.load(fh)
    result["byte_model"] = "F (3 H W + 12 H_out W_out) + 9 H' W'"
    result.setdefault("sizes", {})[a.size] = entry
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
