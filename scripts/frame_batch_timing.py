#!/usr/bin/env python3
"""Forward + backward of one training step over F frames of N poses: ONE rasterizer call (settings.n_frames = F) against F
calls and the torch sum of their gradients -- the same process, the same library, the two forms interleaved, medians over
repeats after a warm-up.  Writes profiles/frame_batch_timing.json.

    python scripts/frame_batch_timing.py [--repeats 30] [--warmup 5] [--limit 120] [--sizes example,c2,c3]

Every size is measured in a CHILD process of its own (a fresh interpreter: this one never touches the GPU), both forms
inside that one process, and the child is ended when it exceeds --limit seconds -- a step that hangs inside a kernel or a
synchronisation included; between steps the child also checks the clock itself and stops cleanly.  The script stops at the
first size that fails or runs out of time and starts nothing after it; a size that does not fit the memory is recorded as
skipped."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"example": dict(P=20_000, W=320, H=208, F=4, N=5, deg=1), "c2": dict(P=100_000, W=800, H=800, F=4, N=8, deg=3),
         "c3": dict(P=1_000_000, W=1920, H=1080, F=2, N=8, deg=3)}
CLOUD = ("means3D", "opacities", "shs", "scales", "rotations")


class OutOfTime(RuntimeError):
    pass


def measure(name, P, W, H, F, N, deg, repeats, warmup, limit):
    import torch
    from casualhdrsplat_amd import GaussianRasterizationSettings, GaussianRasterizer
    from casualhdrsplat_amd import synthetic as S
    dev = torch.device("cuda")
    sc = S.make_scene(P, W, H, deg, seed=0, hdr=True)
    cams = S.perturbed_poses(sc.camera, F * N, seed=1, rot_step_deg=0.05, step=0.002)
    V = torch.stack([c.viewmatrix for c in cams]).to(dev)
    PV = torch.stack([c.projmatrix for c in cams]).to(dev)
    Cp = torch.stack([c.campos for c in cams]).to(dev)
    expo = torch.linspace(0.5, 1.5, F, device=dev).requires_grad_(True)
    crf = sc.crf_table.to(dev).requires_grad_(True)
    leaves = {k: getattr(sc, k).to(dev).requires_grad_(True) for k in CLOUD}
    dL = torch.randn(F, 3, H, W, device=dev)
    cam = sc.camera

    def settings(v, pv, cp, e, n_frames):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=sc.bg.to(dev), scale_modifier=1.0,
            viewmatrix=v[0], projmatrix=pv[0], sh_degree=deg, campos=cp[0], exposure=e, crf_table=crf, crf_range=sc.crf_range,
            viewmatrices=v, projmatrices=pv, camposes=cp, n_frames=n_frames)

    def render(rs):
        m = leaves["means3D"]
        return GaussianRasterizer(rs)(m, torch.zeros_like(m), leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
                                      rotations=leaves["rotations"])[0]

    params = list(leaves.values()) + [expo, crf]

    def batched():
        out = render(settings(V, PV, Cp, expo, F))
        return torch.autograd.grad((out * dL).sum(), params)

    def looped():
        # (autograd's accumulation IS the torch sum of the F gradient sets: one backward of the summed loss)
        loss = 0.0
        for f in range(F):
            s = slice(f * N, (f + 1) * N)
            loss = loss + (render(settings(V[s], PV[s], Cp[s], expo[f], 1)) * dL[f]).sum()
        return torch.autograd.grad(loss, params)

    t_end = time.time() + limit
    times = {"batched": [], "looped": []}
    for it in range(warmup + repeats):
        for form, fn in (("batched", batched), ("looped", looped)) if it % 2 == 0 else (("looped", looped), ("batched", batched)):
            if time.time() > t_end:
                raise OutOfTime(f"{name}: over its limit of {limit} s after {it} steps")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= warmup:
                times[form].append(dt * 1e3)
            if it == 0:
                assert all(torch.isfinite(x).all() for x in g), (name, form)
    med = {k: statistics.median(v) for k, v in times.items()}
    return dict(device=torch.cuda.get_device_name(0), size=name, P=P, W=W, H=H, F=F, N=N, sh_degree=deg, repeats=repeats, warmup=warmup, batched_ms=med["batched"],
                looped_ms=med["looped"], batched_over_looped=med["batched"] / med["looped"],
                batched_ms_min=min(times["batched"]), looped_ms_min=min(times["looped"]))


def one_size(name, repeats, warmup, limit):
    """The child: measures one size and prints its row as one JSON line (exit status 0 also for a size that does not fit)."""
    import torch
    try:
        row = measure(name, repeats=repeats, warmup=warmup, limit=limit, **SIZES[name])
    except torch.cuda.OutOfMemoryError:
        row = dict(size=name, skipped="out of memory", **SIZES[name])
    print("ROW " + json.dumps(row), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds one size may take")
    ap.add_argument("--sizes", default="example,c2,c3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_batch_timing.json"))
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)      # (the child's entry: measure this size only)
    a = ap.parse_args(argv)
    if a.one:
        one_size(a.one, a.repeats, a.warmup, a.limit)
        return 0
    rows, status, device = [], 0, None
    for name in a.sizes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--repeats", str(a.repeats), "--warmup", str(a.warmup),
               "--limit", str(a.limit)]
        try:
            # (the child checks the clock between steps; the margin lets it report that itself before it is ended here)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit + 30)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
            if r.returncode == 0 and line:
                row = json.loads(line[-1][4:])
                device = row.pop("device", device)
            else:
                row = dict(size=name, failed=f"exit status {r.returncode}: {(r.stderr or r.stdout).strip()[-300:]}", **SIZES[name])
        except subprocess.TimeoutExpired:
            row = dict(size=name, failed=f"ended after {a.limit + 30:.0f} s", **SIZES[name])
        rows.append(row)
        print(json.dumps(row), flush=True)
        if "failed" in row:      # the first failure ends the run: nothing more is started on the GPU
            status = 1
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=device, what="forward + backward of one step: one call over F frames (batched) against F calls "
                       "and one backward of the summed loss (looped), both forms in one process per size, interleaved, "
                       "synchronous mode, medians in ms", rows=rows), f, indent=1)
        f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
