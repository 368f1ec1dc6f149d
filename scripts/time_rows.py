#!/usr/bin/env python3
"""The score-driven row edits (casualhdrsplat_amd.rows: keep_top_k, densify_top_k, prune_rows -- hs_rows_plan, allocation, the
gather of the five cloud tensors and both Adam moments) against the torch formulation a trainer writes without them
(torch.topk, a sort of the indices, index_select of the 15 tensors and cat; for the mask p[keep] per tensor), alternated in
one process on the same inputs.

    python scripts/time_rows.py --iters 40 --out profiles/rows_timing.json

Sizes: c3 (1 M Gaussians, SH degree 3) and c2 (100 k, SH degree 0).  Operations: keep_top_k at k = 0.9 P, densify_top_k at
k = 0.05 P, prune_rows with 10 % of the rows marked.  Device events around each call (the fused prune includes its one host
read of P_out, torch's formulations the nonzero() behind every boolean index); every shape is warmed first; medians and
p10 / p90 over --iters iterations.  Every iteration starts from fresh copies of the same cloud (made outside the timed
window).  The PLAN (selection) is also timed alone, through the C ABI into buffers allocated once; "apply" is the whole call
minus the plan (allocation, the gather launch, replace_params).  The torch formulation's selection (topk + sort, or the mask's
nonzero) is timed alone in the same way.  The per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of
this script (--fused-only); `--fold-trace rows_results.db --out profiles/rows_timing.json` adds its medians per kernel and
grid size to the JSON (no GPU needed for that step)."""
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

from casualhdrsplat_amd import GaussianAdam, cloud_param_groups, densify_top_k, keep_top_k, prune_rows
from casualhdrsplat_amd import _lib as L

SIZES = {"c3": (1_000_000, 16), "c2": (100_000, 1)}
NAMES = ("means3D", "opacities", "shs", "scales", "rotations")
OPS = ("keep_top_k", "densify_top_k", "prune_rows")
LOG_1_6 = math.log(1.6)


def make_inputs(P, M, seed):
    g = torch.Generator().manual_seed(seed)
    cloud = dict(means3D=torch.randn(P, 3, generator=g), opacities=2.0 * torch.randn(P, 1, generator=g),
                 shs=torch.randn(P, M, 3, generator=g), scales=math.log(0.02) + 0.7 * torch.randn(P, 3, generator=g),
                 rotations=torch.randn(P, 4, generator=g))
    cloud = {k: v.cuda() for k, v in cloud.items()}
    moments = {k: (0.1 * torch.randn_like(v), 0.01 * torch.rand_like(v)) for k, v in cloud.items()}
    score = torch.rand(P, generator=g).cuda()
    mask = torch.rand(P, generator=g).cuda() < 0.1
    smax = torch.exp(cloud["scales"]).max(dim=1).values.cpu().double()
    extent = 10.0 * float(torch.quantile(smax[:1_000_000], 0.995))
    percent_dense = float(torch.quantile(smax[:1_000_000], 0.667)) / extent
    noise = torch.randn(P, 2, 3, generator=g).cuda()
    return cloud, moments, score, mask, extent, percent_dense, noise


def fused_setup(cloud, moments):
    t = {k: v.clone().requires_grad_(True) for k, v in cloud.items()}
    opt = GaussianAdam(cloud_param_groups(*[t[k] for k in NAMES]), eps=1e-15)
    opt.prepare()
    for k in NAMES:
        opt.state[t[k]]["exp_avg"].copy_(moments[k][0])
        opt.state[t[k]]["exp_avg_sq"].copy_(moments[k][1])
    return opt


def torch_keep(t, mom, score, k):
    idx = torch.topk(score, k).indices.sort().values
    for n in NAMES:
        t[n] = t[n].index_select(0, idx)
        mom[n] = tuple(m.index_select(0, idx) for m in mom[n])
    return t["means3D"].shape[0]


def torch_densify(t, mom, score, k, tau_split, noise):
    P = score.shape[0]
    idx = torch.topk(score, k).indices.sort().values
    big = t["scales"].index_select(0, idx).max(dim=1).values > tau_split
    clone, split = idx[~big], idx[big]
    surv = torch.ones(P, dtype=torch.bool, device=score.device)
    surv[split] = False
    q = torch.nn.functional.normalize(t["rotations"].index_select(0, split))
    w, x, y, z = q.unbind(dim=1)
    rots = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    sg = torch.exp(t["scales"].index_select(0, split))
    kids = [torch.bmm(rots, (sg * noise[split, c]).unsqueeze(-1)).squeeze(-1) + t["means3D"].index_select(0, split) for c in (0, 1)]
    for n in NAMES:
        p = t[n]
        child = p.index_select(0, split)
        if n == "scales":
            child = child - LOG_1_6
        new = [p.index_select(0, clone)] + (kids if n == "means3D" else [child, child])
        t[n] = torch.cat([p[surv]] + new, dim=0)
        mom[n] = tuple(torch.cat([m[surv]] + [torch.zeros_like(x_) for x_ in new], dim=0) for m in mom[n])
    return t["means3D"].shape[0]


def torch_prune(t, mom, mask):
    keep = ~mask
    for n in NAMES:
        t[n] = t[n][keep]
        mom[n] = tuple(m[keep] for m in mom[n])
    return t["means3D"].shape[0]


def time_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


class AbiPlan:
    """hs_rows_plan alone, into buffers allocated once."""

    def __init__(self, mode, P, k, score, mask, scales, tau_split):
        self.lib = L.load()
        self.keep = (torch.empty(self.lib.hs_rows_workspace_bytes(P), dtype=torch.uint8, device="cuda"),
                     torch.empty(P + k + 1, dtype=torch.int32, device="cuda"), torch.empty(8, dtype=torch.int32, device="cuda"),
                     score, mask, scales)
        a = L.hs_rows_args()
        a.P, a.k, a.mode, a.flags, a.tau_split = P, k, mode, L.HS_DENSIFY_RAW_SCALES, tau_split
        a.score, a.mask, a.scales = score.data_ptr(), mask.data_ptr(), scales.data_ptr()
        a.workspace, a.row_map, a.counts, a.counts_host = self.keep[0].data_ptr(), self.keep[1].data_ptr(), self.keep[2].data_ptr(), None
        self.a = a

    def __call__(self):
        L.check(self.lib.hs_rows_plan(C.byref(self.a), torch.cuda.current_stream().cuda_stream), "hs_rows_plan")


def summary(v):
    v = sorted(v)
    return {"median_ms": statistics.median(v), "p10_ms": v[len(v) // 10], "p90_ms": v[9 * len(v) // 10]}


def fold_trace(db_path, out_path):
    """Medians (microseconds) per kernel and grid size of a rocprofv3 kernel-trace database, into the JSON at out_path."""
    import collections
    import re
    import sqlite3
    per = collections.defaultdict(list)
    for name, start, end, grid in sqlite3.connect(db_path).execute("select name, start, end, grid_x from kernels"):
        m = re.search(r"(rows_\w+|densify_\w+)", name)
        if m:
            per[f"{m.group(1)} grid_x={grid}"].append((end - start) / 1e3)
    with open(out_path) as f:
        res = json.load(f)
    res["kernel_trace_us"] = {k: {"launches": len(v), "median": statistics.median(v), "min": min(v)} for k, v in sorted(per.items())}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_trace_us"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fold-trace", default=None, help="a rocprofv3 --kernel-trace database of a --fused-only run: fold it into --out")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true", help="run only the fused path (for the kernel-trace run)")
    ap.add_argument("--sizes", default="c3,c2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.fold_trace:
        return fold_trace(a.fold_trace, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("time_rows.py measures on the GPU only")
    res = {"iters": a.iters, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for name in a.sizes.split(","):
        P, M = SIZES[name]
        cloud, moments, score, mask, extent, percent_dense, noise = make_inputs(P, M, 1)
        tau_split = math.log(percent_dense * extent)
        ks = {"keep_top_k": int(0.9 * P), "densify_top_k": int(0.05 * P), "prune_rows": 0}
        mask_u8 = mask.to(torch.uint8)
        plans = {"keep_top_k": AbiPlan(L.HS_ROWS_KEEP, P, ks["keep_top_k"], score, mask_u8, cloud["scales"], tau_split),
                 "densify_top_k": AbiPlan(L.HS_ROWS_DENSIFY, P, ks["densify_top_k"], score, mask_u8, cloud["scales"], tau_split),
                 "prune_rows": AbiPlan(L.HS_ROWS_MASK, P, 0, score, mask_u8, cloud["scales"], tau_split)}
        fused = {"keep_top_k": lambda o: keep_top_k(o, score, ks["keep_top_k"]),
                 "densify_top_k": lambda o: densify_top_k(o, score, ks["densify_top_k"], extent=extent, percent_dense=percent_dense, noise=noise),
                 "prune_rows": lambda o: prune_rows(o, mask)}
        plain = {"keep_top_k": lambda t, m: torch_keep(t, m, score, ks["keep_top_k"]),
                 "densify_top_k": lambda t, m: torch_densify(t, m, score, ks["densify_top_k"], tau_split, noise),
                 "prune_rows": lambda t, m: torch_prune(t, m, mask)}
        select = {"keep_top_k": lambda: torch.topk(score, ks["keep_top_k"]).indices.sort().values,
                  "densify_top_k": lambda: torch.topk(score, ks["densify_top_k"]).indices.sort().values,
                  "prune_rows": lambda: (~mask).nonzero()}
        out = {"P": P, "M": M, "floats_per_gaussian": 11 + 3 * M}
        for op in OPS:
            t = {"fused": [], "fused_plan": [], "torch": [], "torch_select": []}
            p_fused = p_torch = None
            for it in range(a.warmup + a.iters):
                opt = fused_setup(cloud, moments)
                torch.cuda.synchronize()
                ms, r = time_once(lambda: fused[op](opt))
                p_fused = r.P_out
                del opt, r
                ms_plan, _ = time_once(plans[op])
                if it >= a.warmup:
                    t["fused"].append(ms)
                    t["fused_plan"].append(ms_plan)
                if a.fused_only:
                    continue
                tt = {k: v.clone() for k, v in cloud.items()}
                mm = {k: (m.clone(), v.clone()) for k, (m, v) in moments.items()}
                torch.cuda.synchronize()
                ms, p_torch = time_once(lambda: plain[op](tt, mm))
                del tt, mm
                ms_sel, _ = time_once(select[op])
                if it >= a.warmup:
                    t["torch"].append(ms)
                    t["torch_select"].append(ms_sel)
            assert a.fused_only or p_torch == p_fused, (op, p_fused, p_torch)
            row = {k: summary(v) for k, v in t.items() if v}
            row["fused_apply_ms_derived"] = row["fused"]["median_ms"] - row["fused_plan"]["median_ms"]
            row.update(k=ks[op], P_out=p_fused)
            out[op] = row
            print(name, op, json.dumps(row), flush=True)
        res["sizes"][name] = out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
