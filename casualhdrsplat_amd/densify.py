"""Densify / prune of the cloud (densify.hip, through hs_densify_plan / hs_densify_apply of include/hdrsplat.h): the
published densify_and_prune -- clone small Gaussians with a large view-space gradient, split large ones into two, prune the
transparent and the oversized -- on the five cloud tensors AND the optimizer's moments in one gather, with the optimizer
kept alive across the change of P.

    stats = DensifyStats(P)
    rast = GaussianRasterizer(settings, densify_stats=stats)
    opt = GaussianAdam(cloud_param_groups(means3D, raw_opacities, shs, log_scales, rotations), eps=1e-15)
    ...
    if step % 100 == 0:
        res = densify_and_prune(opt, stats, extent=scene_extent)
        means3D, raw_opacities, shs, log_scales, rotations = (res.params[k] for k in CLOUD_NAMES)
        # stats is resized and zeroed; P changed: re-create whatever was sized by it

The policy, rule by rule, is in the header.  Thresholds are compared in the STORED space (logit opacities, log scales by
default): they are converted once here, in float64, and rounded to float32.  The children's noise is a tensor
torch.randn(P, 2, 3, generator=generator) drawn on the cloud's device and indexed by the source row: the kernels hold no
random-number generator, so the result is a function of the inputs and that tensor, bit for bit.  Several ranks that hold
the same cloud must pass generators with the same seed.

One wait: the number of rows that come out decides the allocations, so the host reads it (from page-locked memory the
plan's last kernel writes) between the plan and the apply.  New rows get zero moments, survivors keep theirs, and the
optimizer's device step count and running products are not touched (GaussianAdam.replace_params).

GPU tensors only, fp32 only: anything else raises (no fallback).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import torch

from . import _lib as L
from .optim import GaussianAdam, _require_gpu
from .rasterizer import DensifyStats, _on_device, _stream

CLOUD_NAMES = ("means3D", "opacities", "shs", "scales", "rotations")
# cloud_param_groups' group names -> (cloud tensor, floats per row or None = any, role of the parameter matrix)
_GROUPS = {"xyz": ("means3D", 3, L.HS_DENSIFY_MEANS), "opacity": ("opacities", 1, L.HS_DENSIFY_COPY),
           "f_dc": ("shs", None, L.HS_DENSIFY_COPY), "f_rest": ("shs", None, L.HS_DENSIFY_COPY),
           "scaling": ("scales", 3, L.HS_DENSIFY_SCALES), "rotation": ("rotations", 4, L.HS_DENSIFY_COPY)}
COUNT_NAMES = ("P_out", "survivors", "clones", "children", "pruned_sources", "split_sources", "P_in")


@dataclass
class DensifyResult:
    params: dict             # CLOUD_NAMES -> the new leaf tensors (requires_grad as the old ones)
    counts: dict             # COUNT_NAMES -> int
    row_map: torch.Tensor    # int32 [P_out]: kind << 30 | source row (see source / kind)

    @property
    def source(self) -> torch.Tensor:
        """Source row of every output row."""
        return self.row_map & 0x3FFFFFFF

    @property
    def kind(self) -> torch.Tensor:
        """0 survivor, 1 clone, 2 / 3 child k = 0 / 1 (HS_DENSIFY_KIND_*)."""
        return (self.row_map >> 30) & 3


def stored_thresholds(extent: float, grad_threshold: float, percent_dense: float, min_opacity: float, max_screen_size,
                      raw_scales: bool, raw_opacity: bool) -> dict:
    """The fields of hs_densify_args that carry the policy: thresholds in the space the values are stored in, computed in
    float64 (ctypes rounds them to float32 when they enter the struct).  min_opacity <= 0 prunes nothing by opacity, >= 1
    everything; max_screen_size None (or 0) switches the radius test AND the world-size test off, as upstream does."""
    if not (extent > 0.0 and math.isfinite(extent)):
        raise ValueError(f"densify_and_prune: extent={extent} must be positive and finite")
    if not (percent_dense > 0.0):
        raise ValueError(f"densify_and_prune: percent_dense={percent_dense} must be positive")
    if math.isnan(grad_threshold) or math.isnan(min_opacity):
        raise ValueError("densify_and_prune: grad_threshold / min_opacity is NaN")
    tau_split = percent_dense * extent
    sigma_max = 0.1 * extent
    if raw_opacity:
        o_min = -math.inf if min_opacity <= 0.0 else (math.inf if min_opacity >= 1.0 else math.log(min_opacity / (1.0 - min_opacity)))
    else:
        o_min = min_opacity
    screen = int(max_screen_size) if max_screen_size else 0
    if screen < 0:
        raise ValueError(f"densify_and_prune: max_screen_size={max_screen_size} is negative")
    return dict(tau_grad=float(grad_threshold), tau_split=math.log(tau_split) if raw_scales else tau_split, o_min=o_min,
                sigma_max=math.inf if not screen else (math.log(sigma_max) if raw_scales else sigma_max), r_max=screen,
                flags=(L.HS_DENSIFY_RAW_SCALES if raw_scales else 0) | (L.HS_DENSIFY_RAW_OPACITY if raw_opacity else 0))


def _cloud_of(optimizer) -> dict:
    """CLOUD_NAMES -> the optimizer's tensor, found by the group names cloud_param_groups sets."""
    if not isinstance(optimizer, GaussianAdam):
        raise TypeError("densify_and_prune needs a casualhdrsplat_amd.GaussianAdam (its moments are gathered with the cloud)")
    found = {}
    for g in optimizer.param_groups:
        name = g.get("name")
        if name not in _GROUPS:
            if g.get("per_gaussian"):
                raise ValueError(f"densify_and_prune: per_gaussian group {name!r} is none of {sorted(_GROUPS)}: its rows "
                                 "cannot follow the cloud")
            continue
        key, width, _ = _GROUPS[name]
        if len(g["params"]) != 1:
            raise ValueError(f"densify_and_prune: group {name!r} must hold exactly one tensor")
        p = g["params"][0]
        if key in found and found[key] is not p:
            raise ValueError(f"densify_and_prune: groups name two different tensors for {key}")
        _require_gpu(p, f"the {name!r} parameter")
        if p.dtype != torch.float32 or not p.is_contiguous() or p.dim() < 1:
            raise ValueError(f"densify_and_prune: the {name!r} parameter must be a contiguous float32 tensor [P, ...]")
        if width is not None and p.numel() != p.shape[0] * width:
            raise ValueError(f"densify_and_prune: the {name!r} parameter must have {width} floats per Gaussian, got shape {tuple(p.shape)}")
        found[key] = p
    missing = [k for k in CLOUD_NAMES if k not in found]
    if missing:
        raise ValueError(f"densify_and_prune: the optimizer has no group for {missing} (groups are found by the names "
                         "cloud_param_groups sets: xyz, opacity, f_dc / f_rest, scaling, rotation)")
    rows = {int(p.shape[0]) for p in found.values()}
    if len(rows) != 1:
        raise ValueError(f"densify_and_prune: the cloud tensors disagree about the number of Gaussians: {sorted(rows)}")
    if len({p.device for p in found.values()}) != 1:
        raise ValueError("densify_and_prune: the cloud tensors must live on one device")
    return found


def _check_stats(stats, P: int, dev) -> None:
    if not isinstance(stats, DensifyStats):
        raise TypeError("densify_and_prune: stats must be a casualhdrsplat_amd.DensifyStats")
    for t, dt, what in ((stats.grad_accum, torch.float32, "grad_accum"), (stats.denom, torch.float32, "denom"),
                        (stats.max_radii, torch.int32, "max_radii")):
        _require_gpu(t, f"stats.{what}")
        if t.dtype != dt or t.shape != (P,) or t.device != dev or not t.is_contiguous():
            raise ValueError(f"densify_and_prune: stats.{what} must be a contiguous {dt} tensor [{P}] on the cloud's device")


def _cloud_matrices(what, optimizer, cloud, P, children) -> list:
    """The cloud's matrices of one gather, in the order of the optimizer's groups: (cloud name, parameter, exp_avg,
    exp_avg_sq, floats per row, role of the parameter).  `children`: the plan may hold split children, so the means and
    scales take the MEANS and SCALES roles; otherwise every parameter is copied."""
    out, seen = [], set()
    for g in optimizer.param_groups:
        name = g.get("name")
        if name not in _GROUPS:
            continue
        key, _, role = _GROUPS[name]
        if key in seen:
            continue
        seen.add(key)
        p = cloud[key]
        st = optimizer._init_state(p)
        m, v = st["exp_avg"], st["exp_avg_sq"]
        for t in (m, v):
            _require_gpu(t, "every moment tensor")
            if t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous() or t.device != p.device:
                raise ValueError(f"{what}: exp_avg / exp_avg_sq must be contiguous float32 tensors of their parameter's shape")
        stride = p.numel() // P if P else max(1, math.prod(p.shape[1:]))
        out.append((key, p, m, v, stride, role if children else L.HS_DENSIFY_COPY))
    return out


def _gather_rows(optimizer, cloud, specs, dsts, P, P_out, row_map, flags, noise=None, extras=()) -> dict:
    """The second half of every edit of the cloud's rows: hs_densify_apply over the matrices of `specs` (_cloud_matrices)
    into `dsts` (per spec: new parameter, exp_avg, exp_avg_sq, [P_out, ...], allocated by the caller) and over `extras`
    (pairs (source, destination) of 4-byte element tensors, COPY role), HS_DENSIFY_MAX_MATRICES per launch; then the new
    tensors take the old ones' places in the optimizer (GaussianAdam.replace_params).  Returns CLOUD_NAMES -> new leaf."""
    dev = cloud["means3D"].device
    mats = []
    for (_, p, m, v, stride, role), (np_, nm, nv) in zip(specs, dsts):
        mats += [(p, np_, stride, role), (m, nm, stride, L.HS_DENSIFY_ZERO_NEW), (v, nv, stride, L.HS_DENSIFY_ZERO_NEW)]
    for src, dst in extras:
        mats.append((src, dst, src.numel() // P if P else max(1, math.prod(src.shape[1:])), L.HS_DENSIFY_COPY))
    lib = L.load()
    a = L.hs_densify_args()
    a.P, a.P_out, a.flags, a.row_map = P, P_out, flags, row_map.data_ptr()
    a.scales, a.rotations = cloud["scales"].data_ptr(), cloud["rotations"].data_ptr()
    a.noise = None if noise is None else noise.data_ptr()
    with _on_device(dev):
        for first in range(0, len(mats), L.HS_DENSIFY_MAX_MATRICES):
            part = mats[first:first + L.HS_DENSIFY_MAX_MATRICES]
            arr = (L.hs_densify_matrix * len(part))()
            for d, (src, dst, stride, role) in zip(arr, part):
                d.src, d.dst, d.row_stride, d.role = src.data_ptr(), dst.data_ptr(), stride, role
            a.matrices, a.n_matrices = arr, len(part)
            L.check(lib.hs_densify_apply(C.byref(a), _stream(dev)), "hs_densify_apply")
    by_key = {spec[0]: dst for spec, dst in zip(specs, dsts)}
    new, mapping = {}, {}
    for key in CLOUD_NAMES:
        old = cloud[key]
        new[key] = by_key[key][0].requires_grad_(old.requires_grad)
        mapping[old] = by_key[key]
    optimizer.replace_params(mapping)
    return new


def densify_and_prune(optimizer, stats, *, extent, grad_threshold=2e-4, percent_dense=0.01, min_opacity=0.005,
                      max_screen_size=None, raw_scales=True, raw_opacity=True, generator=None, noise=None,
                      absgrad=False) -> DensifyResult:
    """One densification of the cloud `optimizer` updates, from the statistics `stats` collected since the last one.
    Returns the new leaf tensors by name, the counts and the row map; the optimizer holds the new tensors (their moments
    gathered, zero for new rows, step count and running products untouched) and `stats` is zeroed at the new size.
    `noise` ([P, 2, 3] float32 on the device) replaces the draw from `generator`.  absgrad=True: the gradient test reads
    `stats.abs_grad_accum` (the AbsGS statistic, DensifyStats(absgrad=True)) where it otherwise reads `stats.grad_accum` --
    the same kernels, another array; `grad_threshold` stays the caller's (AbsGS trainers raise it)."""
    cloud = _cloud_of(optimizer)
    P = int(cloud["means3D"].shape[0])
    dev = cloud["means3D"].device
    _check_stats(stats, P, dev)
    grad_accum = stats.grad_accum
    if absgrad:
        grad_accum = stats.abs_grad_accum
        if grad_accum is None:
            raise ValueError("densify_and_prune: absgrad=True needs stats.abs_grad_accum: create the statistics with "
                             "DensifyStats(P, device, absgrad=True)")
        _require_gpu(grad_accum, "stats.abs_grad_accum")
        if grad_accum.dtype != torch.float32 or grad_accum.shape != (P,) or grad_accum.device != dev or not grad_accum.is_contiguous():
            raise ValueError(f"densify_and_prune: stats.abs_grad_accum must be a contiguous {torch.float32} tensor [{P}] on the "
                             "cloud's device")
    th = stored_thresholds(float(extent), float(grad_threshold), float(percent_dense), float(min_opacity), max_screen_size,
                           bool(raw_scales), bool(raw_opacity))
    if P >= 1 << 30:
        raise ValueError(f"densify_and_prune: {P} Gaussians; the library's limit is 2^30 - 1")
    if noise is None:
        noise = torch.randn(P, 2, 3, device=dev, dtype=torch.float32, generator=generator)
    else:
        _require_gpu(noise, "noise")
        if noise.dtype != torch.float32 or noise.shape != (P, 2, 3) or noise.device != dev or not noise.is_contiguous():
            raise ValueError(f"densify_and_prune: noise must be a contiguous float32 tensor [{P}, 2, 3] on the cloud's device")
    lib = L.load()
    ws_bytes = lib.hs_densify_workspace_bytes(P)
    if ws_bytes < 0:
        L.check(L.HS_EINVAL, "hs_densify_workspace_bytes")
    workspace = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=dev)
    row_map = torch.empty(max(2 * P, 1), dtype=torch.int32, device=dev)
    counts_dev = torch.empty(L.HS_DENSIFY_COUNTS, dtype=torch.int32, device=dev)
    counts_host = torch.full((L.HS_DENSIFY_COUNTS,), -1, dtype=torch.int32).pin_memory()

    a = L.hs_densify_args()
    a.P, a.P_out = P, 0
    for k, v in th.items():
        setattr(a, k, v)
    a.grad_accum, a.denom, a.max_radii = grad_accum.data_ptr(), stats.denom.data_ptr(), stats.max_radii.data_ptr()
    a.opacities, a.scales = cloud["opacities"].data_ptr(), cloud["scales"].data_ptr()
    a.rotations, a.noise = cloud["rotations"].data_ptr(), noise.data_ptr()
    a.workspace, a.row_map = workspace.data_ptr(), row_map.data_ptr()
    a.counts, a.counts_host = counts_dev.data_ptr(), counts_host.data_ptr()
    with _on_device(dev):
        L.check(lib.hs_densify_plan(C.byref(a), _stream(dev)), "hs_densify_plan")
        torch.cuda.current_stream(dev).synchronize()       # the one wait: P_out decides the allocations below
    got = [int(x) for x in counts_host.tolist()]
    if got[6] != P or got[0] < 0 or got[0] > 2 * P:
        raise RuntimeError(f"hs_densify_plan left counts {got} for {P} Gaussians")
    P_out = got[0]

    # the five tensors and their moments: at most 15 matrices, one launch
    specs = _cloud_matrices("densify_and_prune", optimizer, cloud, P, children=True)
    dsts = []
    # (allocated by the caller of the gather: the poisoned-buffer tests name a buffer by the function that asked for it)
    for _, p, _, _, _, _ in specs:
        shape = (P_out,) + tuple(p.shape[1:])
        dsts.append((torch.empty(shape, dtype=torch.float32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev),
                     torch.empty(shape, dtype=torch.float32, device=dev)))
    new = _gather_rows(optimizer, cloud, specs, dsts, P, P_out, row_map, th["flags"], noise)
    stats.resize(P_out)
    return DensifyResult(params={k: new[k] for k in CLOUD_NAMES}, counts=dict(zip(COUNT_NAMES, got)), row_map=row_map[:P_out])
