"""Score-driven edits of the cloud's rows (rows.hip, through hs_rows_plan and hs_densify_apply of include/hdrsplat.h): prune
by a mask, keep a budget of the best rows, clone / split the k best rows -- on the five cloud tensors AND the optimizer's
moments in one gather, with the optimizer kept alive across the change of P.

    stats = accumulate_contributions(...)                       # importance.py, or any per-Gaussian score of the trainer's
    res = prune_rows(opt, stats.weight_max < 0.01)              # RadSplat-style: one host read of P_out
    res = keep_top_k(opt, stats.weight_max, 900_000)            # a budget: P_out = k, no host read
    res = densify_top_k(opt, dstats.mean_grad(), 50_000, extent=scene_extent)      # P_out = P + k, no host read
    means3D, raw_opacities, shs, log_scales, rotations = (res.params[k] for k in CLOUD_NAMES)

Which score to use, and when, stays with the trainer.  The order on scores is the header's: NaN below every number, -0 equal
to +0, otherwise numeric; among equal scores the lower row wins, so the selection is a function of the inputs alone, bit for
bit.  `densify_top_k` splits a selected row whose largest stored scale exceeds percent_dense * extent (converted to the
stored space as densify.stored_thresholds does) into two children and clones the others, exactly as `densify_and_prune`
does with the rows its gradient threshold selects; nothing is pruned.

`keep_top_k` and `densify_top_k` never wait for the device: the host knows the number of rows that come out before any
kernel runs.  `prune_rows` makes the one read `densify_and_prune` makes.  Survivors keep their moments, new rows get zero
moments, and the optimizer's device step count and running products are not touched (GaussianAdam.replace_params).

`extras`: further per-Gaussian tensors [P, ...] of a 4-byte dtype (a filter_3D, the fields of a ContributionStats or
DensifyStats, a trainer's own arrays) follow the rows, copied bit for bit in the same launches -- sixteen matrices per
launch, the cloud's fifteen first -- and come back at their new length in `RowsResult.extras`.

GPU tensors only, fp32 only: anything else raises (no fallback).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib as L
from .densify import CLOUD_NAMES, _cloud_matrices, _cloud_of, _gather_rows, stored_thresholds
from .optim import _require_gpu
from .rasterizer import _on_device, _stream

COUNT_NAMES = ("P_out", "survivors", "clones", "children", "pruned_sources", "split_sources", "P_in", "ties")


@dataclass
class RowsResult:
    params: dict             # CLOUD_NAMES -> the new leaf tensors (requires_grad as the old ones)
    row_map: torch.Tensor    # int32 [P_out]: kind << 30 | source row (see source / kind)
    counts: torch.Tensor     # int32 [8] ON THE DEVICE: COUNT_NAMES (reading it is the caller's wait)
    P_out: int
    extras: list             # the `extras` at their new length, in the order given

    @property
    def source(self) -> torch.Tensor:
        """Source row of every output row."""
        return self.row_map & 0x3FFFFFFF

    @property
    def kind(self) -> torch.Tensor:
        """0 survivor, 1 clone, 2 / 3 child k = 0 / 1 (HS_DENSIFY_KIND_*)."""
        return (self.row_map >> 30) & 3


def _check_extras(what, extras, P, dev) -> list:
    if isinstance(extras, torch.Tensor):
        raise TypeError(f"{what}: extras must be a sequence of tensors, not a tensor")
    extras = list(extras)
    for i, t in enumerate(extras):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: extras[{i}] must be a torch.Tensor")
        if t.element_size() != 4 or t.is_complex():
            raise ValueError(f"{what}: extras[{i}] has dtype {t.dtype}; a 4-byte dtype (float32, int32) is needed")
        if t.dim() >= 1 and t.shape[0] == P and t.is_contiguous():
            _require_gpu(t, f"extras[{i}]")
        if t.dim() < 1 or t.shape[0] != P or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{what}: extras[{i}] must be a contiguous tensor [{P}, ...] on the cloud's device, got shape {tuple(t.shape)}")
    return extras


def _check_k(what, k, P) -> int:
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"{what}: k={k!r} must be an int")
    if not 0 <= k <= P:
        raise ValueError(f"{what}: k={k} outside [0, P = {P}]")
    return k


def _check_score(what, score, P, dev) -> torch.Tensor:
    if not isinstance(score, torch.Tensor):
        raise TypeError(f"{what}: score must be a torch.Tensor")
    if score.dtype == torch.float32 and score.shape == (P,) and score.is_contiguous():
        _require_gpu(score, "score")       # (a well-formed tensor in the wrong place: say that)
    if score.dtype != torch.float32 or score.shape != (P,) or score.device != dev or not score.is_contiguous():
        raise ValueError(f"{what}: score must be a contiguous float32 tensor [{P}] on the cloud's device")
    return score


def _check_mask(what, mask, P, dev) -> torch.Tensor:
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{what}: mask must be a torch.Tensor")
    if mask.dtype in (torch.bool, torch.uint8) and mask.shape == (P,) and mask.is_contiguous():
        _require_gpu(mask, "mask")
    if mask.dtype not in (torch.bool, torch.uint8) or mask.shape != (P,) or mask.device != dev or not mask.is_contiguous():
        raise ValueError(f"{what}: mask must be a contiguous bool or uint8 tensor [{P}] on the cloud's device")
    return mask


def _plan_and_gather(what, optimizer, cloud, mode, k, extras, *, score=None, mask=None, tau_split=0.0, flags=0, noise=None) -> RowsResult:
    """hs_rows_plan, the allocations, the gather.  MASK mode reads P_out from page-locked memory; the others know it."""
    P, dev = int(cloud["means3D"].shape[0]), cloud["means3D"].device
    if P >= 1 << 30:
        raise ValueError(f"{what}: {P} Gaussians; the library's limit is 2^30 - 1")
    lib = L.load()
    ws_bytes = lib.hs_rows_workspace_bytes(P)
    if ws_bytes < 0:
        L.check(L.HS_EINVAL, "hs_rows_workspace_bytes")
    specs = _cloud_matrices(what, optimizer, cloud, P, children=mode == L.HS_ROWS_DENSIFY)
    workspace = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    row_map = torch.empty(max(P + (k if mode == L.HS_ROWS_DENSIFY else 0), 1), dtype=torch.int32, device=dev)
    counts = torch.empty(L.HS_DENSIFY_COUNTS, dtype=torch.int32, device=dev)
    counts_host = torch.full((L.HS_DENSIFY_COUNTS,), -1, dtype=torch.int32).pin_memory() if mode == L.HS_ROWS_MASK else None

    a = L.hs_rows_args()
    a.P, a.k, a.mode, a.flags, a.tau_split = P, k, mode, flags, tau_split
    a.score = None if score is None else score.data_ptr()
    a.mask = None if mask is None else mask.data_ptr()
    a.scales = cloud["scales"].data_ptr()
    a.workspace, a.row_map, a.counts = workspace.data_ptr(), row_map.data_ptr(), counts.data_ptr()
    a.counts_host = None if counts_host is None else counts_host.data_ptr()
    with _on_device(dev):
        L.check(lib.hs_rows_plan(C.byref(a), _stream(dev)), "hs_rows_plan")
        if mode == L.HS_ROWS_MASK:
            torch.cuda.current_stream(dev).synchronize()   # the one wait: P_out decides the allocations below
    if mode == L.HS_ROWS_MASK:
        got = [int(x) for x in counts_host.tolist()]
        if got[6] != P or got[0] < 0 or got[0] > P:
            raise RuntimeError(f"hs_rows_plan left counts {got} for {P} Gaussians")
        P_out = got[0]
    else:
        P_out = k if mode == L.HS_ROWS_KEEP else P + k

    dsts = []
    for _, p, _, _, _, _ in specs:
        shape = (P_out,) + tuple(p.shape[1:])
        dsts.append((torch.empty(shape, dtype=torch.float32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev),
                     torch.empty(shape, dtype=torch.float32, device=dev)))
    out_extras = []
    for t in extras:
        out_extras.append(torch.empty((P_out,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev))
    new = _gather_rows(optimizer, cloud, specs, dsts, P, P_out, row_map, flags, noise, list(zip(extras, out_extras)))
    return RowsResult(params={key: new[key] for key in CLOUD_NAMES}, row_map=row_map[:P_out], counts=counts, P_out=P_out,
                      extras=out_extras)


def prune_rows(optimizer, mask, *, extras=()) -> RowsResult:
    """Remove the rows with mask[i] true (a bool or uint8 tensor [P] on the cloud's device; true = the row leaves, as in
    upstream's prune_points) from the cloud `optimizer` updates, its moments and `extras`.  One host read: P_out."""
    what = "prune_rows"
    cloud = _cloud_of(optimizer)
    P, dev = int(cloud["means3D"].shape[0]), cloud["means3D"].device
    mask = _check_mask(what, mask, P, dev)
    extras = _check_extras(what, extras, P, dev)
    return _plan_and_gather(what, optimizer, cloud, L.HS_ROWS_MASK, 0, extras, mask=mask)


def keep_top_k(optimizer, score, k, *, extras=()) -> RowsResult:
    """Keep the k rows with the best `score` (float32 [P]; the header's order: NaN lowest, ties to the lower row) of the cloud
    `optimizer` updates, in source order; the others leave.  No host read, no wait: P_out = k."""
    what = "keep_top_k"
    cloud = _cloud_of(optimizer)
    P, dev = int(cloud["means3D"].shape[0]), cloud["means3D"].device
    score = _check_score(what, score, P, dev)
    k = _check_k(what, k, P)
    extras = _check_extras(what, extras, P, dev)
    return _plan_and_gather(what, optimizer, cloud, L.HS_ROWS_KEEP, k, extras, score=score)


def densify_top_k(optimizer, score, k, *, extent, percent_dense=0.01, raw_scales=True, generator=None, noise=None,
                  extras=()) -> RowsResult:
    """Densify the k rows with the best `score`: a selected row whose largest scale exceeds percent_dense * extent is split
    into two children (scales / 1.6, means drawn inside the source with `noise` [P, 2, 3], indexed by the source row, or a
    draw from `generator`), the others are cloned; every other row survives.  No host read, no wait: P_out = P + k."""
    what = "densify_top_k"
    cloud = _cloud_of(optimizer)
    P, dev = int(cloud["means3D"].shape[0]), cloud["means3D"].device
    score = _check_score(what, score, P, dev)
    k = _check_k(what, k, P)
    extras = _check_extras(what, extras, P, dev)
    try:
        th = stored_thresholds(float(extent), 0.0, float(percent_dense), 0.0, None, bool(raw_scales), False)
    except ValueError as e:
        raise ValueError(str(e).replace("densify_and_prune", what)) from None
    if noise is None:
        noise = torch.randn(P, 2, 3, device=dev, dtype=torch.float32, generator=generator)
    else:
        if not isinstance(noise, torch.Tensor):
            raise TypeError(f"{what}: noise must be a torch.Tensor")
        _require_gpu(noise, "noise")
        if noise.dtype != torch.float32 or noise.shape != (P, 2, 3) or noise.device != dev or not noise.is_contiguous():
            raise ValueError(f"{what}: noise must be a contiguous float32 tensor [{P}, 2, 3] on the cloud's device")
    return _plan_and_gather(what, optimizer, cloud, L.HS_ROWS_DENSIFY, k, extras, score=score, tau_split=th["tau_split"],
                            flags=th["flags"], noise=noise)
