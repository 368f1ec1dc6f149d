"""The 3D smoothing filter of Mip-Splatting (smoothing.hip, through hs_smoothing_filter / hs_smoothing_apply /
hs_smoothing_apply_backward of include/hdrsplat.h).  The rasterizer's `antialiasing` flag is the publication's 2D screen-space
filter; this is the per-Gaussian half: a radius, computed from ALL training cameras in one launch pair, below which no camera
resolves the Gaussian, folded into the scales and opacities the rasterizer runs on.

    filter = compute_filter_3D(xyz, viewmatrices, fx, fy, W, H)         # [P] float32; after every densification
    rast = GaussianRasterizer(settings, parameterization="raw", filter_3D=filter)
    rast.filter_3D = compute_filter_3D(...)                             # a plain attribute: swap it after a refinement

The header states the arithmetic operation by operation; tests/smoothing_reference.py restates it in numpy and the GPU tests
compare bits.  Densify, MCMC and GaussianAdam keep working on the stored, unfiltered tensors, as published.

GPU tensors only, fp32 only: anything else raises (no fallback).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .rasterizer import _on_device, _stream

_NEEDS_GPU = ("casualhdrsplat_amd computes the 3D filter on an MI355X only: xyz must live on a cuda (HIP) device "
              "(no CPU fallback)")


def _per_camera(name: str, v, n_cams: int, dev) -> torch.Tensor:
    """One float32 value per camera on `dev` from a scalar, a sequence or a tensor."""
    if isinstance(v, torch.Tensor):
        t = v.detach().to(device=dev, dtype=torch.float32).reshape(-1)
    elif isinstance(v, (int, float)):
        return torch.full((n_cams,), float(v), dtype=torch.float32, device=dev)
    else:
        t = torch.tensor([float(x) for x in v], dtype=torch.float32, device=dev)
    if t.numel() == 1 and n_cams != 1:
        return t.expand(n_cams)
    if t.numel() != n_cams:
        raise ValueError(f"compute_filter_3D: {name} holds {t.numel()} values for {n_cams} cameras")
    return t


def compute_filter_3D(xyz: torch.Tensor, viewmatrices: torch.Tensor, focal_x, focal_y, width, height, *,
                      return_views: bool = False):
    """filter [P] float32 on xyz's device: ((d_i or D) / max fx) * sqrt(0.2), d_i the smallest depth of Gaussian i over the
    cameras that see it (depth > 0.2, projection within 15 % of the image), D the largest d_i, for a Gaussian seen by none.
    All zeros when no Gaussian is seen or there is no camera.

    viewmatrices: [C, 4, 4] or [F, N, 4, 4] (or [C, 16]) in the rasterizer's transposed convention (Camera.viewmatrix).
    focal_x, focal_y, width, height: pixels; scalars, or one value per camera (sequence or tensor).
    return_views: also return n_views [P] int32, the number of cameras that see each Gaussian.
    Runs under no_grad and waits for nothing."""
    if not isinstance(xyz, torch.Tensor) or not isinstance(viewmatrices, torch.Tensor):
        raise TypeError("compute_filter_3D: xyz and viewmatrices must be torch.Tensors")
    if xyz.dtype != torch.float32:
        raise TypeError(f"compute_filter_3D: xyz must be float32, got {xyz.dtype}")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"compute_filter_3D: xyz must have shape [P, 3], got {tuple(xyz.shape)}")
    if viewmatrices.dtype != torch.float32:
        raise TypeError(f"compute_filter_3D: viewmatrices must be float32, got {viewmatrices.dtype}")
    shape = tuple(viewmatrices.shape)
    if not ((len(shape) in (3, 4) and shape[-2:] == (4, 4)) or (len(shape) == 2 and shape[1] == 16)):
        raise ValueError(f"compute_filter_3D: viewmatrices must have shape [C, 4, 4], [F, N, 4, 4] or [C, 16], got {shape}")
    P, n_cams = int(xyz.shape[0]), viewmatrices.numel() // 16
    if P >= 1 << 30:
        raise ValueError(f"compute_filter_3D: {P} Gaussians; the library's limit is 2^30 - 1")
    if n_cams >= 1 << 20:
        raise ValueError(f"compute_filter_3D: {n_cams} cameras; the library's limit is 2^20 - 1")
    if xyz.device.type != "cuda":
        raise RuntimeError(_NEEDS_GPU)
    dev = xyz.device
    with torch.no_grad():
        intr = torch.stack([_per_camera(n, v, n_cams, dev) for n, v in
                            (("focal_x", focal_x), ("focal_y", focal_y), ("width", width), ("height", height))], dim=1).contiguous()
        xyz = xyz.detach().contiguous()
        views = viewmatrices.detach().to(dev).reshape(n_cams, 16).contiguous()
        out = torch.empty(P, dtype=torch.float32, device=dev)
        n_views = torch.empty(P, dtype=torch.int32, device=dev) if return_views else None
        if P > 0:
            lib = L.load()
            ws_bytes = lib.hs_smoothing_filter_workspace_bytes(P)
            if ws_bytes < 0:
                L.check(L.HS_EINVAL, "hs_smoothing_filter_workspace_bytes")
            workspace = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
            a = L.hs_smoothing_filter_args()
            a.P, a.C = P, n_cams
            a.xyz, a.filter, a.workspace = xyz.data_ptr(), out.data_ptr(), workspace.data_ptr()
            a.viewmatrices = views.data_ptr() if n_cams else None
            a.intrinsics = intr.data_ptr() if n_cams else None
            a.n_views = None if n_views is None else n_views.data_ptr()
            with _on_device(dev):
                L.check(lib.hs_smoothing_filter(C.byref(a), _stream(dev)), "hs_smoothing_filter")
    return (out, n_views) if return_views else out


def check_filter_3D(filter_3D, P: int, dev) -> torch.Tensor:
    """The filter a rasterizer call uses, as a flat [P] view; ValueError unless it is a contiguous float32 [P] or [P, 1]
    tensor on the cloud's device that does not require grad (the filter is a constant of the step)."""
    f = filter_3D
    if not isinstance(f, torch.Tensor):
        raise ValueError("filter_3D must be a torch.Tensor (what compute_filter_3D returns)")
    if f.dtype != torch.float32:
        raise ValueError(f"filter_3D must be float32, got {f.dtype}")
    if tuple(f.shape) not in ((P,), (P, 1)):
        raise ValueError(f"filter_3D must have shape [{P}] or [{P}, 1] (one radius per Gaussian), got {tuple(f.shape)}")
    if not f.is_contiguous():
        raise ValueError("filter_3D must be contiguous")
    if f.requires_grad:
        raise ValueError("filter_3D must not require grad: the filter is a constant and gets no gradient")
    if f.device != dev:
        raise ValueError(f"filter_3D lives on {f.device}, the cloud on {dev}")
    return f.reshape(-1)


def apply_filter_3D(opacity_raw: torch.Tensor, scales_raw: torch.Tensor, filter_3D: torch.Tensor):
    """(opacities, scales) of the stored logits / log scales with the filter folded in (hs_smoothing_apply, one kernel), in
    new tensors of the stored tensors' shapes: s' = sqrt(exp(l)^2 + f^2), o' = sigmoid(x) sqrt(prod_k exp(l_k)^2 / s'_k^2).
    No autograd: the rasterizer's parameterization="raw" path is the differentiable one."""
    for name, t in (("opacity_raw", opacity_raw), ("scales_raw", scales_raw)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"apply_filter_3D: {name} must be a contiguous float32 tensor")
    P = int(scales_raw.numel() // 3)
    if scales_raw.numel() != 3 * P or opacity_raw.numel() != P:
        raise ValueError(f"apply_filter_3D: {opacity_raw.numel()} opacities for {scales_raw.numel()} scale values")
    dev = opacity_raw.device
    if dev.type != "cuda" or scales_raw.device != dev:
        raise RuntimeError(_NEEDS_GPU.replace("xyz", "the cloud"))
    f = check_filter_3D(filter_3D, P, dev)
    with torch.no_grad():
        op = torch.empty(tuple(opacity_raw.shape), dtype=torch.float32, device=dev)
        sc = torch.empty(tuple(scales_raw.shape), dtype=torch.float32, device=dev)
        if P > 0:
            a = L.hs_smoothing_apply_args()
            a.P = P
            a.opacity_raw, a.scales_raw, a.filter = opacity_raw.data_ptr(), scales_raw.data_ptr(), f.data_ptr()
            a.opacities, a.scales = op.data_ptr(), sc.data_ptr()
            with _on_device(dev):
                L.check(L.load().hs_smoothing_apply(C.byref(a), _stream(dev)), "hs_smoothing_apply")
    return op, sc
