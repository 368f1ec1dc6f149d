"""Bilateral-grid image correction ("Bilateral Guided Radiance Field Processing", SIGGRAPH 2024), fused (bilagrid.hip, through
the C ABI of include/hdrsplat.h): every training frame owns a small 3-D lattice of 3 x 4 affine colour matrices addressed by
pixel position and luma, the rendered image is sliced through it between the rasterizer and the loss, and a total-variation
term keeps the lattice smooth -- per-frame white balance, vignetting and local tone mapping go into the grids instead of
into the radiance.

    grids = BilateralGrid(n_frames, device="cuda")                   # identity-initialised [n_frames, 12, 8, 16, 16]
    image = grids(rasterizer(...)[0], frame_index)                    # [3, H, W] -> [3, H, W]
    loss = photometric_loss(image, target) + 10.0 * grids.tv_loss()

One kernel forward, one backward to the image, two to the grids (a gather per lattice column in a fixed order, no atomics:
the same inputs give the same bits) and two + one for the total variation.  Nothing here reads a value on the host and
nothing is copied or cleared: everything works inside graphs.GraphedStep / torch.cuda.graph, and the grid ids may change
between replays when they are given as a device tensor.  GPU tensors only (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .rasterizer import _on_device, _stream

MAX_L, MAX_XY = 16, 64


def _args(image: torch.Tensor, grids: torch.Tensor, ids: torch.Tensor) -> L.hs_bilagrid_args:
    a = L.hs_bilagrid_args()
    a.F, _, a.H, a.W = image.shape
    a.G, _, a.L, a.Y, a.X = grids.shape
    a.image, a.grids, a.grid_ids = image.data_ptr(), grids.data_ptr(), ids.data_ptr()
    return a


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, grids, ids):
        lib = L.load()
        a = _args(image, grids, ids)
        out = torch.empty_like(image)
        a.out = out.data_ptr()
        with _on_device(image.device):
            L.check(lib.hs_bilagrid_slice(C.byref(a), _stream(image.device)), "hs_bilagrid_slice")
        ctx.save_for_backward(image, grids, ids)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        image, grids, ids = ctx.saved_tensors
        lib = L.load()
        a = _args(image, grids, ids)
        g = grad_out.detach().to(torch.float32).contiguous()
        a.dL_dout = g.data_ptr()
        d_image = d_grids = ws = None
        if ctx.needs_input_grad[0]:
            d_image = torch.empty_like(image)
            a.dL_dimage = d_image.data_ptr()
        if ctx.needs_input_grad[1]:
            nbytes = lib.hs_bilagrid_workspace_bytes(a.F, a.H, a.W, a.G, a.L, a.Y, a.X)
            if nbytes < 0:
                L.check(L.HS_EINVAL, "hs_bilagrid_workspace_bytes")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
            if ws.data_ptr() % 256:
                raise RuntimeError("slice_image: the allocator returned a workspace that is not 256-byte aligned")
            d_grids = torch.empty_like(grids)
            a.workspace, a.dL_dgrids = ws.data_ptr(), d_grids.data_ptr()
        if d_image is not None or d_grids is not None:
            with _on_device(image.device):
                L.check(lib.hs_bilagrid_slice_backward(C.byref(a), _stream(image.device)), "hs_bilagrid_slice_backward")
        return d_image, d_grids, None


def _tv_args(grids: torch.Tensor) -> L.hs_bilagrid_tv_args:
    a = L.hs_bilagrid_tv_args()
    a.G, _, a.L, a.Y, a.X = grids.shape
    a.grids = grids.data_ptr()
    return a


class _TV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        lib = L.load()
        a = _tv_args(grids)
        ws = torch.empty(L.HS_BILAGRID_TV_WORKSPACE_BYTES, dtype=torch.uint8, device=grids.device)
        if ws.data_ptr() % 256:
            raise RuntimeError("tv_loss: the allocator returned a workspace that is not 256-byte aligned")
        out = torch.empty(1, dtype=torch.float32, device=grids.device)
        a.tv, a.workspace = out.data_ptr(), ws.data_ptr()
        with _on_device(grids.device):
            L.check(lib.hs_bilagrid_tv(C.byref(a), _stream(grids.device)), "hs_bilagrid_tv")
        ctx.save_for_backward(grids)
        return out[0]

    @staticmethod
    def backward(ctx, grad_tv):
        (grids,) = ctx.saved_tensors
        lib = L.load()
        a = _tv_args(grids)
        g = grad_tv.detach().to(torch.float32).reshape(1).contiguous()
        d_grids = torch.empty_like(grids)
        a.dL_dtv, a.dL_dgrids = g.data_ptr(), d_grids.data_ptr()
        with _on_device(grids.device):
            L.check(lib.hs_bilagrid_tv_backward(C.byref(a), _stream(grids.device)), "hs_bilagrid_tv_backward")
        return d_grids


def _checked_grids(grids, what: str) -> torch.Tensor:
    if not isinstance(grids, torch.Tensor):
        raise TypeError(f"{what}: grids must be a torch.Tensor")
    if grids.dtype != torch.float32:
        raise TypeError(f"{what}: grids must be float32, got {grids.dtype}")
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"{what}: grids must be [G, 12, L, Y, X], got {tuple(grids.shape)}")
    G, _, Lz, Y, X = grids.shape
    if G < 1 or not (1 <= Lz <= MAX_L) or not (1 <= Y <= MAX_XY) or not (1 <= X <= MAX_XY):
        raise ValueError(f"{what}: grids {tuple(grids.shape)} outside G >= 1, 1 <= L <= {MAX_L}, 1 <= Y, X <= {MAX_XY}")
    if grids.device.type != "cuda":
        raise RuntimeError(f"casualhdrsplat_amd computes {what} on an MI355X only: grids must live on a cuda (HIP) device "
                           "(no CPU fallback)")
    return grids.contiguous()


def _checked(image, grids, grid_ids):
    if not isinstance(image, torch.Tensor):
        raise TypeError("slice_image: image must be a torch.Tensor")
    if image.dtype != torch.float32:
        raise TypeError(f"slice_image: image must be float32, got {image.dtype}")
    if image.dim() not in (3, 4) or image.shape[-3] != 3 or image.numel() == 0:
        raise ValueError(f"slice_image: image must be [3, H, W] or [F, 3, H, W], got {tuple(image.shape)}")
    if image.device.type != "cuda":
        raise RuntimeError("casualhdrsplat_amd computes slice_image on an MI355X only: image must live on a cuda (HIP) device "
                           "(no CPU fallback)")
    grids = _checked_grids(grids, "slice_image")
    if grids.device != image.device:
        raise ValueError("slice_image: image and grids live on different devices")
    F = 1 if image.dim() == 3 else image.shape[0]
    G = grids.shape[0]
    if isinstance(grid_ids, torch.Tensor):
        if grid_ids.dtype != torch.int32:
            raise TypeError(f"slice_image: a grid_ids tensor must be int32, got {grid_ids.dtype}")
        if grid_ids.device != image.device:
            raise RuntimeError("slice_image: a grid_ids tensor must live on the image's device (it is read there, never on the "
                               "host; pass Python ints otherwise)")
        if grid_ids.numel() != F or grid_ids.dim() > 1:
            raise ValueError(f"slice_image: grid_ids must hold one id per frame ({F}), got {tuple(grid_ids.shape)}")
        ids = grid_ids.reshape(F).contiguous()
    else:
        seq = [grid_ids] if isinstance(grid_ids, int) and not isinstance(grid_ids, bool) else grid_ids
        try:
            seq = list(seq)
        except TypeError:
            raise TypeError("slice_image: grid_ids must be an int, a sequence of ints or an int32 device tensor") from None
        if not all(isinstance(i, int) and not isinstance(i, bool) for i in seq):
            raise TypeError("slice_image: grid_ids must be an int, a sequence of ints or an int32 device tensor")
        if len(seq) != F:
            raise ValueError(f"slice_image: grid_ids must hold one id per frame ({F}), got {len(seq)}")
        for i in seq:
            if i >= G:
                raise ValueError(f"slice_image: grid id {i} outside the {G} grids (negative ids mean no grid)")
        ids = torch.tensor([max(i, -1) for i in seq], dtype=torch.int32).to(image.device, non_blocking=True)
    return image.contiguous(), grids, ids


def slice_image(image: torch.Tensor, grids: torch.Tensor, grid_ids) -> torch.Tensor:
    """`image` ([3, H, W] or [F, 3, H, W], fp32, on the GPU: the rasterizer's layout) sliced through the bilateral grids
    `grids` ([G, 12, L, Y, X] fp32): frame f goes through grid grid_ids[f]; differentiable in `image` and `grids`.
    `grid_ids`: an int, a sequence of ints (checked on the host: < G; a negative id means "no grid" -- the frame comes out
    as it went in, e.g. an evaluation view) or an int32 tensor on the image's device, which is never read back (an id
    outside [0, G) is the identity there too) and may be rewritten between replays of a captured graph."""
    single = isinstance(image, torch.Tensor) and image.dim() == 3
    image, grids, ids = _checked(image, grids, grid_ids)
    out = _Slice.apply(image.unsqueeze(0) if single else image, grids, ids)
    return out[0] if single else out


def tv_loss(grids: torch.Tensor) -> torch.Tensor:
    """Total variation of `grids` ([G, 12, L, Y, X] fp32 on the GPU): over the lattice axes of size > 1, the mean squared
    difference of neighbouring cells along the axis.  A 0-dim device tensor, differentiable in `grids`."""
    return _TV.apply(_checked_grids(grids, "tv_loss"))


def identity_grids(num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8, device=None) -> torch.Tensor:
    """[num, 12, grid_W, grid_Y, grid_X] fp32: every cell the identity matrix (coefficients 0, 5, 10 equal to 1)."""
    g = torch.zeros(num, 12, grid_W, grid_Y, grid_X, dtype=torch.float32, device=device)
    g[:, (0, 5, 10)] = 1.0
    return g


class BilateralGrid(torch.nn.Module):
    """`num` bilateral grids of grid_X x grid_Y cells and grid_W luma planes (gsplat's names and defaults), one per training
    frame, initialised to the identity.  forward(image, grid_ids) = slice_image(image, self.grids, grid_ids); tv_loss() the
    total variation of the parameter.  Who shares a grid and how the grids are optimised is the trainer's business."""

    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8, device=None):
        super().__init__()
        if num < 1 or not (1 <= grid_W <= MAX_L) or not (1 <= grid_Y <= MAX_XY) or not (1 <= grid_X <= MAX_XY):
            raise ValueError(f"BilateralGrid: num={num}, grid_X={grid_X}, grid_Y={grid_Y}, grid_W={grid_W} outside num >= 1, "
                             f"1 <= grid_W <= {MAX_L}, 1 <= grid_X, grid_Y <= {MAX_XY}")
        self.grids = torch.nn.Parameter(identity_grids(num, grid_X, grid_Y, grid_W, device))

    def forward(self, image: torch.Tensor, grid_ids) -> torch.Tensor:
        return slice_image(image, self.grids, grid_ids)

    def tv_loss(self) -> torch.Tensor:
        return tv_loss(self.grids)
