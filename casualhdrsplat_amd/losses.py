"""The photometric training loss of the published 3DGS train.py, fused (loss.hip, through the C ABI of include/hdrsplat.h):

    loss = (1 - lambda_dssim) * mean|image - target| + lambda_dssim * (1 - SSIM(image, target))

SSIM as the published ssim(): 11 x 11 Gaussian window (sigma 1.5), zero padding, C1 = 0.01^2, C2 = 0.03^2, averaged over
every channel and pixel.  Two kernels forward (the tiles' sums, then one fixed-order fp64 reduction: the same inputs give the
same bits) and one backward, whose upstream gradient is read on the device.  Nothing here reads a value on the host and
nothing is copied or cleared: both functions work inside graphs.GraphedStep.  GPU tensors only (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .rasterizer import _on_device, _stream


def _args(image: torch.Tensor, target: torch.Tensor, lambda_dssim: float) -> L.hs_loss_args:
    H, W = image.shape[-2], image.shape[-1]
    a = L.hs_loss_args()
    a.planes, a.H, a.W = image.numel() // max(1, H * W), H, W
    a.lambda_dssim = lambda_dssim
    a.image, a.target = image.data_ptr(), target.data_ptr()
    return a


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, target, lambda_dssim, with_grad):
        lib = L.load()
        a = _args(image, target, lambda_dssim)
        pairs = lib.hs_loss_workspace_bytes(a.planes, a.H, a.W, 0)
        if pairs < 0:
            L.check(L.HS_EINVAL, "hs_loss_workspace_bytes")
        nbytes = lib.hs_loss_workspace_bytes(a.planes, a.H, a.W, 1) if with_grad else pairs
        ws = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
        if ws.data_ptr() % 256:
            raise RuntimeError("photometric_loss: the allocator returned a workspace that is not 256-byte aligned")
        out = torch.empty(3, dtype=torch.float32, device=image.device)
        a.workspace, a.out = ws.data_ptr(), out.data_ptr()
        a.partials = ws.data_ptr() + pairs if with_grad else None
        with _on_device(image.device):
            L.check(lib.hs_photometric_loss(C.byref(a), _stream(image.device)), "hs_photometric_loss")
        ctx.lambda_dssim = lambda_dssim
        ctx.ws, ctx.pairs = (ws, pairs) if with_grad else (None, 0)
        ctx.save_for_backward(image, target)
        ctx.set_materialize_grads(False)
        terms = out[1:]
        ctx.mark_non_differentiable(terms)
        return out[0], terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        if grad_loss is None:
            return None, None, None, None
        if ctx.ws is None:
            raise RuntimeError("photometric_loss: the forward ran without gradients (no partials were kept)")
        image, target = ctx.saved_tensors
        g = grad_loss.detach().to(torch.float32).contiguous()
        lib = L.load()
        a = _args(image, target, ctx.lambda_dssim)
        d_image = torch.empty_like(image)
        a.partials = ctx.ws.data_ptr() + ctx.pairs
        a.dL_dloss, a.dL_dimage = g.data_ptr(), d_image.data_ptr()
        with _on_device(image.device):
            L.check(lib.hs_photometric_loss_backward(C.byref(a), _stream(image.device)), "hs_photometric_loss_backward")
        return d_image, None, None, None


def _checked(image: torch.Tensor, target: torch.Tensor, lambda_dssim: float):
    for name, t in (("image", image), ("target", target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() not in (3, 4):
            raise ValueError(f"{name} must be [C, H, W] or [B, C, H, W], got {tuple(t.shape)}")
    if image.shape != target.shape:
        raise ValueError(f"image {tuple(image.shape)} and target {tuple(target.shape)} differ in shape")
    if target.requires_grad:
        raise ValueError("target requires grad: the loss has no gradient with respect to the target (detach it)")
    if not (0.0 <= float(lambda_dssim) <= 1.0):
        raise ValueError(f"lambda_dssim={lambda_dssim} outside [0, 1]")
    for name, t in (("image", image), ("target", target)):
        if t.device.type != "cuda":
            raise RuntimeError(f"casualhdrsplat_amd computes the loss on an MI355X only: {name} must live on a cuda (HIP) "
                               "device (no CPU fallback)")
    if image.device != target.device:
        raise ValueError("image and target live on different devices")
    return image.contiguous(), target.contiguous()


def photometric_loss(image: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, return_terms: bool = False):
    """(1 - lambda_dssim) * L1 + lambda_dssim * (1 - SSIM) of `image` against `target` ([C, H, W] or [B, C, H, W], fp32, on
    the GPU, same shape), differentiable in `image`.  A 0-dim tensor; with return_terms=True also the detached
    (l1_mean, ssim_mean) for logging: `loss, (l1, ssim) = photometric_loss(..., return_terms=True)`."""
    image, target = _checked(image, target, lambda_dssim)
    with_grad = torch.is_grad_enabled() and image.requires_grad
    loss, terms = _PhotometricLoss.apply(image, target, float(lambda_dssim), with_grad)
    if return_terms:
        return loss, (terms[0], terms[1])
    return loss


def ssim(image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Mean SSIM of the published ssim() (window 11, size_average=True), differentiable in `image`: the same kernels with
    lambda_dssim = 1, returned as 1 - loss.  Without gradients the forward keeps no partials."""
    return 1.0 - photometric_loss(image, target, 1.0)
