"""Per-Gaussian feature compositing (features.hip, through hs_composite_features / hs_composite_features_backward of
include/hdrsplat.h): C extra channels stored per Gaussian -- a semantic or language feature field, a depth or a normal, or a
per-Gaussian statistic to look at (ContributionStats.weight_sum, DensifyStats.mean_abs_grad(), filter_3D, a VQ code) --
composited per pixel with the blending weights w = alpha * T of a finished forward:

    out = rasterizer(...)                                   # forward with grad, or keep_state=True under no_grad
    feat = composite_features(out[0], features)             # [n_poses, C, H, W];  features: float32 [P, C]
    loss = (feat.view(F, N, C, H, W).mean(1) - target).square().mean()      # the blur average is the caller's
    loss.backward()                                         # features.grad only

One replay of the frame instead of ceil(C / 3) rasterizer passes with colors_precomp.  The gradient reaches `features` ONLY:
the blending weights are constants of the call, so the geometry (means, covariances, opacities) gets no gradient through
these channels.  include/hdrsplat.h states the definition; tests/features_reference.py restates it in numpy.  GPU tensors
only, fp32 only.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .importance import _WORKSPACES_MAX, _dims_key
from .rasterizer import _f32c, _on_device, _state_of, _stream

MAX_CHANNELS = 512

_WORKSPACES: dict = {}    # (device, dims) -> the backward's workspace of calls with those dims


def feature_workspace(dims, dev) -> torch.Tensor:
    """The workspace hs_composite_features_backward uses for forwards of these dims on `dev`: one per (device, dims), kept
    between calls; its size does not depend on C.  Every word is written before it is read: its contents never matter."""
    key = (str(dev),) + _dims_key(dims)
    ws = _WORKSPACES.get(key)
    if ws is None:
        nbytes = L.load().hs_composite_features_workspace_bytes(C.byref(dims))
        if nbytes < 0:
            L.check(L.HS_EINVAL, "hs_composite_features_workspace_bytes")
        while len(_WORKSPACES) >= _WORKSPACES_MAX:
            _WORKSPACES.pop(next(iter(_WORKSPACES)))
        ws = _WORKSPACES[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return ws


def _features_forward(st, features: torch.Tensor) -> torch.Tensor:
    d = st.dims
    dev = st.geom.device
    n_channels = int(features.shape[1])
    out = torch.empty((int(d.n_poses), n_channels, int(d.H), int(d.W)), dtype=torch.float32, device=dev)
    a = L.hs_composite_features_args()
    a.dims = d
    a.geom, a.binning, a.image = st.geom.data_ptr(), st.binning.data_ptr(), st.image.data_ptr()
    a.n_channels = n_channels
    a.features = features.data_ptr() if features.numel() else None
    a.out = out.data_ptr()
    with _on_device(dev):
        L.check(L.load().hs_composite_features(C.byref(a), _stream(dev)), "hs_composite_features")
    return out


def _features_backward(st, n_channels: int, dL_dout: torch.Tensor) -> torch.Tensor:
    d = st.dims
    dev = st.geom.device
    grad = torch.empty((int(d.P), n_channels), dtype=torch.float32, device=dev)
    if int(d.P) == 0:
        return grad
    a = L.hs_composite_features_bwd_args()
    a.dims = d
    a.geom, a.binning, a.image = st.geom.data_ptr(), st.binning.data_ptr(), st.image.data_ptr()
    a.ws = feature_workspace(d, dev).data_ptr()
    a.n_channels = n_channels
    a.dL_dout = dL_dout.data_ptr()
    a.dL_dfeatures = grad.data_ptr()
    with _on_device(dev):
        L.check(L.load().hs_composite_features_backward(C.byref(a), _stream(dev)), "hs_composite_features_backward")
    return grad


class _CompositeFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, st):
        # the node keeps the forward's state: its three workspaces outlive a later forward of the same rasterizer (every
        # forward allocates fresh ones, so the handle never goes stale).  The state holds inputs of its forward only, never
        # an output: no reference cycle through this node
        ctx.st = st
        ctx.n_channels = int(features.shape[1])
        return _features_forward(st, _f32c(features, st.geom.device))

    @staticmethod
    def backward(ctx, dL_dout):
        if dL_dout is None:
            return None, None
        st = ctx.st
        return _features_backward(st, ctx.n_channels, _f32c(dL_dout, st.geom.device)), None


def composite_features(out, features: torch.Tensor) -> torch.Tensor:
    """Composite the per-Gaussian `features` with the blending weights of the forward behind `out`:
    result[k, c, p] = sum over the entries g composited at pixel p of pose k, front to back, of w * features[g, c].

    out: what accumulate_contributions accepts -- an output tensor of a GaussianRasterizer forward with grad enabled, or a
         GaussianRasterizer(..., keep_state=True) after a no_grad forward.  Any parameterization, filter_3D, N poses,
         n_frames = F, synchronous or fixed-capacity mode.  The state of THAT forward is used (and kept alive by the result's
         autograd node) whatever the rasterizer renders afterwards.
    features: float32 [P, C] on the forward's device, 1 <= C <= 512.
    Returns float32 [n_poses, C, H, W] (pose k of frame f at f * N + k): no background, no 1 / N, no pose average, not
    normalised by the accumulated opacity; a pixel nothing reaches is 0.  It requires grad exactly when `features` does, and
    the gradient reaches `features` only -- never the geometry (means, covariances, opacities) of the forward.
    One kernel on the current stream (backward: three per pass of eight or four channels); nothing waits for the host.  A fixed-capacity
    forward whose binning overflowed gives all zeros, and an all-zero gradient (the device decides)."""
    what = "composite_features"
    st = _state_of(out)
    d = st.dims
    P = int(d.P)
    dev = st.geom.device
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32:
        raise TypeError(f"{what}: features must be a float32 torch.Tensor")
    if features.device != dev:
        raise ValueError(f"{what}: features lives on {features.device}, the forward on {dev}")
    if features.dim() != 2 or int(features.shape[0]) != P:
        raise ValueError(f"{what}: features must have shape [{P}, C] (the forward had {P} Gaussians), got {tuple(features.shape)}")
    if not 1 <= int(features.shape[1]) <= MAX_CHANNELS:
        raise ValueError(f"{what}: C={int(features.shape[1])} outside [1, {MAX_CHANNELS}]")
    return _CompositeFeatures.apply(features, st)
