"""Depth-distortion loss (distort.hip, through hs_distortion / hs_distortion_backward of include/hdrsplat.h): the regulariser
of Mip-NeRF 360 on the blending weights of a ray (2DGS uses it, gsplat ships it as distloss=True), per pixel of a finished
forward:

    L_p = sum_i sum_j w_i w_j |s_i - s_j|,    w = alpha * T,    s = 1 / z  (the inverse depth out_invdepth composites)

It pulls the weights of a ray together and starves floaters and the semi-transparent haze in front of the camera that
casually captured video with auto-exposure and motion blur invites.

    out = rasterizer(...)                                   # forward with grad
    geo = dict(means3D=means3D, opacities=opacities, scales=scales, rotations=rotations)    # what the forward was given
    loss = image_loss + lam * distortion_loss(out[0], geo).mean()          # the weighting and the average are the caller's
    loss.backward()                                         # the four tensors' .grad, added to the rasterizer's own

    dmap = distortion_loss(out[0])                          # evaluation form: no gradient; also after a no_grad forward of a
                                                            # GaussianRasterizer(..., keep_state=True)

The term is quadratic in the weights and needs prefix sums along the ray, so it exists only inside the compositing loop: one
front-to-back replay of the frame for the map, one back-to-front replay for the gradient.  include/hdrsplat.h states the
definition; tests/distortion_reference.py restates it in numpy.  GPU tensors only, fp32 only.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .features import GEOMETRY_KEYS, _check_geometry
from .importance import _WORKSPACES_MAX, _dims_key
from .rasterizer import _f32c, _on_device, _ptr, _state_of, _stream

_WORKSPACES: dict = {}    # (device, dims) -> the backward's workspace (pair records, rows, flags)


def distortion_workspace(dims, dev) -> torch.Tensor:
    """The workspace hs_distortion_backward uses for forwards of these dims on `dev`: one per (device, dims), kept between
    calls.  Every word the call reads is one it wrote: its contents never matter."""
    key = (str(dev),) + _dims_key(dims)
    ws = _WORKSPACES.get(key)
    if ws is None:
        nbytes = L.load().hs_distortion_workspace_bytes(C.byref(dims))
        if nbytes < 0:
            L.check(L.HS_EINVAL, "hs_distortion_workspace_bytes")
        while len(_WORKSPACES) >= _WORKSPACES_MAX:
            _WORKSPACES.pop(next(iter(_WORKSPACES)))
        ws = _WORKSPACES[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return ws


def _distortion_forward(st):
    """(distortion, moment), float32 [n_poses, H, W] each"""
    d = st.dims
    dev = st.geom.device
    shape = (int(d.n_poses), int(d.H), int(d.W))
    dist = torch.empty(shape, dtype=torch.float32, device=dev)
    moment = torch.empty(shape, dtype=torch.float32, device=dev)
    a = L.hs_distortion_args()
    a.dims = d
    a.geom, a.binning, a.image = st.geom.data_ptr(), st.binning.data_ptr(), st.image.data_ptr()
    a.out_distortion, a.out_moment = dist.data_ptr(), moment.data_ptr()
    with _on_device(dev):
        L.check(L.load().hs_distortion(C.byref(a), _stream(dev)), "hs_distortion")
    return dist, moment


def _distortion_backward(st, geo, moment: torch.Tensor, dL_ddist: torch.Tensor):
    """dL_dmeans3D, dL_dopacities, dL_dscales, dL_drotations with respect to the tensors the forward was GIVEN: under
    parameterization="raw" (and filter_3D) the rows are converted in place behind the kernels that write them, as
    features._geometry_backward does."""
    lib = L.load()
    d = st.dims
    dev = st.geom.device
    P = int(d.P)
    m3, op, sc, ro = geo["values"]
    grads = [torch.empty((P, n), dtype=torch.float32, device=dev) for n in (3, 1, 3, 4)]
    if P == 0:
        return grads
    a = L.hs_distortion_bwd_args()
    a.dims = d
    a.tanfovx, a.tanfovy, a.scale_modifier, a.flags = st.tanfovx, st.tanfovy, st.scale_modifier, st.flags
    a.viewmatrices, a.projmatrices, a.camposes = _ptr(st.views), _ptr(st.projs), _ptr(st.camposes)
    a.means3D, a.opacities, a.scales, a.rotations = _ptr(m3), _ptr(op), _ptr(sc), _ptr(ro)
    a.geom, a.binning, a.image = st.geom.data_ptr(), st.binning.data_ptr(), st.image.data_ptr()
    a.ws = distortion_workspace(d, dev).data_ptr()
    a.moment, a.dL_ddistortion = moment.data_ptr(), dL_ddist.data_ptr()
    a.dL_dmeans3D, a.dL_dopacities, a.dL_dscales, a.dL_drotations = (g.data_ptr() for g in grads)
    with _on_device(dev):
        L.check(lib.hs_distortion_backward(C.byref(a), _stream(dev)), "hs_distortion_backward")
        raw = geo["raw"]
        if raw is not None:
            b = L.hs_activate_args()
            b.P = P
            b.rotations_raw = _ptr(raw[2])
            b.opacities, b.scales, b.rotations = _ptr(op), _ptr(sc), _ptr(ro)
            b.dL_dopacities, b.dL_dscales, b.dL_drotations = a.dL_dopacities, a.dL_dscales, a.dL_drotations
            b.g_begin, b.g_end = 0, P
            filter_3D = geo["filter_3D"]
            if filter_3D is not None:
                b.dL_dopacities, b.dL_dscales = None, None      # (those two tensors: hs_smoothing_apply_backward)
            L.check(lib.hs_activate_backward(C.byref(b), _stream(dev)), "hs_activate_backward")
            if filter_3D is not None:
                f = L.hs_smoothing_apply_args()
                f.P = P
                f.opacity_raw, f.scales_raw, f.filter = _ptr(raw[0]), _ptr(raw[1]), _ptr(filter_3D)
                f.dL_dopacities, f.dL_dscales = a.dL_dopacities, a.dL_dscales
                f.g_begin, f.g_end = 0, P
                L.check(lib.hs_smoothing_apply_backward(C.byref(f), _stream(dev)), "hs_smoothing_apply_backward")
    return grads


class _DistortionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, geo, means3D, opacities, scales, rotations):
        # (the four tensors supply the graph edges; the values are the forward's own saved tensors, taken when the node is
        # built: the rasterizer's backward may free its node's before this one runs.  Inputs of that forward only: no cycle)
        st = geo["st"]
        ctx.st, ctx.geo = st, geo
        ctx.shapes = tuple(tuple(t.shape) for t in (means3D, opacities, scales, rotations))
        dist, ctx.moment = _distortion_forward(st)
        return dist

    @staticmethod
    def backward(ctx, dL_ddist):
        if dL_ddist is None or not any(ctx.needs_input_grad[1:5]):
            return (None,) * 5
        st = ctx.st
        g = _f32c(dL_ddist, st.geom.device)
        grads = _distortion_backward(st, ctx.geo, ctx.moment, g)
        return (None,) + tuple(t.view(shape) if on else None for t, shape, on in zip(grads, ctx.shapes, ctx.needs_input_grad[1:5]))


def distortion_loss(out, geometry=None) -> torch.Tensor:
    """The per-pixel distortion map of the forward behind `out`: float32 [n_poses, H, W] (pose k of frame f at f * N + k),
    map[k, p] = sum_i sum_j w_i w_j |s_i - s_j| over the entries composited at pixel p of pose k, s = 1 / z.  No background
    term, no 1 / N, no pose average, no normalisation; a pixel with fewer than two contributors is exactly 0.

    out: what composite_features accepts -- an output tensor of a GaussianRasterizer forward with grad enabled, or a
         GaussianRasterizer(..., keep_state=True) after a no_grad forward (evaluation form only).  Any parameterization,
         filter_3D, N poses, n_frames = F, synchronous or fixed-capacity mode.  The state of THAT forward is used (and kept
         alive by the result's autograd node) whatever the rasterizer renders afterwards.
    geometry: None -- the map carries no gradient (requires_grad is False); or a dict with exactly the keys means3D,
         opacities, scales, rotations holding the tensors the forward behind `out` was given (the stored ones under
         parameterization="raw").  The result is then an autograd node whose backward returns the gradients of those four
         (hs_distortion_backward; under "raw" / filter_3D converted to the stored tensors as the rasterizer's backward does),
         and autograd adds them to what the rasterizer's own backward delivers -- in either order.  The VALUES are the
         forward's own saved tensors; the passed tensors supply the graph edges only and are checked as composite_features
         checks them (same refusals: a keep_state rasterizer, cov3Ds_precomp, a view-parallel forward).  No gradient reaches
         the camera poses, means2D or the densification statistics through the term.
    The caller's loss is its own: lam * distortion_loss(out[0], geo).mean().  One kernel on the current stream (backward:
    three); nothing waits for the host.  A fixed-capacity forward whose binning overflowed gives all zeros and all-zero
    gradients (the device decides)."""
    what = "distortion_loss"
    if geometry is None:
        return _distortion_forward(_state_of(out))[0]
    _state_of(out)
    geo = _check_geometry(what, out, geometry)
    return _DistortionLoss.apply(geo, *(geometry[k] for k in GEOMETRY_KEYS))
