"""Per-Gaussian feature compositing (features.hip and featgeo.hip, through hs_composite_features /
hs_composite_features_backward / hs_composite_features_geometry_backward of include/hdrsplat.h): C extra channels stored
per Gaussian -- a semantic or language feature field, a depth or a normal, or a per-Gaussian statistic to look at (ContributionStats.weight_sum, DensifyStats.mean_abs_grad(), filter_3D, a VQ code) --
composited per pixel with the blending weights w = alpha * T of a finished forward:

    out = rasterizer(...)                                   # forward with grad, or keep_state=True under no_grad
    feat = composite_features(out[0], features)             # [n_poses, C, H, W];  features: float32 [P, C]
    loss = (feat.view(F, N, C, H, W).mean(1) - target).square().mean()      # the blur average is the caller's
    loss.backward()                                         # features.grad only

    geo = dict(means3D=means3D, opacities=opacities, scales=scales, rotations=rotations)    # what the forward was given
    feat = composite_features(out[0], features, geometry=geo)
    (image_loss + feature_loss).backward()                  # ... and the four tensors' .grad, added to the rasterizer's own

One replay of the frame instead of ceil(C / 3) rasterizer passes with colors_precomp.  Without `geometry` the gradient
reaches `features` only: the blending weights are constants of the call.  With it the result's autograd node also returns
the gradients of the means, opacities, scales and rotations THROUGH the channels (a depth or normal prior moves Gaussians, an
opacity regulariser on an all-ones channel acts), from a back-to-front replay of its own.  include/hdrsplat.h states both
definitions; tests/features_reference.py restates the first in numpy.  GPU tensors only, fp32 only.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .importance import _WORKSPACES_MAX, _dims_key
from .rasterizer import GaussianRasterizer, _f32c, _on_device, _ptr, _state_of, _stream

MAX_CHANNELS = 512
GEOMETRY_KEYS = ("means3D", "opacities", "scales", "rotations")

_WORKSPACES: dict = {}    # (device, dims) -> the backward's workspace of calls with those dims
_GEOMETRY_WORKSPACES: dict = {}    # (device, dims) -> the geometry backward's workspace (pair records, rows, flags)


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


def geometry_workspace(dims, dev) -> torch.Tensor:
    """The workspace hs_composite_features_geometry_backward uses for forwards of these dims on `dev`: one per (device,
    dims), kept between calls; its size does not depend on C.  Every word the call reads is one it wrote."""
    key = (str(dev),) + _dims_key(dims)
    ws = _GEOMETRY_WORKSPACES.get(key)
    if ws is None:
        nbytes = L.load().hs_composite_features_geometry_workspace_bytes(C.byref(dims))
        if nbytes < 0:
            L.check(L.HS_EINVAL, "hs_composite_features_geometry_workspace_bytes")
        while len(_GEOMETRY_WORKSPACES) >= _WORKSPACES_MAX:
            _GEOMETRY_WORKSPACES.pop(next(iter(_GEOMETRY_WORKSPACES)))
        ws = _GEOMETRY_WORKSPACES[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
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


def _geometry_backward(st, geo, features: torch.Tensor, dL_dout: torch.Tensor):
    """dL_dmeans3D, dL_dopacities, dL_dscales, dL_drotations through the channels, with respect to the tensors the forward
    was GIVEN: under parameterization="raw" (and filter_3D) the rows are converted in place behind the kernels that write
    them, as rasterizer._launch_backward's to_stored does."""
    lib = L.load()
    d = st.dims
    dev = st.geom.device
    P = int(d.P)
    m3, op, sc, ro = geo["values"]
    grads = [torch.empty((P, n), dtype=torch.float32, device=dev) for n in (3, 1, 3, 4)]
    if P == 0:
        return grads
    a = L.hs_composite_features_geometry_args()
    a.dims = d
    a.tanfovx, a.tanfovy, a.scale_modifier, a.flags = st.tanfovx, st.tanfovy, st.scale_modifier, st.flags
    a.viewmatrices, a.projmatrices, a.camposes = _ptr(st.views), _ptr(st.projs), _ptr(st.camposes)
    a.means3D, a.opacities, a.scales, a.rotations = _ptr(m3), _ptr(op), _ptr(sc), _ptr(ro)
    a.geom, a.binning, a.image = st.geom.data_ptr(), st.binning.data_ptr(), st.image.data_ptr()
    a.ws = geometry_workspace(d, dev).data_ptr()
    a.n_channels = int(features.shape[1])
    a.features, a.dL_dout = features.data_ptr(), dL_dout.data_ptr()
    a.dL_dmeans3D, a.dL_dopacities, a.dL_dscales, a.dL_drotations = (g.data_ptr() for g in grads)
    with _on_device(dev):
        L.check(lib.hs_composite_features_geometry_backward(C.byref(a), _stream(dev)), "hs_composite_features_geometry_backward")
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


def _check_geometry(what: str, out, geometry) -> dict:
    """The forward behind `out` as the geometry backward needs it: its state, the VALUES of its means, opacities, scales and
    rotations (the forward's own saved tensors; under parameterization="raw" the activated ones plus the stored ones) and
    the shapes of the passed tensors, which supply the graph edges only."""
    if not isinstance(geometry, dict) or set(geometry) != set(GEOMETRY_KEYS):
        got = sorted(geometry) if isinstance(geometry, dict) else type(geometry).__name__
        raise ValueError(f"{what}: geometry must be a dict with exactly the keys {GEOMETRY_KEYS}, got {got}")
    fn = getattr(out, "grad_fn", None)
    if isinstance(out, GaussianRasterizer) or fn is None or not hasattr(fn, "st") or not hasattr(fn, "saved_tensors"):
        raise ValueError(f"{what}: geometry needs `out` to be an output tensor of a GaussianRasterizer forward with grad enabled "
                         "(its autograd node holds the tensors the forward was given); a keep_state rasterizer after a "
                         "no_grad forward has no graph to send gradients into")
    st = fn.st
    if fn.has[3]:
        raise ValueError(f"{what}: geometry is not supported for a forward with cov3Ds_precomp (no scales and rotations to "
                         "send the covariance gradient to)")
    aux, deferred = getattr(fn, "aux", None) or {}, getattr(fn, "deferred", None) or {}
    if aux.get("reduce_group") is not None or deferred.get("gather_group") is not None:
        raise ValueError(f"{what}: geometry is not supported for a view-parallel forward (reduce_group / gather_group): its "
                         "gradient rows are exchanged by the rasterizer's own backward")
    saved = fn.saved_tensors
    raw = tuple(saved[9:12]) if getattr(fn, "raw", False) else None
    values = (saved[0], saved[1], saved[4], saved[5])
    given = (saved[0],) + raw if raw is not None else values      # what the caller passed to the forward
    dev = st.geom.device
    for k, ref in zip(GEOMETRY_KEYS, given):
        t = geometry[k]
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: geometry[{k!r}] must be a torch.Tensor")
        if t.device != dev:
            raise ValueError(f"{what}: geometry[{k!r}] lives on {t.device}, the forward on {dev}")
        if tuple(t.shape) != tuple(ref.shape):
            raise ValueError(f"{what}: geometry[{k!r}] has shape {tuple(t.shape)}, the forward was given {tuple(ref.shape)}")
        if t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0 and t.data_ptr() != ref.data_ptr():
            raise ValueError(f"{what}: geometry[{k!r}] is not the tensor the forward behind `out` was given")
    return dict(st=st, values=values, raw=raw, filter_3D=getattr(fn, "filter_3D", None) if raw is not None else None)


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


class _CompositeFeaturesGeometry(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, geo, means3D, opacities, scales, rotations):
        # (the four tensors supply the graph edges; the values are the forward's own saved tensors, taken when the node is
        # built: the rasterizer's backward may free its node's before this one runs.  Inputs of that forward only: no cycle)
        st = geo["st"]
        ctx.st, ctx.geo = st, geo
        ctx.n_channels = int(features.shape[1])
        ctx.shapes = tuple(tuple(t.shape) for t in (means3D, opacities, scales, rotations))
        f = _f32c(features, st.geom.device)
        ctx.features = f
        return _features_forward(st, f)

    @staticmethod
    def backward(ctx, dL_dout):
        if dL_dout is None:
            return (None,) * 6
        st = ctx.st
        g = _f32c(dL_dout, st.geom.device)
        need = ctx.needs_input_grad
        grad_f = _features_backward(st, ctx.n_channels, g) if need[0] else None
        geo = (None,) * 4
        if any(need[2:6]):
            geo = tuple(t.view(shape) if on else None
                        for t, shape, on in zip(_geometry_backward(st, ctx.geo, ctx.features, g), ctx.shapes, need[2:6]))
        return (grad_f, None) + geo


def composite_features(out, features: torch.Tensor, geometry=None) -> torch.Tensor:
    """Composite the per-Gaussian `features` with the blending weights of the forward behind `out`:
    result[k, c, p] = sum over the entries g composited at pixel p of pose k, front to back, of w * features[g, c].

    out: what accumulate_contributions accepts -- an output tensor of a GaussianRasterizer forward with grad enabled, or a
         GaussianRasterizer(..., keep_state=True) after a no_grad forward.  Any parameterization, filter_3D, N poses,
         n_frames = F, synchronous or fixed-capacity mode.  The state of THAT forward is used (and kept alive by the result's
         autograd node) whatever the rasterizer renders afterwards.
    features: float32 [P, C] on the forward's device, 1 <= C <= 512.
    Returns float32 [n_poses, C, H, W] (pose k of frame f at f * N + k): no background, no 1 / N, no pose average, not
    normalised by the accumulated opacity; a pixel nothing reaches is 0.  Without `geometry` it requires grad exactly when
    `features` does, and the gradient reaches `features` only.
    geometry: None, or a dict with exactly the keys means3D, opacities, scales, rotations holding the tensors the forward
         behind `out` was given (the stored ones under parameterization="raw").  The result's autograd node then also returns
         the gradients of those four through the channels (hs_composite_features_geometry_backward; under "raw" / filter_3D
         converted to the stored tensors as the rasterizer's backward does), and autograd adds them to what the rasterizer's
         own backward delivers -- in either order.  The VALUES are the forward's own saved tensors: `out` must be an output
         tensor of a forward with grad (a keep_state rasterizer is refused); the passed tensors supply the graph edges only
         and are checked for shape, device and -- where float32, contiguous and 16-byte aligned -- identity.  ValueError for
         a forward with cov3Ds_precomp or a view-parallel one (reduce_group / gather_group).  No gradient reaches the camera
         poses, means2D or the densification statistics through the channels.  `dL_dfeatures` has the same bits either way.
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
    if geometry is None:
        return _CompositeFeatures.apply(features, st)
    geo = _check_geometry(what, out, geometry)
    return _CompositeFeaturesGeometry.apply(features, geo, *(geometry[k] for k in GEOMETRY_KEYS))
