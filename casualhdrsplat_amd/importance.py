"""Per-Gaussian blending-weight statistics (contrib.hip, through hs_contribution of include/hdrsplat.h): how much each
Gaussian contributes to the images of a finished forward -- the sum, the maximum and the number of its blending weights
w = alpha * T over the pixels, optionally weighted per pixel.  The quantity exists only inside the compositing loop; it is
what contribution-based pruning (RadSplat: max w below a threshold), global significance scores (LightGaussian: hit count,
summed weight) and error-driven densification (sum of error * w) decide from.  WHICH policy to run stays with the trainer:

    stats = ContributionStats(P, device)
    for view in training_views:
        out = rasterizer(...)                                   # forward with grad, or keep_state=True under no_grad
        accumulate_contributions(out, stats)                    # or pixel_weight=per_pixel_error
    prune = stats.weight_max < 0.01

include/hdrsplat.h states the definition; tests/contribution_reference.py restates it in numpy.  GPU tensors only, fp32 only.

The backward-side twin (absgrad.hip, through hs_abs_gradient): the absolute screen-gradient statistic of AbsGS -- per
Gaussian, the sum over the pixels of the MAGNITUDE of each pixel's term of dL/dmean2D, where DensifyStats.grad_accum holds
the magnitude of the sum.  The signed terms cancel across a large blurry Gaussian, which is the one that most needs
splitting.  A GaussianRasterizer given a DensifyStats(P, device, absgrad=True) collects it inside every backward;
accumulate_abs_gradients does the same outside autograd, from explicit upstream gradients:

    stats = DensifyStats(P, device, absgrad=True)
    rast = GaussianRasterizer(settings, densify_stats=stats)        # every backward adds to stats.abs_grad_accum
    ...
    densify_and_prune(opt, stats, extent=extent, grad_threshold=4e-4, absgrad=True)

tests/absgrad_reference.py restates that definition.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib as L
from .rasterizer import DensifyStats, _f32c, _on_device, _state_of, _stream


class ContributionStats:
    """`weight_sum` += sum of e * w, `weight_max` = max(weight_max, e * w), `pixel_count` += pixels with e * w > 0, per
    Gaussian, over every accumulate_contributions call given this object (e: the pixel's weight, 1 without a weight image)."""

    def __init__(self, P: int, device="cuda"):
        self.weight_sum = torch.zeros(P, dtype=torch.float32, device=device)
        self.weight_max = torch.zeros(P, dtype=torch.float32, device=device)
        self.pixel_count = torch.zeros(P, dtype=torch.int32, device=device)

    def reset(self) -> None:
        self.weight_sum.zero_(); self.weight_max.zero_(); self.pixel_count.zero_()

    def resize(self, P: int) -> None:
        """Zeroed statistics for a cloud of P Gaussians on the same device (after a refinement changed P: the rows moved)."""
        dev = self.weight_sum.device
        self.weight_sum = torch.zeros(P, dtype=torch.float32, device=dev)
        self.weight_max = torch.zeros(P, dtype=torch.float32, device=dev)
        self.pixel_count = torch.zeros(P, dtype=torch.int32, device=dev)


_WORKSPACES: dict = {}    # (device, dims) -> the contribution workspace of calls with those dims
_WORKSPACES_MAX = 4


def _dims_key(d) -> tuple:
    return (int(d.P), int(d.W), int(d.H), int(d.n_poses), int(d.capacity), int(d.n_frames))


def contribution_workspace(dims, dev) -> torch.Tensor:
    """The workspace hs_contribution uses for forwards of these dims on `dev`: one per (device, dims), kept between calls.
    Every word is written before it is read: its contents never matter."""
    key = (str(dev),) + _dims_key(dims)
    ws = _WORKSPACES.get(key)
    if ws is None:
        nbytes = L.load().hs_contribution_workspace_bytes(C.byref(dims))
        if nbytes < 0:
            L.check(L.HS_EINVAL, "hs_contribution_workspace_bytes")
        while len(_WORKSPACES) >= _WORKSPACES_MAX:
            _WORKSPACES.pop(next(iter(_WORKSPACES)))
        ws = _WORKSPACES[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return ws


def accumulate_contributions(out, stats: ContributionStats, pixel_weight: Optional[torch.Tensor] = None) -> None:
    """Add the blending-weight statistics of the forward behind `out` to `stats`, in place.

    out: an output tensor of a GaussianRasterizer forward with grad enabled, or a GaussianRasterizer(..., keep_state=True)
         after a no_grad forward (what inspect_state accepts).  Any parameterization, filter_3D, N poses, n_frames = F,
         synchronous or fixed-capacity mode.
    pixel_weight: None (every pixel weighs 1), or float32 [H, W] (one frame) or [F, H, W] on the same device; a pixel whose
         weight is exactly 0 takes part in nothing (a mask).
    Three kernels on the current stream; nothing waits for the host.  A fixed-capacity forward whose binning overflowed
    adds nothing (the device decides), so accumulating before the overflow is known is safe."""
    st = _state_of(out)
    d = st.dims
    P = int(d.P)
    dev = st.geom.device
    for name in ("weight_sum", "weight_max", "pixel_count"):
        t = getattr(stats, name)
        want = torch.int32 if name == "pixel_count" else torch.float32
        if t.dtype != want or tuple(t.shape) != (P,) or t.device != dev or not t.is_contiguous():
            raise ValueError(f"accumulate_contributions: stats.{name} must be a contiguous {want} [{P}] tensor on {dev} "
                             f"(the forward had {P} Gaussians), got {t.dtype} {tuple(t.shape)} on {t.device}")
    F = max(int(d.n_frames), 1)
    H, W = int(d.H), int(d.W)
    if pixel_weight is not None:
        if not isinstance(pixel_weight, torch.Tensor) or pixel_weight.dtype != torch.float32:
            raise TypeError("accumulate_contributions: pixel_weight must be a float32 torch.Tensor")
        if pixel_weight.device != dev:
            raise ValueError(f"accumulate_contributions: pixel_weight lives on {pixel_weight.device}, the forward on {dev}")
        if tuple(pixel_weight.shape) not in (((H, W), (1, H, W)) if F == 1 else ((F, H, W),)):
            raise ValueError("accumulate_contributions: pixel_weight must have shape " +
                             (f"[{H}, {W}] or [1, {H}, {W}]" if F == 1 else f"[{F}, {H}, {W}] (one image per frame)") +
                             f", got {tuple(pixel_weight.shape)}")
        pixel_weight = pixel_weight.detach().contiguous()
    if P == 0:
        return
    a = L.hs_contribution_args()
    a.dims = d
    a.geom, a.binning, a.image = st.geom.data_ptr(), st.binning.data_ptr(), st.image.data_ptr()
    a.ws = contribution_workspace(d, dev).data_ptr()
    a.pixel_weight = None if pixel_weight is None else pixel_weight.data_ptr()
    a.weight_sum, a.weight_max, a.pixel_count = (stats.weight_sum.data_ptr(), stats.weight_max.data_ptr(),
                                                 stats.pixel_count.data_ptr())
    with _on_device(dev):
        L.check(L.load().hs_contribution(C.byref(a), _stream(dev)), "hs_contribution")


_ABS_WORKSPACES: dict = {}    # (device, dims) -> the abs-gradient workspace of calls with those dims


def abs_gradient_workspace(dims, dev) -> torch.Tensor:
    """The workspace hs_abs_gradient uses for forwards of these dims on `dev`: one per (device, dims), kept between calls.
    Every word is written before it is read: its contents never matter."""
    key = (str(dev),) + _dims_key(dims)
    ws = _ABS_WORKSPACES.get(key)
    if ws is None:
        nbytes = L.load().hs_abs_gradient_workspace_bytes(C.byref(dims))
        if nbytes < 0:
            L.check(L.HS_EINVAL, "hs_abs_gradient_workspace_bytes")
        while len(_ABS_WORKSPACES) >= _WORKSPACES_MAX:
            _ABS_WORKSPACES.pop(next(iter(_ABS_WORKSPACES)))
        ws = _ABS_WORKSPACES[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return ws


def _launch_abs_gradient(st, gcol, ghdr, galpha, ginvd, accum: torch.Tensor) -> None:
    """Enqueue hs_abs_gradient for the forward state `st` on the current stream of its device (the caller has made that
    device current).  The gradients are contiguous float32 tensors on that device (or None), `accum` a checked [P] tensor."""
    d = st.dims
    if int(d.P) == 0:
        return
    dev = st.geom.device
    exposure, crf_table = st.keep[0], st.keep[1]
    a = L.hs_abs_gradient_args()
    a.dims = d
    a.flags = st.flags
    a.crf_K, a.crf_umin, a.crf_umax = st.crf_K, st.crf_range[0], st.crf_range[1]
    a.bg = st.bg.data_ptr()
    a.exposure = None if exposure is None else exposure.data_ptr()
    a.crf_table = None if crf_table is None else crf_table.data_ptr()
    a.geom, a.binning, a.image = st.geom.data_ptr(), st.binning.data_ptr(), st.image.data_ptr()
    a.ws = abs_gradient_workspace(d, dev).data_ptr()
    a.dL_dout_color = gcol.data_ptr()
    a.dL_dout_hdr = None if ghdr is None else ghdr.data_ptr()
    a.dL_dout_alpha = None if galpha is None else galpha.data_ptr()
    a.dL_dout_invdepth = None if ginvd is None else ginvd.data_ptr()
    a.abs_grad_accum = accum.data_ptr()
    L.check(L.load().hs_abs_gradient(C.byref(a), _stream(dev)), "hs_abs_gradient")


def _abs_target(what: str, target, P: int, dev) -> torch.Tensor:
    if isinstance(target, DensifyStats):
        if target.abs_grad_accum is None:
            raise ValueError(f"{what}: the DensifyStats has no abs_grad_accum: create it with DensifyStats(P, device, absgrad=True)")
        target = target.abs_grad_accum
    if not isinstance(target, torch.Tensor):
        raise TypeError(f"{what}: target must be a DensifyStats(absgrad=True) or a float32 [P] torch.Tensor")
    if target.dtype != torch.float32 or tuple(target.shape) != (P,) or target.device != dev or not target.is_contiguous():
        raise ValueError(f"{what}: abs_grad_accum must be a contiguous {torch.float32} [{P}] tensor on {dev} "
                         f"(the forward had {P} Gaussians), got {target.dtype} {tuple(target.shape)} on {target.device}")
    return target


def accumulate_abs_gradients(out, dL_dout: torch.Tensor, target, *, dL_dout_hdr: Optional[torch.Tensor] = None,
                             dL_dout_alpha: Optional[torch.Tensor] = None,
                             dL_dout_invdepth: Optional[torch.Tensor] = None) -> None:
    """Add the absolute screen-gradient statistic of the forward behind `out`, under the upstream gradient `dL_dout`, to
    `target`, in place: per frame, abs_grad_accum += sqrt(a_x^2 + a_y^2) with a_x, a_y the sums over the frame's poses and
    pixels of |t_x|, |t_y| (include/hdrsplat.h, hs_abs_gradient).

    out: what accumulate_contributions accepts.
    dL_dout: float32 [3, H, W] (one frame) or [F, 3, H, W]: the gradient with respect to the colour image(s), as autograd
         would hand it to the rasterizer's backward.  dL_dout_hdr: the same shape, the gradient with respect to the radiance
         image(s) of an HDR forward.  dL_dout_alpha / dL_dout_invdepth: [H, W], one frame only.
    target: a DensifyStats(P, device, absgrad=True) or a float32 [P] tensor.  `denom` is never touched.
    Three kernels on the current stream; nothing waits for the host.  A fixed-capacity forward whose binning overflowed
    adds nothing (the device decides)."""
    what = "accumulate_abs_gradients"
    st = _state_of(out)
    d = st.dims
    P, H, W = int(d.P), int(d.H), int(d.W)
    F = max(int(d.n_frames), 1)
    dev = st.geom.device
    accum = _abs_target(what, target, P, dev)
    image_shapes = ((3, H, W), (1, 3, H, W)) if F == 1 else ((F, 3, H, W),)
    image_text = f"[3, {H}, {W}] or [1, 3, {H}, {W}]" if F == 1 else f"[{F}, 3, {H}, {W}] (one image per frame)"
    grads = []
    for name, t, shapes, text, need in (("dL_dout", dL_dout, image_shapes, image_text, True),
                                        ("dL_dout_hdr", dL_dout_hdr, image_shapes, image_text, False),
                                        ("dL_dout_alpha", dL_dout_alpha, ((H, W),), f"[{H}, {W}]", False),
                                        ("dL_dout_invdepth", dL_dout_invdepth, ((H, W),), f"[{H}, {W}]", False)):
        if t is None and not need:
            grads.append(None)
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be a float32 torch.Tensor")
        if t.device != dev:
            raise ValueError(f"{what}: {name} lives on {t.device}, the forward on {dev}")
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{what}: {name} must have shape {text}, got {tuple(t.shape)}")
        grads.append(_f32c(t, dev))
    if F > 1 and (dL_dout_alpha is not None or dL_dout_invdepth is not None):
        raise ValueError(f"{what}: dL_dout_alpha / dL_dout_invdepth are per-image gradients and are not supported with "
                         f"n_frames={F}")
    if dL_dout_hdr is not None and not (st.flags & L.HS_FLAG_HDR):
        raise ValueError(f"{what}: dL_dout_hdr was given, but the forward was not an HDR forward")
    with _on_device(dev):
        _launch_abs_gradient(st, grads[0], grads[1], grads[2], grads[3], accum)
