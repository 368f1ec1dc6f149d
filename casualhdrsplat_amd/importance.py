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
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib as L
from .rasterizer import _on_device, _state_of, _stream


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
