"""Depth-normal consistency (normals.hip, through hs_normal_consistency* / hs_gaussian_normals* of include/hdrsplat.h): the
regulariser 2DGS, GOF, RaDe-GS, PGSR and dn-splatter pair with the distortion term.  The composited per-Gaussian normals must
agree with the normals of the surface the composited depth describes -- what turns "compact along the ray" into "a surface",
and the entry point for monocular normal priors.

    color, radii, alpha, invd = rasterizer(...)                         # return_alpha=True, return_invdepth=True
    geo = dict(means3D=means3D, opacities=opacities, scales=scales, rotations=rotations)
    n = gaussian_normals(rotations, scales, means3D, campos)            # [P, 3], world frame
    N = composite_features(color, n, geometry=geo)[0]                   # [3, H, W], sum w n
    loss = image_loss + lam * normal_consistency_loss(invd, N, fx, fy, alpha=alpha, weight=alpha.detach(),
                                                      cam_to_world=viewmatrix[:3, :3]).mean()

One kernel each way for the image-space term (the backward gathers per depth sample with its halo in LDS: no atomics, no
workspace, the same bits on every run) and one each way for the per-Gaussian normal.  Nothing is read on the host, nothing
is cleared or copied: the calls capture into a HIP graph.  GPU tensors only, fp32 only (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from .rasterizer import _f32c, _on_device, _stream


def _nc_args(invdepth, alpha, normals, weight, rot, fx, fy) -> L.hs_normal_consistency_args:
    a = L.hs_normal_consistency_args()
    a.B, a.H, a.W = invdepth.shape
    a.fx, a.fy = fx, fy
    a.invdepth, a.normals = invdepth.data_ptr(), normals.data_ptr()
    a.alpha = None if alpha is None else alpha.data_ptr()
    a.weight = None if weight is None else weight.data_ptr()
    a.cam_to_world = None if rot is None else rot.data_ptr()
    return a


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, invdepth, normals, alpha, weight, rot, fx, fy, want_normals):
        a = _nc_args(invdepth, alpha, normals, weight, rot, fx, fy)
        out = torch.empty_like(invdepth)
        a.out = out.data_ptr()
        dn = None
        if want_normals:
            dn = torch.empty_like(normals)
            a.depth_normals = dn.data_ptr()
        with _on_device(invdepth.device):
            L.check(L.load().hs_normal_consistency(C.byref(a), _stream(invdepth.device)), "hs_normal_consistency")
        ctx.save_for_backward(invdepth, normals, alpha, weight, rot)
        ctx.fxy = (fx, fy)
        if want_normals:
            ctx.mark_non_differentiable(dn)
            return out, dn
        return out

    @staticmethod
    def backward(ctx, grad_out, *_):
        invdepth, normals, alpha, weight, rot = ctx.saved_tensors
        need = ctx.needs_input_grad
        if grad_out is None or not any(need[:3]):
            return (None,) * 8
        a = _nc_args(invdepth, alpha, normals, weight, rot, *ctx.fxy)
        g = _f32c(grad_out, invdepth.device)
        a.dL_dout = g.data_ptr()
        d_inv = d_n = d_a = None
        if need[0]:
            d_inv = torch.empty_like(invdepth)
            a.dL_dinvdepth = d_inv.data_ptr()
        if need[1]:
            d_n = torch.empty_like(normals)
            a.dL_dnormals = d_n.data_ptr()
        if need[2]:
            d_a = torch.empty_like(alpha)
            a.dL_dalpha = d_a.data_ptr()
        with _on_device(invdepth.device):
            L.check(L.load().hs_normal_consistency_backward(C.byref(a), _stream(invdepth.device)), "hs_normal_consistency_backward")
        return d_inv, d_n, d_a, None, None, None, None, None


def _checked_map(what, name, t, like=None, channels=False):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    if like is None:
        if t.dim() not in (2, 3) or t.numel() == 0:
            raise ValueError(f"{what}: {name} must be [H, W] or [B, H, W], got {tuple(t.shape)}")
    else:
        want = tuple(like.shape[:-2]) + (3,) + tuple(like.shape[-2:]) if channels else tuple(like.shape)
        if tuple(t.shape) != want:
            raise ValueError(f"{what}: {name} must be {list(want)} (invdepth is {list(like.shape)}), got {tuple(t.shape)}")
        if t.device != like.device:
            raise ValueError(f"{what}: invdepth and {name} live on different devices")
    return t


def _intrinsic(what, name, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{what}: {name} must be a Python float, got {type(v).__name__}")
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{what}: {name}={v} must be finite and positive")
    return float(v)


def normal_consistency_loss(invdepth, normals, fx, fy, alpha=None, weight=None, cam_to_world=None, return_depth_normals=False):
    """The per-pixel normal-consistency map, float32 of the shape of `invdepth`: w * (1 - <normals, n>) with n the unit normal of
    the surface the depth image describes, at INTERIOR pixels, exactly 0 elsewhere.

    invdepth: [H, W] or [B, H, W], what the rasterizer's return_invdepth delivers (sum w / z).
    alpha:    same shape or None (1), what return_alpha delivers.  A sample is valid when invdepth and alpha are finite and
              > 0; its depth is z = alpha / invdepth, back-projected to P = z ((x + 0.5 - W/2) / fx, (y + 0.5 - H/2) / fy, 1)
              (the principal point is the centre, as everywhere in this rasterizer).  A pixel is interior when it is not on
              the frame's border and it and its four axis neighbours are valid; there
              n_d = c / |c|, c = (P(x, y+1) - P(x, y-1)) x (P(x+1, y) - P(x-1, y)), which faces the camera.
    normals:  [3, H, W] or [B, 3, H, W]: the composited sum w n composite_features returns for gaussian_normals, or any normal
              image.  Used as given: nothing is normalised.
    weight:   None or a map of the shape of invdepth, a constant of the call (2DGS: alpha.detach()).
    cam_to_world: None or a [3, 3] / [B, 3, 3] row-major rotation R taking the depth normal into the frame `normals` is expressed
              in: n = R n_d.  For a view matrix as the rasterizer takes it (the transposed world-to-view matrix) that is
              viewmatrix[:3, :3] read row-major -- its rows are already the columns of the world-to-view rotation.
    fx, fy:   Python floats, the focal lengths in pixels (W / (2 tanfovx), H / (2 tanfovy)).
    return_depth_normals: also return n as [B, 3, H, W] ([3, H, W]), zero off the interior, not differentiable -- for display
              and for supervision by a normal prior.

    Differentiable in normals, invdepth and alpha (each gradient computed only when needed, every element written: exactly 0
    at invalid samples and at samples that feed no interior pixel); weight, fx, fy and cam_to_world receive none.  A frame with
    W < 3 or H < 3 gives zeros.  The weighting and the average are the caller's: lam * normal_consistency_loss(...).mean()."""
    what = "normal_consistency_loss"
    invdepth = _checked_map(what, "invdepth", invdepth)
    single = invdepth.dim() == 2
    normals = _checked_map(what, "normals", normals, invdepth, channels=True)
    if alpha is not None:
        alpha = _checked_map(what, "alpha", alpha, invdepth)
    if weight is not None:
        weight = _checked_map(what, "weight", weight, invdepth).detach()
    fx, fy = _intrinsic(what, "fx", fx), _intrinsic(what, "fy", fy)
    B = 1 if single else invdepth.shape[0]
    H, W = invdepth.shape[-2:]
    if 3 * B * H * W >= 2 ** 31:
        raise ValueError(f"{what}: 3*B*H*W={3 * B * H * W} must be below 2^31")
    if cam_to_world is not None:
        if not isinstance(cam_to_world, torch.Tensor):
            raise TypeError(f"{what}: cam_to_world must be a torch.Tensor")
        if cam_to_world.dtype != torch.float32:
            raise TypeError(f"{what}: cam_to_world must be float32, got {cam_to_world.dtype}")
        if tuple(cam_to_world.shape) not in ((3, 3), (B, 3, 3)):
            raise ValueError(f"{what}: cam_to_world must be [3, 3] or [{B}, 3, 3], got {tuple(cam_to_world.shape)}")
        if cam_to_world.device != invdepth.device:
            raise ValueError(f"{what}: invdepth and cam_to_world live on different devices")
    if invdepth.device.type != "cuda":
        raise RuntimeError(f"casualhdrsplat_amd computes {what} on an MI355X only: invdepth must live on a cuda (HIP) device "
                           "(no CPU fallback)")
    if cam_to_world is not None:
        cam_to_world = cam_to_world.detach().expand(B, 3, 3).contiguous()
    shape = (B, H, W)
    res = _NormalConsistency.apply(invdepth.reshape(shape).contiguous(), normals.reshape(B, 3, H, W).contiguous(),
                                   None if alpha is None else alpha.reshape(shape).contiguous(),
                                   None if weight is None else weight.reshape(shape).contiguous(),
                                   cam_to_world, fx, fy, bool(return_depth_normals))
    if not return_depth_normals:
        return res[0] if single else res
    out, dn = res
    return (out[0], dn[0]) if single else (out, dn)


def _gn_args(rotations, scales, means3D, campos) -> L.hs_gaussian_normals_args:
    a = L.hs_gaussian_normals_args()
    a.P = rotations.shape[0]
    a.rotations, a.scales, a.means3D, a.campos = rotations.data_ptr(), scales.data_ptr(), means3D.data_ptr(), campos.data_ptr()
    return a


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rotations, scales, means3D, campos):
        a = _gn_args(rotations, scales, means3D, campos)
        out = torch.empty((rotations.shape[0], 3), dtype=torch.float32, device=rotations.device)
        a.normals = out.data_ptr()
        with _on_device(rotations.device):
            L.check(L.load().hs_gaussian_normals(C.byref(a), _stream(rotations.device)), "hs_gaussian_normals")
        ctx.save_for_backward(rotations, scales, means3D, campos)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rotations, scales, means3D, campos = ctx.saved_tensors
        if grad_out is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        a = _gn_args(rotations, scales, means3D, campos)
        g = _f32c(grad_out, rotations.device)
        d_rot = torch.empty_like(rotations)
        a.dL_dnormals, a.dL_drotations = g.data_ptr(), d_rot.data_ptr()
        with _on_device(rotations.device):
            L.check(L.load().hs_gaussian_normals_backward(C.byref(a), _stream(rotations.device)), "hs_gaussian_normals_backward")
        return d_rot, None, None, None


def gaussian_normals(rotations, scales, means3D, campos) -> torch.Tensor:
    """The per-Gaussian normal to composite, float32 [P, 3]: the shortest axis of the ellipsoid, turned to the camera.

    rotations [P, 4] (w, x, y, z), not necessarily unit: q / |q| goes through the rotation matrix R the rasterizer builds.
    scales [P, 3]: k = the index of the smallest (the lowest index on a tie).  Any monotone map of the scales gives the same
    k, so the stored log-scales of parameterization="raw" may be passed as they are.
    means3D [P, 3], campos [3] (a device tensor, never read on the host): n = column k of R when it points to the camera
    (n . (campos - mean) >= 0), else its negative.  |q| = 0 gives n = 0.

    Differentiable in `rotations` only (through R and the normalisation; k and the sign are constants; |q| = 0: a zero row);
    scales, means3D and campos receive no gradient."""
    what = "gaussian_normals"
    names = ("rotations", "scales", "means3D", "campos")
    tensors = (rotations, scales, means3D, campos)
    for name, t in zip(names, tensors):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    if rotations.dim() != 2 or rotations.shape[1] != 4:
        raise ValueError(f"{what}: rotations must be [P, 4], got {tuple(rotations.shape)}")
    P = rotations.shape[0]
    for name, t in (("scales", scales), ("means3D", means3D)):
        if tuple(t.shape) != (P, 3):
            raise ValueError(f"{what}: {name} must be [{P}, 3] (rotations is [{P}, 4]), got {tuple(t.shape)}")
    if campos.numel() != 3:
        raise ValueError(f"{what}: campos must hold 3 floats, got {tuple(campos.shape)}")
    for name, t in zip(names, tensors):
        if t.device != rotations.device:
            raise ValueError(f"{what}: rotations and {name} live on different devices")
    if rotations.device.type != "cuda":
        raise RuntimeError(f"casualhdrsplat_amd computes {what} on an MI355X only: rotations must live on a cuda (HIP) device "
                           "(no CPU fallback)")
    if P >= 2 ** 30:
        raise ValueError(f"{what}: P={P} outside [0, 2^30)")
    dev = rotations.device
    rot = rotations.contiguous()
    if rot.data_ptr() % 16:
        rot = rot.clone()
    return _GaussianNormals.apply(rot, _f32c(scales, dev), _f32c(means3D, dev), _f32c(campos.reshape(3), dev))
