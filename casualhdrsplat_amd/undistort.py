"""Lens undistortion of captured frames, fused with the downscale to the training resolution (undistort.hip, through the C ABI
of include/hdrsplat.h): the step between a COLMAP camera with distortion and the pinhole rasterizer with its centred
principal point.

    cam = scene_io.read_cameras("sparse/0/cameras.bin")[1]            # SIMPLE_RADIAL, OPENCV, OPENCV_FISHEYE, ...
    umap = undistort_map(cam, factor=2)                                # once per camera
    targets = undistort_frames(frames_u8, umap)                        # [F, H, W, 3] uint8 -> [F, 3, H_out, W_out] fp32 in [0, 1]
    view = scene_io.colmap_view(image, umap.camera)                    # the pinhole the targets were resampled to

The camera the frames are resampled to (undistorted_camera) is host arithmetic in float64: the largest centred pinhole grid,
at the source's focal lengths, none of whose pixels samples outside the source (COLMAP's blank_pixels = 0 rule).  The map
and the per-frame bilinear remap with its S x S area filter are HIP kernels whose fp32 operation order is stated at the top of
undistort.hip and restated in tests/undistort_reference.py.  GPU tensors only (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import _lib as L
from .rasterizer import _on_device, _stream
from .scene_io import ColmapCamera

MODELS = L.HS_CAMERA_MODELS                  # the index is the model id of COLMAP and of hs_undistort_args.model
FACTORS = (1, 2, 3, 4, 8)
MAX_SIDE = 16384
_N_PARAMS = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4, "SIMPLE_RADIAL": 4, "RADIAL": 5, "OPENCV": 8, "OPENCV_FISHEYE": 8,
             "FULL_OPENCV": 12}
_ONE_FOCAL = ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL")


def intrinsics(camera: ColmapCamera) -> Tuple[float, float, float, float, np.ndarray]:
    """(fx, fy, cx, cy, k): the camera's intrinsics and its distortion coefficients in COLMAP's order (float64).  ValueError
    for a model that is not undistorted here (FOV, THIN_PRISM_FISHEYE, the *_RADIAL_FISHEYE models), a wrong number of
    parameters, or values that are not finite / focal lengths that are not positive."""
    if camera.model not in _N_PARAMS:
        raise ValueError(f"undistort: camera model {camera.model} is not supported (supported: {', '.join(MODELS)})")
    p = np.asarray(camera.params, np.float64).reshape(-1)
    if p.size != _N_PARAMS[camera.model]:
        raise ValueError(f"undistort: model {camera.model} takes {_N_PARAMS[camera.model]} parameters, got {p.size}")
    if not np.all(np.isfinite(p)):
        raise ValueError(f"undistort: camera {camera.id} has parameters that are not finite")
    if camera.model in _ONE_FOCAL:
        fx, fy, cx, cy, k = p[0], p[0], p[1], p[2], p[3:]
    else:
        fx, fy, cx, cy, k = p[0], p[1], p[2], p[3], p[4:]
    if not (fx > 0 and fy > 0):
        raise ValueError(f"undistort: camera {camera.id} has a focal length that is not positive ({fx}, {fy})")
    if not (2 <= int(camera.width) <= MAX_SIDE and 2 <= int(camera.height) <= MAX_SIDE):
        raise ValueError(f"undistort: a {camera.width} x {camera.height} source is outside 2 <= W, H <= {MAX_SIDE}")
    return float(fx), float(fy), float(cx), float(cy), k.copy()


def distort(model: str, k, u, v):
    """The forward model: pinhole (u, v) -> distorted (ud, vd), both in normalised coordinates, in the dtype of u (float64 on
    the host).  `k`: the coefficients after the intrinsics, in COLMAP's order."""
    u, v = np.asarray(u), np.asarray(v)
    if model in ("SIMPLE_PINHOLE", "PINHOLE"):
        return u.copy(), v.copy()
    r2 = u * u + v * v
    if model == "SIMPLE_RADIAL":
        rad = k[0] * r2
        return u + u * rad, v + v * rad
    if model == "RADIAL":
        rad = k[0] * r2 + k[1] * r2 * r2
        return u + u * rad, v + v * rad
    if model in ("OPENCV", "FULL_OPENCV"):
        uv = u * v
        tu = 2 * k[2] * uv + k[3] * (r2 + 2 * u * u)
        tv = 2 * k[3] * uv + k[2] * (r2 + 2 * v * v)
        if model == "OPENCV":
            rad = k[0] * r2 + k[1] * r2 * r2
            return u + u * rad + tu, v + v * rad + tv
        r4, r6 = r2 * r2, r2 * r2 * r2
        s = (1 + k[0] * r2 + k[1] * r4 + k[4] * r6) / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6)
        return u * s + tu, v * s + tv
    if model == "OPENCV_FISHEYE":
        r = np.sqrt(r2)
        t = np.arctan(r)
        t2 = t * t
        td = t * (1 + k[0] * t2 + k[1] * t2 ** 2 + k[2] * t2 ** 3 + k[3] * t2 ** 4)
        tiny = r <= 1e-8
        s = np.where(tiny, 1.0, td / np.where(tiny, 1.0, r))
        return u * s, v * s
    raise ValueError(f"undistort: camera model {model} is not supported (supported: {', '.join(MODELS)})")


def undistort_points(model: str, k, ud, vd, tol: float = 1e-12):
    """The inverse of `distort` in float64: Newton's iteration on the forward model from (ud, vd), with a central-difference
    Jacobian.  ValueError when a point does not reach |distort(u, v) - (ud, vd)| <= tol, or reaches it where the model's
    Jacobian has lost its positive determinant or trace (past a fold of the model, a singular Jacobian, coefficients that are
    not finite)."""
    ud, vd = np.asarray(ud, np.float64), np.asarray(vd, np.float64)
    u, v = ud.copy(), vd.copy()
    h = 1e-6

    def jacobian(u, v):
        au, av = distort(model, k, u + h, v)
        bu, bv = distort(model, k, u - h, v)
        cu, cv = distort(model, k, u, v + h)
        du, dv = distort(model, k, u, v - h)
        return (au - bu) / (2 * h), (cu - du) / (2 * h), (av - bv) / (2 * h), (cv - dv) / (2 * h)

    with np.errstate(all="ignore"):
        for _ in range(60):
            fu, fv = distort(model, k, u, v)
            ru, rv = fu - ud, fv - vd
            if not (np.all(np.isfinite(ru)) and np.all(np.isfinite(rv))):
                break
            if max(np.abs(ru).max(initial=0.0), np.abs(rv).max(initial=0.0)) <= 1e-15:
                break
            j00, j01, j10, j11 = jacobian(u, v)
            det = j00 * j11 - j01 * j10
            u = u - (j11 * ru - j01 * rv) / det
            v = v - (j00 * rv - j10 * ru) / det
        fu, fv = distort(model, k, u, v)
        err = np.maximum(np.abs(fu - ud), np.abs(fv - vd))
        j00, j01, j10, j11 = jacobian(u, v)
        # past a fold of the model the iteration can land on another preimage: there the forward model mirrors or turns
        unfolded = (j00 * j11 - j01 * j10 > 0) & (j00 + j11 > 0)
    if not (np.all(err <= tol) and np.all(unfolded)):                       # (a NaN fails the comparisons)
        raise ValueError(f"undistort: Newton's iteration on the {model} model did not converge to the pinhole preimage (worst "
                         f"residual {float(np.nanmax(err)) if np.any(np.isfinite(err)) else float('nan'):.3g}): degenerate "
                         "distortion")
    return u, v


def undistorted_camera(camera: ColmapCamera, factor: int = 1) -> ColmapCamera:
    """The PINHOLE camera the frames of `camera` are resampled to: the source's fx, fy divided by `factor`, the principal point
    at exactly (W_out / 2, H_out / 2), and the largest size none of whose pixels samples outside the source.  With the
    centres of the source's border pixels undistorted (x = 0.5 and x = W - 0.5 at every row centre, y = 0.5 and y = H - 0.5
    at every column centre; normalised coordinates u = (x - cx) / fx, v = (y - cy) / fy):
        a = min(-max u_left, min u_right),  b = min(-max v_top, min v_bottom),
        W' = 2 factor floor(fx a / factor),  H' = 2 factor floor(fy b / factor),  W_out = W' / factor,  H_out = H' / factor.
    scene_io.colmap_view(image, result) is then the view of the undistorted frames.  ValueError: a size that is not
    positive, a Newton failure, an unsupported model."""
    if int(factor) != factor or factor < 1:
        raise ValueError(f"undistort: factor={factor} must be a positive integer")
    factor = int(factor)
    fx, fy, cx, cy, k = intrinsics(camera)
    W, H = int(camera.width), int(camera.height)
    ys, xs = np.arange(H) + 0.5, np.arange(W) + 0.5
    side = lambda x, y: undistort_points(camera.model, k, (x - cx) / fx, (y - cy) / fy)
    u_left, _ = side(np.full(H, 0.5), ys)
    u_right, _ = side(np.full(H, W - 0.5), ys)
    _, v_top = side(xs, np.full(W, 0.5))
    _, v_bottom = side(xs, np.full(W, H - 0.5))
    a = min(-u_left.max(), u_right.min())
    b = min(-v_top.max(), v_bottom.min())
    Wf = 2 * factor * int(np.floor(fx * a / factor))
    Hf = 2 * factor * int(np.floor(fy * b / factor))
    if Wf <= 0 or Hf <= 0:
        raise ValueError(f"undistort: camera {camera.id} leaves no undistorted image at factor {factor} ({Wf} x {Hf})")
    if Wf > MAX_SIDE or Hf > MAX_SIDE:
        raise ValueError(f"undistort: the undistorted grid {Wf} x {Hf} is outside W', H' <= {MAX_SIDE}")
    Wo, Ho = Wf // factor, Hf // factor
    return ColmapCamera(camera.id, "PINHOLE", Wo, Ho, np.array([fx / factor, fy / factor, Wo / 2.0, Ho / 2.0], np.float64))


def kernel_parameters(camera: ColmapCamera):
    """(model id, [fx, fy, cx, cy] float32, k[8] float32): what hs_undistort_map is given -- the camera rounded to fp32."""
    fx, fy, cx, cy, k = intrinsics(camera)
    k8 = np.zeros(8, np.float32)
    k8[:k.size] = k.astype(np.float32)
    return MODELS.index(camera.model), np.array([fx, fy, cx, cy], np.float32), k8


class UndistortMap(NamedTuple):
    map: torch.Tensor                 # [H', W', 2] fp32: the source position (COLMAP pixel coordinates) of every full-resolution pixel
    valid: torch.Tensor               # [H', W'] uint8: 1 where that position lies inside the hull of the source's pixel centres
    camera: ColmapCamera              # the PINHOLE camera of the undistorted frames (undistorted_camera)
    factor: int                       # S: an output pixel is the mean of S x S map entries
    source_size: Tuple[int, int]      # (W, H) of the frames the map samples


def _device(what: str, device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"casualhdrsplat_amd computes {what} on an MI355X only: it must live on a cuda (HIP) device "
                           "(no CPU fallback)")
    return dev


def undistort_map(camera: ColmapCamera, factor: int = 1, device="cuda") -> UndistortMap:
    """The resampling map of `camera` at downscale `factor` (1, 2, 3, 4 or 8), computed once per camera on the GPU."""
    if factor not in FACTORS:
        raise ValueError(f"undistort_map: factor={factor} is none of {FACTORS}")
    out_cam = undistorted_camera(camera, factor)
    model, f4, k8 = kernel_parameters(camera)
    dev = _device("undistort_map", device)
    Wf, Hf = out_cam.width * factor, out_cam.height * factor
    grid = torch.empty((Hf, Wf, 2), dtype=torch.float32, device=dev)
    valid = torch.empty((Hf, Wf), dtype=torch.uint8, device=dev)
    a = L.hs_undistort_args()
    a.model, a.W, a.H, a.Wf, a.Hf = model, int(camera.width), int(camera.height), Wf, Hf
    a.fx, a.fy, a.cx, a.cy = (float(x) for x in f4)
    a.k = (C.c_float * 8)(*[float(x) for x in k8])
    a.map, a.valid = grid.data_ptr(), valid.data_ptr()
    with _on_device(dev):
        L.check(L.load().hs_undistort_map(C.byref(a), _stream(dev)), "hs_undistort_map")
    return UndistortMap(grid, valid, out_cam, int(factor), (int(camera.width), int(camera.height)))


def remap_frames(frames: torch.Tensor, grid: torch.Tensor, factor: int = 1) -> torch.Tensor:
    """out [F, 3, H' / factor, W' / factor] fp32: every output pixel is the mean of the factor x factor bilinear samples of
    `frames` (uint8 [F, H, W, 3], then divided by 255, or fp32 [F, 3, H, W]) at the entries of `grid` ([H', W', 2] fp32, source
    positions in COLMAP pixel coordinates; a NaN samples as 0, positions outside the source clamp to its border)."""
    for name, t in (("frames", frames), ("map", grid)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"undistort_frames: {name} must be a torch.Tensor")
    if frames.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"undistort_frames: frames must be uint8 [F, H, W, 3] or float32 [F, 3, H, W], got {frames.dtype}")
    u8 = frames.dtype == torch.uint8
    if frames.dim() != 4 or frames.shape[3 if u8 else 1] != 3:
        raise ValueError("undistort_frames: frames must be uint8 [F, H, W, 3] or float32 [F, 3, H, W], got "
                         f"{frames.dtype} {tuple(frames.shape)}")
    if grid.dtype != torch.float32 or grid.dim() != 3 or grid.shape[2] != 2:
        raise ValueError(f"undistort_frames: the map must be float32 [H', W', 2], got {grid.dtype} {tuple(grid.shape)}")
    if factor not in FACTORS:
        raise ValueError(f"undistort_frames: factor={factor} is none of {FACTORS}")
    F = frames.shape[0]
    H, W = (frames.shape[1], frames.shape[2]) if u8 else (frames.shape[2], frames.shape[3])
    Hf, Wf = grid.shape[0], grid.shape[1]
    if Hf % factor or Wf % factor:
        raise ValueError(f"undistort_frames: the map's {Wf} x {Hf} grid is no multiple of factor={factor}")
    Ho, Wo = Hf // factor, Wf // factor
    if not (2 <= W <= MAX_SIDE and 2 <= H <= MAX_SIDE and Wf <= MAX_SIDE and Hf <= MAX_SIDE):
        raise ValueError(f"undistort_frames: frames {W} x {H} / map {Wf} x {Hf} outside 2 <= W, H <= {MAX_SIDE}, W', H' <= {MAX_SIDE}")
    if 3 * F * H * W >= 1 << 31 or 3 * F * Ho * Wo >= 1 << 31:
        raise ValueError(f"undistort_frames: {F} frames of {W} x {H} -> {Wo} x {Ho} hold 2^31 elements or more: pass fewer at a time")
    for name, t in (("frames", frames), ("map", grid)):
        _device(f"undistort_frames ({name})", t.device)
    if grid.device != frames.device:
        raise ValueError("undistort_frames: frames and map live on different devices")
    frames, grid = frames.detach().contiguous(), grid.detach().contiguous()
    out = torch.empty((F, 3, Ho, Wo), dtype=torch.float32, device=frames.device)
    a = L.hs_undistort_args()
    a.W, a.H, a.Wf, a.Hf, a.F, a.factor, a.frames_u8 = W, H, Wf, Hf, F, int(factor), int(u8)
    a.map, a.frames, a.out = grid.data_ptr(), frames.data_ptr(), out.data_ptr()
    with _on_device(frames.device):
        L.check(L.load().hs_undistort_remap(C.byref(a), _stream(frames.device)), "hs_undistort_remap")
    return out


def undistort_frames(frames: torch.Tensor, umap: UndistortMap) -> torch.Tensor:
    """[F, 3, H_out, W_out] fp32: the frames of umap's source camera (uint8 [F, H, W, 3] as a decoder delivers them -- the
    result is then in [0, 1] -- or fp32 [F, 3, H, W]) undistorted and downscaled by umap.factor in one pass.  A single
    [H, W, 3] uint8 or [3, H, W] fp32 frame returns [3, H_out, W_out]."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError("undistort_frames: frames must be a torch.Tensor")
    single = frames.dim() == 3
    batch = frames.unsqueeze(0) if single else frames
    if batch.dim() == 4 and batch.dtype in (torch.uint8, torch.float32):
        got = (batch.shape[2], batch.shape[1]) if batch.dtype == torch.uint8 else (batch.shape[3], batch.shape[2])
        if tuple(got) != tuple(umap.source_size):
            raise ValueError(f"undistort_frames: frames of {got[0]} x {got[1]}, the map samples a {umap.source_size[0]} x "
                             f"{umap.source_size[1]} source")
    out = remap_frames(batch, umap.map, umap.factor)
    return out[0] if single else out
