"""TSDF fusion of rendered depth maps and mesh extraction (tsdf.hip, through hs_tsdf_* of include/hdrsplat.h): the step from a
cloud trained with the surface regularisers (distortion_loss, normal_consistency_loss) to the surface itself.

    color, radii, alpha, invd = rasterizer(...)                        # return_alpha=True, return_invdepth=True, per view
    vol = TSDFVolume.from_bounds(lo, hi, voxel_size=0.02, color=True)
    vol.integrate(invdepths, viewmatrices, fx, fy, alpha=alphas, color=colors)      # [F, H, W], [F, 4, 4], [F, 3, H, W]
    vertices, faces, colors = vol.extract_mesh()
    scene_io.save_mesh_ply("mesh.ply", vertices, faces, colors)

integrate is ONE launch: every sample of the volume walks the frames in order and the volume moves through memory once per
call, whatever the number of frames; two calls over consecutive runs of frames leave the bits of one call over all of them.
extract_mesh is marching tetrahedra on the lattice (six tetrahedra per cell along the body diagonal): no case is ambiguous,
the vertex of an edge is computed from the edge alone, so the mesh is watertight wherever the volume is observed.  Its order
is fixed (vertices by sample and edge, faces by cell and tetrahedron) and the same bits come out on every run.  It reads two
numbers on the host (the mesh's sizes, as densify_and_prune reads its counts); nothing else synchronises.  A vertex on the rim
of the observed region may be referenced by no face: nothing is compacted.  Zero-area faces (a sample of exactly 0) stay.
The fp32 operation order is stated at the top of tsdf.hip and restated in tests/tsdf_reference.py.  No gradients.  GPU tensors
only, fp32 only (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .rasterizer import _on_device, _stream

MAX_SAMPLES = 1 << 30
MAX_SIDE = 65536


def _device(what: str, device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"casualhdrsplat_amd computes {what} on an MI355X only: it must live on a cuda (HIP) device "
                           "(no CPU fallback)")
    return dev


def _positive(what: str, name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{what}: {name} must be a Python float, got {type(v).__name__}")
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{what}: {name}={v} must be finite and positive")
    return float(np.float32(v))


def _triple(what: str, name: str, v) -> tuple:
    try:
        t = tuple(float(x) for x in v)
    except TypeError:
        raise TypeError(f"{what}: {name} must be three numbers") from None
    if len(t) != 3 or not all(math.isfinite(x) for x in t):
        raise ValueError(f"{what}: {name} must be three finite numbers, got {v!r}")
    return t


def _frames(what: str, name: str, t, shape=None, like=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be {list(shape)}, got {tuple(t.shape)}")
    if like is not None and t.device != like.device:
        raise ValueError(f"{what}: invdepth and {name} live on different devices")
    return t


class TSDFVolume:
    """A dense truncated signed distance volume: `tsdf` [nz, ny, nx] (1 where nothing was seen), `weight` [nz, ny, nx] (the
    number of frames that saw the sample) and, with color=True, `color` [3, nz, ny, nx].  Sample (i, j, k) sits at
    origin + voxel_size * (i, j, k).  The three tensors are plain attributes: fill them directly if you like."""

    def __init__(self, origin, voxel_size, dims, trunc=None, color: bool = False, device="cuda"):
        self._configure(origin, voxel_size, dims, trunc, color)
        dev = _device("a TSDFVolume", device)
        nx, ny, nz = self.dims
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=dev)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev)
        self.color = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=dev) if color else None

    def _configure(self, origin, voxel_size, dims, trunc, color):
        """The host side of a volume: everything but the tensors (float values are rounded to fp32, as the kernels take them)."""
        what = "TSDFVolume"
        self.origin = tuple(float(np.float32(x)) for x in _triple(what, "origin", origin))
        self.voxel_size = _positive(what, "voxel_size", voxel_size)
        try:
            d = tuple(int(n) for n in dims)
            exact = all(n == m for n, m in zip(d, dims))
        except (TypeError, ValueError):
            raise TypeError(f"{what}: dims must be three integers (nx, ny, nz)") from None
        if len(d) != 3 or not exact:
            raise TypeError(f"{what}: dims must be three integers (nx, ny, nz), got {dims!r}")
        if min(d) < 2:
            raise ValueError(f"{what}: dims={d} must be at least 2 each")
        if d[0] * d[1] * d[2] > MAX_SAMPLES:
            raise ValueError(f"{what}: dims={d} hold more than 2^30 samples")
        self.dims = d
        self.trunc = 4.0 * self.voxel_size if trunc is None else _positive(what, "trunc", trunc)
        self.has_color = bool(color)
        self.tsdf = self.weight = self.color = None
        return self

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size, **kwargs) -> "TSDFVolume":
        """The smallest volume with sample (0, 0, 0) at `lo` whose samples reach `hi` on every axis."""
        lo, hi = _triple("TSDFVolume.from_bounds", "lo", lo), _triple("TSDFVolume.from_bounds", "hi", hi)
        h = _positive("TSDFVolume.from_bounds", "voxel_size", voxel_size)
        if not all(b > a for a, b in zip(lo, hi)):
            raise ValueError(f"TSDFVolume.from_bounds: hi={hi} must be above lo={lo} on every axis")
        dims = tuple(max(2, int(math.ceil((b - a) / h)) + 1) for a, b in zip(lo, hi))
        return cls(lo, h, dims, **kwargs)

    def reset(self) -> None:
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    # -- the volume as the library sees it --
    def _volume_args(self, what: str) -> L.hs_tsdf_args:
        nx, ny, nz = self.dims
        parts = [("tsdf", self.tsdf, (nz, ny, nx)), ("weight", self.weight, (nz, ny, nx))]
        if self.has_color:
            parts.append(("color", self.color, (3, nz, ny, nx)))
        for name, t, shape in parts:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what}: the volume's {name} must be a contiguous float32 tensor of shape {list(shape)}")
        for name, t, shape in parts:
            _device(f"{what} (the volume's {name})", t.device)
            if t.device != self.tsdf.device:
                raise ValueError(f"{what}: the volume's tsdf and {name} live on different devices")
        a = L.hs_tsdf_args()
        a.nx, a.ny, a.nz = nx, ny, nz
        a.origin = (C.c_float * 3)(*self.origin)
        a.voxel_size, a.trunc = self.voxel_size, self.trunc
        a.tsdf, a.weight = self.tsdf.data_ptr(), self.weight.data_ptr()
        a.color = self.color.data_ptr() if self.has_color else None
        return a

    def integrate(self, invdepth, viewmatrices, fx, fy, alpha=None, color=None, min_alpha: float = 0.5,
                  max_depth: float = math.inf) -> None:
        """Fuse F frames into the volume, in place.

        invdepth, alpha: [F, H, W], what the rasterizer's return_invdepth and return_alpha deliver.  A pixel is used when both
                  are finite and > 0 (alpha None: 1) and alpha >= min_alpha; its depth alpha / invdepth must be <= max_depth.
        viewmatrices: [F, 4, 4], world to camera in the rasterizer's transposed convention (scene_io.colmap_view).
        fx, fy:   focal lengths in pixels; the principal point is the centre of the frame.
        color:    [F, 3, H, W], any image of the frames (the LDR or the HDR output); given exactly when the volume has colour.
        Every sample projects to its nearest pixel in every frame; sdf = depth - z is dropped below -trunc, clamped at
        trunc, and averaged in: tsdf = (tsdf * w + sdf / trunc) / (w + 1), colour the same, w += 1."""
        what = "TSDFVolume.integrate"
        if not isinstance(invdepth, torch.Tensor):
            raise TypeError(f"{what}: invdepth must be a torch.Tensor")
        if invdepth.dtype != torch.float32:
            raise TypeError(f"{what}: invdepth must be float32, got {invdepth.dtype}")
        if invdepth.dim() != 3 or invdepth.numel() == 0:
            raise ValueError(f"{what}: invdepth must be [F, H, W] with F, H, W >= 1, got {tuple(invdepth.shape)}")
        F, H, W = invdepth.shape
        if H > MAX_SIDE or W > MAX_SIDE:
            raise ValueError(f"{what}: frames of {W} x {H} are outside H, W <= {MAX_SIDE}")
        if 3 * F * H * W >= 1 << 31:
            raise ValueError(f"{what}: {F} frames of {W} x {H} hold 2^31 / 3 pixels or more: pass fewer at a time")
        _frames(what, "viewmatrices", viewmatrices, (F, 4, 4), invdepth)
        if alpha is not None:
            _frames(what, "alpha", alpha, (F, H, W), invdepth)
        if self.has_color and color is None:
            raise ValueError(f"{what}: the volume has colour: pass color [F, 3, H, W]")
        if color is not None:
            if not self.has_color:
                raise ValueError(f"{what}: color given for a volume without colour (TSDFVolume(..., color=True))")
            _frames(what, "color", color, (F, 3, H, W), invdepth)
        fx, fy = _positive(what, "fx", fx), _positive(what, "fy", fy)
        if isinstance(min_alpha, bool) or not isinstance(min_alpha, (int, float)) or math.isnan(min_alpha):
            raise ValueError(f"{what}: min_alpha={min_alpha!r} must be a number")
        if isinstance(max_depth, bool) or not isinstance(max_depth, (int, float)) or not max_depth > 0:
            raise ValueError(f"{what}: max_depth={max_depth!r} must be > 0 (math.inf: no limit)")
        _device(f"{what} (invdepth)", invdepth.device)
        a = self._volume_args(what)
        if invdepth.device != self.tsdf.device:
            raise ValueError(f"{what}: invdepth and the volume live on different devices")
        keep = [t.detach().contiguous() if t is not None else None for t in (invdepth, viewmatrices, alpha, color)]
        a.F, a.H, a.W = F, H, W
        a.fx, a.fy, a.min_alpha, a.max_depth = fx, fy, float(min_alpha), float(max_depth)
        a.invdepth, a.viewmatrices = keep[0].data_ptr(), keep[1].data_ptr()
        a.alpha = None if keep[2] is None else keep[2].data_ptr()
        a.frame_color = None if keep[3] is None else keep[3].data_ptr()
        with _on_device(invdepth.device):
            L.check(L.load().hs_tsdf_integrate(C.byref(a), _stream(invdepth.device)), "hs_tsdf_integrate")

    def extract_mesh(self, min_weight: float = 1.0):
        """(vertices [V, 3] fp32 in world coordinates, faces [T, 3] int32[, colors [V, 3] fp32 for a volume with colour]): the
        zero level set of the samples with weight >= min_weight, faces wound so that the normal points into free space.  Empty
        tensors when the volume holds no face."""
        what = "TSDFVolume.extract_mesh"
        if isinstance(min_weight, bool) or not isinstance(min_weight, (int, float)) or math.isnan(min_weight):
            raise ValueError(f"{what}: min_weight={min_weight!r} must be a number")
        a = self._volume_args(what)
        dev = self.tsdf.device
        lib = L.load()
        nx, ny, nz = self.dims
        workspace = torch.empty(int(lib.hs_tsdf_mesh_workspace_bytes(nx, ny, nz)), dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        a.min_weight = float(min_weight)
        a.workspace, a.totals = workspace.data_ptr(), totals.data_ptr()
        with _on_device(dev):
            L.check(lib.hs_tsdf_mesh_plan(C.byref(a), _stream(dev)), "hs_tsdf_mesh_plan")
            V, T = (int(n) for n in totals.tolist())         # the one host read
            if V >= 1 << 31 or T >= 1 << 31:
                raise RuntimeError(f"{what}: the mesh would hold {V} vertices and {T} faces, 2^31 or more: use a coarser volume")
            if T == 0:
                V = 0
            vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((T, 3), dtype=torch.int32, device=dev)
            colors = torch.empty((V, 3), dtype=torch.float32, device=dev) if self.has_color else None
            if T > 0:
                a.n_vertices, a.n_faces = V, T
                a.vertices, a.faces = vertices.data_ptr(), faces.data_ptr()
                a.colors = colors.data_ptr() if self.has_color else None
                L.check(lib.hs_tsdf_mesh_emit(C.byref(a), _stream(dev)), "hs_tsdf_mesh_emit")
        return (vertices, faces, colors) if self.has_color else (vertices, faces)
