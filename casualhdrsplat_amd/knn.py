"""Mean squared distance to the three nearest neighbours of every point (knn.hip, through hs_knn_mean_dist_sq of
include/hdrsplat.h): the isotropic scale of the published SfM initialisation -- what upstream computes with
simple_knn.distCUDA2 -- for a cloud that lives on the GPU.

    d2 = knn_mean_dist2(xyz)                       # [P] float32, xyz a CUDA float32 [P, 3] tensor
    cloud = scene_io.init_from_points(xyz, rgb, device="cuda")

The header states the contract operation by operation; tests/knn_reference.py restates it in numpy and the GPU tests
compare bits.  The search is exact (Morton order, boxes pruned by a lower bound that never exceeds a computed distance), so
the result does not depend on the order of the points or on the sort.  One wait: the host reads the status word the
kernels leave (a radix pass that gave up) before it hands the distances out.

GPU tensors only, fp32 only: anything else raises (no fallback).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .rasterizer import SortChainStalled, _on_device, _stream


class _KnnSortStalled(SortChainStalled):
    def __init__(self):
        RuntimeError.__init__(
            self, "libhdrsplat: a radix pass of the Morton sort of hs_knn_mean_dist_sq gave up waiting for a predecessor's "
                  "status word (status = 2) and the distances are invalid -- is another process running the same kernels on "
                  "this GPU?  The passes are ticket-ordered; repeat the call")


def knn_mean_dist2(xyz: torch.Tensor) -> torch.Tensor:
    """mean_d2[i] = ((b0 + b1) + b2) / k over the k = min(3, P - 1) smallest squared distances from point i to the OTHER
    points (excluded by index: coincident points give exact zeros); 0 for a single point.  float32 [P] on xyz's device."""
    if not isinstance(xyz, torch.Tensor):
        raise TypeError("knn_mean_dist2: xyz must be a torch.Tensor (float32 [P, 3] on a cuda device)")
    if xyz.dtype != torch.float32:
        raise TypeError(f"knn_mean_dist2: xyz must be float32, got {xyz.dtype}")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"knn_mean_dist2: xyz must have shape [P, 3], got {tuple(xyz.shape)}")
    if xyz.device.type != "cuda":
        raise RuntimeError("casualhdrsplat_amd searches neighbours on an MI355X only: xyz must live on a cuda (HIP) device "
                           "(no CPU fallback)")
    P = int(xyz.shape[0])
    if P >= 1 << 30:
        raise ValueError(f"knn_mean_dist2: {P} points; the library's limit is 2^30 - 1")
    dev = xyz.device
    xyz = xyz.detach().contiguous()
    out = torch.empty(P, dtype=torch.float32, device=dev)
    if P == 0:
        return out
    if not bool(torch.isfinite(xyz).all()):
        raise ValueError("knn_mean_dist2: xyz holds non-finite coordinates")
    lib = L.load()
    ws_bytes = lib.hs_knn_workspace_bytes(P)
    if ws_bytes < 0:
        L.check(L.HS_EINVAL, "hs_knn_workspace_bytes")
    workspace = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    a = L.hs_knn_args()
    a.P, a.xyz, a.mean_d2 = P, xyz.data_ptr(), out.data_ptr()
    a.workspace, a.status = workspace.data_ptr(), status.data_ptr()
    with _on_device(dev):
        L.check(lib.hs_knn_mean_dist_sq(C.byref(a), _stream(dev)), "hs_knn_mean_dist_sq")
    if int(status.item()) != 0:                      # the one wait
        raise _KnnSortStalled()
    return out
