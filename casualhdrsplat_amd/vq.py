"""k-means vector quantisation, fused (vq.hip, through the C ABI of include/hdrsplat.h): the codebook compression of a finished
cloud's view-dependent SH coefficients -- LightGaussian's "VecTree" step, gsplat's PngCompression k-means on shN, Compact3D.
At SH degree 3 the 45 `f_rest` floats of a Gaussian become one 16-bit index into a shared codebook; the DC term, which carries
the HDR radiance, stays fp32.

    sh_codebook, sh_codes = quantize_sh(shs, K=4096, weights=stats.weight_sum)     # importance.ContributionStats
    scene_io.save_vq("cloud.npz", cloud, sh_codebook, sh_codes)
    shs = dequantize_sh(shs[:, :1], sh_codebook, sh_codes)

Lloyd's assignment is one kernel whose result is a stated order of fp32 operations (bit for bit the numpy restatement in
tests/vq_reference.py); the weighted centroid update is a stable counting sort of the rows by code and a fixed-order fp64
segmented sum, with no atomics: the same inputs give the same codebook bits on every run.  Nothing here reads a value on the
host.  GPU tensors only (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib as L
from .rasterizer import _on_device, _stream

MAX_D, MAX_K, MAX_N = 48, 65536, 1 << 30


class VQResult(NamedTuple):
    codebook: torch.Tensor   # [K, D] fp32
    codes: torch.Tensor      # [N] int32: the exact argmin against `codebook`
    dist2: torch.Tensor      # [N] fp32: the squared distance of every row to its centroid


def _checked(what: str, x, codebook, codes=None, weights=None):
    named = [("x", x, torch.float32, 2), ("codebook", codebook, torch.float32, 2)]
    if codes is not None:
        named.append(("codes", codes, torch.int32, 1))
    if weights is not None:
        named.append(("weights", weights, torch.float32, 1))
    for name, t, dtype, dim in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor")
        if t.dtype != dtype:
            raise TypeError(f"{what}: {name} must be {dtype}, got {t.dtype}")
        if t.dim() != dim:
            raise ValueError(f"{what}: {name} must have {dim} dimension(s), got {tuple(t.shape)}")
    N, D = x.shape
    K = codebook.shape[0]
    if codebook.shape[1] != D:
        raise ValueError(f"{what}: x {tuple(x.shape)} and codebook {tuple(codebook.shape)} differ in D")
    if not (0 <= N <= MAX_N and 1 <= D <= MAX_D and 1 <= K <= MAX_K):
        raise ValueError(f"{what}: N={N}, D={D}, K={K} outside 0 <= N <= 2^30, 1 <= D <= {MAX_D}, 1 <= K <= {MAX_K}")
    for name, t, _, _ in named[2:]:
        if t.shape[0] != N:
            raise ValueError(f"{what}: {name} must hold one entry per row ({N}), got {tuple(t.shape)}")
    for name, t, _, _ in named:
        if t.device.type != "cuda":
            raise RuntimeError(f"casualhdrsplat_amd computes {what} on an MI355X only: {name} must live on a cuda (HIP) device "
                               "(no CPU fallback)")
        if t.device != x.device:
            raise ValueError(f"{what}: x and {name} live on different devices")
    return tuple(t.detach().contiguous() for _, t, _, _ in named)


def _args(x: torch.Tensor, codebook: torch.Tensor) -> L.hs_vq_args:
    a = L.hs_vq_args()
    a.N, a.D = x.shape
    a.K = codebook.shape[0]
    a.x, a.codebook_in = x.data_ptr(), codebook.data_ptr()
    return a


def _workspace(N: int, D: int, K: int, device) -> torch.Tensor:
    nbytes = L.load().hs_vq_workspace_bytes(N, D, K)
    if nbytes < 0:
        L.check(L.HS_EINVAL, "hs_vq_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if ws.data_ptr() % 256:
        raise RuntimeError("kmeans_update: the allocator returned a workspace that is not 256-byte aligned")
    return ws


def _assign(x, codebook, codes, dist2) -> None:
    a = _args(x, codebook)
    a.codes, a.dist2 = codes.data_ptr(), dist2.data_ptr()
    with _on_device(x.device):
        L.check(L.load().hs_vq_assign(C.byref(a), _stream(x.device)), "hs_vq_assign")


def _update(x, codes, codebook, weights, out, counts, ws) -> None:
    a = _args(x, codebook)
    a.codes, a.weights = codes.data_ptr(), (weights.data_ptr() if weights is not None else None)
    a.codebook_out, a.counts, a.workspace = out.data_ptr(), counts.data_ptr(), ws.data_ptr()
    with _on_device(x.device):
        L.check(L.load().hs_vq_update(C.byref(a), _stream(x.device)), "hs_vq_update")


def kmeans_assign(x: torch.Tensor, codebook: torch.Tensor):
    """(codes [N] int32, dist2 [N] fp32): for every row of `x` ([N, D] fp32 on the GPU) the index of the nearest row of
    `codebook` ([K, D] fp32) and the squared distance to it -- squared differences added in fp32 in ascending d, the lowest k
    on a tie, bit for bit the numpy restatement (tests/vq_reference.py)."""
    x, codebook = _checked("kmeans_assign", x, codebook)
    codes = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    dist2 = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _assign(x, codebook, codes, dist2)
    return codes, dist2


def kmeans_update(x: torch.Tensor, codes: torch.Tensor, codebook: torch.Tensor, weights: Optional[torch.Tensor] = None):
    """(new_codebook [K, D] fp32, counts [K] int32): every centroid becomes the `weights`-weighted mean (None: the plain mean)
    of the rows of `x` whose code names it, summed in fp64 in a fixed order; a cluster without members, or whose weights are
    all zero, keeps its row of `codebook` bit for bit.  counts = members per cluster, whatever their weights."""
    x, codebook, codes, *w = _checked("kmeans_update", x, codebook, codes, weights)
    out = torch.empty_like(codebook)
    counts = torch.empty(codebook.shape[0], dtype=torch.int32, device=x.device)
    _update(x, codes, codebook, w[0] if w else None, out, counts, _workspace(x.shape[0], x.shape[1], codebook.shape[0], x.device))
    return out, counts


def kmeans(x: torch.Tensor, K: int, *, iters: int = 10, weights: Optional[torch.Tensor] = None, init=None,
           generator: Optional[torch.Generator] = None) -> VQResult:
    """Lloyd's k-means of the rows of `x` ([N, D] fp32 on the GPU) into `K` centroids: `iters` rounds of assignment and
    (weighted) update, then a final assignment, so that the returned codes are the exact argmin against the returned
    codebook.  `init`: K row indices (a sequence or an integer tensor) or a [K, D] codebook; by default the first K entries
    of a CPU torch.randperm(N, generator=generator), which needs N >= K (ValueError).  An empty cluster keeps its centroid.
    Every buffer is allocated before the loop and nothing is read back to the host."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("kmeans: x must be a [N, D] tensor")
    N = x.shape[0]
    if not (1 <= int(K) <= MAX_K) or iters < 0:
        raise ValueError(f"kmeans: K={K} outside [1, {MAX_K}] or iters={iters} negative")
    K = int(K)
    if isinstance(init, torch.Tensor) and init.dim() == 2:
        codebook = init
        if codebook.shape[0] != K:
            raise ValueError(f"kmeans: init holds {codebook.shape[0]} centroids, K={K}")
    else:
        if init is None:
            if N < K:
                raise ValueError(f"kmeans: {N} rows cannot seed K={K} centroids (pass init=)")
            rows = torch.randperm(N, generator=generator)[:K]
        else:
            rows = torch.as_tensor(init).reshape(-1).to(torch.int64)
            if rows.numel() != K:
                raise ValueError(f"kmeans: init holds {rows.numel()} row indices, K={K}")
        codebook = x.detach()[rows.to(x.device)]
    x, codebook, *w = _checked("kmeans", x, codebook, None, weights)
    w = w[0] if w else None
    D = x.shape[1]
    book = [codebook.clone(), torch.empty_like(codebook)]
    codes = torch.empty(N, dtype=torch.int32, device=x.device)
    dist2 = torch.empty(N, dtype=torch.float32, device=x.device)
    counts = torch.empty(K, dtype=torch.int32, device=x.device)
    ws = _workspace(N, D, K, x.device) if iters else None
    for _ in range(iters):
        _assign(x, book[0], codes, dist2)
        _update(x, codes, book[0], w, book[1], counts, ws)
        book.reverse()
    _assign(x, book[0], codes, dist2)
    return VQResult(book[0], codes, dist2)


def quantize_sh(shs: torch.Tensor, K: int = 4096, *, iters: int = 10, weights: Optional[torch.Tensor] = None,
                generator: Optional[torch.Generator] = None, init=None):
    """(sh_codebook [K, M-1, 3] fp32, sh_codes [P] int32): k-means of the view-dependent coefficients shs[:, 1:, :] of a cloud
    (`shs` [P, M, 3] fp32 on the GPU), each Gaussian's flattened to one row of D = 3 (M - 1).  `weights` [P]: a per-Gaussian
    significance, e.g. importance.ContributionStats.weight_sum.  The DC term is not touched.  M = 1 has nothing to quantise
    (ValueError).  `init` as in kmeans."""
    if not isinstance(shs, torch.Tensor):
        raise TypeError("quantize_sh: shs must be a torch.Tensor")
    if shs.dim() != 3 or shs.shape[2] != 3:
        raise ValueError(f"quantize_sh: shs must be [P, M, 3], got {tuple(shs.shape)}")
    M = shs.shape[1]
    if M < 2:
        raise ValueError("quantize_sh: M = 1: a degree-0 cloud has no view-dependent coefficients to quantise")
    if 3 * (M - 1) > MAX_D:
        raise ValueError(f"quantize_sh: M={M}: rows of {3 * (M - 1)} floats, at most {MAX_D}")
    rows = shs.detach()[:, 1:, :].reshape(shs.shape[0], 3 * (M - 1)).contiguous()
    if weights is not None and isinstance(weights, torch.Tensor):
        weights = weights.detach().reshape(-1)
    r = kmeans(rows, K, iters=iters, weights=weights, init=init, generator=generator)
    return r.codebook.reshape(K, M - 1, 3), r.codes


def dequantize_sh(sh_dc: torch.Tensor, sh_codebook: torch.Tensor, sh_codes: torch.Tensor) -> torch.Tensor:
    """shs [P, M, 3]: the DC term `sh_dc` [P, 1, 3] as it is, followed by sh_codebook[sh_codes] ([K, M-1, 3] gathered by
    [P] integer codes).  A plain torch gather on whatever device the tensors live."""
    if sh_dc.dim() != 3 or sh_dc.shape[1:] != (1, 3) or sh_codebook.dim() != 3 or sh_codebook.shape[2] != 3:
        raise ValueError(f"dequantize_sh: sh_dc must be [P, 1, 3] and sh_codebook [K, M-1, 3], got {tuple(sh_dc.shape)} and "
                         f"{tuple(sh_codebook.shape)}")
    if sh_codes.dim() != 1 or sh_codes.shape[0] != sh_dc.shape[0]:
        raise ValueError(f"dequantize_sh: sh_codes must hold one code per Gaussian ({sh_dc.shape[0]}), got {tuple(sh_codes.shape)}")
    return torch.cat([sh_dc, sh_codebook[sh_codes.long()]], dim=1)
