"""MCMC refinement of the cloud (mcmc.hip and mcmc_reg.hip, through hs_mcmc_sample / hs_mcmc_update / hs_mcmc_noise /
hs_mcmc_regularize of include/hdrsplat.h): the second published densification policy, "3D Gaussian Splatting as Markov Chain
Monte Carlo" -- a fixed row budget, dead Gaussians moved onto live ones instead of pruned, a position noise after every
optimizer step, and the opacity / scale regularisers that make Gaussians die.

    opt = GaussianAdam(cloud_param_groups(means3D, raw_opacities, shs, log_scales, rotations), eps=1e-15)
    ...
    loss.backward()
    terms = regularize(opt, opacity_reg=0.01, scale_reg=0.01)   # += d(lambda_o mean|o| + lambda_s mean|s|) into .grad, in place
    opt.step()                                           # every row: the regularisers act on Gaussians no frame saw, too
    inject_noise(opt, noise_lr=5e5)                      # every step, one launch
    if step % 100 == 0:
        relocate(opt, min_opacity=0.005)                 # in place: P does not change, nothing is read back
        res = grow(opt, cap_max=1_000_000)               # P -> min(cap_max, int(1.05 P)): known before any kernel runs
        means3D, raw_opacities, shs, log_scales, rotations = (res.params[k] for k in CLOUD_NAMES)

The rules are in the header.  Sampling is by opacity with INTEGER weights (2^24 sigmoid, rounded) whose prefix sums are
exact, so a draw is a function of its random word and the opacities alone, bit for bit.  The kernels hold no random-number
generator: `relocate` and `grow` draw an int64 tensor of random words, `inject_noise` a [P, 3] normal tensor, on the
cloud's device from `generator` (or take them as `u` / `xi`).  Several ranks that hold the same cloud must seed their
generators alike -- otherwise their clouds diverge.

No host wait anywhere: `relocate` and `inject_noise` change the optimizer's tensors in place; `grow` allocates at a size
computed on the host, gathers with hs_densify_apply (new rows get zero moments) and hands the tensors to
GaussianAdam.replace_params, so the device step count and running products are not touched.  Counts stay on the device.

The regularisers are a call, not two torch lines: under parameterization="raw" the rasterizer's backward hands the stored
opacities and scales a .grad that is a view into its one flat gradient buffer, and a second autograd contribution to the
same leaf would make the engine sum the two into a tensor of its own -- the view, which the chunked all-reduce and
GaussianAdam rely on, would be lost.  `regularize` adds into the rows that exist (one launch, two with the values).

Not here: WHEN to refine (examples/train_synthetic.py --mcmc shows one schedule).

GPU tensors only, fp32 only: anything else raises (no fallback).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import torch

from . import _lib as L
from .densify import CLOUD_NAMES, _cloud_of
from .optim import _require_gpu
from .rasterizer import _on_device, _stream

COUNT_NAMES = ("P", "dead", "draws", "sources", "S_is_zero")


@dataclass
class RelocateResult:
    counts: torch.Tensor     # int32 [8] ON THE DEVICE: COUNT_NAMES, then zeros (reading it is the caller's wait)
    source: torch.Tensor     # int32 [P]: the row a dead row was moved onto, -1 where the row was not dead
    cnt: torch.Tensor        # int32 [P]: how many dead rows were moved onto each row


@dataclass
class GrowResult:
    params: dict             # CLOUD_NAMES -> the leaf tensors the optimizer now holds (its own when n_new == 0)
    n_new: int
    row_map: torch.Tensor | None   # int32 [P + n_new]: kind << 30 | source row (densify's format); None when n_new == 0
    counts: torch.Tensor | None    # as RelocateResult.counts; None when n_new == 0

    @property
    def source(self):
        """Source row of every output row."""
        return None if self.row_map is None else self.row_map & 0x3FFFFFFF


def stored_min_opacity(min_opacity: float, raw_opacity: bool) -> float:
    """hs_mcmc_args.o_min: the dead threshold in the space the opacities are stored in, in float64 (ctypes rounds it to
    float32 when it enters the struct) -- densify.stored_thresholds' rule."""
    if math.isnan(min_opacity) or not (0.0 <= min_opacity <= 1.0):
        raise ValueError(f"min_opacity={min_opacity} must lie in [0, 1]")
    if not raw_opacity:
        return min_opacity
    return -math.inf if min_opacity <= 0.0 else (math.inf if min_opacity >= 1.0 else math.log(min_opacity / (1.0 - min_opacity)))


def workspace_layout(P: int, n_draws: int) -> dict:
    """Byte offsets inside the workspace of hs_mcmc_sample (the header's formula): prefix, blocks, cnt, sources, bytes."""
    a = lambda x: (x + 255) // 256 * 256        # noqa: E731
    out, o = {}, 0
    for name, n in (("prefix", 8 * P), ("blocks", 16 * ((P + 255) // 256 + 1)), ("cnt", 4 * P), ("sources", 4 * n_draws)):
        out[name] = o
        o += a(n)
    out["bytes"] = o
    return out


def _words(what, u, n, dev, generator):
    if u is None:
        return torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device=dev, generator=generator)
    if not isinstance(u, torch.Tensor):
        raise TypeError(f"{what}: u must be a torch.Tensor")
    _require_gpu(u, "u")
    if u.dtype != torch.int64 or u.shape != (n,) or u.device != dev or not u.is_contiguous():
        raise ValueError(f"{what}: u must be a contiguous int64 tensor [{n}] on the cloud's device")
    return u


def _moments(what, optimizer, cloud, dev):
    out = {}
    for key in CLOUD_NAMES:
        p = cloud[key]
        st = optimizer._init_state(p)
        m, v = st["exp_avg"], st["exp_avg_sq"]
        for t in (m, v):
            _require_gpu(t, "every moment tensor")
            if t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{what}: exp_avg / exp_avg_sq must be contiguous float32 tensors of their parameter's shape")
        out[key] = (m, v)
    return out


def _sample_args(what, cloud, P, n_draws, mode, min_opacity, raw_scales, raw_opacity, u, dev):
    lib = L.load()
    if P >= 1 << 30:
        raise ValueError(f"{what}: {P} Gaussians; the library's limit is 2^30 - 1")
    nbytes = lib.hs_mcmc_workspace_bytes(P, n_draws)
    if nbytes < 0:
        L.check(L.HS_EINVAL, "hs_mcmc_workspace_bytes")
    workspace = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
    counts = torch.empty(L.HS_MCMC_COUNTS, dtype=torch.int32, device=dev)
    a = L.hs_mcmc_args()
    a.P, a.n_draws, a.mode = P, n_draws, mode
    a.flags = (L.HS_DENSIFY_RAW_SCALES if raw_scales else 0) | (L.HS_DENSIFY_RAW_OPACITY if raw_opacity else 0)
    a.o_min, a.min_opacity = stored_min_opacity(min_opacity, raw_opacity), min_opacity
    a.opacities, a.scales = cloud["opacities"].data_ptr(), cloud["scales"].data_ptr()
    a.u, a.workspace, a.counts, a.counts_host = u.data_ptr(), workspace.data_ptr(), counts.data_ptr(), None
    return lib, a, workspace, counts


def relocate(optimizer, *, min_opacity=0.005, raw_scales=True, raw_opacity=True, generator=None, u=None) -> RelocateResult:
    """Move every dead Gaussian (opacity not above `min_opacity`) of the cloud `optimizer` updates onto a live one drawn by
    opacity, in place: the sources' opacities and scales are corrected for the copies that now share their place and their
    Adam moments zeroed; a dead row becomes a copy of its corrected source and keeps its moments.  P does not change and
    nothing is read back.  `u` ([P] int64 on the device) replaces the draw from `generator`: row i uses u[i]."""
    what = "relocate"
    cloud = _cloud_of(optimizer)
    P, dev = int(cloud["means3D"].shape[0]), cloud["means3D"].device
    min_opacity = float(min_opacity)
    stored_min_opacity(min_opacity, bool(raw_opacity))
    u = _words(what, u, P, dev, generator)
    moments = _moments(what, optimizer, cloud, dev)
    lib, a, workspace, counts = _sample_args(what, cloud, P, P, L.HS_MCMC_RELOCATE, min_opacity, bool(raw_scales), bool(raw_opacity), u, dev)
    mats = []
    for key in CLOUD_NAMES:
        p = cloud[key]
        stride = p.numel() // P if P else max(1, math.prod(p.shape[1:]))
        mats += [(p, stride, L.HS_DENSIFY_COPY), (moments[key][0], stride, L.HS_DENSIFY_ZERO_NEW), (moments[key][1], stride, L.HS_DENSIFY_ZERO_NEW)]
    arr = (L.hs_densify_matrix * len(mats))()
    for d, (t, stride, role) in zip(arr, mats):
        d.src, d.dst, d.row_stride, d.role = None, t.data_ptr(), stride, role
    a.matrices, a.n_matrices = arr, len(mats)
    with _on_device(dev):
        L.check(lib.hs_mcmc_sample(C.byref(a), _stream(dev)), "hs_mcmc_sample")
        L.check(lib.hs_mcmc_update(C.byref(a), _stream(dev)), "hs_mcmc_update")
    lay = workspace_layout(P, P)
    return RelocateResult(counts=counts, source=workspace[lay["sources"]:lay["sources"] + 4 * P].view(torch.int32),
                          cnt=workspace[lay["cnt"]:lay["cnt"] + 4 * P].view(torch.int32))


def grow(optimizer, *, cap_max, factor=1.05, min_opacity=0.005, raw_scales=True, raw_opacity=True, generator=None, u=None) -> GrowResult:
    """Grow the cloud to min(cap_max, int(factor P)) rows: the new rows are copies of rows drawn by opacity (every row
    weighted, draw k uses u[k]), whose opacities and scales are corrected as in `relocate`; the sources keep their Adam
    moments, the new rows get zeros.  The size is computed on the host, so nothing is read back; the optimizer holds the
    new tensors afterwards (GaussianAdam.replace_params).  With nothing to add the optimizer's own tensors are returned and
    nothing is launched."""
    what = "grow"
    cloud = _cloud_of(optimizer)
    P, dev = int(cloud["means3D"].shape[0]), cloud["means3D"].device
    if isinstance(cap_max, bool) or not isinstance(cap_max, int) or cap_max < 0:
        raise ValueError(f"{what}: cap_max={cap_max!r} must be a non-negative int")
    factor = float(factor)
    if not (1.0 <= factor <= 2.0):
        raise ValueError(f"{what}: factor={factor} must lie in [1, 2] (a source row is cloned by the existing gather: at most P new rows)")
    min_opacity = float(min_opacity)
    stored_min_opacity(min_opacity, bool(raw_opacity))
    n_new = max(0, min(cap_max, int(factor * P)) - P)
    if n_new == 0:
        return GrowResult(params={k: cloud[k] for k in CLOUD_NAMES}, n_new=0, row_map=None, counts=None)
    u = _words(what, u, n_new, dev, generator)
    moments = _moments(what, optimizer, cloud, dev)
    lib, a, workspace, counts = _sample_args(what, cloud, P, n_new, L.HS_MCMC_GROW, min_opacity, bool(raw_scales), bool(raw_opacity), u, dev)
    P_out = P + n_new
    row_map = torch.empty(P_out, dtype=torch.int32, device=dev)
    a.row_map = row_map.data_ptr()
    new, new_m, mats = {}, {}, []
    for key in CLOUD_NAMES:
        p = cloud[key]
        shape = (P_out,) + tuple(p.shape[1:])
        stride = p.numel() // P
        new[key] = torch.empty(shape, dtype=torch.float32, device=dev)
        new_m[key] = (torch.empty(shape, dtype=torch.float32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev))
        mats += [(p, new[key], stride, L.HS_DENSIFY_COPY), (moments[key][0], new_m[key][0], stride, L.HS_DENSIFY_ZERO_NEW),
                 (moments[key][1], new_m[key][1], stride, L.HS_DENSIFY_ZERO_NEW)]
    arr = (L.hs_densify_matrix * len(mats))()
    for d, (src, dst, stride, role) in zip(arr, mats):
        d.src, d.dst, d.row_stride, d.role = src.data_ptr(), dst.data_ptr(), stride, role
    g = L.hs_densify_args()
    g.P, g.P_out, g.flags = P, P_out, a.flags
    g.row_map, g.matrices, g.n_matrices = row_map.data_ptr(), arr, len(mats)
    with _on_device(dev):
        L.check(lib.hs_mcmc_sample(C.byref(a), _stream(dev)), "hs_mcmc_sample")
        L.check(lib.hs_mcmc_update(C.byref(a), _stream(dev)), "hs_mcmc_update")       # (sources only: no matrices)
        L.check(lib.hs_densify_apply(C.byref(g), _stream(dev)), "hs_densify_apply")
    mapping = {}
    for key in CLOUD_NAMES:
        old = cloud[key]
        new[key].requires_grad_(old.requires_grad)
        mapping[old] = (new[key], *new_m[key])
    optimizer.replace_params(mapping)
    return GrowResult(params={k: new[k] for k in CLOUD_NAMES}, n_new=n_new, row_map=row_map, counts=counts)


def inject_noise(optimizer, *, noise_lr=5e5, lr=None, raw_scales=True, raw_opacity=True, generator=None, xi=None) -> None:
    """The per-step position noise: means += Sigma (xi g lr noise_lr) with Sigma = R diag(sigma^2) R^T the Gaussian's
    covariance and g = sigmoid(-100 (opacity - 0.005)) a gate that spares opaque Gaussians; in place, one launch.  `lr`
    defaults to the learning rate of the optimizer's `xyz` group; `xi` ([P, 3] float32 on the device) replaces the draw
    from `generator`."""
    what = "inject_noise"
    cloud = _cloud_of(optimizer)
    P, dev = int(cloud["means3D"].shape[0]), cloud["means3D"].device
    if lr is None:
        lr = next(g["lr"] for g in optimizer.param_groups if g.get("name") == "xyz")
    scaler = float(lr) * float(noise_lr)
    if not math.isfinite(scaler):
        raise ValueError(f"{what}: lr * noise_lr = {scaler} must be finite")
    if xi is None:
        xi = torch.randn(P, 3, device=dev, dtype=torch.float32, generator=generator)
    else:
        if not isinstance(xi, torch.Tensor):
            raise TypeError(f"{what}: xi must be a torch.Tensor")
        _require_gpu(xi, "xi")
        if xi.dtype != torch.float32 or xi.shape != (P, 3) or xi.device != dev or not xi.is_contiguous():
            raise ValueError(f"{what}: xi must be a contiguous float32 tensor [{P}, 3] on the cloud's device")
    if P >= 1 << 30:
        raise ValueError(f"{what}: {P} Gaussians; the library's limit is 2^30 - 1")
    a = L.hs_mcmc_noise_args()
    a.P, a.scaler = P, scaler
    a.flags = (L.HS_DENSIFY_RAW_SCALES if raw_scales else 0) | (L.HS_DENSIFY_RAW_OPACITY if raw_opacity else 0)
    a.means3D, a.opacities, a.scales = cloud["means3D"].data_ptr(), cloud["opacities"].data_ptr(), cloud["scales"].data_ptr()
    a.rotations, a.xi = cloud["rotations"].data_ptr(), xi.data_ptr()
    with _on_device(dev):
        L.check(L.load().hs_mcmc_noise(C.byref(a), _stream(dev)), "hs_mcmc_noise")


def _reg_weight(what, name, v):
    v = float(v)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"{what}: {name}={v} must be finite and not negative")
    return v


def regularize(optimizer, *, opacity_reg=0.01, scale_reg=0.01, raw_scales=True, raw_opacity=True, value=True):
    """The publication's regularisers opacity_reg * mean|opacity| + scale_reg * mean|scale| (activated values), as the
    gradient they add: call after backward() and before optimizer.step().  Adds, in place, into the .grad of the cloud's
    `opacity` and `scaling` tensors -- the tensors stay where they are (grad.data_ptr() does not change), so a .grad that is a
    view of the rasterizer's flat gradient buffer remains one.  Returns the two terms as a float32 [2] tensor on the device
    (reading it is the caller's wait), or None with value=False (one launch less).  A tensor whose weight is 0 is not touched
    and needs no .grad.  The regularisers act on ALL rows, also those no frame of the step saw: an MCMC step is
    `optimizer.step()` without visibility= (a masked step would leave the unseen rows' gradient unapplied)."""
    what = "regularize"
    cloud = _cloud_of(optimizer)
    lam_o, lam_s = _reg_weight(what, "opacity_reg", opacity_reg), _reg_weight(what, "scale_reg", scale_reg)
    P, dev = int(cloud["means3D"].shape[0]), cloud["means3D"].device
    grads = {}
    for key, lam in (("opacities", lam_o), ("scales", lam_s)):
        if lam == 0.0:
            grads[key] = None
            continue
        p = cloud[key]
        g = p.grad
        if g is None:
            raise ValueError(f"{what}: the {key} tensor has no .grad: call after backward()")
        _require_gpu(g, f"the gradient of the {key}")
        if g.dtype != torch.float32 or g.shape != p.shape or g.device != dev or not g.is_contiguous():
            raise ValueError(f"{what}: the .grad of the {key} must be a contiguous float32 tensor of its parameter's shape and device")
        grads[key] = g
    if P >= 1 << 30:
        raise ValueError(f"{what}: {P} Gaussians; the library's limit is 2^30 - 1")
    if lam_o == 0.0 and lam_s == 0.0 and not value:
        return None
    lib = L.load()
    a = L.hs_mcmc_reg_args()
    a.P, a.lambda_opacity, a.lambda_scale = P, lam_o, lam_s
    a.flags = (L.HS_DENSIFY_RAW_SCALES if raw_scales else 0) | (L.HS_DENSIFY_RAW_OPACITY if raw_opacity else 0)
    a.opacities, a.scales = cloud["opacities"].data_ptr(), cloud["scales"].data_ptr()
    a.dL_dopacities = None if grads["opacities"] is None else grads["opacities"].data_ptr()
    a.dL_dscales = None if grads["scales"] is None else grads["scales"].data_ptr()
    terms = workspace = None
    if value:
        nbytes = lib.hs_mcmc_reg_workspace_bytes(P)
        if nbytes < 0:
            L.check(L.HS_EINVAL, "hs_mcmc_reg_workspace_bytes")
        workspace = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
        terms = torch.empty(2, dtype=torch.float32, device=dev)
        a.loss, a.workspace = terms.data_ptr(), workspace.data_ptr()
    with _on_device(dev):
        L.check(lib.hs_mcmc_regularize(C.byref(a), _stream(dev)), "hs_mcmc_regularize")
    return terms
