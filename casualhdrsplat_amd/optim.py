"""Fused Adam for the Gaussian cloud (adam.hip, through hs_adam_step of include/hdrsplat.h): every parameter group in one
launch, optionally restricted to the Gaussians the step saw.

    opt = GaussianAdam(cloud_param_groups(means3D, opacities, shs, scales, rotations), eps=1e-15)
    ...
    image, radii = rasterizer(...)
    photometric_loss(image, gt).backward()
    opt.step(visibility=radii)          # rows with radii <= 0 are not read and not written

The update rule is torch.optim.Adam's (bias-corrected, no weight decay, no AMSGrad) in fp32, with a stated order of
correctly rounded operations (see the header): the same inputs give the same bits on every run.

SPARSE IS NOT DENSE WITH ZERO GRADIENTS.  With `visibility`, a `per_gaussian=True` group skips the rows that are not
visible: parameter, exp_avg and exp_avg_sq keep their bits -- the moments do not decay and the momentum does not move the
row, as in the published sparse Adam of the accelerated rasterizer.  Dense Adam on an exactly-zero gradient would do both.
The step count is one number for the whole optimizer (torch keeps one per parameter; they are equal there too unless a
parameter sat out a step with `.grad is None`, which here advances the count all the same).

Step count, bias corrections and the hyper-parameters are read ON THE DEVICE: `enqueue()` launches two kernels and nothing
else, so it can be recorded in a HIP graph; `set_lr()` between replays changes the table the replay reads.

GPU tensors only, fp32 only, contiguous only: anything else raises (no fallback).
"""
from __future__ import annotations

import ctypes as C
import struct

import torch

from . import _lib as L
from .rasterizer import _on_device, _stream

# learning rates of the published 3DGS training script (arguments/__init__.py: OptimizationParams)
UPSTREAM_LR = dict(means3D=0.00016, opacities=0.05, shs_dc=0.0025, shs_rest=0.0025 / 20.0, scales=0.005, rotations=0.001)
UPSTREAM_EPS = 1e-15


def cloud_param_groups(means3D, opacities, shs, scales, rotations, spatial_lr_scale: float = 1.0, lr: dict | None = None):
    """The usual groups of a cloud with upstream's learning rates (`lr` overrides entries of UPSTREAM_LR): positions
    (scaled by `spatial_lr_scale`), opacities, the SH coefficients as TWO column groups of one tensor -- DC, columns
    0..2 of the [P, M * 3] rows, and the rest at a twentieth of the rate --, scales, rotations.  Every group is
    `per_gaussian`: `step(visibility=...)` applies to it.  Pass eps=UPSTREAM_EPS (1e-15) to the optimizer for upstream's."""
    r = dict(UPSTREAM_LR, **(lr or {}))
    width = shs.numel() // max(1, shs.shape[0])
    groups = [dict(params=[means3D], lr=r["means3D"] * spatial_lr_scale, per_gaussian=True, name="xyz"),
              dict(params=[opacities], lr=r["opacities"], per_gaussian=True, name="opacity"),
              dict(params=[shs], lr=r["shs_dc"], per_gaussian=True, columns=(0, min(3, width)), name="f_dc")]
    if width > 3:
        groups.append(dict(params=[shs], lr=r["shs_rest"], per_gaussian=True, columns=(3, width), name="f_rest"))
    groups += [dict(params=[scales], lr=r["scales"], per_gaussian=True, name="scaling"),
               dict(params=[rotations], lr=r["rotations"], per_gaussian=True, name="rotation")]
    return groups


def _require_gpu(t: torch.Tensor, what: str) -> None:
    if t.device.type != "cuda":
        raise RuntimeError(f"casualhdrsplat_amd updates parameters on an MI355X only: {what} must live on a cuda (HIP) device "
                           "(no CPU fallback)")


def check_visibility(visibility: torch.Tensor, rows: int | None):
    """(kind, tensor) of a visibility argument: the forward's int32 radii (visible = > 0) or a bool / uint8 mask.  `rows`:
    the Gaussians of the per_gaussian groups (None: there are none)."""
    if not isinstance(visibility, torch.Tensor):
        raise TypeError("visibility must be a torch.Tensor (the forward's int32 radii, or a bool / uint8 mask)")
    if visibility.dtype == torch.int32:
        kind = L.HS_ADAM_MASK_RADII
    elif visibility.dtype in (torch.bool, torch.uint8):
        kind = L.HS_ADAM_MASK_BYTES
    else:
        raise TypeError(f"visibility must be int32 radii or a bool / uint8 mask, got {visibility.dtype}")
    if visibility.dim() != 1:
        raise ValueError(f"visibility must have one entry per Gaussian ([P]), got shape {tuple(visibility.shape)}")
    if rows is not None and visibility.numel() != rows:
        raise ValueError(f"visibility has length {visibility.numel()}, the per_gaussian groups have {rows} rows")
    _require_gpu(visibility, "visibility")
    if not visibility.is_contiguous():
        raise ValueError("visibility must be contiguous")
    return kind, visibility


class GaussianAdam(torch.optim.Optimizer):
    """torch.optim.Adam's rule through one fused HIP launch.  Param groups are ordinary dicts with `lr`, `betas`, `eps` and

    per_gaussian  True: dim 0 of the group's tensors is the Gaussian; `step(visibility=...)` skips its invisible rows
    columns       (a, b): the group is columns [a, b) of its tensors seen as [shape[0], numel / shape[0]] matrices.  One
                  tensor may sit in several groups with disjoint column ranges (SH DC / rest with two learning rates); it
                  keeps ONE exp_avg / exp_avg_sq, as in a single torch group.

    At most 16 (group, tensor) pairs.  Per-parameter state is `step`, `exp_avg`, `exp_avg_sq` under torch's names:
    `state_dict()` / `load_state_dict()` interchange with torch.optim.Adam over the same groups.  On load the products
    beta^t are rebuilt from `step` with pow; an uninterrupted run multiplies them up step by step, so a resumed run equals it
    to rounding, not bit for bit.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        per_gaussian=False, columns=None)
        self._entries = None          # [(group index, tensor)] in hyper-table order, fixed once built
        self._dev_state = None        # uint8 [hs_adam_state_bytes]: step count and running products, on the device
        self._dev_hyper = None        # float64 [n, 4]
        self._host_hyper = None
        super().__init__(params, defaults)

    # ---- groups ----

    @staticmethod
    def _check_group(g: dict) -> None:
        if g["weight_decay"] != 0:
            raise ValueError("GaussianAdam: weight_decay is not supported (out of scope: use 0)")
        if g["amsgrad"]:
            raise ValueError("GaussianAdam: amsgrad is not supported")
        if g["maximize"]:
            raise ValueError("GaussianAdam: maximize is not supported")
        b1, b2 = g["betas"]
        if not (g["lr"] >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and g["eps"] >= 0.0):
            raise ValueError(f"GaussianAdam: bad hyper-parameters lr={g['lr']} betas={g['betas']} eps={g['eps']}")

    @staticmethod
    def _matrix(p: torch.Tensor, g: dict):
        """(rows, row_stride, col_begin, col_count) of tensor `p` in group `g`."""
        if g["columns"] is None and not g["per_gaussian"]:
            return p.numel(), 1, 0, 1
        rows = p.shape[0] if p.dim() > 0 else 1
        stride = p.numel() // rows if rows else 1
        a, b = (0, stride) if g["columns"] is None else g["columns"]
        return rows, max(stride, 1), int(a), int(b) - int(a)

    def add_param_group(self, param_group: dict) -> None:
        """As torch's, except that a tensor may appear in several groups when their `columns` do not overlap."""
        if not isinstance(param_group, dict):
            raise TypeError(f"param group must be a dict, got {type(param_group)}")
        g = dict(param_group)
        ps = g["params"]
        g["params"] = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        for k, v in self.defaults.items():
            g.setdefault(k, v)
        self._check_group(g)
        for p in g["params"]:
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"GaussianAdam can only optimize Tensors, got {type(p)}")
            if not p.is_leaf and not p.retains_grad:
                raise ValueError("can't optimize a non-leaf Tensor")
            if p.dtype != torch.float32:
                raise TypeError(f"GaussianAdam: parameters must be float32, got {p.dtype}")
            _require_gpu(p, "every parameter")
            if not p.is_contiguous():
                raise ValueError("GaussianAdam: parameters must be contiguous")
            rows, stride, a, n = self._matrix(p, g)
            if p.numel() and not (0 <= a and n >= 1 and a + n <= stride):
                raise ValueError(f"GaussianAdam: columns={g['columns']} outside the {stride} columns of a {tuple(p.shape)} tensor")
            for og in self.param_groups:
                for q in og["params"]:
                    if q is p:
                        _, _, oa, on = self._matrix(q, og)
                        if og["columns"] is None or g["columns"] is None or (a < oa + on and oa < a + n):
                            raise ValueError("some parameters appear in more than one parameter group with overlapping columns")
        if len({id(p) for p in g["params"]}) != len(g["params"]):
            raise ValueError("a parameter group lists a tensor twice")
        self.param_groups.append(g)
        self._entries = None          # (the tables are rebuilt, from the step count, at the next step)

    # ---- device tables ----

    def _device(self):
        for g in self.param_groups:
            for p in g["params"]:
                return p.device
        return None

    def _read_t(self) -> int:
        if self._dev_state is None:
            return 0
        return int(self._dev_state[:8].view(torch.int64).item())

    def _hyper_rows(self):
        return [[float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])]
                for gi, _ in self._entries for g in (self.param_groups[gi],)]

    def _build(self, t: int | None = None) -> None:
        """Lay out the (group, tensor) pairs, allocate the device tables and seed them for step count `t` (default: the
        count the current tables hold).  Host-to-device copies: never inside a capture."""
        if t is None:
            t = self._read_t()
        entries = [(gi, p) for gi, g in enumerate(self.param_groups) for p in g["params"]]
        if len(entries) > L.HS_ADAM_MAX_GROUPS:
            raise ValueError(f"GaussianAdam: {len(entries)} (group, tensor) pairs; one launch takes at most {L.HS_ADAM_MAX_GROUPS}")
        if not entries:
            raise ValueError("GaussianAdam: no parameters")
        dev = self._device()
        if any(p.device != dev for _, p in entries):
            raise ValueError("GaussianAdam: all parameters must live on one device")
        for g in self.param_groups:
            self._check_group(g)
        self._entries = entries
        nbytes = L.load().hs_adam_state_bytes(len(entries))
        if nbytes < 0:
            L.check(L.HS_EINVAL, "hs_adam_state_bytes")
        rows = self._hyper_rows()
        # state: u64 t | per group at 64 + 64 g: fp64 beta1^t, fp64 beta2^t, then what the tick kernel derives (pow here,
        # running products on the device: equal to rounding)
        blob = bytearray(nbytes)
        struct.pack_into("<Q", blob, 0, t)
        for i, (_, b1, b2, _) in enumerate(rows):
            struct.pack_into("<dd", blob, 64 + 64 * i, b1 ** t, b2 ** t)
        self._dev_state = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
        self._dev_hyper = torch.tensor(rows, dtype=torch.float64).to(dev)
        self._host_hyper = rows
        if self._dev_state.data_ptr() % 16 or self._dev_hyper.data_ptr() % 8:
            raise RuntimeError("GaussianAdam: the allocator returned a misaligned table")

    def _sync_hyper(self) -> None:
        rows = self._hyper_rows()
        if rows != self._host_hyper:
            for g in self.param_groups:
                self._check_group(g)
            self._dev_hyper.copy_(torch.tensor(rows, dtype=torch.float64))
            self._host_hyper = rows

    def _init_state(self, p: torch.Tensor) -> dict:
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def prepare(self, all_params: bool = True) -> None:
        """Everything a step needs that is not a kernel: the moment tensors (of every parameter, or with all_params=False
        of those that have a gradient now), the device tables, the upload of changed hyper-parameters.  `step()` does this
        itself; call it once before capturing `enqueue()`."""
        if self._entries is None:
            self._build()
        self._sync_hyper()
        for _, p in self._entries:
            if all_params or p.grad is not None:
                self._init_state(p)

    def set_lr(self, lr, group: int | None = None) -> None:
        """Set the learning rate of one group (or of all: a number, or one per group) and upload the table: the next
        step -- or the next replay of a captured one -- uses it."""
        if group is not None:
            self.param_groups[group]["lr"] = float(lr)
        else:
            lrs = [float(lr)] * len(self.param_groups) if not hasattr(lr, "__len__") else [float(x) for x in lr]
            if len(lrs) != len(self.param_groups):
                raise ValueError(f"set_lr: {len(lrs)} learning rates for {len(self.param_groups)} groups")
            for g, x in zip(self.param_groups, lrs):
                g["lr"] = x
        if self._entries is None:
            self._build()
        self._sync_hyper()

    def replace_params(self, mapping: dict) -> None:
        """Swap tensors: `mapping` is {old parameter: (new parameter, exp_avg, exp_avg_sq)} -- what a densification hands
        over (densify.densify_and_prune), the number of rows may differ.  The new tensors take the old ones' places in the
        param groups, the per-parameter state and the launch order; the DEVICE step count and the running products beta^t
        are not touched, so the next step is the one an uninterrupted run would take (rebuilding the optimizer through
        load_state_dict would re-seed the products with pow)."""
        for old, (new, m, v) in mapping.items():
            if not any(q is old for g in self.param_groups for q in g["params"]):
                raise ValueError("GaussianAdam.replace_params: a tensor to replace is not one of the optimizer's parameters")
            for t, what in ((new, "parameter"), (m, "exp_avg"), (v, "exp_avg_sq")):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError(f"GaussianAdam.replace_params: the new {what} must be a contiguous float32 tensor")
                _require_gpu(t, f"the new {what}")
            if m.shape != new.shape or v.shape != new.shape or new.shape[1:] != old.shape[1:]:
                raise ValueError("GaussianAdam.replace_params: exp_avg / exp_avg_sq must have the new parameter's shape, and the "
                                 "new parameter the old one's shape behind dim 0")
            if not new.is_leaf:
                raise ValueError("can't optimize a non-leaf Tensor")
        for old, (new, m, v) in mapping.items():
            for g in self.param_groups:
                g["params"] = [new if q is old else q for q in g["params"]]
            st = self.state.pop(old, {})
            self.state[new] = {"step": st.get("step", torch.tensor(0.0, dtype=torch.float32)), "exp_avg": m, "exp_avg_sq": v}
            if self._entries is not None:
                self._entries = [(gi, new if q is old else q) for gi, q in self._entries]

    # ---- the step ----

    def enqueue(self, visibility: torch.Tensor | None = None) -> None:
        """The two kernels of one step on the current stream, and nothing else (no allocation once `prepare()` has run, no
        copy, no host read): what a captured step calls.  Hyper-parameters are those last uploaded (`step`, `set_lr`,
        `prepare`)."""
        if self._entries is None:
            raise RuntimeError("GaussianAdam.enqueue: call prepare() (or step()) first: the device tables do not exist yet")
        groups = (L.hs_adam_group * len(self._entries))()
        per_gaussian_rows = None
        any_grad = False
        for i, (gi, p) in enumerate(self._entries):
            g = self.param_groups[gi]
            rows, stride, a, n = self._matrix(p, g)
            G = groups[i]
            G.row_stride, G.col_begin, G.col_count = max(stride, 1), a, max(n, 1)
            G.masked = 1 if g["per_gaussian"] else 0
            if g["per_gaussian"]:
                if per_gaussian_rows is not None and rows != per_gaussian_rows:
                    raise ValueError(f"GaussianAdam: per_gaussian groups disagree about the number of Gaussians ({per_gaussian_rows} and {rows})")
                per_gaussian_rows = rows
            grad = p.grad
            if grad is None or p.numel() == 0:
                G.rows = 0          # skipped, as in torch: nothing to do, no pointer looked at
                continue
            if grad.is_sparse:
                raise RuntimeError("GaussianAdam does not support sparse gradients (pass visibility= instead)")
            if grad.dtype != torch.float32 or grad.shape != p.shape or grad.device != p.device or not grad.is_contiguous():
                raise ValueError("GaussianAdam: every .grad must be a contiguous float32 tensor of its parameter's shape and device")
            st = self._init_state(p)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if m.dtype != torch.float32 or not m.is_contiguous() or m.device != p.device or \
                    v.dtype != torch.float32 or not v.is_contiguous() or v.device != p.device:
                raise ValueError("GaussianAdam: exp_avg / exp_avg_sq must be contiguous float32 tensors on the parameter's device")
            G.param, G.grad, G.exp_avg, G.exp_avg_sq = p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr()
            G.rows = rows
            any_grad = True
        if not any_grad:
            return
        a = L.hs_adam_args()
        a.groups, a.n_groups = groups, len(self._entries)
        a.mask_kind, a.mask, a.mask_len = L.HS_ADAM_MASK_NONE, None, 0
        if visibility is not None:
            kind, vis = check_visibility(visibility, per_gaussian_rows)
            a.mask_kind, a.mask, a.mask_len = kind, vis.data_ptr(), vis.numel()
        a.state, a.hyper = self._dev_state.data_ptr(), self._dev_hyper.data_ptr()
        dev = self._dev_state.device
        with _on_device(dev):
            L.check(L.load().hs_adam_step(C.byref(a), _stream(dev)), "hs_adam_step")

    @torch.no_grad()
    def step(self, visibility: torch.Tensor | None = None, closure=None):
        """One Adam step on every parameter that has a gradient.  visibility=None: dense.  An int32 `radii` (visible = > 0)
        or a bool / uint8 mask of length P: the `per_gaussian` groups skip their invisible rows (see the module docstring:
        not the same as dense Adam with zero gradients); other groups stay dense."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.prepare(all_params=False)
        self.enqueue(visibility)
        return loss

    # ---- torch's state_dict ----

    def _refresh_steps(self) -> None:
        t = float(self._read_t())
        for st in self.state.values():
            if "exp_avg" in st:
                st["step"] = torch.tensor(t, dtype=torch.float32)

    def state_dict(self):
        """torch.optim.Adam's layout; `step` is read back from the device (waits for the stream)."""
        if self._dev_state is not None:
            self._refresh_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        """Accepts a torch.optim.Adam state dict over the same groups.  All parameters must be at the same step; the
        products beta^t are rebuilt from it with pow (equal to an uninterrupted run's running products to rounding only)."""
        ours = [(g["per_gaussian"], g["columns"]) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, (pg, cols) in zip(self.param_groups, ours):      # (keys a torch.optim.Adam dict does not carry)
            g.setdefault("per_gaussian", pg)
            g.setdefault("columns", cols)
            for k, v in self.defaults.items():
                g.setdefault(k, v)
            self._check_group(g)
        steps = set()
        for p, st in self.state.items():
            if "exp_avg" not in st:
                continue
            steps.add(int(float(st.get("step", 0.0))))
            for k in ("exp_avg", "exp_avg_sq"):
                st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
            st["step"] = torch.tensor(float(st.get("step", 0.0)), dtype=torch.float32)
        if len(steps) > 1:
            raise ValueError(f"GaussianAdam keeps one step count; the loaded parameters are at steps {sorted(steps)}")
        self._build(t=steps.pop() if steps else 0)
