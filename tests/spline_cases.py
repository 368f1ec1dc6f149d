"""The case table of the trajectory-spline tests (tests/test_spline_truth.py on the CPU, tests/test_spline_kernel_gpu.py on
the GPU): knots, corrections and sample times at the places where the pose kernel and the tensor implementation can go
wrong, each with its float64 truth (tests/spline_reference.py), computed once per session and shared.

Every case is generated from a fixed seed.  The inputs are float32 (what the kernel takes); the truth sees them widened to
float64, so every implementation picks the same segment.

  families (base knots):  lookat       knots_from_lookat(J, radius=0.3)
                          free         6-DoF, a random rotation of 0.05 .. 0.2 rad per step plus a translation
                          translation  the same rotation at every knot (relative theta = 0 between all neighbours)
                          identical    free, one knot repeated (log of the identity)
                          angle_4e-4, angle_5e-4, angle_1e-6
                                       free, one pair of neighbours that far apart in rotation: either side of the
                                       implementation's arc-cosine clamp (4.47e-4 rad), and far inside it
                          angle_2.5    free, one pair 2.5 rad apart
  corrections:            zero | w2_0.9e-8, w2_1.1e-8 (|omega|^2 of every knot, either side of the series switch of exp) |
                          randn (0.02 randn) | big (0.02 randn, one knot with |omega| = 1.5)
  times (in this order, cut at T, filled up to T with uniform random times inside t_range):
                          t_max (cubic: j clamps, u = 1), t_min - 0.4, t_max + 0.4 (extrapolation, u < 0 and u > 1),
                          every integer of t_range, the float32 neighbours of every interior integer

  {families} x {corrections} at J = 7 cubic and J = 3 linear with T = 65; {J} x {T} with free knots and randn corrections.
"""
import functools
import math
import zlib

import numpy as np
import torch

import spline_reference as R
from casualhdrsplat_amd import image_formation as IF

FAMILIES = ("lookat", "free", "translation", "identical", "angle_4e-4", "angle_5e-4", "angle_1e-6", "angle_2.5")
DELTAS = ("zero", "w2_0.9e-8", "w2_1.1e-8", "randn", "big")
KNOT_COUNTS = {"linear": (2, 3), "cubic": (4, 5, 7)}
SAMPLE_COUNTS = (1, 2, 3, 64, 65, 4097)


def t_range(J, kind):
    return (1.0, float(J - 2)) if kind == "cubic" else (0.0, float(J - 1))


def _unit(g):
    v = torch.randn(3, generator=g, dtype=torch.float64)
    return v / v.norm()


def _twist(g, angle, shift=0.3):
    return torch.cat([shift * torch.randn(3, generator=g, dtype=torch.float64), angle * _unit(g)])


def base_knots(family, J, g):
    """[J, 4, 4] float32."""
    if family == "lookat":
        return IF.knots_from_lookat(J, radius=0.3).float()
    first = R.exp_se3(_twist(g, 0.7, 1.0))
    steps = [_twist(g, 0.05 + 0.15 * float(torch.rand((), generator=g, dtype=torch.float64))) for _ in range(J - 1)]
    m = (J - 1) // 2                       # the special pair is (m, m + 1): inside the segments the listed times visit
    if family == "translation":
        for s in steps:
            s[3:] = 0.0
    elif family == "identical":
        steps[m][:] = 0.0
    elif family.startswith("angle_"):
        steps[m] = _twist(g, float(family[len("angle_"):]))
    elif family != "free":
        raise ValueError(family)
    knots = [first]
    for s in steps:
        knots.append(R.exp_se3(s) @ knots[-1])
    out = torch.stack(knots).float()
    if family == "identical":
        out[m + 1] = out[m]
    if family == "translation":
        out[:, :3, :3] = out[0, :3, :3]
    return out


def corrections(name, J, g):
    """[J, 6] float32."""
    d = torch.zeros(J, 6, dtype=torch.float64)
    if name.startswith("w2_"):
        for j in range(J):
            d[j] = _twist(g, math.sqrt(float(name[3:])), 0.01)
    elif name in ("randn", "big"):
        d = 0.02 * torch.randn(J, 6, generator=g, dtype=torch.float64)
        if name == "big":
            d[(J - 1) // 2, 3:] = 1.5 * _unit(g)
    elif name != "zero":
        raise ValueError(name)
    return d.float()


def sample_times(J, kind, T, g):
    """[T] float32."""
    lo, hi = t_range(J, kind)
    ts = [hi, lo - 0.4, hi + 0.4] + [float(k) for k in range(int(lo), int(hi) + 1)]
    for k in range(int(lo) + 1, int(hi)):
        ts += [float(np.nextafter(np.float32(k), np.float32(-np.inf))), float(np.nextafter(np.float32(k), np.float32(np.inf)))]
    ts = torch.tensor(ts[:T], dtype=torch.float32)
    fill = (lo + (hi - lo) * torch.rand(T - ts.numel(), generator=g, dtype=torch.float64)).float()
    return torch.cat([ts, fill])


class Case:
    def __init__(self, kind, J, T, family, delta):
        self.kind, self.J, self.T, self.family, self.delta_name = kind, J, T, family, delta
        self.id = f"{kind}-J{J}-T{T}-{family}-{delta}"

    def __repr__(self):
        return self.id

    @functools.cached_property
    def inputs(self):
        """(delta [J, 6], base [J, 4, 4], times [T]), float32, on the CPU."""
        g = torch.Generator().manual_seed(zlib.crc32(self.id.encode()))
        base = base_knots(self.family, self.J, g)
        return corrections(self.delta_name, self.J, g), base, sample_times(self.J, self.kind, self.T, g)

    @functools.cached_property
    def truth(self):
        """(pose [T, 4, 4], seg [T], jacobian [T, 12, 25]) in float64 from the float32 inputs, widened.  Read-only."""
        delta, base, times = self.inputs
        out = R.evaluate(delta.double(), base.double(), times.double(), self.kind)
        assert all(torch.isfinite(o).all() for o in out), f"{self.id}: the truth is not finite (a mis-specified case)"
        return out


def _table():
    cases = [Case(kind, J, 65, family, delta) for kind, J in (("cubic", 7), ("linear", 3)) for family in FAMILIES for delta in DELTAS]
    cases += [Case(kind, J, T, "free", "randn") for kind in ("linear", "cubic") for J in KNOT_COUNTS[kind] for T in SAMPLE_COUNTS
              if not (T == 65 and J in (3, 7))]          # (those two are in the first block already)
    return cases


CASES = _table()


def scales(pose, jac):
    """The largest magnitude of every sample's pose and of its Jacobian: ([T], [T])."""
    return pose[:, :3, :].abs().amax((1, 2)), jac.abs().amax((1, 2))
