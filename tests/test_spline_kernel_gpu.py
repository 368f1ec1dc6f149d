"""hs_spline_poses (csrc/spline.hip) on the MI355X against the independent float64 truth (tests/spline_reference.py), entry by
entry: poses, the whole 12 x 25 Jacobian and the segment index, over the case table of tests/spline_cases.py (knot counts
2 .. 7, 1 .. 4097 samples, integer / end / extrapolated sample times and the float32 neighbours of the integers, identical and
nearly identical neighbouring knots, rotations up to 2.5 rad, corrections either side of the series switch of exp).

The bar of an entry: |got - truth| <= 2^-23 |truth| + 4 E_tensor(family) scale.  2^-23 |truth| is one float32 rounding of a
float64 result with a factor 2 of margin; scale is the largest magnitude in the sample's pose (Jacobian); E_tensor is the
error of the formulation the kernel shares with the tensor implementation, measured on the CPU between that implementation
in float64 and the truth -- never from the kernel -- and recorded in the docstring of tests/test_spline_truth.py; the factor 4
covers the kernel's own order of float64 operations.
"""
import pytest
import torch

import spline_cases as C
import spline_reference as R
from casualhdrsplat_amd import image_formation as IF

pytestmark = pytest.mark.gpu

DEV = "cuda"
# E_tensor per case family: copied from the docstring of tests/test_spline_truth.py, where it was measured (largest of the
# pose and the Jacobian figure of the family, rounded up)
E_TENSOR = {"lookat": 6.6e-11, "free": 5.7e-11, "translation": 1.9e-9, "identical": 1.6e-10, "angle_4e-4": 1.5e-10,
            "angle_5e-4": 2.0e-10, "angle_1e-6": 2.5e-9, "angle_2.5": 4.8e-11}
SENTINEL = -7.25e8


def launch(case, pad=2):
    """One launch on outputs that hold `pad` samples more than the case has, pre-filled with a sentinel:
    (w2c [T + pad, 4, 4], jac [T + pad, 12, 25], seg [T + pad]) on the CPU."""
    from casualhdrsplat_amd import _lib as L
    from casualhdrsplat_amd.rasterizer import _stream
    delta, base, times = (x.to(DEV).contiguous() for x in case.inputs)
    T = case.T
    w2c = torch.full((T + pad, 4, 4), SENTINEL, dtype=torch.float32, device=DEV)
    jac = torch.full((T + pad, 12, 25), SENTINEL, dtype=torch.float32, device=DEV)
    seg = torch.full((T + pad,), -77, dtype=torch.int32, device=DEV)
    with torch.cuda.device(w2c.device):
        L.check(L.load().hs_spline_poses(case.J, T, 1 if case.kind == "cubic" else 0, delta.data_ptr(), base.data_ptr(),
                                         times.data_ptr(), w2c.data_ptr(), jac.data_ptr(), seg.data_ptr(), _stream()), "hs_spline_poses")
    torch.cuda.synchronize()
    return w2c.cpu(), jac.cpu(), seg.cpu()


def _worst(got, truth, floor):
    """(largest excess of |got - truth| over the bar 2^-23 |truth| + floor, its index) -- floor broadcasts per sample."""
    excess = (got.double() - truth).abs() - (2.0 ** -23 * truth.abs() + floor)
    i = int(excess.argmax())
    return float(excess.reshape(-1)[i]), i


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_kernel_matches_the_truth_entry_by_entry(case):
    pose, seg, jac = case.truth
    T = case.T
    w2c, got_jac, got_seg = launch(case)
    # nothing beyond T samples is written
    assert bool((w2c[T:] == SENTINEL).all()) and bool((got_jac[T:] == SENTINEL).all()) and bool((got_seg[T:] == -77).all())
    w2c, got_jac, got_seg = w2c[:T], got_jac[:T], got_seg[:T]
    assert torch.isfinite(w2c).all() and torch.isfinite(got_jac).all()
    assert torch.equal(got_seg.long(), seg), (case.id, "seg")
    assert torch.equal(w2c[:, 3, :], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(T, 4))
    if case.kind == "linear":
        assert bool((got_jac[:, :, 12:24] == 0).all())
    sp, sj = C.scales(pose, jac)
    E = E_TENSOR[case.family]
    e_pose, i_pose = _worst(w2c[:, :3, :], pose[:, :3, :], 4 * E * sp[:, None, None])
    e_jac, i_jac = _worst(got_jac, jac, 4 * E * sj[:, None, None])
    print(f"{case.id}: worst excess over the bar: pose {e_pose:.3e} (flat index {i_pose}), jacobian {e_jac:.3e} ({i_jac})")
    assert e_pose <= 0, (case.id, "pose", e_pose, divmod(i_pose, 12))
    assert e_jac <= 0, (case.id, "jacobian", e_jac, (i_jac // 300, (i_jac % 300) // 25, i_jac % 25))
    # two launches give the same bits
    again = launch(case)
    assert torch.equal(again[0][:T], w2c) and torch.equal(again[1][:T], got_jac) and torch.equal(again[2][:T], got_seg)


def _wrapper_inputs(name, kind, J):
    lo, hi = C.t_range(J, kind)
    if name == "frame_grid":
        # [F, N] = [3, 4] as HDRBlurFormation.cameras_all builds it: frame_times[:, None] + s[None, :] * width[:, None], one
        # frame at each end of t_range (half of its window extrapolates)
        frame_times = torch.tensor([lo, 0.5 * (lo + hi) + 0.13, hi], dtype=torch.float32)
        width = torch.tensor([0.8, 1.0, 0.6], dtype=torch.float32)
        s = (torch.arange(4, dtype=torch.float32) + 0.5) / 4 - 0.5
        return frame_times[:, None] + s[None, :] * width[:, None]
    g = torch.Generator().manual_seed(5)
    full = (lo + (hi - lo) * torch.rand(2 * 13, generator=g, dtype=torch.float64)).float()
    return full, slice(None, None, 2)                      # a strided view: every other element


@pytest.mark.parametrize("kind,J", [("linear", 3), ("cubic", 7)])
@pytest.mark.parametrize("name", ["frame_grid", "strided"])
def test_autograd_wrapper_contracts_the_jacobian(name, kind, J):
    """TrajectorySpline.pose_at on the GPU (_SplinePoses) under random float64 weights: delta.grad and t.grad against the
    truth's Jacobian contracted with the same weights in float64 and scattered into rows seg .. seg + 3.  Bar: float32
    accumulation, |got - ref| <= 2^-23 (number of terms) sum |terms|."""
    case = C.Case(kind, J, 1, "free", "randn")
    delta, base, _ = case.inputs
    src = _wrapper_inputs(name, kind, J)
    if name == "strided":
        full = src[0].to(DEV).requires_grad_(True)
        t_gpu = full[src[1]]
        assert not t_gpu.is_contiguous()
    else:
        full = src.to(DEV).requires_grad_(True)
        t_gpu = full
    times = t_gpu.detach().cpu().reshape(-1)
    T = times.numel()
    pose, seg, jac = R.evaluate(delta.double(), base.double(), times.double(), kind)
    assert torch.isfinite(pose).all() and torch.isfinite(jac).all()
    traj = IF.TrajectorySpline(base, kind=kind).to(DEV)
    with torch.no_grad():
        traj.delta.copy_(delta)
    w = torch.randn(T, 4, 4, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    out = traj.pose_at(t_gpu)
    assert out.shape == (T, 4, 4)
    (out * w.float().to(DEV)).sum().backward()
    w32 = w.float().double()                               # (the weights the GPU saw)
    terms = w32[:, :3, :].reshape(T, 12, 1) * jac          # [T, 12, 25]
    gi, gi_abs = terms.sum(1), terms.abs().sum(1)          # [T, 25]
    ref_d, abs_d, n_d = (torch.zeros(J, 6, dtype=torch.float64) for _ in range(3))
    for s in range(T):
        for k in range(4 if kind == "cubic" else 2):
            row = int(seg[s]) + k
            ref_d[row] += gi[s, 6 * k:6 * k + 6]
            abs_d[row] += gi_abs[s, 6 * k:6 * k + 6]
            n_d[row] += 12
    got_d = traj.delta.grad.cpu().double()
    assert bool(((got_d - ref_d).abs() <= 2.0 ** -23 * n_d * abs_d).all()), (got_d - ref_d).abs().max()
    got_t = full.grad.cpu().double()
    if name == "strided":
        assert bool((got_t[1::2] == 0).all())
        got_t = got_t[::2]
    got_t = got_t.reshape(-1)
    assert bool(((got_t - gi[:, 24]).abs() <= 2.0 ** -23 * 12 * gi_abs[:, 24]).all()), (got_t - gi[:, 24]).abs().max()
    assert float(got_d.abs().sum()) > 0 and float(got_t.abs().sum()) > 0
