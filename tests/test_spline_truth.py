"""The tensor implementation of the trajectory spline (TrajectorySpline.pose_at, fused = False, float64) against the
independent float64 truth (tests/spline_reference.py) over the case table of tests/spline_cases.py: poses and the full
12 x 25 Jacobian, which is assembled from autograd.  The kernel (csrc/spline.hip) shares this implementation's
formulas line by line, so what is measured here -- from two references, never from the kernel -- is the error of the shared
formulation: the floor of the kernel's bar in tests/test_spline_kernel_gpu.py, and asserted to be at most 2^-24 (the
formulation is at least as accurate as the float32 the kernel rounds its outputs to).

E_tensor: the largest |tensor - truth| over a sample's pose (Jacobian) entries divided by the largest magnitude in that
sample's pose (Jacobian); per case family the maximum over its cases (both kinds, all corrections, all samples):

  family        E_tensor pose   E_tensor Jacobian      with the clamped arc-cosine this module found in se3_log (pose / Jacobian)
  lookat        6.3e-14         6.6e-11                3.1e-10 / 7.7e-9
  free          1.1e-14         5.7e-11                2.0e-9  / 2.3e-8      (includes the {J} x {T} cross: 1.1e-14 / 1.2e-12)
  translation   1.7e-13         1.9e-9                 1.2e-9  / 7.8e-8      > 2^-24
  identical     1.3e-14         1.6e-10                2.8e-9  / 7.8e-8      > 2^-24
  angle_4e-4    2.6e-14         1.5e-10                1.7e-9  / 1.5e-7      > 2^-24
  angle_5e-4    3.6e-14         2.0e-10                2.6e-9  / 3.2e-8
  angle_1e-6    1.4e-13         2.5e-9                 2.0e-9  / 7.7e-8      > 2^-24
  angle_2.5     1.6e-14         4.8e-11                2.5e-6  / 4.3e-5      > 2^-24

The right-hand columns are the finding this module made: with the angle from a clamped arc-cosine of the trace, the clamp
(active below 4.47e-4 rad) removed d theta from the Jacobian, about 1e-7 of its scale, and at 2.5 rad the arc-cosine multiplied
the 2^-24 by which the float32 knots miss orthonormality by 1 / sin(theta).  image_formation.se3_log and spline.hip now take
the angle from atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2).

The 1.9e-9 and 2.5e-9 of `translation` and `angle_1e-6` come from their w2 corrections and belong to the tensor
implementation, not to the truth: against fourth-order (Richardson) differences of the pose the truth's autograd is within
2e-12 there, the tensor implementation's 1.4e-9 off.  The relative rotations are about 1e-4 rad, so se3_exp of B_k x_k runs
its closed forms just above their switch (theta^2 = 1e-8), where the derivatives of (1 - cos theta) / theta^2 and
(1 - sin theta / theta) / theta^2 cancel to eight digits.  The kernel shares that, which is what the floor is for.
"""
import pytest
import torch

import spline_cases as C
import spline_reference as R
from casualhdrsplat_amd import image_formation as IF

BAR = 2.0 ** -24


def tensor_result(case, chunk=128):
    """TrajectorySpline.pose_at in tensor form (fused = False, float64) on the case's inputs: (pose [T, 4, 4], jacobian
    [T, 12, 25] in the kernel's layout).  The Jacobian is assembled from autograd: per chunk of samples one batched backward
    pass with a unit vector for every (sample, pose entry); the rows seg .. seg + 3 of d / d delta and the sample's own
    entry of d / d t are the sample's 25 columns."""
    delta, base, times = case.inputs
    traj = IF.TrajectorySpline(base, kind=case.kind).double()
    traj.fused = False
    with torch.no_grad():
        traj.delta.copy_(delta.double())
    seg = case.truth[1]
    nk = 4 if case.kind == "cubic" else 2
    pose = torch.zeros(case.T, 4, 4, dtype=torch.float64)
    jac = torch.zeros(case.T, 12, R.NI, dtype=torch.float64)
    for lo in range(0, case.T, chunk):
        t = times[lo:lo + chunk].double().requires_grad_(True)
        n = t.numel()
        out = traj.pose_at(t)
        pose[lo:lo + n] = out.detach()
        units = torch.eye(n * 12, dtype=torch.float64).reshape(n * 12, n, 12)
        gd, gt = torch.autograd.grad(out[:, :3, :].reshape(n, 12), (traj.delta, t), units, is_grads_batched=True)
        gd, gt = gd.reshape(n, 12, case.J, 6), gt.reshape(n, 12, n)
        rows = seg[lo:lo + n, None] + torch.arange(nk)                                     # [n, nk]
        own = gd[torch.arange(n)[:, None, None], torch.arange(12)[None, :, None], rows[:, None, :]]   # [n, 12, nk, 6]
        jac[lo:lo + n, :, :6 * nk] = own.reshape(n, 12, 6 * nk)
        jac[lo:lo + n, :, 24] = gt[torch.arange(n), :, torch.arange(n)]
    return pose, jac


def errors(case):
    """(E_pose, E_jac): the largest |tensor - truth| over a sample's pose (Jacobian) entries divided by the largest magnitude in
    that sample's pose (Jacobian), maximum over the samples."""
    pose, _, jac = case.truth
    got_pose, got_jac = tensor_result(case)
    sp, sj = C.scales(pose, jac)
    return (float(((got_pose - pose)[:, :3, :].abs().amax((1, 2)) / sp).max()), float(((got_jac - jac).abs().amax((1, 2)) / sj).max()))


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_tensor_implementation_is_within_a_float32_rounding_of_the_truth(case):
    assert all(torch.isfinite(x).all() for x in case.truth), case.id
    e_pose, e_jac = errors(case)
    print(f"{case.id}: E_tensor pose {e_pose:.2e} jacobian {e_jac:.2e}")
    assert e_pose <= BAR and e_jac <= BAR, (case.id, e_pose, e_jac)


def test_truth_exp_and_log_are_inverse_and_central_differences_hold_their_estimate():
    """The truth against itself: log(exp(xi)) = xi across the series switch of the log and up to 2.5 rad, and the central
    differences it uses at identical rotations agree with its autograd, where both exist, within CENTRAL_ERROR."""
    g = torch.Generator().manual_seed(3)
    for angle in (0.0, 1e-9, 1e-6, 4e-4, 0.99e-2, 1.01e-2, 0.3, 2.5):
        xi = torch.cat([torch.randn(3, generator=g, dtype=torch.float64), angle * C._unit(g)])
        assert float((R.log_se3(R.exp_se3(xi)) - xi).abs().max()) <= 1e-14 * max(1.0, float(xi.abs().max())), angle
    case = next(c for c in C.CASES if c.id == "cubic-J7-T65-free-randn")
    delta, base, times = (x.double() for x in case.inputs)
    _, seg, jac = case.truth
    j, offset = R.segment(times, case.J, case.kind)
    idx = j[:, None] + torch.arange(4)
    X = torch.cat([delta[idx].reshape(case.T, 24), times[:, None]], 1)
    worst = 0.0
    for i in range(25):
        e = torch.zeros(25, dtype=torch.float64)
        e[i] = R.H_CENTRAL
        hi, lo = (R._pose(X + s * e, base[idx], j, offset, case.kind)[0] for s in (1, -1))
        col = ((hi - lo) / (2 * R.H_CENTRAL))[:, :3, :].reshape(case.T, 12)
        worst = max(worst, float(((col - jac[:, :, i]).abs().amax(1) / C.scales(case.truth[0], jac)[1]).max()))
    assert worst <= R.CENTRAL_ERROR, worst
