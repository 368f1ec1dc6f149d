"""Independent float64 truth for the trajectory spline (csrc/spline.hip, image_formation.TrajectorySpline.pose_at).

A plain restatement of the model in the header of spline.hip that imports no project code and shares none of the
implementation's formulations:

  knot_j = exp(delta_j) base_j                       left-multiplied se(3) correction, xi = (rho, omega)
  cubic : j = clamp(floor(t) - 1, 0, J - 4), u = t - (j + 1),
          pose = exp(B3 x3) exp(B2 x2) exp(B1 x1) knot_j,   x_k = log(knot_{j+k} knot_{j+k-1}^-1),
          B_k(u) = sum_{i >= k} b_i(u) of the uniform cubic B-spline basis b_0 .. b_3 (cumulative form)
  linear: j = clamp(floor(t), 0, J - 2), u = t - j, pose = exp(u x1) knot_j

  exp : torch.linalg.matrix_exp of the 4 x 4 twist (no Rodrigues formula, no series switch).
  log : theta = atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2) (no arc-cosine, no clamp); omega = k(theta) vee(R - R^T),
        rho = (1 - hat(omega) / 2 + c(theta) hat(omega)^2) t with
            k(theta) = theta / (2 sin theta)                      = 1/2 + theta^2 / 12 + 7 theta^4 / 720 + ...
            c(theta) = (1 - (theta / 2) cot(theta / 2)) / theta^2 = 1/12 + theta^2 / 720 + theta^4 / 30240 + ...
        from their Taylor series (exact rational coefficients from the Bernoulli numbers, carried until the next term is
        below 1e-30) for theta < 1e-2, from the closed forms above it.
  inverse of a knot: [R t; 0 1]^-1 = [R^T, -R^T t; 0 1], the inverse of a RIGID transform.  The knots the kernel takes are
        float32 and orthonormal only to 2^-24, where the general inverse of the 4 x 4 matrix is another function: with it this
        truth moves by 3e-8 .. 1.5e-7 of a pose's scale on the case table, which says nothing about anybody's arithmetic.

Derivatives: float64 reverse-mode autograd through all of the above, 12 passes (one per pose entry; the samples are
independent of each other once every sample carries its own copy of its 24 knot corrections).  The formula of theta has a
square root of zero exactly where two neighbouring knots have the same rotation; the samples governed by such a pair take
their Jacobian from central differences with step H_CENTRAL = 6e-6 (about eps^(1/3)): truncation h^2 |f'''| / 6 ~ 1e-11
and rounding (a few eps) |pose| / h ~ 2e-10 of the Jacobian's scale, CENTRAL_ERROR = 5e-10 in all -- two orders below 2^-24
(tests/test_spline_truth.py checks that estimate against autograd where both exist).
"""
from fractions import Fraction
from math import comb, factorial

import torch

NI = 25                  # columns of a sample's Jacobian: 6 corrections of each of knots j .. j + 3, then the sample time
THETA_SERIES = 1e-2      # below: Taylor series of k and c; above: closed forms
H_CENTRAL = 6e-6
CENTRAL_ERROR = 5e-10    # of the largest Jacobian entry of the sample


def _bernoulli(n):
    B = [Fraction(1)]
    for m in range(1, n + 1):
        B.append(-sum(comb(m + 1, k) * B[k] for k in range(m)) / (m + 1))
    return B


def _series():
    """Coefficients in x = theta^2 of k(theta) = (1/2) theta / sin(theta) and of c(theta) = (1 - (theta/2) cot(theta/2)) /
    theta^2: theta / sin theta = sum (-1)^(n-1) (2^2n - 2) B_2n theta^2n / (2n)!, (theta/2) cot(theta/2) = sum (-1)^n B_2n
    theta^2n / (2n)!.  Cut where the next term is below 1e-30 at theta = THETA_SERIES."""
    B = _bernoulli(40)
    k_all = [Fraction((-1) ** (n - 1) * (2 ** (2 * n) - 2)) * B[2 * n] / factorial(2 * n) / 2 for n in range(20)]
    c_all = [-Fraction((-1) ** n) * B[2 * n] / factorial(2 * n) for n in range(1, 20)]
    out = []
    for co in (k_all, c_all):
        n = next(i for i in range(len(co)) if abs(co[i]) * Fraction(THETA_SERIES) ** (2 * i) < Fraction(1, 10 ** 30))
        out.append([float(v) for v in co[:n]])
    return out


_K_SERIES, _C_SERIES = _series()
assert _K_SERIES[:3] == [0.5, 1.0 / 12.0, 7.0 / 720.0] and _C_SERIES[:2] == [1.0 / 12.0, 1.0 / 720.0]


def _horner(co, x):
    r = torch.full_like(x, co[-1])
    for c in reversed(co[:-1]):
        r = r * x + c
    return r


def _hat(w):
    z = torch.zeros_like(w[..., 0])
    rows = [torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
            torch.stack([-w[..., 1], w[..., 0], z], -1)]
    return torch.stack(rows, -2)


def exp_se3(xi):
    """[..., 6] -> [..., 4, 4]: the matrix exponential of the twist [[hat(omega), rho], [0, 0]]."""
    top = torch.cat([_hat(xi[..., 3:]), xi[..., :3, None]], -1)
    return torch.linalg.matrix_exp(torch.cat([top, torch.zeros_like(top[..., :1, :])], -2))


def rotation_angle(R):
    """(theta, vee(R - R^T)) with theta = atan2(|vee| / 2, (tr R - 1) / 2)."""
    v = torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    s = torch.sqrt((v * v).sum(-1)) / 2
    c = (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1) / 2
    return torch.atan2(s, c), v


def log_se3(T):
    """[..., 4, 4] -> [..., 6] = (rho, omega)."""
    R, t = T[..., :3, :3], T[..., :3, 3]
    th, v = rotation_angle(R)
    series = th < THETA_SERIES
    safe = torch.where(series, torch.ones_like(th), th)        # (the closed forms are evaluated on every sample)
    k = torch.where(series, _horner(_K_SERIES, th * th), safe / (2 * torch.sin(safe)))
    c = torch.where(series, _horner(_C_SERIES, th * th), (1 - (safe / 2) * torch.cos(safe / 2) / torch.sin(safe / 2)) / (safe * safe))
    om = k[..., None] * v
    K = _hat(om)
    Vinv = torch.eye(3, dtype=T.dtype) - K / 2 + c[..., None, None] * (K @ K)
    return torch.cat([(Vinv @ t[..., None])[..., 0], om], -1)


def rigid_inverse(T):
    Rt = T[..., :3, :3].transpose(-1, -2)
    top = torch.cat([Rt, -(Rt @ T[..., :3, 3:])], -1)
    return torch.cat([top, T[..., 3:, :]], -2)


def segment(times, J, kind):
    """(j [T] int64, first knot of each sample's segment; offset of u: u = t - (j + offset))."""
    fl = torch.floor(times).long()
    if kind == "cubic":
        return (fl - 1).clamp(0, J - 4), 1
    return fl.clamp(0, J - 2), 0


def cumulative_basis(u):
    """B_1, B_2, B_3 of the cumulative cubic B-spline, summed from the uniform basis functions."""
    b1 = (3 * u ** 3 - 6 * u ** 2 + 4) / 6
    b2 = (-3 * u ** 3 + 3 * u ** 2 + 3 * u + 1) / 6
    b3 = u ** 3 / 6
    return b1 + b2 + b3, b2 + b3, b3


def _pose(X, Bk, j, offset, kind):
    """X [T, 6 nk + 1]: every sample's own knot corrections and time; Bk [T, nk, 4, 4] its base knots -> [T, 4, 4]."""
    nk = Bk.shape[1]
    knots = exp_se3(X[:, :-1].reshape(-1, nk, 6)) @ Bk
    u = X[:, -1] - (j + offset).to(X.dtype)
    x = log_se3(knots[:, 1:] @ rigid_inverse(knots[:, :-1]))                    # [T, nk - 1, 6]
    pose = knots[:, 0]
    for k, b in enumerate(cumulative_basis(u) if kind == "cubic" else (u,)):
        pose = exp_se3(b[:, None] * x[:, k]) @ pose
    return pose, x


def evaluate(delta, base, times, kind, jacobian=True):
    """delta [J, 6], base [J, 4, 4], times [T] (float64: the float32 values of the kernel's inputs, widened) ->
    pose [T, 4, 4], seg [T] (int64) and the Jacobian [T, 12, 25] in the kernel's layout: row 4 r + c of the top three pose
    rows, columns 6 k + c the corrections of knot seg + k, column 24 the sample time (linear: columns 12 .. 23 zero)."""
    assert delta.dtype == base.dtype == times.dtype == torch.float64 and kind in ("linear", "cubic")
    J, T = delta.shape[0], times.numel()
    nk = 4 if kind == "cubic" else 2
    assert J >= nk
    j, offset = segment(times, J, kind)
    idx = j[:, None] + torch.arange(nk)
    X = torch.cat([delta[idx].reshape(T, 6 * nk), times.reshape(T, 1)], 1).detach()
    Bk = base[idx]
    with torch.no_grad():
        pose, x = _pose(X, Bk, j, offset, kind)
    if not jacobian:
        return pose, j, None
    Xg = X.clone().requires_grad_(True)
    out = _pose(Xg, Bk, j, offset, kind)[0][:, :3, :].reshape(T, 12)
    jac_x = torch.stack([torch.autograd.grad(out[:, i].sum(), Xg, retain_graph=True)[0] for i in range(12)], 1)
    # a pair of neighbours with the same rotation: sqrt(0) in theta, no derivative by autograd there
    with torch.no_grad():
        knots = exp_se3(X[:, :-1].reshape(-1, nk, 6)) @ Bk
        rel = knots[:, 1:] @ rigid_inverse(knots[:, :-1])
        R = rel[..., :3, :3]
        v2 = ((R - R.transpose(-1, -2)) ** 2).sum((-1, -2))
        flat = ((v2 == 0).any(-1) | ~torch.isfinite(jac_x).all(-1).all(-1)).nonzero()[:, 0]
        if flat.numel():
            Xf, Bf, jf = X[flat], Bk[flat], j[flat]
            cols = []
            for i in range(X.shape[1]):
                e = torch.zeros(X.shape[1], dtype=X.dtype)
                e[i] = H_CENTRAL
                hi = _pose(Xf + e, Bf, jf, offset, kind)[0]
                lo = _pose(Xf - e, Bf, jf, offset, kind)[0]
                cols.append(((hi - lo) / (2 * H_CENTRAL))[:, :3, :].reshape(-1, 12))
            jac_x[flat] = torch.stack(cols, -1)
    jac = torch.zeros(T, 12, NI, dtype=torch.float64)
    jac[:, :, :6 * nk] = jac_x[:, :, :-1]
    jac[:, :, 24] = jac_x[:, :, -1]
    return pose, j, jac
