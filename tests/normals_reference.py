"""numpy restatement of the depth-normal consistency term and of the per-Gaussian normal (normals.hip; include/hdrsplat.h
states the definitions).

    truth(...)            the definition in float64 from the PLAIN cross product of back-projected points, and its analytic
                          gradients in float64, derived from that form (not from the kernel's closed form)
    closed_form(..., dtype)   the kernel's order of operations (the top of normals.hip) in numpy float64 or float32
    magnitudes(...)       per output element the first-order rounding magnitude `mag` of that order of operations
    gaussian_normals(..., mode)   the same three for the per-Gaussian normal

The bound the tests hold an fp32 result to: |x - truth| <= 1e-4 |truth| + C 2^-24 mag, zero elements excepted (they are exact).

`mag` is built mechanically: the kernel's formulas are evaluated on values that carry, beside the float64 number, a bound e on
the rounding error accumulated so far in units of 2^-24 (class V).  Inputs are exact (e = 0).  Every operation propagates the
errors of its operands to first order and adds its own rounding: a sum or difference a +- b adds |a| + |b| (the sum of the
absolute values of its terms), a product, quotient or square root adds |result|.  So the rounding of z = a / d and of the
depth differences is carried through the normalisation, the rotation, the dot product, the gather and the chain rule to the
element, cancellation included (a difference of nearly equal depths keeps the error of both).  A negation and a selection
are exact."""
import numpy as np


class V:
    """a float64 array and the first-order bound of its accumulated rounding error, in units of 2^-24"""
    __array_priority__ = 100

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.e + o.e + np.abs(self.v) + np.abs(o.v))

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.e + o.e + np.abs(self.v) + np.abs(o.v))

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, self.e)

    def __mul__(self, o):
        o = V.of(o)
        r = self.v * o.v
        return V(r, np.abs(o.v) * self.e + np.abs(self.v) * o.e + np.abs(r))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        r = self.v / o.v
        return V(r, self.e / np.abs(o.v) + np.abs(r) * o.e / np.abs(o.v) + np.abs(r))

    def __rtruediv__(self, o):
        return V.of(o) / self

    def __getitem__(self, idx):
        return V(self.v[idx], self.e[idx])

    @property
    def shape(self):
        return self.v.shape


def _sqrt(x):
    if isinstance(x, V):
        r = np.sqrt(x.v)
        return V(r, x.e / (2.0 * r) + r)
    return np.sqrt(x)


def _where(mask, x):
    if isinstance(x, V):
        return V(np.where(mask, x.v, 0.0), np.where(mask, x.e, 0.0))
    return np.where(mask, x, x.dtype.type(0))


def _pad(x, pads):
    if isinstance(x, V):
        return V(np.pad(x.v, pads), np.pad(x.e, pads))
    return np.pad(x, pads)


def _stack(xs, axis):
    if isinstance(xs[0], V):
        return V(np.stack([x.v for x in xs], axis), np.stack([x.e for x in xs], axis))
    return np.stack(xs, axis)


def _value(x):
    return x.v if isinstance(x, V) else x


def validity(invdepth, alpha=None):
    """(valid [B, H, W], interior [B, H, W]) of the definition"""
    d = np.asarray(invdepth, np.float64)
    valid = np.isfinite(d) & (d > 0)
    if alpha is not None:
        a = np.asarray(alpha, np.float64)
        valid &= np.isfinite(a) & (a > 0)
    interior = np.zeros_like(valid)
    if valid.shape[1] >= 3 and valid.shape[2] >= 3:
        interior[:, 1:-1, 1:-1] = (valid[:, 1:-1, 1:-1] & valid[:, 1:-1, :-2] & valid[:, 1:-1, 2:] & valid[:, :-2, 1:-1]
                                   & valid[:, 2:, 1:-1])
    return valid, interior


def _inputs(invdepth, normals, fx, fy, alpha, weight, cam_to_world, dL_dout, cast=np.float32):
    """the call's inputs as the kernel receives them: rounded to `cast` (float32), the absent ones filled in"""
    invdepth = np.asarray(invdepth, cast)
    B, H, W = invdepth.shape
    one = np.ones((B, H, W), cast)
    alpha_ = one if alpha is None else np.asarray(alpha, cast)
    weight_ = one if weight is None else np.asarray(weight, cast)
    R = np.broadcast_to(np.eye(3, dtype=cast), (B, 3, 3)) if cam_to_world is None else np.asarray(cam_to_world, cast)
    g = np.zeros((B, H, W), cast) if dL_dout is None else np.asarray(dL_dout, cast)
    return invdepth, np.asarray(normals, cast), float(cast(fx)), float(cast(fy)), alpha_, weight_, R, g


def _centres(H, W):
    xh = np.arange(W, dtype=np.float64) + 0.5 - W / 2.0
    yh = np.arange(H, dtype=np.float64) + 0.5 - H / 2.0
    return xh, yh


def _kernel(invdepth, normals, fx, fy, alpha, weight, cam_to_world, dL_dout, mode):
    """the order of operations of normals.hip; mode = np.float64 / np.float32 (plain arrays) or "mag" (V)"""
    d, N, fx, fy, a, w, R, g = _inputs(invdepth, normals, fx, fy, alpha, weight, cam_to_world, dL_dout)
    B, H, W = d.shape
    valid, interior = validity(d, alpha)
    dt = np.float64 if mode == "mag" else mode
    wrap = V if mode == "mag" else (lambda x: x)
    zero = lambda *shape: wrap(np.zeros(shape, dt))
    res = dict(valid=valid, interior=interior)
    if H < 3 or W < 3:
        res.update(out=zero(B, H, W), depth_normals=zero(B, 3, H, W), d_normals=zero(B, 3, H, W), d_invdepth=zero(B, H, W),
                   d_alpha=zero(B, H, W))
        return res
    ds = wrap(np.where(valid, d, 1).astype(dt))
    z = wrap(np.where(valid, a, 1).astype(dt)) / ds
    xh_, yh_ = _centres(H, W)
    xh = xh_[1:-1].astype(dt)[None, None, :]
    yh = yh_[1:-1].astype(dt)[None, :, None]
    core = (slice(None), slice(1, -1), slice(1, -1))
    inner = interior[core]
    zl, zr, zu, zd = z[:, 1:-1, :-2], z[:, 1:-1, 2:], z[:, :-2, 1:-1], z[:, 2:, 1:-1]
    sx, sy = zr + zl, zd + zu
    rx, ry = (zr - zl) / sx, (zd - zu) / sy
    m = [fx * rx, fy * ry, -((ry * yh + rx * xh) + 1.0)]
    ln = _sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    nd = [m[0] / ln, m[1] / ln, m[2] / ln]
    Rm = R.astype(dt)
    r_ = lambda i, j: wrap(Rm[:, i, j][:, None, None])
    n = [(r_(i, 0) * nd[0] + r_(i, 1) * nd[1]) + r_(i, 2) * nd[2] for i in range(3)]
    Nc = [wrap(N[:, k][core].astype(dt)) for k in range(3)]
    wc = wrap(w[core].astype(dt))
    out = wc * (1.0 - ((Nc[0] * n[0] + Nc[1] * n[1]) + Nc[2] * n[2]))
    full = lambda x: _pad(_where(inner, x), ((0, 0), (1, 1), (1, 1)))
    res["out"] = full(out)
    res["depth_normals"] = _stack([full(n[k]) for k in range(3)], 1)
    # backward
    gw = wrap(g[core].astype(dt)) * wc
    res["d_normals"] = _stack([full(-(gw * n[k])) for k in range(3)], 1)
    v = [-(gw * ((r_(0, j) * Nc[0] + r_(1, j) * Nc[1]) + r_(2, j) * Nc[2])) for j in range(3)]
    t = (nd[0] * v[0] + nd[1] * v[1]) + nd[2] * v[2]
    u = [(v[j] - nd[j] * t) / ln for j in range(3)]
    hx = (u[0] * fx - u[2] * xh) / (sx * sx)
    hy = (u[1] * fy - u[2] * yh) / (sy * sy)
    send = [full(hx * (zl + zl)), full(-(hx * (zr + zr))), full(hy * (zu + zu)), full(-(hy * (zd + zd)))]
    # the sample at (x, y) takes send[0] of (x - 1, y), send[1] of (x + 1, y), send[2] of (x, y - 1), send[3] of (x, y + 1)
    p0 = _pad(send[0], ((0, 0), (0, 0), (1, 0)))[:, :, :-1]
    p1 = _pad(send[1], ((0, 0), (0, 0), (0, 1)))[:, :, 1:]
    p2 = _pad(send[2], ((0, 0), (1, 0), (0, 0)))[:, :-1, :]
    p3 = _pad(send[3], ((0, 0), (0, 1), (0, 0)))[:, 1:, :]
    dz = ((p0 + p1) + p2) + p3
    res["d_invdepth"] = _where(valid, -((dz * z) / ds))
    res["d_alpha"] = _where(valid, dz / ds)
    return res


KEYS = ("out", "depth_normals", "d_normals", "d_invdepth", "d_alpha")


def closed_form(invdepth, normals, fx, fy, alpha=None, weight=None, cam_to_world=None, dL_dout=None, dtype=np.float64):
    return _kernel(invdepth, normals, fx, fy, alpha, weight, cam_to_world, dL_dout, dtype)


def magnitudes(invdepth, normals, fx, fy, alpha=None, weight=None, cam_to_world=None, dL_dout=None):
    """{key: mag} for KEYS, beside valid / interior"""
    r = _kernel(invdepth, normals, fx, fy, alpha, weight, cam_to_world, dL_dout, "mag")
    return {k: (r[k].e if k in KEYS else r[k]) for k in r}


def truth(invdepth, normals, fx, fy, alpha=None, weight=None, cam_to_world=None, dL_dout=None, cast=np.float32):
    """The definition in float64 from the plain cross product, and its analytic gradients: with uc = dL/dc,
    dL/dA = uc x Bv and dL/dBv = A x uc for c = Bv x A; P = z ray, so a sample's dL/dz = ray . dL/dP.  cast=np.float64: the inputs are taken as they are (finite differences)."""
    d, N, fx, fy, a, w, R, g = _inputs(invdepth, normals, fx, fy, alpha, weight, cam_to_world, dL_dout, cast)
    d, N, a, w, R, g = (x.astype(np.float64) for x in (d, N, a, w, R, g))
    B, H, W = d.shape
    valid, interior = validity(d, alpha)
    res = dict(valid=valid, interior=interior, out=np.zeros((B, H, W)), depth_normals=np.zeros((B, 3, H, W)),
               d_normals=np.zeros((B, 3, H, W)), d_invdepth=np.zeros((B, H, W)), d_alpha=np.zeros((B, H, W)))
    if H < 3 or W < 3:
        return res
    ds = np.where(valid, d, 1.0)
    z = np.where(valid, a, 1.0) / ds
    xh, yh = _centres(H, W)
    ray = np.stack(np.broadcast_arrays(xh[None, :] / fx, yh[:, None] / fy, np.ones((H, W))), -1)      # [H, W, 3]
    P = z[..., None] * ray[None]
    A = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    Bv = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    c = np.cross(Bv, A)
    ln = np.linalg.norm(c, axis=-1, keepdims=True)
    nd = c / ln
    n = np.einsum("bij,bhwj->bhwi", R, nd)
    inner = interior[:, 1:-1, 1:-1]
    Nc = np.moveaxis(N[:, :, 1:-1, 1:-1], 1, -1)
    wc, gc = w[:, 1:-1, 1:-1], g[:, 1:-1, 1:-1]
    res["out"][:, 1:-1, 1:-1] = np.where(inner, wc * (1.0 - (Nc * n).sum(-1)), 0.0)
    res["depth_normals"][:, :, 1:-1, 1:-1] = np.moveaxis(np.where(inner[..., None], n, 0.0), -1, 1)
    gw = np.where(inner, gc * wc, 0.0)[..., None]
    res["d_normals"][:, :, 1:-1, 1:-1] = np.moveaxis(-gw * np.where(inner[..., None], n, 0.0), -1, 1)
    v = np.einsum("bij,bhwi->bhwj", R, -gw * Nc)                      # dL/dnd = R^T dL/dn
    uc = np.where(inner[..., None], (v - nd * (nd * v).sum(-1, keepdims=True)) / ln, 0.0)
    gA, gB = np.cross(uc, Bv), np.cross(A, uc)
    dP = np.zeros_like(P)
    dP[:, 1:-1, 2:] += gA
    dP[:, 1:-1, :-2] -= gA
    dP[:, 2:, 1:-1] += gB
    dP[:, :-2, 1:-1] -= gB
    dz = (dP * ray[None]).sum(-1)
    res["d_invdepth"] = np.where(valid, -dz * z / ds, 0.0)
    res["d_alpha"] = np.where(valid, dz / ds, 0.0)
    return res


def needed(got, ref, mag):
    """the largest constant any element needs in |got - ref| <= 1e-4 |ref| + C 2^-24 mag; inf where an element whose reference
    is exactly zero with no magnitude is not zero"""
    got, ref, mag = (np.asarray(x, np.float64) for x in (got, ref, mag))
    excess = np.abs(got - ref) - 1e-4 * np.abs(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(excess > 0, excess / (2.0 ** -24 * mag), 0.0)
    need = np.where(np.isfinite(need), need, np.where(excess > 0, np.inf, 0.0))
    return float(need.max()) if need.size else 0.0


# ---- the per-Gaussian normal ----

def _columns(w, x, y, z):
    return ([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + w * z), 2.0 * (x * z - w * y)],
            [2.0 * (x * y - w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z + w * x)],
            [2.0 * (x * z + w * y), 2.0 * (y * z - w * x), 1.0 - 2.0 * (x * x + y * y)])


def _pick(k, trio):
    """element i of the result is trio[k[i]][i] (a selection: exact)"""
    if isinstance(trio[0], V):
        return V(_pick(k, [t.v for t in trio]), _pick(k, [t.e for t in trio]))
    return np.where(k == 0, trio[0], np.where(k == 1, trio[1], trio[2]))


def shortest_axis(scales):
    """the index of the smallest scale, the lowest index on a tie"""
    return np.argmin(np.asarray(scales), axis=1)


def gaussian_normals(rotations, scales, means3D, campos, dL_dnormals=None, mode=np.float64):
    """dict(normals [P, 3], d_rotations [P, 4], k, sign, live) in the kernel's order of operations; mode np.float64 (the truth),
    np.float32 (the restatement) or "mag" (the values are the rounding magnitudes).  k comes from the scales as given; the sign
    from the arithmetic of the mode."""
    q = np.asarray(rotations, np.float32)
    P = q.shape[0]
    dt = np.float64 if mode == "mag" else mode
    wrap = V if mode == "mag" else (lambda x: x)
    g = np.zeros((P, 3), np.float32) if dL_dnormals is None else np.asarray(dL_dnormals, np.float32)
    # the kernel's |q| is the square root of the fp32 sum of squares: a row counts as |q| = 0 (zeros both ways) unless every
    # component is finite and that sum is finite and positive (hdrsplat.h states the range)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ss = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    live = np.isfinite(q).all(1) & np.isfinite(ss) & (ss > 0)
    qs = np.where(live[:, None], q, np.float32(1)).astype(dt)
    c = [wrap(qs[:, i]) for i in range(4)]
    ln = _sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + c[3] * c[3])
    w, x, y, z = (ci / ln for ci in c)
    cols = _columns(w, x, y, z)
    k = shortest_axis(scales)
    col = [_pick(k, [cols[j][i] for j in range(3)]) for i in range(3)]
    cam = np.broadcast_to(np.asarray(campos, np.float32).reshape(1, 3), (P, 3)).astype(dt)
    mean = np.asarray(means3D, np.float32).astype(dt)
    e = [wrap(cam[:, i]) - wrap(mean[:, i]) for i in range(3)]
    dot = (col[0] * e[0] + col[1] * e[1]) + col[2] * e[2]
    sign = np.where(_value(dot) >= 0, 1.0, -1.0).astype(dt)
    normals = _stack([_where(live, col[i] * wrap(sign)) for i in range(3)], 1)
    gs = [wrap((g[:, i].astype(dt)) * sign) for i in range(3)]
    g0, g1, g2 = gs
    d = [None] * 3
    d[0] = [2.0 * (z * g1 - y * g2), 2.0 * (y * g1 + z * g2), 2.0 * (x * g1 - w * g2) - 4.0 * (y * g0), 2.0 * (w * g1 + x * g2) - 4.0 * (z * g0)]
    d[1] = [2.0 * (x * g2 - z * g0), 2.0 * (y * g0 + w * g2) - 4.0 * (x * g1), 2.0 * (x * g0 + z * g2), 2.0 * (y * g2 - w * g0) - 4.0 * (z * g1)]
    d[2] = [2.0 * (y * g0 - x * g1), 2.0 * (z * g0 - w * g1) - 4.0 * (x * g2), 2.0 * (w * g0 + z * g1) - 4.0 * (y * g2), 2.0 * (x * g0 + y * g1)]
    dq = [_pick(k, [d[j][i] for j in range(3)]) for i in range(4)]
    qh = [w, x, y, z]
    t = ((w * dq[0] + x * dq[1]) + y * dq[2]) + z * dq[3]
    rows = [(dq[i] - qh[i] * t) / ln for i in range(4)]
    d_rot = _stack([_where(live, r) for r in rows], 1)
    if mode == "mag":
        return dict(normals=normals.e, d_rotations=d_rot.e, k=k, sign=sign, live=live, margin=np.abs(dot.v), margin_mag=dot.e)
    return dict(normals=normals, d_rotations=d_rot, k=k, sign=sign, live=live)
