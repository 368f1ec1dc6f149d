"""numpy restatement of the 3D smoothing filter (include/hdrsplat.h: hs_smoothing_filter, hs_smoothing_apply,
hs_smoothing_apply_backward), operation for operation in float32, and the float64 evaluation of the same formulas the bounds
are stated against.

The filter (`filter_3d`): per Gaussian and camera
    xc = ((m0 x + m4 y) + m8 z) + m12, yc, zc likewise;   u = (xc / zc) fx + 0.5 W;   v = (yc / zc) fy + 0.5 H
    valid = zc > 0.2 and -0.15 W <= u <= 1.15 W and -0.15 H <= v <= 1.15 H
    d_i = min zc over the valid cameras, n_i their number, D = max d_i over n_i > 0, fmax = max fx
    filter_i = ((n_i > 0 ? d_i : D) / fmax) * sqrt(0.2);   zeros when nothing is seen
Only IEEE arithmetic, minimum and maximum: the device's result equals this one bit for bit.

Applying it (`apply`), with o = 1 / (1 + exp(-x)) and s = exp(l):
    q = s s;  f2 = f f;  v = q + f2;  s' = sqrt(v);  r = q / v;  t = f2 / v  (v == 0: r = 1, t = 0);  c = sqrt((r0 r1) r2);  o' = o c
and its chain rule (`backward`), with the forward's values:
    d_o = ((g_o c) o) (1 - o);     d_k = (g_k s'_k) r_k + (g_o o') t_k      (t_k == 0: the second term is not added)
Only exp differs between this file and the device (numpy's and the device library's expf are different functions, each within a
few ulp); `apply` and `backward` take the device's own o and s (what hs_activate wrote) in place of exp, and then everything is
IEEE arithmetic and comes out bit for bit.

With dtype=np.float64 the same functions evaluate the same formulas in float64.  As in tests/activation_reference.py the
float64 BACKWARD runs on the float32 values of the forward (o, s', r, t, c, o' -- its inputs: the kernel recomputes exactly
those bits): the bound is on the arithmetic of the conversion, not on the forward's error a second time.  (A float64 chain from
the stored logits would measure 1 - o at x = 17, where float32 has two bits left, and nothing else.)

The bounds, per element, in units of 2^-24 (`worst_c` of tests/activation_reference.py measures the constant c of each):
    scale             |s' - s'64|  <= c s'64                      (s' >= exp(l): never denormal on these inputs)
    opacity           |o' - o'64|  <= c o'64 + 2^-126             (o is denormal at x = -88, zero at x = -100)
    opacity gradient  |d_o - d_o64| <= c |d_o64| + 2^-126
    scale gradient    |d_k - d_k64| <= c (|g_k s'_k r_k| + |g_o o' t_k|)       the sum of its two terms
Each bar is twice the constant the float32 restatement shows against float64 on `inputs()` (10^6 seeded rows), rounded up to a
power of two: tests/test_smoothing.py::test_bars_are_twice_the_measured_constants measures them, holds the bars to that rule
and prints the constants of the machine it runs on (MEASURED below: what numpy gave when the bars were set); the GPU tests
import the bars.
"""
import numpy as np

from activation_reference import FLOOR, SPECIAL_LOGITS, UNIT, bar_of, same_bits, worst_c  # noqa: F401  (re-exported)

F = np.float32
NEAR = F(0.2)
LO, HI = F(-0.15), F(1.15)
SQRT_FIFTH = F(0.4472135901451111)          # sqrt(0.2) in float32
assert SQRT_FIFTH.view(np.uint32) == 0x3ee4f92e
CAM_CHUNK = 64                              # cameras the kernel stages at a time (smoothing.hip, kSmCamChunk)
ROWS = 1_000_000

MEASURED = dict(scale=4.27, opacity=8.84, opacity_grad=3.59, scale_grad=2.95)
BARS = dict(scale=16.0, opacity=32.0, opacity_grad=8.0, scale_grad=8.0)
# every constant depends on the host's expf: the forward's directly, the backward's through the forward values it starts from


def inputs(n=ROWS, seed=0):
    """The rows of the CPU measurement: logits N(0, 3) followed by SPECIAL_LOGITS, log scales U(-9, 3), filters e^U(-9, 1)
    with every 16th an exact zero, and upstream gradients N(0, 1) for both tensors (float32)."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([3.0 * rng.standard_normal(n), np.array(SPECIAL_LOGITS)]).astype(F)
    rows = x.shape[0]
    l = rng.uniform(-9.0, 3.0, size=(rows, 3)).astype(F)
    f = np.exp(rng.uniform(-9.0, 1.0, size=rows)).astype(F)
    f[::16] = 0.0
    g_o = rng.standard_normal(rows).astype(F)
    g_s = rng.standard_normal((rows, 3)).astype(F)
    return x, l, f, g_o, g_s


# ---- the filter ----

def filter_3d(xyz, views, intr):
    """(filter [P] float32, n_views [P] int32) of positions [P, 3], cameras [C, 16] (transposed convention) and intrinsics
    [C, 4] = (fx, fy, W, H), float32 operation for operation."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    views = np.asarray(views, F).reshape(-1, 16)
    intr = np.asarray(intr, F).reshape(-1, 4)
    P = xyz.shape[0]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    d = np.full(P, np.inf, F)
    n = np.zeros(P, np.int32)
    half = F(0.5)
    with np.errstate(all="ignore"):
        for m, (fx, fy, W, H) in zip(views, intr):
            xc = ((m[0] * x + m[4] * y) + m[8] * z) + m[12]
            yc = ((m[1] * x + m[5] * y) + m[9] * z) + m[13]
            zc = ((m[2] * x + m[6] * y) + m[10] * z) + m[14]
            u = (xc / zc) * fx + half * W
            v = (yc / zc) * fy + half * H
            valid = (zc > NEAR) & (u >= LO * W) & (u <= HI * W) & (v >= LO * H) & (v <= HI * H)
            d = np.where(valid & (zc < d), zc, d).astype(F)
            n += valid
        seen = n > 0
        if not seen.any():
            return np.zeros(P, F), n
        D = d[seen].max()
        fx = intr[:, 0]
        fmax = fx[~np.isnan(fx)].max() if (~np.isnan(fx)).any() else F(-np.inf)
        out = (np.where(seen, d, D).astype(F) / F(fmax)) * SQRT_FIFTH
    assert out.dtype == F
    return out, n


# ---- applying it ----

def _as(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype)


def apply(x, l, f, dtype=F, o=None, s=None):
    """The forward of rows (x [P], l [P, 3], f [P]): dict(o, s, sp, r, t, c, oc) -- sp = s', oc = o'.  `o` / `s`: activated
    values to use in place of 1 / (1 + exp(-x)) and exp(l) (the device's own, for the bit-for-bit comparison)."""
    one, zero = dtype(1.0), dtype(0.0)
    x, l, f = _as(x, dtype).reshape(-1), _as(l, dtype).reshape(-1, 3), _as(f, dtype).reshape(-1, 1)
    with np.errstate(all="ignore"):
        o = one / (one + np.exp(-x)) if o is None else _as(o, dtype).reshape(-1)
        s = np.exp(l) if s is None else _as(s, dtype).reshape(-1, 3)
        q = s * s
        f2 = f * f
        v = q + f2
        sp = np.sqrt(v)
        nz = v != zero
        r = np.where(nz, q / np.where(nz, v, one), one)
        t = np.where(nz, f2 / np.where(nz, v, one), zero)
        # (v is NaN: nz is true and the NaN propagates, as on the device)
        c = np.sqrt((r[:, 0] * r[:, 1]) * r[:, 2])
        oc = o * c
    out = dict(o=o, s=s, sp=sp, r=r, t=t, c=c, oc=oc)
    assert all(a.dtype == dtype for a in out.values())
    return out


def backward(g_o, g_s, fwd, dtype=F):
    """(d_o [P], d_s [P, 3]) from the gradients with respect to o' and s' and the forward's values `fwd` (what `apply`
    returned; float32 values stay what they are, whatever `dtype` evaluates in)."""
    one, zero = dtype(1.0), dtype(0.0)
    g_o, g_s = _as(g_o, dtype).reshape(-1), _as(g_s, dtype).reshape(-1, 3)
    o, c, oc = (_as(fwd[k], dtype) for k in ("o", "c", "oc"))
    sp, r, t = (_as(fwd[k], dtype) for k in ("sp", "r", "t"))
    with np.errstate(all="ignore"):
        d_o = ((g_o * c) * o) * (one - o)
        first = (g_s * sp) * r
        d_s = np.where(t == zero, first, first + (g_o * oc)[:, None] * t)
    assert d_o.dtype == dtype and d_s.dtype == dtype
    return d_o, d_s


def scale_grad_scale(g_o, g_s, fwd):
    """|g_k s'_k r_k| + |g_o o' t_k| per element, float64: what the scale gradient's error is measured in."""
    D = np.float64
    g_o, g_s = _as(g_o, D).reshape(-1), _as(g_s, D).reshape(-1, 3)
    return np.abs(g_s * _as(fwd["sp"], D) * _as(fwd["r"], D)) + np.abs((g_o * _as(fwd["oc"], D))[:, None] * _as(fwd["t"], D))


def forward_constants(x, l, f, got_o, got_s):
    """{quantity: c} of opacities `got_o` and scales `got_s` against float64 on the stored inputs."""
    ref = apply(x, l, f, np.float64)
    return dict(scale=worst_c(np.reshape(got_s, (-1, 3)), ref["sp"], ref["sp"]),
                opacity=worst_c(np.reshape(got_o, -1), ref["oc"], ref["oc"], FLOOR))


def backward_constants(g_o, g_s, fwd, got_o, got_s):
    """{quantity: c} of the stored-space gradients against the float64 chain rule on the float32 forward values `fwd`."""
    d_o, d_s = backward(g_o, g_s, fwd, np.float64)
    return dict(opacity_grad=worst_c(np.reshape(got_o, -1), d_o, np.abs(d_o), FLOOR),
                scale_grad=worst_c(np.reshape(got_s, (-1, 3)), d_s, scale_grad_scale(g_o, g_s, fwd)))
