"""numpy restatement of the activations of the stored cloud (include/hdrsplat.h, hs_activate / hs_activate_backward), operation
for operation, and the float64 evaluation of the same formulas the bounds are stated against.

Forward (`activate`), one correctly rounded operation per numpy ufunc call in float32:
    o  = 1 / (1 + exp(-x))
    s  = exp(l)
    n  = max(sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3), 1e-12);   q^ = q / n
Backward (`backward`), from the gradient g with respect to the activated value and the ACTIVATED values the forward wrote:
    (g o) (1 - o);   g s;   d = ((q^0 g0 + q^1 g1) + q^2 g2) + q^3 g3,  (g - q^ d) / n  with n from the stored q as above,
    and g / 1e-12 where the clamp was active (|q| < 1e-12)
With dtype=np.float64 the same functions evaluate the same formulas in float64 -- the backward on the SAME float32 activated
values, which are its inputs: the bound is on the arithmetic of the conversion, not on the forward's error a second time.

Only exp differs between this file and the device (numpy's and the device library's expf are different functions, each within
a few ulp): everything else is IEEE arithmetic and comes out bit for bit.

The bounds, per element, in units of 2^-24 (`worst_c` measures the constant c of each):
    sigmoid             |o - o64|   <= c o64 + 2^-126          (x = -100 gives 0 in float32; results below 2^-126 are denormal)
    exp                 |s - s64|   <= c s64
    normalise           |q^ - q^64| <= c
    sigmoid gradient    |g' - g'64| <= c |g'64| + 2^-126       (o may be denormal: so may the product)
    exp gradient        |g' - g'64| <= c |g'64|
    rotation gradient   |g' - g'64| <= c (|g| + |q^| sum_j |q^_j g_j|) / n     a cancellation bound: g - q^ d loses what g and
                                                                              q^ d share, so the error scales with the terms
(The 2^-126 in the sigmoid GRADIENT's bound is an addition to the plain relative bound the feature's specification states for
it: that specification's own rows x = +-88 make o -- and with it g o -- denormal, where a product carries an absolute rounding
error of up to 2^-150 and no relative bound can hold; for results larger than 2^-102 the floor is below one unit of the relative term.)
Each bar is twice the constant the float32 restatement shows against float64 on `inputs()` (10^6 seeded rows), rounded up to a
power of two: tests/test_raw_parameters.py::test_bars_are_twice_the_measured_constants measures them and holds the bars to
that rule and prints the constants of the machine it runs on (MEASURED below: what numpy gave when the bars were set); the
GPU tests import the bars.
"""
import math

import numpy as np

F = np.float32
EPS = F(1e-12)                       # torch.nn.functional.normalize's clamp, as float32: the kernels' 1e-12f
UNIT = 2.0 ** -24
FLOOR = 2.0 ** -126                  # smallest normal float32

MEASURED = dict(sigmoid=3.60, exp=3.40, normalise=2.51, sigmoid_grad=2.86, exp_grad=1.00, rotation_grad=4.40)
BARS = dict(sigmoid=8.0, exp=8.0, normalise=8.0, sigmoid_grad=8.0, exp_grad=2.0, rotation_grad=16.0)
USES_EXP = ("sigmoid", "exp")    # the constants that depend on the host's expf
SPECIAL_LOGITS = (17.0, -17.0, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0, 0.0)
ROWS = 1_000_000


def inputs(n=ROWS, seed=0):
    """The rows of the CPU measurement: logits N(0, 3) followed by SPECIAL_LOGITS, log scales U(-9, 3), quaternions
    N(0, 1) e^U(-3, 3), and upstream gradients N(0, 1) for each (float32)."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([3.0 * rng.standard_normal(n), np.array(SPECIAL_LOGITS)]).astype(F)
    l = rng.uniform(-9.0, 3.0, size=(n, 3)).astype(F)
    q = (rng.standard_normal((n, 4)) * np.exp(rng.uniform(-3.0, 3.0, size=(n, 1)))).astype(F)
    g = dict(opacities=rng.standard_normal(x.shape).astype(F), scales=rng.standard_normal(l.shape).astype(F),
             rotations=rng.standard_normal(q.shape).astype(F))
    return x, l, q, g


def _as(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype)


def quat_length(q, dtype=F):
    """sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3), [rows, 1]: the length before the clamp."""
    q = _as(q, dtype).reshape(-1, 4)
    return np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]


def activate(x=None, l=None, q=None, dtype=F):
    """(opacities, scales, rotations) of the stored (logits, log scales, quaternions); None stays None."""
    one = dtype(1.0)
    x, l = _as(x, dtype), _as(l, dtype)
    with np.errstate(over="ignore", under="ignore"):
        o = None if x is None else one / (one + np.exp(-x))
        s = None if l is None else np.exp(l)
    r = None
    if q is not None:
        shape = np.shape(q)
        n = np.maximum(quat_length(q, dtype), dtype(EPS))
        r = (_as(q, dtype).reshape(-1, 4) / n).reshape(shape)
    return o, s, r


def backward(g_o=None, o=None, g_s=None, s=None, g_q=None, qhat=None, q=None, dtype=F):
    """The gradients with respect to the stored values from those with respect to the activated ones; `o`, `s`, `qhat`
    are the activated values (float32, whatever `dtype` evaluates in), `q` the stored quaternions."""
    one = dtype(1.0)
    with np.errstate(under="ignore"):
        d_o = None if g_o is None else (_as(g_o, dtype) * _as(o, dtype)) * (one - _as(o, dtype))
        d_s = None if g_s is None else _as(g_s, dtype) * _as(s, dtype)
    d_q = None
    if g_q is not None:
        shape = np.shape(g_q)
        g, u = _as(g_q, dtype).reshape(-1, 4), _as(qhat, dtype).reshape(-1, 4)
        n = quat_length(q, dtype)
        d = (((u[:, 0] * g[:, 0] + u[:, 1] * g[:, 1]) + u[:, 2] * g[:, 2]) + u[:, 3] * g[:, 3])[:, None]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            d_q = np.where(n < dtype(EPS), g / dtype(EPS), (g - u * d) / n).reshape(shape)
    return d_o, d_s, d_q


def rotation_grad_scale(g_q, qhat, q):
    """(|g| + |q^| sum_j |q^_j g_j|) / n per element, float64: what the rotation gradient's error is measured in."""
    g, u = _as(g_q, np.float64).reshape(-1, 4), _as(qhat, np.float64).reshape(-1, 4)
    n = np.maximum(quat_length(q, np.float64), np.float64(EPS))
    return ((np.abs(g) + np.abs(u) * np.abs(u * g).sum(axis=1, keepdims=True)) / n).reshape(np.shape(g_q))


def worst_c(got, ref64, scale, floor=0.0):
    """The smallest c with |got - ref64| <= c 2^-24 scale + floor on every element (inf where that needs scale > 0 and it is
    not, or where `got` is not finite)."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    scale = np.broadcast_to(np.asarray(scale, np.float64), got.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return math.inf
    excess = np.maximum(np.abs(got - ref64) - floor, 0.0)
    if (excess[scale <= 0] > 0).any():
        return math.inf
    ok = scale > 0
    return float((excess[ok] / (UNIT * scale[ok])).max()) if ok.any() else 0.0


def forward_constants(x, l, q, got):
    """{quantity: c} of the activated tensors `got` = (o, s, q^) (any may be None) against float64 on the stored inputs."""
    o64, s64, r64 = activate(x, l, q, np.float64)
    c = {}
    if got[0] is not None:
        c["sigmoid"] = worst_c(got[0], o64, o64, FLOOR)
    if got[1] is not None:
        c["exp"] = worst_c(got[1], s64, s64)
    if got[2] is not None:
        c["normalise"] = worst_c(got[2], r64, 1.0)
    return c


def backward_constants(g, act, q, got):
    """{quantity: c} of the stored-space gradients `got` = (d_o, d_s, d_q) against the float64 chain rule applied to the
    activated-space gradients g = (g_o, g_s, g_q) and the float32 activated values act = (o, s, q^)."""
    d64 = backward(g[0], act[0], g[1], act[1], g[2], act[2], q, np.float64)
    c = {}
    if got[0] is not None:
        c["sigmoid_grad"] = worst_c(got[0], d64[0], np.abs(d64[0]), FLOOR)
    if got[1] is not None:
        c["exp_grad"] = worst_c(got[1], d64[1], np.abs(d64[1]))
    if got[2] is not None:
        c["rotation_grad"] = worst_c(got[2], d64[2], rotation_grad_scale(g[2], act[2], q))
    return c


def bar_of(c):
    """Twice the measured constant, rounded up to a power of two."""
    return 2.0 ** math.ceil(math.log2(2.0 * c))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
