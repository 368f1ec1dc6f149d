"""numpy fp32 restatement of the fused Adam step (include/hdrsplat.h, hs_adam_step), element for element: the bit-level
reference the GPU tests hold adam.hip to.

Per call (`tick`): t += 1; per group the RUNNING PRODUCTS B1 *= beta1, B2 *= beta2 in fp64 (1 before the first step), then
    step_size = float32(lr / (1 - B1)),  bc2 = float32(sqrt(1 - B2)),  b1 = float32(beta1), b2 = float32(beta2),
    omb1 = float32(1 - beta1), omb2 = float32(1 - beta2) (the difference in fp64, rounded once), e = float32(eps)
Per element (`update`), every operation one correctly rounded fp32 operation (numpy's + - * / sqrt on float32 arrays are;
separate ufunc calls cannot contract), in this order:
    m' = b1 * m + omb1 * g
    v' = b2 * v + (omb2 * g) * g
    d  = sqrt(v') / bc2 + e
    p' = p - step_size * (m' / d)
Sparse rule: rows that are not visible keep param, exp_avg and exp_avg_sq untouched.
"""
import math

import numpy as np

F = np.float32


class Derived:
    __slots__ = ("step_size", "bc2", "b1", "b2", "omb1", "omb2", "eps")


class AdamReference:
    """State of one optimizer: the step count and, per group, the fp64 running products."""

    def __init__(self, n_groups, t=0, B1=None, B2=None):
        self.t = t
        self.B1 = list(B1) if B1 is not None else [1.0] * n_groups
        self.B2 = list(B2) if B2 is not None else [1.0] * n_groups

    def tick(self, hyper):
        """hyper: one (lr, beta1, beta2, eps) of Python floats per group.  Advances the state, returns one Derived per group."""
        first = self.t == 0
        self.t += 1
        out = []
        for i, (lr, beta1, beta2, eps) in enumerate(hyper):
            self.B1[i] = (1.0 if first else self.B1[i]) * beta1
            self.B2[i] = (1.0 if first else self.B2[i]) * beta2
            d = Derived()
            d.step_size = F(lr / (1.0 - self.B1[i]))
            d.bc2 = F(math.sqrt(1.0 - self.B2[i]))
            d.b1, d.b2 = F(beta1), F(beta2)
            d.omb1, d.omb2 = F(1.0 - beta1), F(1.0 - beta2)
            d.eps = F(eps)
            out.append(d)
        return out


def update(p, g, m, v, d, visible=None):
    """In place on float32 arrays of one shape ([rows, ...]); `visible`: bool [rows] or None (dense)."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32
    with np.errstate(all="ignore"):
        if visible is None:
            idx = slice(None)
        else:
            idx = np.asarray(visible, dtype=bool)
        gg, mm, vv, pp = g[idx], m[idx], v[idx], p[idx]
        m1 = d.b1 * mm + d.omb1 * gg
        v1 = d.b2 * vv + (d.omb2 * gg) * gg
        den = np.sqrt(v1) / d.bc2 + d.eps
        p1 = pp - d.step_size * (m1 / den)
        assert m1.dtype == v1.dtype == den.dtype == p1.dtype == np.float32
        m[idx], v[idx], p[idx] = m1, v1, p1


def same_bits(a, b):
    """Bitwise equality of two float32 arrays, NaN payloads aside (NaN where the other has NaN)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    eq = a.view(np.uint32) == b.view(np.uint32)
    return bool(np.all(eq | (np.isnan(a) & np.isnan(b))))


def pinned_case(seed=0, rows=20000, cols=48, steps=50):
    """The 50-step closeness case: parameters, and per step gradients spanning 1e-8 .. 1 in scale with 5 % exact zeros."""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal((rows, cols)).astype(np.float32)
    scale = 10.0 ** rng.uniform(-8.0, 0.0, size=(rows, cols))
    grads = []
    for _ in range(steps):
        g = (scale * rng.standard_normal((rows, cols))).astype(np.float32)
        g[rng.random((rows, cols)) < 0.05] = 0.0
        grads.append(g)
    return p0, grads


PINNED_HYPER = (1e-2, 0.9, 0.999, 1e-15)     # eps: upstream's
