"""numpy restatement of hs_mcmc_regularize (include/hdrsplat.h, mcmc_reg.hip) in float32 -- one ufunc per operation, numpy's
exp standing in for expf -- and in float64, plus the cases the CPU and GPU tests share.

    ko = (float)(lambda_o / P),  ks = (float)(lambda_s / (3 P))
    raw opacities:   o = 1 / (1 + exp(-x));  g <- g + ko * ((1 - o) * o)        stored linear:  g <- g + ko * sign(x)
    raw scales:      s = exp(x);             g <- g + ks * s                    stored linear:  g <- g + ks * sign(x)
    loss = {(float)(lambda_o * (sum o / P)), (float)(lambda_s * (sum s / (3 P)))}   the elements o, s (|x| when stored linear)
                                                                                  converted to double and added in double

The comparison every test makes (`check`):  |value - float64| <= bar * (2^-24 * mag + 2^-149), with
    mag = |g_old| + (lambda_o / P) * o       opacities        (stored linear: |g_old| + (lambda_o / P) * |sign x|, the size of
    mag = |g_old| + (lambda_s / 3 P) * s     scales            the two addends: the added term does not shrink with |x|)
    mag = the term itself                    loss
2^-149, the smallest float32 step, is the absolute error a result in the subnormal range carries instead of a relative one
(x = -104: the float64 sigmoid is 7e-46, float32 has no such number and gives 0).  Two rules about the float32 RANGE, since
the float64 evaluation does not overflow where float32 does: an activated scale exp(x) beyond the largest float32 is the
infinity the arithmetic above -- and the rasterizer -- see (x = 104), and a float64 result beyond the largest float32 is that
infinity.  Where the float64 value is infinite or NaN the value under test must be the same infinity / a NaN: no row is left
out of the comparison.
"""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -149
FLT_MAX = float(np.finfo(np.float32).max)
RAW_OPACITY, RAW_SCALES = 1, 2

# The cases of the GPU comparison
SIZES = [1, 257, 10007, 262144]
LAMBDA_O, LAMBDA_S = 0.01, 0.01          # the publication's defaults
# The constant of the bound, measured on the CPU (tests/test_mcmc_regularize.py::test_reg_bar_is_twice_the_measured_constant):
# worst c of the float32 restatement against the float64 evaluation over SIZES x {raw, stored linear} x {with, without the
# special rows}, gradients and loss terms: 4.23 (the raw opacities' gradient at P = 262 144: numpy's float32 exp, then the
# roundings of 1 + e, of the quotient, of 1 - o against o, of the product, of ko and of the sum; the raw scales reach 3.53,
# the stored-linear forms 1.31, the loss terms 1.32).  The bar is twice that, rounded up to a power of two: device expf and
# numpy's exp may differ by an ulp or two.
REG_C_MEASURED = 4.23
REG_BAR = 16.0

SPECIALS = [0.0, -0.0, 88.0, -88.0, 104.0, -104.0, math.inf, -math.inf, math.nan]


def case_seed(P):
    return P % 97 + 5


def make_case(P, seed=None, special=True):
    """dict(P, opacities [P, 1], scales [P, 3], g_o [P, 1], g_s [P, 3]) in float32: logits uniform in [-12, 12], log-scales
    in [-10, 3]; with `special` (and P >= 257) rows 1..9 of the opacities and rows 11..19 of the scales (one column each, in
    turn) hold SPECIALS.  The incoming gradient is normal around 1e-4 with zeros, -0.0 and (P >= 257) three NaN rows."""
    rng = np.random.default_rng(case_seed(P) if seed is None else seed)
    o = rng.uniform(-12.0, 12.0, (P, 1)).astype(F)
    s = rng.uniform(-10.0, 3.0, (P, 3)).astype(F)
    g_o = (1e-4 * rng.standard_normal((P, 1))).astype(F)
    g_s = (1e-4 * rng.standard_normal((P, 3))).astype(F)
    if P >= 257:
        if special:
            for k, v in enumerate(SPECIALS):
                o[1 + k, 0] = v
                s[11 + k, k % 3] = v
            s[20] = [math.inf, -88.0, math.nan]
        for g in (g_o, g_s):
            g[2::7] = 0.0
            g[5::11] = -0.0
            g[21:24] = math.nan
        g_o[3], g_s[13, 1] = 0.0, 0.0        # a zero and a -0.0 gradient on special rows too
        g_o[4], g_s[14, 2] = -0.0, -0.0
    return dict(P=P, opacities=o, scales=s, g_o=g_o, g_s=g_s)


def _sign(x):
    with np.errstate(all="ignore"):
        return np.where(np.isnan(x), x, (x > 0).astype(x.dtype) - (x < 0).astype(x.dtype))


def regularize(case, lam_o=LAMBDA_O, lam_s=LAMBDA_S, flags=RAW_OPACITY | RAW_SCALES, dtype=F):
    """The header's arithmetic in `dtype` (float32: the restatement, one rounding per operation; float64: the truth, with the
    weights lambda / P unrounded).  Returns dict(g_o, g_s, loss [2], mag_o, mag_s, mag_loss [2]); a gradient whose lambda is 0
    is returned as it came.  The loss of an empty cloud is {0, 0}."""
    P = case["P"]
    f32 = dtype == F
    out = {}
    with np.errstate(all="ignore"):
        for key, gkey, lam, n, raw in (("opacities", "g_o", lam_o, P, flags & RAW_OPACITY), ("scales", "g_s", lam_s, 3 * P, flags & RAW_SCALES)):
            x = case[key].astype(dtype)
            g = case[gkey].astype(dtype)
            k64 = lam / n if n else 0.0
            k = F(k64) if f32 else k64
            if key == "opacities" and raw:
                o = dtype(1) / (dtype(1) + np.exp(-x))
                term, elem, size = (dtype(1) - o) * o, o, o
            elif raw:
                e = np.exp(x)
                if not f32:
                    e = np.where(e > FLT_MAX, np.inf, e)       # the float32 range of the activated scale (module docstring)
                term, elem, size = e, e, e
            else:
                sg = _sign(x)
                term, elem, size = sg, np.abs(x), np.abs(sg)
            new = g + k * term if lam != 0.0 else g
            if not f32:
                new = np.where(np.abs(new) > FLT_MAX, np.copysign(np.inf, new), new)
            S = float(np.sum(elem.astype(np.float64).reshape(-1))) if n else 0.0
            loss64 = lam * (S / n) if n else 0.0
            short = "o" if key == "opacities" else "s"
            out["g_" + short] = new
            out["mag_" + short] = np.abs(case[gkey].astype(np.float64)) + k64 * size.astype(np.float64)
            out["loss_" + short] = F(loss64) if f32 else (math.copysign(math.inf, loss64) if abs(loss64) > FLT_MAX else loss64)
    out["loss"] = np.array([out.pop("loss_o"), out.pop("loss_s")], dtype=dtype)
    out["mag_loss"] = np.abs(out["loss"].astype(np.float64))
    return out


def check(value, ref64, mag, bar, what):
    """Hold `value` (float32) to the float64 `ref64` on the module's bound; returns the worst c = |value - ref64| / (2^-24 mag +
    2^-149) over the finite elements.  Raises AssertionError naming the first element that misses."""
    v = np.asarray(value, dtype=np.float64).reshape(-1)
    r = np.asarray(ref64, dtype=np.float64).reshape(-1)
    m = np.asarray(mag, dtype=np.float64).reshape(-1)
    assert v.shape == r.shape == m.shape, (what, v.shape, r.shape, m.shape)
    nan, inf = np.isnan(r), np.isinf(r)
    bad = nan != np.isnan(v)
    assert not bad.any(), f"{what}: NaN where the reference has none, or the reverse: first at {int(np.nonzero(bad)[0][0])}"
    bad = inf & (v != r)
    assert not bad.any(), f"{what}: the reference is infinite, the value is not that infinity: first at {int(np.nonzero(bad)[0][0])}"
    fin = ~nan & ~inf
    with np.errstate(all="ignore"):
        c = np.abs(v[fin] - r[fin]) / (U * m[fin] + TINY)
    worst = float(c.max()) if c.size else 0.0
    if not worst <= bar:
        i = int(np.nonzero(fin)[0][int(np.argmax(c))])
        raise AssertionError(f"{what}: c = {worst:.3f} beyond the bar {bar} at element {i}: {v[i]!r} against float64 {r[i]!r}, mag {m[i]!r}")
    return worst


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
