"""numpy restatement of the densify / prune of the cloud (include/hdrsplat.h, hs_densify_plan / hs_densify_apply), row for
row: the reference the GPU tests hold densify.hip to -- bit for bit wherever no library function enters.

Plan (`plan`), per source row, float32, one correctly rounded operation per numpy ufunc call:
    g = grad_accum / denom, 0 where denom == 0 or the quotient is NaN;  sel = g >= tau_grad
    s = max of the stored scales by comparisons (s0; s1 if s1 > s; s2 if s2 > s);  big = s > tau_split
    prune(o, r, s) = o < o_min or (r_max > 0 and r > r_max) or (sigma on and s > sigma_max)
    not sel: survives iff not prune(o, r, s);  sel and not big: survives + clone iff not prune(o, r, s)
    sel and big: the row goes, two children iff not prune(o, r, child(s)), child(x) = x / 1.6 (raw: x - log(1.6) in float32)
Output order survivors | clones | children k = 0 | children k = 1, each in source order; row_map = kind << 30 | source.
Apply (`gather`, `child_means`): COPY, ZERO_NEW (zeros for every new row), SCALES (child(x) for children), MEANS
    (w, x, y, z) = q / sqrt(((w w + x x) + y y) + z z);  v_j = sigma_j * xi[source, k, j]
    mean_c = ((Rc0 v0 + Rc1 v1) + Rc2 v2) + mu_c   with upstream's build_rotation for R
`child_means(..., dtype=np.float64)` is the float64 evaluation the raw-scale bound is stated against.
"""
import math

import numpy as np

F = np.float32
LOG_1_6 = np.log(F(1.6))            # float32: bits 0x3ef0a452 (HS_DENSIFY_LOG_1_6)
assert LOG_1_6.dtype == np.float32 and LOG_1_6.view(np.uint32) == 0x3EF0A452
COPY, ZERO_NEW, MEANS, SCALES = 0, 1, 2, 3
SRC_MASK = (1 << 30) - 1
NAMES = ("means3D", "opacities", "shs", "scales", "rotations")
ROLES = dict(means3D=MEANS, opacities=COPY, shs=COPY, scales=SCALES, rotations=COPY)

# The cases of the GPU comparison and the raw-scale bound of their child means:
#     |hip - ref64| <= RAW_MEAN_BAR * 2^-24 * (|mu_c| + sum_j sigma_j |xi_j|)
# Measured on the CPU (tests/test_densify.py::test_raw_mean_bar_is_twice_the_measured_constant): the float32 restatement
# against the float64 evaluation over the eight raw-scale cases below has a worst c of 8.03 (P = 1 000 000, M = 1); twice that,
# rounded up to a power of two (device expf and the host's differ by an ulp or two), is 32.
RAW_MEAN_C_MEASURED = 8.03
RAW_MEAN_BAR = 32.0
SIZES = [(P, M) for P in (1, 10007, 262144, 1_000_000) for M in (1, 16)]


def case_seed(P, M):
    return P % 97 + M


def thresholds(extent, grad_threshold=2e-4, percent_dense=0.01, min_opacity=0.005, max_screen_size=None, raw_scales=True,
               raw_opacity=True):
    """Stored-space thresholds: converted in float64, rounded to float32 (what the front end puts into hs_densify_args)."""
    tau_split, sigma_max = percent_dense * extent, 0.1 * extent
    if raw_opacity:
        o_min = -math.inf if min_opacity <= 0 else (math.inf if min_opacity >= 1 else math.log(min_opacity / (1.0 - min_opacity)))
    else:
        o_min = min_opacity
    screen = int(max_screen_size) if max_screen_size else 0
    return dict(tau_grad=F(grad_threshold), tau_split=F(math.log(tau_split) if raw_scales else tau_split), o_min=F(o_min),
                sigma_max=F(math.inf if not screen else (math.log(sigma_max) if raw_scales else sigma_max)), r_max=screen,
                raw_scales=bool(raw_scales), raw_opacity=bool(raw_opacity))


def child_scale(x, raw):
    x = np.asarray(x, dtype=F)
    return x - LOG_1_6 if raw else x / F(1.6)


def plan(grad_accum, denom, max_radii, opacities, scales, th):
    """(codes uint8 [P], row_map uint32 [P_out], counts list of 8)."""
    P = grad_accum.shape[0]
    assert grad_accum.dtype == denom.dtype == opacities.dtype == scales.dtype == np.float32 and max_radii.dtype == np.int32
    scales = scales.reshape(P, 3)
    opacities = opacities.reshape(P)
    with np.errstate(all="ignore"):
        g = grad_accum / denom
        g = np.where((denom == 0) | np.isnan(g), F(0), g)
        sel = g >= th["tau_grad"]
        s = scales[:, 0].copy()
        s = np.where(scales[:, 1] > s, scales[:, 1], s)
        s = np.where(scales[:, 2] > s, scales[:, 2], s)
        split = sel & (s > th["tau_split"])
        st = np.where(split, child_scale(s, th["raw_scales"]), s)
        sigma_on = not (np.isposinf(th["sigma_max"]) or (not th["raw_scales"] and th["sigma_max"] == 0))
        prune = opacities < th["o_min"]
        if th["r_max"] > 0:
            prune |= max_radii > th["r_max"]
        if sigma_on:
            prune |= st > th["sigma_max"]
    codes = np.where(prune, 0, np.where(split, 3, np.where(sel, 2, 1))).astype(np.uint8)
    idx = np.arange(P, dtype=np.uint32)
    surv, clone, kept = idx[(codes == 1) | (codes == 2)], idx[codes == 2], idx[codes == 3]
    row_map = np.concatenate([surv, clone | np.uint32(1 << 30), kept | np.uint32(2 << 30), kept | np.uint32(3 << 30)]).astype(np.uint32)
    counts = [int(row_map.size), int(surv.size), int(clone.size), 2 * int(kept.size), P - int(surv.size) - int(kept.size),
              int(split.sum()), P, 0]
    return codes, row_map, counts


def rotation_rows(q, dtype=F):
    """The three rows of upstream's build_rotation of q / |q| ([n, 4] as w, x, y, z), each operation in `dtype`."""
    q = q.astype(dtype)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    with np.errstate(all="ignore"):
        n = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
        one, two = dtype(1), dtype(2)
        return ((one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)),
                (two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)),
                (two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)))


def child_means(means, scales, rotations, noise, src, k, raw_scales, dtype=F):
    """Means of child k[i] of source rows src[i]: [n, 3] in `dtype` (float32: the stated order, bit for bit the kernel's
    with stored-linear scales; float64: the evaluation the raw-scale bound refers to).  Also returns the bound's magnitude
    |mu_c| + sum_j sigma_j |xi_j| in float64."""
    sc = scales.reshape(-1, 3)[src].astype(dtype)
    with np.errstate(all="ignore"):
        sg = np.exp(sc) if raw_scales else sc
        xi = noise.reshape(-1, 2, 3)[src, k].astype(dtype)
        v = sg * xi
        R = rotation_rows(rotations.reshape(-1, 4)[src], dtype)
        mu = means.reshape(-1, 3)[src].astype(dtype)
        out = np.stack([((R[c][0] * v[:, 0] + R[c][1] * v[:, 1]) + R[c][2] * v[:, 2]) + mu[:, c] for c in range(3)], axis=1)
        assert out.dtype == dtype
        s64 = np.exp(scales.reshape(-1, 3)[src].astype(np.float64)) if raw_scales else scales.reshape(-1, 3)[src].astype(np.float64)
        mag = np.abs(means.reshape(-1, 3)[src].astype(np.float64)) + \
            (s64 * np.abs(noise.reshape(-1, 2, 3)[src, k].astype(np.float64))).sum(axis=1, keepdims=True)
    return out, mag


def gather(src_array, row_map, role, raw_scales=False, cloud=None, noise=None):
    """Output rows of one matrix ([P, ...] -> [P_out, ...]).  `cloud` (means3D / scales / rotations) and `noise`: MEANS only."""
    src = (row_map & np.uint32(SRC_MASK)).astype(np.int64)
    kind = (row_map >> np.uint32(30)).astype(np.int64)
    out = src_array[src].copy()
    if role == ZERO_NEW:
        out[kind != 0] = 0
    elif role == SCALES:
        ch = kind >= 2
        out[ch] = child_scale(out[ch], raw_scales)
    elif role == MEANS:
        ch = kind >= 2
        m, _ = child_means(src_array, cloud["scales"], cloud["rotations"], noise, src[ch], kind[ch] - 2, raw_scales)
        out[ch] = m.reshape(out[ch].shape)
    return out


def densify(case, th):
    """The whole operation on a case of `make_case`: (new cloud dict, new moments dict name -> (m, v), row_map, counts)."""
    c = case["cloud"]
    _, row_map, counts = plan(case["grad_accum"], case["denom"], case["max_radii"], c["opacities"], c["scales"], th)
    new = {k: gather(c[k], row_map, ROLES[k], th["raw_scales"], c, case["noise"]) for k in NAMES}
    mom = {k: tuple(gather(x, row_map, ZERO_NEW) for x in case["moments"][k]) for k in NAMES}
    return new, mom, row_map, counts


def raw_mean_c(case, th, row_map):
    """Worst c of |float32 restatement - float64 evaluation| <= c 2^-24 (|mu_c| + sum_j sigma_j |xi_j|) over the child means
    of a case (0.0 when it has no children)."""
    src = (row_map & np.uint32(SRC_MASK)).astype(np.int64)
    kind = (row_map >> np.uint32(30)).astype(np.int64)
    ch = kind >= 2
    if not ch.any():
        return 0.0
    c = case["cloud"]
    m32, mag = child_means(c["means3D"], c["scales"], c["rotations"], case["noise"], src[ch], kind[ch] - 2, th["raw_scales"])
    m64, _ = child_means(c["means3D"], c["scales"], c["rotations"], case["noise"], src[ch], kind[ch] - 2, th["raw_scales"], np.float64)
    return float((np.abs(m32.astype(np.float64) - m64) / (2.0 ** -24 * mag)).max())


def same_bits(a, b):
    """Bitwise equality of two float32 arrays, NaN payloads aside (NaN where the other has NaN)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    eq = a.view(np.uint32) == b.view(np.uint32)
    return bool(np.all(eq | (np.isnan(a) & np.isnan(b))))


def make_case(P, M, seed=0, raw_scales=True, raw_opacity=True):
    """A cloud of P Gaussians with M SH coefficients, random non-zero moments, statistics with denom == 0 (3 % of the rows)
    and NaN (1 %), the noise, and policy parameters (`policy`: the keyword arguments of densify_and_prune / thresholds)
    placed at quantiles of the data: about 10 % of the rows are cloned, 5 % split, 5 % pruned."""
    rng = np.random.default_rng(seed)
    n = max(P, 1)
    log_s = (math.log(0.02) + 0.7 * rng.standard_normal((n, 3))).astype(F)
    logit_o = (2.0 * rng.standard_normal((n, 1))).astype(F)
    sig, opa = np.exp(log_s.astype(np.float64)), 1.0 / (1.0 + np.exp(-logit_o.astype(np.float64)))
    cloud = dict(means3D=rng.standard_normal((n, 3)).astype(F), opacities=logit_o if raw_opacity else opa.astype(F),
                 shs=rng.standard_normal((n, M, 3)).astype(F), scales=log_s if raw_scales else sig.astype(F),
                 rotations=(rng.standard_normal((n, 4)) * 10.0 ** rng.uniform(-1, 1, (n, 1))).astype(F))
    moments = {k: ((0.1 * rng.standard_normal(v.shape)).astype(F), (0.01 * rng.random(v.shape) + 1e-6).astype(F)) for k, v in cloud.items()}
    denom = rng.integers(1, 30, n).astype(F)
    grad_accum = (denom * 2e-4 * np.exp(rng.standard_normal(n))).astype(F)
    u = rng.random(n)
    denom[u < 0.03] = 0.0                      # never rasterized: 0 / 0 below, x / 0 here
    grad_accum[u < 0.015] = 0.0
    grad_accum[(u >= 0.03) & (u < 0.04)] = np.nan
    max_radii = rng.integers(0, 100, n).astype(np.int32)
    with np.errstate(all="ignore"):
        g = grad_accum / denom
    g = np.where((denom == 0) | np.isnan(g), 0.0, g)
    smax = sig.max(axis=1)
    extent = float(10.0 * np.quantile(smax, 0.995))
    policy = dict(extent=extent, grad_threshold=float(np.quantile(g, 0.85)), percent_dense=float(np.quantile(smax, 0.667)) / extent,
                  min_opacity=float(np.quantile(opa, 0.04)), max_screen_size=98, raw_scales=raw_scales, raw_opacity=raw_opacity)
    cut = lambda x: x[:P]                      # noqa: E731  (P = 0: empty arrays of the right widths)
    return dict(P=P, M=M, cloud={k: cut(v) for k, v in cloud.items()}, moments={k: (cut(a), cut(b)) for k, (a, b) in moments.items()},
                grad_accum=cut(grad_accum), denom=cut(denom), max_radii=cut(max_radii),
                noise=rng.standard_normal((n, 2, 3)).astype(F)[:P], policy=policy)
