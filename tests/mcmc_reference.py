"""numpy restatement of the MCMC refinement of the cloud (include/hdrsplat.h, hs_mcmc_sample / hs_mcmc_update /
hs_mcmc_noise), row for row: the reference the GPU tests hold mcmc.hip to.

Sampling (`sample`): dead = not (o > o_min) on the stored value; the weight is the integer rint(2^24 sigmoid(o)) with exp in
float64 (0 for NaN, and for dead rows of a relocation); prefix sums and S are exact integers; a draw is (u S) >> 64 with
Python ints and the first row whose inclusive prefix exceeds it.  These are compared BIT FOR BIT (the fixture keeps every
weight away from a rounding boundary, `nudge`, so that a last-bit difference of exp cannot move one).
Correction of a source (`correction`): float64 throughout, in the header's loop order; compared within one float32 ulp.
Noise (`noise`): the header's order of operations in float32 (numpy exp stands in for expf) or float64; compared within
    |hip - ref64| <= NOISE_BAR 2^-24 (|mu_c| + sum_ij |Sigma_ij| |v_j|),   Sigma = R diag(s^2) R^T,  v = xi g scaler
"""
import math

import numpy as np

import densify_reference as DR

F = np.float32
NAMES = DR.NAMES
CLONE = 1 << 30
RELOCATE, GROW = 0, 1
N_MAX = 51
ONE_MINUS_EPS = 1.0 - 2.0 ** -23

# The cases of the GPU comparison: (P, M)
SIZES = [(1, 1), (1, 16), (257, 1), (257, 16), (10007, 1), (262144, 1)]
# The constant of the noise bound, measured on the CPU (tests/test_mcmc.py::test_noise_bar_is_twice_the_measured_constant):
# worst c of the float32 restatement against the float64 evaluation over the cases above, raw and stored-linear (29.63 at
# P = 262 144, raw); the bar is twice that, rounded
# up to a power of two (device expf and numpy's exp differ by an ulp or two, and the gate multiplies that by up to 100).
NOISE_C_MEASURED = 29.63
NOISE_BAR = 64.0
NOISE_SCALER = 80.0          # lr_xyz 1.6e-4 x noise_lr 5e5


def case_seed(P, M):
    return P % 89 + M


def stored_o_min(min_opacity, raw_opacity):
    if raw_opacity:
        o = -math.inf if min_opacity <= 0 else (math.inf if min_opacity >= 1 else math.log(min_opacity / (1.0 - min_opacity)))
    else:
        o = min_opacity
    return F(o)


def sigmoid64(x):
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def real_weights(opacities, raw_opacity):
    """2^24 sigmoid(o) before rounding, float64 (0 for NaN)."""
    o = np.asarray(opacities, dtype=F).reshape(-1)
    s = sigmoid64(o) if raw_opacity else np.minimum(np.maximum(o.astype(np.float64), 0.0), 1.0)
    return np.where(np.isnan(o), 0.0, 16777216.0 * s)


def nudge(opacities, raw_opacity, margin=2.0 ** -16):
    """Move every opacity whose real weight lies within `margin` of a rounding boundary (k + 1/2) to the next float, until
    none does.  Returns (opacities, rows moved)."""
    o = np.array(opacities, dtype=F).reshape(-1)
    moved = np.zeros(o.shape, dtype=bool)
    for _ in range(8):
        w = real_weights(o, raw_opacity)
        near = np.abs((w - np.floor(w)) - 0.5) < margin
        if not near.any():
            break
        o[near] = np.nextafter(o[near], F(np.inf))
        moved |= near
    else:
        raise AssertionError("nudge did not settle")
    return o.reshape(np.shape(opacities)), int(moved.sum())


def sample(opacities, u, o_min, raw_opacity, mode, n_draws=None):
    """dict(dead bool [P], w uint64 [P], S int, sources int32 [n_draws], cnt uint32 [P], counts list of 8, row_map or None)."""
    o = np.asarray(opacities, dtype=F).reshape(-1)
    P = o.size
    with np.errstate(all="ignore"):
        dead = ~(o > o_min)
    w = np.rint(real_weights(o, raw_opacity)).astype(np.uint64)
    if mode == RELOCATE:
        w[dead] = 0
        n_draws = P
    C = np.cumsum(w, dtype=np.uint64)
    S = int(C[-1]) if P else 0
    assert S == sum(int(x) for x in w) and S < 1 << 54
    uu = np.asarray(u, dtype=np.int64).view(np.uint64)
    rows = np.nonzero(dead)[0] if mode == RELOCATE else np.arange(n_draws)
    sources = np.full(n_draws, -1, dtype=np.int32)
    cnt = np.zeros(P, dtype=np.uint32)
    if S > 0 and rows.size:
        t = np.array([(int(uu[k]) * S) >> 64 for k in rows], dtype=np.uint64)
        src = np.searchsorted(C, t, side="right")                  # first i with C_i > t
        assert (w[src] > 0).all()
        sources[rows] = src
        cnt = np.bincount(src, minlength=P).astype(np.uint32)
    draws = int((sources >= 0).sum())
    counts = [P, int(dead.sum()), draws, int((cnt > 0).sum()), 1 if S == 0 else 0, 0, 0, 0]
    row_map = None
    if mode == GROW:
        new = np.where(sources >= 0, sources, np.arange(n_draws) % max(P, 1)).astype(np.uint32)
        row_map = np.concatenate([np.arange(P, dtype=np.uint32), new | np.uint32(CLONE)])
    return dict(dead=dead, w=w, S=S, sources=sources, cnt=cnt, counts=counts, row_map=row_map)


def D_sum(x, r):
    """D = sum_{n = 1..r} sum_{k = 0..n-1} C(n-1, k) (-1)^k x^(k+1) / sqrt(k + 1) in the header's loop order (x^(k+1) a running
    product, the binomials exact), float64, for an array x and one r; and the sum of the terms' magnitudes."""
    x = np.asarray(x, dtype=np.float64)
    D, A = np.zeros(x.shape), np.zeros(x.shape)
    for n in range(1, int(r) + 1):
        b, xp, sg = 1.0, x.copy(), 1.0
        for k in range(n):
            assert b == math.comb(n - 1, k)
            term = ((b * sg) * xp) / math.sqrt(k + 1)
            D = D + term
            A = A + np.abs(term)
            b = (b * (n - 1 - k)) / (k + 1)
            xp = xp * x
            sg = -sg
    return D, A


def factor(o, x, r, with_cond=False):
    """The scale factor o / D(x) of one row (and the condition sum|term| / |sum| of D)."""
    with np.errstate(all="ignore"):
        D, A = D_sum(np.float64(x), r)
        return (float(o / D), float(A / abs(D))) if with_cond else float(o / D)


def correction(opacities, scales, cnt, min_opacity, raw_opacity, raw_scales):
    """The update of every row with cnt >= 1, float64: (new stored opacities [P] float64, new stored scales [P, 3] float64,
    condition sum|term| / |sum| of D [P]); rows with cnt == 0 carry their old values (cond 0)."""
    o_st = np.asarray(opacities, dtype=F).reshape(-1).astype(np.float64)
    s_st = np.asarray(scales, dtype=F).reshape(-1, 3).astype(np.float64)
    new_o, new_s, cond = o_st.copy(), s_st.copy(), np.zeros(o_st.size)
    ratio = np.minimum(cnt.astype(np.int64) + 1, N_MAX)
    with np.errstate(all="ignore"):
        for r in np.unique(ratio[cnt > 0]):
            idx = np.nonzero((cnt > 0) & (ratio == r))[0]
            o = sigmoid64(o_st[idx]) if raw_opacity else o_st[idx]
            x = 1.0 - np.power(1.0 - o, 1.0 / float(r))
            D, A = D_sum(x, r)
            xc = np.minimum(np.maximum(x, min_opacity), ONE_MINUS_EPS)
            new_o[idx] = np.log(xc / (1.0 - xc)) if raw_opacity else xc
            f = o / D
            new_s[idx] = s_st[idx] + np.log(f)[:, None] if raw_scales else s_st[idx] * f[:, None]
            cond[idx] = A / np.abs(D)
    return new_o, new_s, cond


def relocate(case, u, min_opacity):
    """The whole relocation on a case: (new cloud, new moments, the sample dict, float64 opacities / scales of the update)."""
    raw_o, raw_s = case["raw_opacity"], case["raw_scales"]
    c = case["cloud"]
    smp = sample(c["opacities"], u, stored_o_min(min_opacity, raw_o), raw_o, RELOCATE)
    o64, s64, _ = correction(c["opacities"], c["scales"], smp["cnt"], min_opacity, raw_o, raw_s)
    new = {k: v.copy() for k, v in c.items()}
    upd = smp["cnt"] > 0
    new["opacities"].reshape(-1)[upd] = o64[upd].astype(F)
    new["scales"].reshape(-1, 3)[upd] = s64[upd].astype(F)
    dead = smp["sources"] >= 0
    for k in NAMES:
        new[k][dead] = new[k][smp["sources"][dead]]
    mom = {k: tuple(m.copy() for m in case["moments"][k]) for k in NAMES}
    for k in NAMES:
        for m in mom[k]:
            m[upd] = 0
    return new, mom, smp, (o64, s64)


def grow(case, u, n_new, min_opacity):
    """(new cloud [P + n_new], new moments, the sample dict, float64 opacities / scales of the update)."""
    raw_o, raw_s = case["raw_opacity"], case["raw_scales"]
    c = case["cloud"]
    smp = sample(c["opacities"], u, stored_o_min(min_opacity, raw_o), raw_o, GROW, n_new)
    o64, s64, _ = correction(c["opacities"], c["scales"], smp["cnt"], min_opacity, raw_o, raw_s)
    upd = smp["cnt"] > 0
    cur = {k: v.copy() for k, v in c.items()}
    cur["opacities"].reshape(-1)[upd] = o64[upd].astype(F)
    cur["scales"].reshape(-1, 3)[upd] = s64[upd].astype(F)
    new = {k: DR.gather(cur[k], smp["row_map"], DR.COPY) for k in NAMES}
    mom = {k: tuple(DR.gather(m, smp["row_map"], DR.ZERO_NEW) for m in case["moments"][k]) for k in NAMES}
    return new, mom, smp, (o64, s64)


def noise(means, opacities, scales, rotations, xi, scaler, raw_opacity, raw_scales, dtype=F):
    """means' [P, 3] in `dtype` in the header's order of operations, gs [P] in `dtype`, and the bound's magnitude
    |mu_c| + sum_ij |Sigma_ij| |v_j| in float64 (from the float64 evaluation's own gate)."""
    T = dtype
    P = means.reshape(-1, 3).shape[0]
    with np.errstate(all="ignore"):
        o = opacities.reshape(P).astype(T)
        if raw_opacity:
            o = T(1) / (T(1) + np.exp(-o))
        t = (T(1) - o) - T(F(0.995))
        g = T(1) / (T(1) + np.exp(T(-100) * t))
        gs = g * T(F(scaler))
        s = scales.reshape(P, 3).astype(T)
        if raw_scales:
            s = np.exp(s)
        v = xi.reshape(P, 3).astype(T) * gs[:, None]
        R = DR.rotation_rows(rotations.reshape(P, 4), T)
        b = [(s[:, j] * s[:, j]) * ((R[0][j] * v[:, 0] + R[1][j] * v[:, 1]) + R[2][j] * v[:, 2]) for j in range(3)]
        mu = means.reshape(P, 3).astype(T)
        out = np.stack([((R[c][0] * b[0] + R[c][1] * b[1]) + R[c][2] * b[2]) + mu[:, c] for c in range(3)], axis=1)
        assert out.dtype == T and gs.dtype == T
        out = np.where((gs == 0)[:, None], mu, out)
        # magnitude, float64
        R64 = DR.rotation_rows(rotations.reshape(P, 4), np.float64)
        s64 = np.exp(scales.reshape(P, 3).astype(np.float64)) if raw_scales else scales.reshape(P, 3).astype(np.float64)
        o64 = sigmoid64(opacities.reshape(P)) if raw_opacity else opacities.reshape(P).astype(np.float64)
        g64 = 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - o64) - float(F(0.995)))))
        v64 = np.abs(xi.reshape(P, 3).astype(np.float64) * (g64 * float(F(scaler)))[:, None])
        Rm = np.stack([np.stack(R64[c], axis=1) for c in range(3)], axis=1)            # [P, 3, 3]
        Sig = np.einsum("pik,pk,pjk->pij", Rm, s64 * s64, Rm)
        mag = np.abs(means.reshape(P, 3).astype(np.float64)) + np.einsum("pij,pj->p", np.abs(Sig), v64)[:, None]
    return out, gs, mag


def noise_c(case, xi, scaler=NOISE_SCALER):
    """Worst c of |float32 restatement - float64 evaluation| <= c 2^-24 mag over a case's rows (NaN rows aside)."""
    c = case["cloud"]
    args = (c["means3D"], c["opacities"], c["scales"], c["rotations"], xi, scaler, case["raw_opacity"], case["raw_scales"])
    a32, _, mag = noise(*args)
    a64, _, _ = noise(*args, dtype=np.float64)
    ok = ~np.isnan(a64).any(axis=1)
    return float((np.abs(a32.astype(np.float64) - a64)[ok] / (2.0 ** -24 * mag[ok])).max()) if ok.any() else 0.0


def make_case(P, M, seed=0, raw=True, dead_frac=0.05, min_opacity=0.005, nan=True):
    """A cloud of P Gaussians with M SH coefficients and random non-zero moments: about `dead_frac` of the rows at or below
    `min_opacity`, 1 % NaN opacities (`nan`, from 100 rows on), a few rows at 1 - 2^-20, every weight at least 2^-16 away from a rounding boundary."""
    rng = np.random.default_rng(seed)
    n = max(P, 1)
    logit_o = (1.0 + 2.0 * rng.standard_normal(n))
    logit_o = np.maximum(logit_o, -5.0)                                   # alive: sigmoid(-5) = 0.0067 > 0.005
    r = rng.random(n)
    logit_o[r < dead_frac] = rng.uniform(-9.0, -5.4, n)[r < dead_frac]     # dead: sigmoid(-5.4) = 0.0045
    logit_o[(r >= dead_frac) & (r < dead_frac + 0.002)] = math.log((1 - 2.0 ** -20) / 2.0 ** -20)
    stored = logit_o.astype(F) if raw else sigmoid64(logit_o).astype(F)
    if nan and P > 100:
        stored[(r >= 0.5) & (r < 0.51)] = np.nan
    # (stored-linear opacities: the weight is rint(2^24 o), exact in float64 with no library function: nothing to keep apart)
    stored, moved = nudge(stored, raw) if raw else (stored, 0)
    log_s = (math.log(0.02) + 0.7 * rng.standard_normal((n, 3))).astype(F)
    cloud = dict(means3D=rng.standard_normal((n, 3)).astype(F), opacities=stored.reshape(n, 1),
                 shs=rng.standard_normal((n, M, 3)).astype(F), scales=log_s if raw else np.exp(log_s.astype(np.float64)).astype(F),
                 rotations=(rng.standard_normal((n, 4)) * 10.0 ** rng.uniform(-1, 1, (n, 1))).astype(F))
    moments = {k: ((0.1 * rng.standard_normal(v.shape)).astype(F), (0.01 * rng.random(v.shape) + 1e-6).astype(F)) for k, v in cloud.items()}
    cut = lambda x: x[:P]                      # noqa: E731
    return dict(P=P, M=M, cloud={k: cut(v) for k, v in cloud.items()}, moments={k: (cut(a), cut(b)) for k, (a, b) in moments.items()},
                raw_opacity=raw, raw_scales=raw, min_opacity=min_opacity, nudged=moved,
                u=rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64, endpoint=True)[:P],
                xi=rng.standard_normal((n, 3)).astype(F)[:P])


def within_one_ulp(got32, ref64, floor=2.0 ** -40):
    """|got - ref| <= max(one float32 ulp at ref, floor), elementwise -> bool array."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    ulp = np.spacing(np.abs(ref64).astype(F)).astype(np.float64)
    return np.abs(np.asarray(got32, dtype=np.float64) - ref64) <= np.maximum(ulp, floor)
