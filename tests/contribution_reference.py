"""Numpy restatement of the blending-weight statistics (include/hdrsplat.h, hs_contribution): the definition, tile by tile
as oracle/torch_rasterizer.render walks a frame, from an oracle forward dict (ranges, point_list, xy, conic_opacity).

For every pixel p and every entry g the published rule composites there -- power <= 0, alpha = min(0.99, o e^power) >=
1 / 255, before the entry at which T (1 - alpha) < 1e-4 ends the pixel -- with w = alpha T_before and e = pixel_weight[p]
(1 without a weight image; a pixel whose weight is exactly 0 takes part in nothing):

    sum[g]   = sum of e w          max[g] = max of e w (-inf where no term)          count[g] = number of terms with e w > 0

and, for the bound the GPU test holds the kernel to (|hip - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S, helpers.C_BOUND):

    S[g]     = sum of |e| w (4 + number of contributors composited before the entry at that pixel)
    S_max[g] = that weight of the single largest term (the one `max` is)

-- the weight of helpers.assert_grads_bounded: every earlier step costs T an ulp, and the term itself a few more (the
falloff's exponent, alpha, the product with T and with e).  `dtype` selects the arithmetic: float64 is the reference, float32
(sequential float32 products, numpy's exp) is what test_contribution.py holds against it to show the bound is not vacuous.
"""
from __future__ import annotations

import numpy as np

TILE = 16


def contributions(fwd: dict, W: int, H: int, pixel_weight=None, dtype=np.float64) -> dict:
    """The statistics of ONE pose.  Returns dict(sum, max, count, S, S_max [P]; pairs = number of contributing (pixel, entry)
    pairs with a non-zero pixel weight; final_T [H, W] of this evaluation; n_contrib [H, W])."""
    D = dtype
    xy = np.asarray(fwd["xy"]).astype(D)
    co = np.asarray(fwd["conic_opacity"]).astype(D)
    P = xy.shape[0]
    ranges = np.asarray(fwd["ranges"]).astype(np.int64)
    point_list = np.asarray(fwd["point_list"]).astype(np.int64)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    e_img = np.ones((H, W), D) if pixel_weight is None else np.asarray(pixel_weight).astype(D).reshape(H, W)
    out_sum, out_S = np.zeros(P, np.float64), np.zeros(P, np.float64)
    out_max, out_Smax = np.full(P, -np.inf), np.zeros(P, np.float64)
    out_count = np.zeros(P, np.int64)
    final_T = np.ones((H, W), D)
    n_contrib = np.zeros((H, W), np.int64)
    pairs = 0
    oy, ox = np.meshgrid(np.arange(TILE), np.arange(TILE), indexing="ij")
    for t in range(gx * gy):
        r0, r1 = int(ranges[t, 0]), int(ranges[t, 1])
        if r1 <= r0:
            continue
        ty, tx = divmod(t, gx)
        y0, x0 = ty * TILE, tx * TILE
        h, w = min(TILE, H - y0), min(TILE, W - x0)
        ids = point_list[r0:r1]
        pxs = (x0 + ox[:h, :w]).reshape(-1).astype(D)
        pys = (y0 + oy[:h, :w]).reshape(-1).astype(D)
        e = e_img[y0:y0 + h, x0:x0 + w].reshape(-1)
        dx = xy[ids, 0][None, :] - pxs[:, None]
        dy = xy[ids, 1][None, :] - pys[:, None]
        con = co[ids]
        power = D(-0.5) * (con[None, :, 0] * dx * dx + con[None, :, 2] * dy * dy) - con[None, :, 1] * dx * dy
        with np.errstate(over="ignore"):
            alpha = np.minimum(D(0.99), con[None, :, 3] * np.exp(power))
        valid = (power <= 0) & (alpha >= D(1.0 / 255.0))
        one_m = np.where(valid, D(1) - alpha, D(1))
        T_incl = np.cumprod(one_m, axis=1, dtype=D)                 # (sequential products in D)
        alive = T_incl >= D(0.0001)                                 # prefix mask: False from the terminating entry on
        contrib = valid & alive
        T_before = np.concatenate([np.ones((T_incl.shape[0], 1), D), T_incl[:, :-1]], axis=1)
        wgt = alpha * T_before
        before = np.cumsum(contrib, axis=1) - contrib               # contributors composited before the entry at that pixel
        Tf = np.where(alive, one_m, D(1)).prod(axis=1, dtype=D)
        pos = np.arange(1, ids.size + 1)
        final_T[y0:y0 + h, x0:x0 + w] = Tf.reshape(h, w)
        n_contrib[y0:y0 + h, x0:x0 + w] = np.where(contrib, pos[None, :], 0).max(axis=1).reshape(h, w)
        take = contrib & (e != 0)[:, None]
        if not take.any():
            continue
        pairs += int(take.sum())
        g = np.broadcast_to(ids[None, :], take.shape)[take]
        v = (e[:, None] * wgt)[take]                                 # e w, in D
        s_w = (np.abs(e)[:, None].astype(np.float64) * wgt.astype(np.float64) * (4.0 + before))[take]
        v64 = v.astype(np.float64)
        out_sum += np.bincount(g, weights=v64, minlength=P)
        out_S += np.bincount(g, weights=s_w, minlength=P)
        out_count += np.bincount(g[v > 0], minlength=P)
        # the largest term of every Gaussian in this tile, with its own weight
        order = np.lexsort((v64, g))
        g_s, v_s, s_s = g[order], v64[order], s_w[order]
        lastof = np.r_[g_s[1:] != g_s[:-1], True]
        gg, vv, ss = g_s[lastof], v_s[lastof], s_s[lastof]
        up = vv > out_max[gg]
        out_max[gg[up]] = vv[up]
        out_Smax[gg[up]] = ss[up]
    return dict(sum=out_sum, max=out_max, count=out_count, S=out_S, S_max=out_Smax, pairs=pairs, final_T=final_T,
                n_contrib=n_contrib)


def accumulate(arrays, stats: dict):
    """What a call leaves in (weight_sum, weight_max, pixel_count) that held `arrays` before it (float64 / int64): a
    Gaussian no term reached keeps its values."""
    ws, wm, pc = (np.array(a, copy=True) for a in arrays)
    hit = stats["max"] > -np.inf
    ws[hit] += stats["sum"][hit]
    wm[hit] = np.maximum(wm[hit], stats["max"][hit])
    pc[hit] += stats["count"][hit]
    return ws, wm, pc


def needed_constant(got, ref, S):
    """The largest (|got - ref| - 1e-4 |ref|) / (2^-24 S) over the elements (0 where the difference is inside 1e-4 |ref|;
    inf where it is not and S is 0): what C_BOUND has to cover."""
    got, ref, S = (np.asarray(a, np.float64) for a in (got, ref, S))
    excess = np.abs(got - ref) - 1e-4 * np.abs(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(excess > 0, excess / (2.0 ** -24 * S), 0.0)
    need = np.where(np.isfinite(need), need, np.where(excess > 0, np.inf, 0.0))
    return float(need.max()) if need.size else 0.0
