"""Numpy restatement of the per-Gaussian feature compositing (include/hdrsplat.h, hs_composite_features and its backward):
the definition, tile by tile as contribution_reference walks a frame, from an oracle forward dict (ranges, point_list, xy,
conic_opacity).

For every pixel p and every entry g the published rule composites there -- power <= 0, alpha = min(0.99, o e^power) >=
1 / 255, before the entry at which T (1 - alpha) < 1e-4 ends the pixel -- with w = alpha T_before:

    out[c, p]  = sum of w features[g, c]   (list order, front to back)        grad[g, c] = sum over p of w dL[c, p]

and, for the bound the GPU test holds the kernels to (|hip - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S, helpers.C_BOUND):

    S_out[c, p]  = sum of w |features[g, c]| (4 + n_p)      n_p: the number of contributors composited at the pixel -- T's
                   drift before the term, and the running sum's roundings after it
    S_grad[g, c] = sum of w |dL[c, p]| (4 + contributors composited before the entry at that pixel), as
                   contribution_reference's S

`dtype` selects the arithmetic: float64 is the reference; float32 (sequential float32 products and sums in list order,
numpy's exp) is what test_features.py holds against it to show the bound is not vacuous.  One pose; finite inputs.
"""
from __future__ import annotations

import numpy as np

from contribution_reference import needed_constant  # noqa: F401  (the tests take it from here)

TILE = 16


def composite(fwd: dict, W: int, H: int, features, dL=None, dtype=np.float64) -> dict:
    """features [P, C]; dL [C, H, W] or None.  Returns dict(out, S_out [C, H, W]; grad, S_grad [P, C] (zeros without dL);
    final_T [H, W] of this evaluation; n_contrib [H, W]; count [H, W]: contributors composited at the pixel)."""
    D = dtype
    xy = np.asarray(fwd["xy"]).astype(D)
    co = np.asarray(fwd["conic_opacity"]).astype(D)
    P = xy.shape[0]
    feat = np.asarray(features).astype(D)
    assert feat.ndim == 2 and feat.shape[0] == P and np.isfinite(feat).all()
    C = feat.shape[1]
    dl = None if dL is None else np.asarray(dL).astype(D).reshape(C, H, W)
    ranges = np.asarray(fwd["ranges"]).astype(np.int64)
    point_list = np.asarray(fwd["point_list"]).astype(np.int64)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    out, S_out = np.zeros((C, H, W), D), np.zeros((C, H, W), np.float64)
    grad, S_grad = np.zeros((P, C), D), np.zeros((P, C), np.float64)
    final_T = np.ones((H, W), D)
    n_contrib = np.zeros((H, W), np.int64)
    count = np.zeros((H, W), np.int64)
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
        wz = np.where(contrib, alpha * T_before, D(0))              # the weight where composited (selected, not multiplied)
        before = np.cumsum(contrib, axis=1) - contrib
        n_p = contrib.sum(axis=1)
        pos = np.arange(1, ids.size + 1)
        final_T[y0:y0 + h, x0:x0 + w] = np.where(alive, one_m, D(1)).prod(axis=1, dtype=D).reshape(h, w)
        n_contrib[y0:y0 + h, x0:x0 + w] = np.where(contrib, pos[None, :], 0).max(axis=1).reshape(h, w)
        count[y0:y0 + h, x0:x0 + w] = n_p.reshape(h, w)
        f_t = feat[ids]                                              # [entries, C]
        if D is np.float64:
            o_t = wz @ f_t                                           # [pixels, C]
        else:   # the running sum of the definition, term by term in D
            o_t = np.stack([np.cumsum(wz * f_t[None, :, c], axis=1, dtype=D)[:, -1] for c in range(C)], axis=1)
        wz64 = wz.astype(np.float64)
        s_t = (wz64 @ np.abs(f_t).astype(np.float64)) * (4.0 + n_p)[:, None]
        out[:, y0:y0 + h, x0:x0 + w] = o_t.T.reshape(C, h, w)
        S_out[:, y0:y0 + h, x0:x0 + w] = s_t.T.reshape(C, h, w)
        if dl is not None:
            d_t = dl[:, y0:y0 + h, x0:x0 + w].reshape(C, -1).T       # [pixels, C]
            np.add.at(grad, ids, (wz.T @ d_t).astype(D))
            np.add.at(S_grad, ids, (wz64 * (4.0 + before)).T @ np.abs(d_t).astype(np.float64))
    return dict(out=out, S_out=S_out, grad=grad, S_grad=S_grad, final_T=final_T, n_contrib=n_contrib, count=count)
