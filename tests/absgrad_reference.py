"""Numpy restatement of the absolute screen-gradient statistic (include/hdrsplat.h, hs_abs_gradient): the definition, tile by
tile as oracle/torch_rasterizer.render walks a frame, from an oracle forward dict (ranges, point_list, xy, conic_opacity, rgb,
depths) and the per-pixel gradient dL/dH of the loss with respect to THIS pose's radiance image (the 1 / N of the pose
average, the CRF chain, dL_dout_hdr already inside it).

For every pixel p and every entry g the published rule composites there -- power <= 0, alpha = min(0.99, o e^power) >=
1 / 255, before the entry at which T (1 - alpha) < 1e-4 ends the pixel -- walked back to front with q starting at bg . dL
(minus dL_dalpha) and q_{i-1} = q_i + alpha_i (c_i . dL - q_i)   (c . dL gains 1 / depth * dL_dinvdepth):

    w   = o G T_i (c_i . dL - q_i)                       the factor the backward multiplies dx, dy by  (G = e^power)
    t_x = -(A dx + B dy) w W / 2        t_y = -(C dy + B dx) w H / 2

    abs_x[g] = sum |t_x|     abs_y[g] = sum |t_y|        signed_x[g] = sum t_x     signed_y[g] = sum t_y

and, for the bound the GPU test holds the kernel to (|hip - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S, helpers.C_BOUND), the same
sums with every signed quantity replaced by its magnitude -- |c| . |dL| for c . dL, the recurrence for q run on those
magnitudes (qa starts at |bg| . |dL| + |dL_dalpha|, qa_{i-1} = (1 - alpha_i) qa_i + alpha_i |c_i| . |dL|: what bounds |q| and
every intermediate of it), |c . dL - q| <= |c| . |dL| + qa, |A dx| + |B dy| for |A dx + B dy| -- each term weighted by
(4 + the number of contributors of that pixel): every step of the walk costs T an ulp, and the term itself a few more.

    S_x[g], S_y[g]

`statistic` folds poses and the square root: a = sqrt(abs_x^2 + abs_y^2) with S = sqrt(S_x^2 + S_y^2) (the length of a
vector moves by at most the length of its error).  `dtype` selects the arithmetic: float64 is the reference, float32
(sequential float32 operations, numpy's exp) is what test_absgrad.py holds against it to show the bound is not vacuous.
"""
from __future__ import annotations

import numpy as np

TILE = 16


def abs_gradients(fwd: dict, W: int, H: int, dL, bg, dL_alpha=None, dL_invdepth=None, dtype=np.float64) -> dict:
    """The sums of ONE pose.  dL: [3, H, W] (dL/dH of this pose); bg: [3]; dL_alpha / dL_invdepth: [H, W] or None, already
    divided by the number of poses.  Returns dict(abs_x, abs_y, signed_x, signed_y, S_x, S_y [P] float64; hit [P] bool: some
    term exists; pairs; final_T, n_contrib [H, W] of this evaluation)."""
    D = dtype
    xy = np.asarray(fwd["xy"]).astype(D)
    co = np.asarray(fwd["conic_opacity"]).astype(D)
    rgb = np.asarray(fwd["rgb"]).astype(D)
    P = xy.shape[0]
    invd = (D(1) / np.asarray(fwd["depths"]).astype(D)) if dL_invdepth is not None else np.zeros(P, D)
    ranges = np.asarray(fwd["ranges"]).astype(np.int64)
    point_list = np.asarray(fwd["point_list"]).astype(np.int64)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    dL = np.asarray(dL).astype(D).reshape(3, H, W)
    bg = np.asarray(bg).astype(D).reshape(3)
    dLa = np.zeros((H, W), D) if dL_alpha is None else np.asarray(dL_alpha).astype(D).reshape(H, W)
    dLd = np.zeros((H, W), D) if dL_invdepth is None else np.asarray(dL_invdepth).astype(D).reshape(H, W)
    out = {k: np.zeros(P, np.float64) for k in ("abs_x", "abs_y", "signed_x", "signed_y", "S_x", "S_y")}
    hit = np.zeros(P, bool)
    final_T = np.ones((H, W), D)
    n_contrib = np.zeros((H, W), np.int64)
    pairs = 0
    half_W, half_H = D(0.5) * D(W), D(0.5) * D(H)
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
        g3 = dL[:, y0:y0 + h, x0:x0 + w].reshape(3, -1)             # [3, pixels]
        ga = dLa[y0:y0 + h, x0:x0 + w].reshape(-1)
        gd = dLd[y0:y0 + h, x0:x0 + w].reshape(-1)
        dx = xy[ids, 0][None, :] - pxs[:, None]
        dy = xy[ids, 1][None, :] - pys[:, None]
        con = co[ids]
        power = D(-0.5) * (con[None, :, 0] * dx * dx + con[None, :, 2] * dy * dy) - con[None, :, 1] * dx * dy
        with np.errstate(over="ignore"):
            G = np.exp(power)
            alpha = np.minimum(D(0.99), con[None, :, 3] * G)
        valid = (power <= 0) & (alpha >= D(1.0 / 255.0))
        one_m = np.where(valid, D(1) - alpha, D(1))
        T_incl = np.cumprod(one_m, axis=1, dtype=D)                 # (sequential products in D)
        alive = T_incl >= D(0.0001)                                 # prefix mask: False from the terminating entry on
        contrib = valid & alive
        T_before = np.concatenate([np.ones((T_incl.shape[0], 1), D), T_incl[:, :-1]], axis=1)
        Tf = np.where(alive, one_m, D(1)).prod(axis=1, dtype=D)
        pos = np.arange(1, ids.size + 1)
        final_T[y0:y0 + h, x0:x0 + w] = Tf.reshape(h, w)
        last = np.where(contrib, pos[None, :], 0).max(axis=1)
        n_contrib[y0:y0 + h, x0:x0 + w] = last.reshape(h, w)
        if not contrib.any():
            continue
        n_pix = contrib.sum(axis=1)                                 # contributors of the pixel
        # c . dL and its magnitude, per (pixel, entry)
        col = rgb[ids]
        cd = (g3[0][:, None] * col[None, :, 0] + g3[1][:, None] * col[None, :, 1]) + g3[2][:, None] * col[None, :, 2]
        cda = (np.abs(g3[0])[:, None] * np.abs(col[None, :, 0]) + np.abs(g3[1])[:, None] * np.abs(col[None, :, 1])
               + np.abs(g3[2])[:, None] * np.abs(col[None, :, 2]))
        if dL_invdepth is not None:
            cd = cd + gd[:, None] * invd[ids][None, :]
            cda = cda + np.abs(gd)[:, None] * np.abs(invd[ids])[None, :]
        # the walk, back to front: one column per step, every pixel at once
        q = ((bg[0] * g3[0] + bg[1] * g3[1]) + bg[2] * g3[2]) - ga
        qa = (np.abs(bg[0] * g3[0]) + np.abs(bg[1] * g3[1])) + np.abs(bg[2] * g3[2]) + np.abs(ga)
        wv = np.zeros_like(cd)                                      # w of the definition
        wa = np.zeros_like(cd)                                      # its magnitude bound
        for i in range(int(last.max()) - 1, -1, -1):
            on = contrib[:, i]
            if not on.any():
                continue
            a_i = np.where(on, alpha[:, i], D(0))
            diff = cd[:, i] - q
            diffa = cda[:, i] + qa
            oG = con[i, 3] * G[:, i]
            wv[:, i] = np.where(on, oG * (T_before[:, i] * diff), D(0))
            wa[:, i] = np.where(on, oG * (T_before[:, i] * diffa), D(0))
            q = q + a_i * diff
            qa = (D(1) - a_i) * qa + a_i * cda[:, i]
        A, B, Cc = con[None, :, 0], con[None, :, 1], con[None, :, 2]
        tx_ = -(A * dx + B * dy) * wv * half_W
        ty_ = -(Cc * dy + B * dx) * wv * half_H
        bx = (np.abs(A * dx) + np.abs(B * dy)) * wa * half_W * (D(4) + n_pix[:, None].astype(D))
        by = (np.abs(Cc * dy) + np.abs(B * dx)) * wa * half_H * (D(4) + n_pix[:, None].astype(D))
        pairs += int(contrib.sum())
        gg = np.broadcast_to(ids[None, :], contrib.shape)[contrib]
        hit[gg] = True
        for key, v in (("abs_x", np.abs(tx_)), ("abs_y", np.abs(ty_)), ("signed_x", tx_), ("signed_y", ty_), ("S_x", bx),
                       ("S_y", by)):
            out[key] += np.bincount(gg, weights=v[contrib].astype(np.float64), minlength=P)
    out.update(hit=hit, pairs=pairs, final_T=final_T, n_contrib=n_contrib)
    return out


def statistic(poses) -> dict:
    """What ONE frame adds: `poses` = the abs_gradients results of the frame's poses, ascending.  Returns dict(a, S [P];
    hit [P]; abs_x, abs_y, signed_x, signed_y, S_x, S_y summed over the poses)."""
    keys = ("abs_x", "abs_y", "signed_x", "signed_y", "S_x", "S_y")
    tot = {k: sum(p[k] for p in poses) for k in keys}
    hit = np.zeros_like(poses[0]["hit"])
    for p in poses:
        hit = hit | p["hit"]
    tot.update(a=np.sqrt(tot["abs_x"] ** 2 + tot["abs_y"] ** 2), S=np.sqrt(tot["S_x"] ** 2 + tot["S_y"] ** 2), hit=hit)
    return tot


def accumulate(before, frames):
    """What a call leaves in abs_grad_accum that held `before` (float64 [P]): per frame (a `statistic` result), ascending,
    += a for the Gaussians with a term; the others keep their value."""
    acc = np.array(before, np.float64, copy=True)
    for fr in frames:
        acc[fr["hit"]] += fr["a"][fr["hit"]]
    return acc


def needed_constant(got, ref, S):
    """The largest (|got - ref| - 1e-4 |ref|) / (2^-24 S) over the elements (0 where the difference is inside 1e-4 |ref|;
    inf where it is not and S is 0): what C_BOUND has to cover."""
    got, ref, S = (np.asarray(a, np.float64) for a in (got, ref, S))
    excess = np.abs(got - ref) - 1e-4 * np.abs(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(excess > 0, excess / (2.0 ** -24 * S), 0.0)
    need = np.where(np.isfinite(need), need, np.where(excess > 0, np.inf, 0.0))
    return float(need.max()) if need.size else 0.0


def hdr_pose_gradients(T, sc, fwds, dL_ldr, blur_domain="ldr", dL_hdr=None):
    """dL/dH_k [N, 3, H, W] (float64) of an HDR frame of N poses: the oracle's tone-map (T = oracle.torch_rasterizer) under
    float64 autograd on the oracle's radiance images `fwds[k]["color"]`, the blur average in `blur_domain`, plus dL_hdr / N."""
    import torch
    Hs = [torch.tensor(np.asarray(f["color"], np.float64), requires_grad=True) for f in fwds]
    N = len(Hs)
    dt = torch.tensor(float(sc.exposure), dtype=torch.float64)
    tab = sc.crf_table.double()
    if blur_domain == "ldr":
        ldr = torch.stack([T.tonemap(h, dt, tab, sc.crf_range) for h in Hs]).mean(dim=0)
    else:
        ldr = T.tonemap(torch.stack(Hs).mean(dim=0), dt, tab, sc.crf_range)
    loss = (ldr * torch.tensor(np.asarray(dL_ldr, np.float64))).sum()
    if dL_hdr is not None:
        loss = loss + (torch.stack(Hs).mean(dim=0) * torch.tensor(np.asarray(dL_hdr, np.float64))).sum()
    loss.backward()
    return np.stack([h.grad.numpy() for h in Hs])
