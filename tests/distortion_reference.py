"""Numpy restatement of the depth-distortion loss (include/hdrsplat.h, hs_distortion and hs_distortion_backward): the
definition, tile by tile as features_reference walks a frame, from an oracle forward dict (ranges, point_list, xy,
conic_opacity, depths), and the projection of its per-instance screen rows to the four geometry tensors.

For every pixel p and the entries i = 1..n the published rule composites there -- power <= 0, alpha = min(0.99, o e^power) >=
1 / 255, before the entry at which T (1 - alpha) < 1e-4 ends the pixel -- front to back with w = alpha T_before, s = 1 / z,
A_i = sum_{j <= i} w_j, D_i = sum_{j <= i} w_j s_j:

    out[p]    = 2 sum_i w_i (D_{i-1} - s_i A_{i-1})          moment[p] = D_n

and, given gamma[p] = dL / d out[p], with A+_i, D+_i the sums over j > i:

    v_i       = 2 [ (D_{i-1} - s_i A_{i-1}) + (s_i A+_i - D+_i) ]
    dL/dalpha_i = gamma (T_i v_i - (sum_{j > i} w_j v_j) / (1 - alpha_i))      (the closed form of the recurrence
                  dL/dalpha_i = gamma T_i (v_i - q_i), q_{i-1} = q_i + alpha_i (v_i - q_i), q_n = 0)
    dL/ds_i   = gamma 2 w_i (A+_i - A_{i-1})

and from dL/dalpha the render backward's screen rows per instance: {d mean2D x, y (NDC-scaled: times W / 2, H / 2), d conic
A, B, C, d opacity, d inverse depth} (ROWS).

The bound the GPU test holds the kernels to is |hip - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S (helpers.C_BOUND).  S is built
beside every number by the project's rule: every difference is replaced by the sum of the absolute values of its operands
(|D| + s A for D - s A, A+ + A_{i-1} for A+ - A_{i-1}, the two halves of v_i and the two terms of dL/dalpha_i added), and
every term is weighted by 4 plus the number of compositing and running-sum steps behind it:

    map       term i:  4 + b_i + n          b_i contributors composited before it at the pixel (T's drift), n the pixel's
                                            contributors (b_i additions made the prefix sums, n - b_i follow in the loss's sum)
    moment    term i:  4 + n                (as features_reference's S_out)
    backward  entry i: 4 + (n - b_i) + n    n - b_i divisions rebuilt T_i from final_T; the totals the prefix sums are taken
                                            from carry n additions, the suffix sums fewer

`dtype=np.float32` evaluates the same sums sequentially in float32, in distort.hip's order of operations (sums relative to
s0 = 1 / z of the tile's first entry, A_n = 1 - final_T, the prefix part as the total about s_i minus the suffix part), with
numpy's exp and a division where the kernels use v_exp_f32 and v_rcp_f32 and without fma: what test_distortion.py holds
against the float64 result to show that the bound is neither vacuous nor unreachable.  The DECISIONS are the float64 ones in
both modes.  One pose per call; finite inputs.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import torch_rasterizer as TR

TILE = 16
ROWS = ("mean2D_x", "mean2D_y", "conic_A", "conic_B", "conic_C", "opacity", "invdepth")
# (key of the HIP result "d_<key>", key of the truth): helpers.assert_grads_bounded's `keys`
GEO_KEYS = [("means3D", "dL_dmeans3D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"), ("rotations", "dL_drots")]


def _rcumsum_excl(x):
    """sum over j > i along axis 1"""
    return np.cumsum(x[:, ::-1], axis=1)[:, ::-1] - x


def distortion(fwd: dict, W: int, H: int, gamma=None, dtype=np.float64) -> dict:
    """gamma [H, W] or None.  Returns dict(out, moment, S_out, S_moment [H, W]; rows, S_rows [P, 7] in the order of ROWS
    (zeros without gamma); final_T [H, W] of this evaluation; n_contrib, count [H, W])."""
    D = dtype
    xy64 = np.asarray(fwd["xy"]).astype(np.float64)
    co64 = np.asarray(fwd["conic_opacity"]).astype(np.float64)
    z_in = np.asarray(fwd["depths"])      # float32 from the oracle (a float64 array is taken as it is: torch_loss)
    P = xy64.shape[0]
    g_img = None if gamma is None else np.asarray(gamma).astype(np.float64).reshape(H, W)
    ranges = np.asarray(fwd["ranges"]).astype(np.int64)
    point_list = np.asarray(fwd["point_list"]).astype(np.int64)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    out, moment = np.zeros((H, W), D), np.zeros((H, W), D)
    S_out, S_mom = np.zeros((H, W)), np.zeros((H, W))
    rows, S_rows = np.zeros((P, 7), np.float64), np.zeros((P, 7), np.float64)
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
        sl = (slice(y0, y0 + h), slice(x0, x0 + w))
        ids = point_list[r0:r1]
        pxs = (x0 + ox[:h, :w]).reshape(-1).astype(np.float64)
        pys = (y0 + oy[:h, :w]).reshape(-1).astype(np.float64)
        # ---- the decisions and the float64 quantities ----
        dx = xy64[ids, 0][None, :] - pxs[:, None]
        dy = xy64[ids, 1][None, :] - pys[:, None]
        con = co64[ids]
        power = -0.5 * (con[None, :, 0] * dx * dx + con[None, :, 2] * dy * dy) - con[None, :, 1] * dx * dy
        with np.errstate(over="ignore"):
            G = np.exp(np.minimum(power, 0.0))
            alpha = np.minimum(0.99, con[None, :, 3] * G)
        valid = (power <= 0) & (alpha >= 1.0 / 255.0)
        one_m = np.where(valid, 1.0 - alpha, 1.0)
        T_incl = np.cumprod(one_m, axis=1)
        alive = T_incl >= 0.0001                                     # prefix mask: False from the terminating entry on
        contrib = valid & alive
        before = np.cumsum(contrib, axis=1) - contrib
        n_p = contrib.sum(axis=1)
        pos = np.arange(1, ids.size + 1)
        n_contrib[sl] = np.where(contrib, pos[None, :], 0).max(axis=1).reshape(h, w)
        count[sl] = n_p.reshape(h, w)
        last = int(np.where(contrib, pos[None, :], 0).max())          # the tile's deepest contributor
        gam = None if g_img is None else g_img[sl].reshape(-1)
        if D is np.float32:
            res = _tile_f32(xy64[ids].astype(D), con.astype(D), z_in[ids].astype(D), pxs.astype(D), pys.astype(D), contrib, last,
                            None if gam is None else gam.astype(D), W, H)
            out[sl], moment[sl], final_T[sl] = (res[k].reshape(h, w) for k in ("out", "moment", "final_T"))
            if gam is not None:
                rows[ids] += res["rows"]
            continue
        T_before = np.concatenate([np.ones((T_incl.shape[0], 1)), T_incl[:, :-1]], axis=1)
        wz = np.where(contrib, alpha * T_before, 0.0)                 # the weight where composited (selected, not multiplied)
        final_T[sl] = np.where(alive, one_m, 1.0).prod(axis=1).reshape(h, w)
        s = (1.0 / z_in[ids].astype(np.float64))[None, :]
        ws = wz * s
        A_prev = np.cumsum(wz, axis=1) - wz
        D_prev = np.cumsum(ws, axis=1) - ws
        pre, pre_abs = D_prev - s * A_prev, np.abs(D_prev) + s * A_prev
        wt_f = 4.0 + before + n_p[:, None]
        out[sl] = (2.0 * (wz * pre).sum(axis=1)).reshape(h, w)
        S_out[sl] = (2.0 * (wz * pre_abs * wt_f).sum(axis=1)).reshape(h, w)
        moment[sl] = ws.sum(axis=1).reshape(h, w)
        S_mom[sl] = (ws.sum(axis=1) * (4.0 + n_p)).reshape(h, w)
        if gam is None:
            continue
        A_suf, D_suf = _rcumsum_excl(wz), _rcumsum_excl(ws)
        suf, suf_abs = s * A_suf - D_suf, s * A_suf + np.abs(D_suf)
        wt_b = 4.0 + 2.0 * n_p[:, None] - before
        v = 2.0 * (pre + suf)
        S_v = 2.0 * (pre_abs + suf_abs) * wt_b
        g = gam[:, None]
        dalpha = np.where(contrib, g * (T_before * v - _rcumsum_excl(wz * v) / one_m), 0.0)
        S_dalpha = np.where(contrib, np.abs(g) * (T_before * S_v + _rcumsum_excl(wz * S_v) / one_m), 0.0)
        ds = g * 2.0 * wz * (A_suf - A_prev)
        S_ds = np.abs(g) * 2.0 * wz * (A_suf + A_prev) * wt_b
        # alpha = o G passes its gradient through the 0.99 cap: d alpha / d power = o G, d alpha / d o = G
        sw = con[None, :, 3] * G * dalpha
        sw_abs = con[None, :, 3] * G * S_dalpha
        cA, cB, cC = con[:, 0], con[:, 1], con[:, 2]
        v0, v1 = (sw * dx).sum(axis=0), (sw * dy).sum(axis=0)
        a0, a1 = (sw_abs * np.abs(dx)).sum(axis=0), (sw_abs * np.abs(dy)).sum(axis=0)
        r = np.stack([-(cA * v0 + cB * v1) * 0.5 * W, -(cC * v1 + cB * v0) * 0.5 * H,
                      -0.5 * (sw * dx * dx).sum(axis=0), -(sw * dx * dy).sum(axis=0), -0.5 * (sw * dy * dy).sum(axis=0),
                      (G * dalpha).sum(axis=0), ds.sum(axis=0)], axis=1)
        ra = np.stack([(np.abs(cA) * a0 + np.abs(cB) * a1) * 0.5 * W, (np.abs(cC) * a1 + np.abs(cB) * a0) * 0.5 * H,
                       0.5 * (sw_abs * dx * dx).sum(axis=0), (sw_abs * np.abs(dx * dy)).sum(axis=0),
                       0.5 * (sw_abs * dy * dy).sum(axis=0), (G * S_dalpha).sum(axis=0), S_ds.sum(axis=0)], axis=1)
        rows[ids] += r          # (an instance is on a tile's list once)
        S_rows[ids] += ra
    return dict(out=out, moment=moment, S_out=S_out, S_moment=S_mom, rows=rows, S_rows=S_rows, final_T=final_T,
                n_contrib=n_contrib, count=count)


def _tile_f32(xy, con, z, pxs, pys, contrib, last, gam, W, H):
    """One tile in float32, entry by entry in distort.hip's order of operations; `contrib` [pixels, entries]: the decisions."""
    F = np.float32
    n_px, n_e = contrib.shape
    s0 = F(1) / z[0]
    sr = F(1) / z - s0
    dx = xy[:, 0][None, :] - pxs[:, None]
    dy = xy[:, 1][None, :] - pys[:, None]
    power = F(-0.5) * (con[None, :, 0] * dx * dx + con[None, :, 2] * dy * dy) - con[None, :, 1] * dx * dy
    with np.errstate(over="ignore"):
        G = np.exp(np.minimum(power, F(0))).astype(F)
    alpha = np.minimum(F(0.99), con[None, :, 3] * G)
    T, A, Dd, loss = np.ones(n_px, F), np.zeros(n_px, F), np.zeros(n_px, F), np.zeros(n_px, F)
    for j in range(last):
        c = contrib[:, j]
        if not c.any():
            continue
        a = alpha[:, j]
        wj = a * T
        loss = np.where(c, loss + wj * (Dd - sr[j] * A), loss)
        Dd = np.where(c, Dd + wj * sr[j], Dd)
        A = np.where(c, A + wj, A)
        T = np.where(c, T * (F(1) - a), T)
    res = dict(out=loss + loss, moment=Dd + s0 * A, final_T=T.copy())
    if gam is None:
        return res
    g2 = F(2) * gam
    An = F(1) - T
    M0 = res["moment"] - s0 * An
    q, Ap, Dp = np.zeros(n_px, F), np.zeros(n_px, F), np.zeros(n_px, F)
    sums = np.zeros((n_e, 7), F)
    for j in range(last - 1, -1, -1):
        c = contrib[:, j]
        if not c.any():
            continue
        ae = np.where(c, alpha[:, j], F(0))
        T = T * (F(1) / (F(1) - ae))
        wj = ae * T
        suf = sr[j] * Ap - Dp
        tot = M0 - sr[j] * An
        cd = g2 * (tot + (suf + suf))
        ds = (g2 * wj) * ((Ap + Ap) + (wj - An))
        Ap = Ap + wj
        Dp = Dp + wj * sr[j]
        diff = cd - q
        dop = np.where(c, G[:, j] * (diff * T), F(0))
        q = q + ae * diff
        sw = con[j, 3] * dop
        m = sw * dy[:, j]
        sums[j] = [(sw * dx[:, j]).sum(dtype=F), m.sum(dtype=F), (sw * dx[:, j] * dx[:, j]).sum(dtype=F),
                   (m * dx[:, j]).sum(dtype=F), (m * dy[:, j]).sum(dtype=F), dop.sum(dtype=F), ds.sum(dtype=F)]
    cA, cB, cC = con[:, 0], con[:, 1], con[:, 2]
    res["rows"] = np.stack([-(cA * sums[:, 0] + cB * sums[:, 1]) * F(0.5 * W), -(cC * sums[:, 1] + cB * sums[:, 0]) * F(0.5 * H),
                            F(-0.5) * sums[:, 2], -sums[:, 3], F(-0.5) * sums[:, 4], sums[:, 5], sums[:, 6]], axis=1).astype(np.float64)
    return res


# ---- the projection of the rows to the four tensors ----

def view_of(cam, dt=torch.float64):
    return TR.View(cam.W, cam.H, cam.tanfovx, cam.tanfovy, cam.viewmatrix.to(dt), cam.projmatrix.to(dt), cam.campos.to(dt))


def screen_quantities(view, means3D, opacities, scales, rotations, scale_modifier=1.0, antialias=False):
    """The seven per-instance quantities the rows are gradients of, in the order of ROWS (xy in pixels), from
    oracle.torch_rasterizer.preprocess; and the visibility mask."""
    pre = TR.preprocess(view, means3D, opacities, 0, colors_precomp=torch.zeros_like(means3D), scales=scales, rotations=rotations,
                        scale_modifier=scale_modifier, antialiasing=antialias)
    vis = pre["visible"]
    inv = 1.0 / torch.where(vis, pre["depth"], torch.ones_like(pre["depth"]))
    q = [pre["xy"][:, 0], pre["xy"][:, 1], pre["conic"][:, 0], pre["conic"][:, 1], pre["conic"][:, 2], pre["opacity"], inv]
    return q, vis, pre


def project(cams, rows, S_rows, means3D, opacities, scales, rotations, scale_modifier=1.0, antialias=False) -> dict:
    """rows, S_rows: one [P, 7] array per pose (ROWS order, mean2D NDC-scaled).  An instance's seven quantities depend on
    its own Gaussian only, so one backward pass of sum_g q_k[g] gives every d q_k / d theta: truth = sum_k J_k rows_k,
    S = sum_k |J_k| S_rows_k, summed over the poses.  Returns {dL_dX, abs_dL_dX} for X in GEO_KEYS, float64."""
    dt = torch.float64
    leaves = [torch.as_tensor(np.asarray(t, np.float64)).clone().requires_grad_(True)
              for t in (means3D, np.asarray(opacities, np.float64).reshape(-1, 1), scales, rotations)]
    names = [rk for _, rk in GEO_KEYS]
    acc = {n: np.zeros(tuple(l.shape)) for n, l in zip(names, leaves)}
    acc.update({"abs_" + n: np.zeros(tuple(l.shape)) for n, l in zip(names, leaves)})
    for cam, r, sr in zip(cams, rows, S_rows):
        q, vis, _ = screen_quantities(view_of(cam, dt), *leaves, scale_modifier=scale_modifier, antialias=antialias)
        unit = [0.5 * cam.W, 0.5 * cam.H, 1.0, 1.0, 1.0, 1.0, 1.0]      # the mean2D rows are gradients per NDC unit
        on = vis.numpy()
        for k in range(7):
            J = torch.autograd.grad(q[k].sum(), leaves, retain_graph=True, allow_unused=True)
            rk = np.where(on, np.asarray(r)[:, k] / unit[k], 0.0)
            sk = np.where(on, np.asarray(sr)[:, k] / unit[k], 0.0)
            assert not np.asarray(r)[~on].any(), "a culled instance has a row"
            for n, l, j in zip(names, leaves, J):
                if j is None:
                    continue
                j = np.where(on[:, None], j.numpy(), 0.0)
                acc[n] += j * rk[:, None]
                acc["abs_" + n] += np.abs(j) * sk[:, None]
    return acc


def truth(fwds, cams, gammas, sc) -> dict:
    """The float64 truth of a call over `cams` (one oracle forward dict and one gamma [H, W] per pose) for the scene `sc`:
    dict(out, moment, S_out, S_moment [n_poses, H, W], n_contrib; dL_dX / abs_dL_dX for X in GEO_KEYS)."""
    W, H = cams[0].W, cams[0].H
    per = [distortion(f, W, H, g) for f, g in zip(fwds, gammas)]
    res = project(cams, [p["rows"] for p in per], [p["S_rows"] for p in per], sc.means3D.numpy(), sc.opacities.numpy(),
                  sc.scales.numpy(), sc.rotations.numpy(), float(getattr(sc, "scale_modifier", 1.0)),
                  bool(getattr(sc, "antialias", False)))
    for k in ("out", "moment", "S_out", "S_moment", "n_contrib"):
        res[k] = np.stack([p[k] for p in per])
    return res


def torch_loss(view, means3D, opacities, scales, rotations, gamma, scale_modifier=1.0, antialias=False, want_map=False):
    """sum(gamma * map) through preprocess, bin_tiles and a torch copy of the sum (the pairwise prefix form), differentiable
    in float64 by autograd alone -- the published conventions of oracle.torch_rasterizer.render (decisions are constants, the
    0.99 cap passes the gradient through).  Also returns the forward dict the numpy restatement takes."""
    _, _, pre = screen_quantities(view, means3D, opacities, scales, rotations, scale_modifier, antialias)
    point_list, ranges, _ = TR.bin_tiles(view, pre)
    W, H = view.W, view.H
    dt = pre["xy"].dtype
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    oy, ox = torch.meshgrid(torch.arange(TILE), torch.arange(TILE), indexing="ij")
    xy, conic, opac = pre["xy"], pre["conic"], pre["opacity"]
    z = pre["depth"]
    inv = 1.0 / z
    total = torch.zeros((), dtype=dt)
    img = torch.zeros(H, W, dtype=dt)
    for t in range(gx * gy):
        r0, r1 = int(ranges[t, 0]), int(ranges[t, 1])
        if r1 <= r0:
            continue
        ty, tx = divmod(t, gx)
        y0, x0 = ty * TILE, tx * TILE
        h, w = min(TILE, H - y0), min(TILE, W - x0)
        ids = point_list[r0:r1]
        pxs = (x0 + ox[:h, :w]).reshape(-1).to(dt)
        pys = (y0 + oy[:h, :w]).reshape(-1).to(dt)
        dx = xy[ids][None, :, 0] - pxs[:, None]
        dy = xy[ids][None, :, 1] - pys[:, None]
        con = conic[ids]
        power = -0.5 * (con[None, :, 0] * dx * dx + con[None, :, 2] * dy * dy) - con[None, :, 1] * dx * dy
        raw = opac[ids][None, :] * torch.exp(power)
        alpha = raw + (torch.clamp(raw, max=0.99) - raw).detach()
        valid = (power <= 0) & (alpha.detach() >= 1.0 / 255.0)
        one_m = torch.where(valid, 1.0 - alpha, torch.ones_like(alpha))
        T_incl = torch.cumprod(one_m, dim=1)
        contrib = valid & (T_incl.detach() >= 0.0001)
        wgt = torch.where(contrib, alpha * (T_incl / one_m), torch.zeros_like(alpha))
        s = inv[ids][None, :]
        A_prev = torch.cumsum(wgt, dim=1) - wgt
        D_prev = torch.cumsum(wgt * s, dim=1) - wgt * s
        m = 2.0 * (wgt * (D_prev - s * A_prev)).sum(dim=1).reshape(h, w)
        total = total + (m * gamma[y0:y0 + h, x0:x0 + w]).sum()
        img[y0:y0 + h, x0:x0 + w] = m.detach()
    fwd = dict(xy=xy.detach().numpy(), conic_opacity=torch.cat([conic, opac[:, None]], dim=1).detach().numpy(),
               depths=z.detach().numpy(), ranges=ranges.numpy(), point_list=point_list.numpy())
    return (total, fwd, img) if want_map else (total, fwd)
