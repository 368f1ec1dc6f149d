"""Shared test plumbing: scene -> (HIP path through the C ABI) and scene -> (CPU oracle), plus comparators.

The HIP path is casualhdrsplat_amd (product).  The oracle (oracle/) is only ever the checker.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from casualhdrsplat_amd import synthetic as S


def settings_from_scene(sc: S.Scene, device, cameras=None, hdr=False, blur_domain="ldr", requires_grad=False,
                        radiance_activation="relu_shift"):
    from casualhdrsplat_amd import GaussianRasterizationSettings
    cam = sc.camera
    kw = {}
    exposure = crf = None
    if hdr:
        exposure = sc.exposure.clone().to(device).requires_grad_(requires_grad)
        crf = sc.crf_table.clone().to(device).requires_grad_(requires_grad)
        kw.update(exposure=exposure, crf_table=crf, crf_range=sc.crf_range, blur_domain=blur_domain)
    if cameras is not None:
        kw.update(viewmatrices=torch.stack([c.viewmatrix for c in cameras]).to(device),
                  projmatrices=torch.stack([c.projmatrix for c in cameras]).to(device),
                  camposes=torch.stack([c.campos for c in cameras]).to(device))
    rs = GaussianRasterizationSettings(
        image_height=cam.H, image_width=cam.W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=sc.bg.to(device),
        scale_modifier=float(getattr(sc, "scale_modifier", 1.0)), viewmatrix=cam.viewmatrix.to(device),
        projmatrix=cam.projmatrix.to(device),
        sh_degree=sc.sh_degree, campos=cam.campos.to(device), prefiltered=False, debug=False,
        antialiasing=bool(getattr(sc, "antialias", False)), radiance_activation=radiance_activation, **kw)
    return rs, exposure, crf


def run_hip(sc: S.Scene, device="cuda", cameras=None, hdr=False, blur_domain="ldr", backward=True, capacity=None,
            use_cov_precomp=None, use_colors_precomp=None, grad_hdr=None, radiance_activation="relu_shift", dL_image=None,
            invdepth_grad=None, alpha_grad=None):
    """Forward (+ backward with sc.dL_dimage, or `dL_image` [3,H,W] when given) through GaussianRasterizer on the GPU.
    `invdepth_grad` / `alpha_grad` [H,W]: turn on return_invdepth / return_alpha, add sum(output * gradient) to the loss and
    return the images as res["invdepth"] / res["alpha"]."""
    from casualhdrsplat_amd import GaussianRasterizer, inspect_state
    rs, exposure, crf = settings_from_scene(sc, device, cameras, hdr, blur_domain, requires_grad=backward,
                                            radiance_activation=radiance_activation)
    leaf = {}

    def mk(name, t):
        leaf[name] = t.clone().to(device).requires_grad_(backward)
        return leaf[name]

    means3D = mk("means3D", sc.means3D)
    means2D = mk("means2D", torch.zeros_like(sc.means3D))
    opac = mk("opacities", sc.opacities)
    kwargs = {}
    if use_colors_precomp is not None:
        kwargs["colors_precomp"] = mk("colors_precomp", use_colors_precomp)
    else:
        kwargs["shs"] = mk("shs", sc.shs)
    if use_cov_precomp is not None:
        kwargs["cov3D_precomp"] = mk("cov3D_precomp", use_cov_precomp)
    else:
        kwargs["scales"] = mk("scales", sc.scales)
        kwargs["rotations"] = mk("rotations", sc.rotations)
    rast = GaussianRasterizer(rs, capacity=capacity, return_alpha=alpha_grad is not None,
                              return_invdepth=invdepth_grad is not None)
    out = rast(means3D, means2D, opac, **kwargs)
    res = {"color": out[0].detach().cpu().numpy(), "radii": out[1].cpu().numpy()}
    if hdr:
        res["hdr"] = out[2].detach().cpu().numpy()
    # (the outputs' order: colour, radii, [radiance], [accumulated opacity], [inverse depth])
    extra = []
    nxt = 3 if hdr else 2
    for name, up in (("alpha", alpha_grad), ("invdepth", invdepth_grad)):
        if up is not None:
            res[name] = out[nxt].detach().cpu().numpy()
            extra.append((out[nxt], torch.as_tensor(np.asarray(up, np.float32))))
            nxt += 1
    if backward:
        st = inspect_state(out[0])
        res["state"] = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
        dL_t = sc.dL_dimage if dL_image is None else torch.as_tensor(np.asarray(dL_image, np.float32))
        loss = (out[0] * dL_t.to(device)).sum()
        if grad_hdr is not None:
            loss = loss + (out[2] * grad_hdr.to(device)).sum()
        for img, up in extra:
            loss = loss + (img * up.to(device)).sum()
        loss.backward()
        for k, v in leaf.items():
            res["d_" + k] = v.grad.detach().cpu().numpy() if v.grad is not None else None
        if hdr:
            res["d_exposure"] = exposure.grad.detach().cpu().numpy()
            res["d_crf_table"] = crf.grad.detach().cpu().numpy()
    torch.cuda.synchronize()
    return res


def make_wild(sc: S.Scene, rng) -> S.Scene:
    """Perturbs a synthetic scene (whose Gaussians are all in view, sigma 0.5-8 px) into the cases a real one has:
    Gaussians behind the camera or closer than the 0.2 cull distance, far outside the image, huge and minute ones,
    fully transparent and fully opaque ones, and exact duplicates (equal depth keys: the stable sort order decides)."""
    P = sc.means3D.shape[0]
    if P < 8:
        return sc
    pick = lambda frac: torch.from_numpy(rng.random(P) < frac)
    m = pick(0.08); sc.means3D[m, 2] = -sc.means3D[m, 2]                       # behind the camera
    m = pick(0.05); sc.means3D[m, 2] = torch.from_numpy(rng.uniform(0.0, 0.25, int(m.sum())).astype(np.float32))
    m = pick(0.08); sc.means3D[m, 0] *= float(rng.uniform(3.0, 20.0))          # far off to the side
    m = pick(0.08); sc.scales[m] *= float(rng.uniform(10.0, 40.0))             # covers a large part of the image
    m = pick(0.08); sc.scales[m] *= 0.01                                        # far below a pixel
    m = pick(0.05); sc.opacities[m] = 0.0
    m = pick(0.05); sc.opacities[m] = 1.0
    m = pick(0.10)
    src = torch.from_numpy(rng.integers(0, P, P))
    for name in ("means3D", "scales", "rotations"):                            # duplicates: same geometry, own colour
        t = getattr(sc, name)
        t[m] = t[src[m]]
    return sc


def sweep_case(rng, case: int) -> dict:
    """One configuration of the randomized sweep (test_randomized_configurations_vs_oracle, scripts/sweep_case.py): every
    draw from `rng` a case makes happens here, so a script can replay case k of a seed by calling this k + 1 times."""
    P = int(rng.integers(1, 3000))
    W, H = int(rng.integers(17, 230)), int(rng.integers(17, 170))
    deg = int(rng.integers(0, 4))
    n_poses = int(rng.integers(1, 4))
    hdr = bool(rng.integers(0, 2))
    seed = int(rng.integers(0, 1000))
    act = ("relu_shift", "relu_shift", "relu_shift", "exp", "softplus")[int(rng.integers(0, 5))]
    dom = "hdr" if int(rng.integers(0, 3)) == 0 else "ldr"
    what = f"case {case}: P={P} {W}x{H} deg={deg} poses={n_poses} hdr={hdr} seed={seed} act={act} dom={dom}"
    sc = S.make_scene(P, W, H, deg, seed=seed, hdr=hdr)
    if act == "exp":
        sc.shs[:, 0] *= 0.25   # keep e^s inside a sane range (and inside the CRF table's for most Gaussians)
    if int(rng.integers(0, 2)):
        sc.bg = torch.from_numpy(rng.random(3).astype(np.float32))     # background colour (default of the scenes: 0)
    if int(rng.integers(0, 3)) == 0:
        sc.scale_modifier = float(rng.uniform(0.5, 1.5))               # the published settings' global scale factor
    wild = int(rng.integers(0, 3)) == 0
    if wild:
        sc = make_wild(sc, rng)
    deep = int(rng.integers(0, 4)) == 0
    if deep:
        sc.opacities *= float(rng.uniform(0.02, 0.1))   # faint layers: long contributor lists, no early termination
    if int(rng.integers(0, 4)) == 0:
        sc.antialias = True                                            # newer published rasterizer: opacity compensation
    precomp = int(rng.integers(0, 5)) == 0                             # colours and 3D covariances handed in directly
    what += (f" bg={[round(float(v), 2) for v in sc.bg]} mod={getattr(sc, 'scale_modifier', 1.0):.2f} "
             f"aa={getattr(sc, 'antialias', False)} precomp={precomp} wild={wild} deep={deep}")
    cams = S.blur_poses(W, H, n_poses, step=0.03) if n_poses > 1 else None
    colors = None
    if precomp and not (hdr or n_poses > 1):   # (precomputed inputs are exercised on the single-pose linear path)
        colors = torch.from_numpy(rng.random((P, 3)).astype(np.float32))
    return dict(P=P, W=W, H=H, deg=deg, n_poses=n_poses, hdr=hdr, seed=seed, act=act, dom=dom, sc=sc, cams=cams,
                precomp=precomp, colors=colors, what=what)


def optional_outputs_case(rng, c: dict) -> dict:
    """What a case of the optional-outputs sweep (tests/test_optional_outputs_gpu.py) draws AFTER sweep_case(rng, case) gave
    `c`: which of the inverse-depth and accumulated-opacity outputs carry an upstream gradient (0: inverse depth, 1: opacity,
    2: both) and those gradients, N(0, 1) x 3 -- the same order of magnitude as the colour's.  Kept out of sweep_case so that
    the draws of the existing sweep do not move."""
    which = int(rng.integers(0, 3))
    gD = (rng.standard_normal((c["H"], c["W"])) * 3.0).astype(np.float32)
    gA = (rng.standard_normal((c["H"], c["W"])) * 3.0).astype(np.float32)
    names = ("invdepth", "alpha", "invdepth+alpha")[which]
    return dict(which=names, invdepth_grad=gD if which != 1 else None, alpha_grad=gA if which != 0 else None,
                what=c["what"] + f" outputs={names}")


def oracle_camera(O, sc: S.Scene, cam=None, radiance_activation="relu_shift"):
    cam = cam or sc.camera
    oc = O.Camera(cam.W, cam.H, cam.tanfovx, cam.tanfovy, cam.viewmatrix.numpy(), cam.projmatrix.numpy(),
                  cam.campos.numpy(), sc.bg.numpy(), float(getattr(sc, "scale_modifier", 1.0)), sc.sh_degree,
                  radiance_activation=radiance_activation)
    oc.antialias = bool(getattr(sc, "antialias", False))
    return oc


def run_oracle(O, sc: S.Scene, cam=None, dL=None, backward=True, use_cov_precomp=None, use_colors_precomp=None,
               radiance_activation="relu_shift", bounds=False, dL_invdepth=None, dL_alpha=None):
    """Single-pose LDR/linear render through the C oracle (a4..a12); `dL_invdepth` / `dL_alpha` [H,W]: gradients on the
    inverse-depth and accumulated-opacity images next to the colour's."""
    ocam = oracle_camera(O, sc, cam, radiance_activation)
    kw = {}
    if use_colors_precomp is not None:
        kw["colors_precomp"] = use_colors_precomp.numpy()
    else:
        kw["shs"] = sc.shs.numpy()
    if use_cov_precomp is not None:
        kw["cov3D_precomp"] = use_cov_precomp.numpy()
    else:
        kw["scales"] = sc.scales.numpy()
        kw["rotations"] = sc.rotations.numpy()
    f = O.forward(ocam, sc.means3D.numpy(), sc.opacities.numpy(), **kw)
    b = None
    if backward:
        dL = sc.dL_dimage.numpy() if dL is None else dL
        b = O.backward(ocam, f, dL, sc.means3D.numpy(), bounds=bounds, dL_dinvdepth_img=dL_invdepth, dL_dalpha_img=dL_alpha,
                       **kw)
    return f, b


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rel_err(got, ref, floor):
    """max |got-ref| / max(|ref|, floor) and the fraction of elements above 1e-4 of that measure."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    e = np.abs(got - ref) / np.maximum(np.abs(ref), floor)
    return float(e.max()) if e.size else 0.0, float((e > 1e-4).mean()) if e.size else 0.0


def grad_floor(ref):
    """Absolute floor for relative comparison of a gradient tensor: 1e-3 of its RMS.  An fp32 sum of
    many signed per-pixel terms carries an absolute error proportional to the magnitude of the terms,
    not of the (possibly cancelling) total, so elements far below the tensor's scale are compared
    against the scale."""
    ref = np.asarray(ref, np.float64)
    rms = float(np.sqrt((ref ** 2).mean())) if ref.size else 0.0
    return max(1e-3 * rms, 1e-30)


def _pose_map(fn, items, workers):
    """fn over the poses, in order; `workers` > 1: on that many threads (the C oracle holds no global state and ctypes
    releases the interpreter lock for the duration of a call -- full-size frames, 12 s per pose and direction)."""
    items = list(items)
    if workers <= 1 or len(items) <= 1:
        return [fn(x) for x in items]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(workers, len(items))) as ex:
        return list(ex.map(fn, items))


def run_oracle_hdr(O, sc: S.Scene, cameras=None, blur_domain="ldr", dL_ldr=None, dL_hdr=None,
                   radiance_activation="relu_shift", workers=1, fwds=None, bounds=False, dL_invdepth=None, dL_alpha=None):
    """HDR image formation with the C oracle: per pose H_k (a4..a9), tone-map (a15), average over poses;
    backward chains tonemap_bwd into the rasterizer backward per pose and sums (in pose order, whatever `workers`).
    Returns dict of outputs and gradients (numpy).
    `dL_invdepth` / `dL_alpha` [H,W]: gradients on the frame's inverse-depth / accumulated-opacity image; both images are
    the mean over the poses (rasterizer.py), so every pose's backward takes 1 / N of them."""
    cams = cameras or [sc.camera]
    N = len(cams)
    share = lambda g: None if g is None else (np.asarray(g, np.float32) / np.float32(N)).astype(np.float32)
    gD, gA = share(dL_invdepth), share(dL_alpha)
    dL_ldr = sc.dL_dimage.numpy() if dL_ldr is None else dL_ldr
    dt = float(sc.exposure)
    tab = sc.crf_table.numpy()
    umin, umax = sc.crf_range
    # (`fwds`: the forwards of an earlier call on the same scene and cameras -- a second backward with another dL;
    #  `bounds`: sum |terms| next to every gradient element, O.backward(bounds=True), summed over the poses)
    fs = fwds if fwds is not None else _pose_map(
        lambda c: run_oracle(O, sc, cam=c, backward=False, radiance_activation=radiance_activation)[0], cams, workers)
    Hs = [f["color"] for f in fs]
    Hm = np.mean(np.stack(Hs), axis=0, dtype=np.float64).astype(np.float32)
    if blur_domain == "ldr":
        ldr = np.mean(np.stack([O.tonemap_fwd(h, dt, tab, umin, umax) for h in Hs]), axis=0, dtype=np.float64).astype(np.float32)
    else:
        ldr = O.tonemap_fwd(Hm, dt, tab, umin, umax)
    out = {"ldr": ldr, "hdr": Hm, "fwd": fs}
    gsum, dtab_sum, dexp_sum = None, np.zeros_like(tab, dtype=np.float64), 0.0
    if blur_domain == "hdr":
        dHm, dtab, dexp = O.tonemap_bwd(Hm, dt, tab, umin, umax, dL_ldr)
        dtab_sum += dtab
        dexp_sum += dexp
    keys = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dshs", "dL_dscales", "dL_drots"]

    def pose_backward(k):
        if blur_domain == "ldr":
            dH, dtab, dexp = O.tonemap_bwd(Hs[k], dt, tab, umin, umax, dL_ldr / N)
        else:
            dH, dtab, dexp = dHm / N, None, 0.0
        if dL_hdr is not None:
            dH = dH + dL_hdr / N
        ocam = oracle_camera(O, sc, cams[k], radiance_activation)
        b = O.backward(ocam, fs[k], dH.astype(np.float32), sc.means3D.numpy(), shs=sc.shs.numpy(),
                       scales=sc.scales.numpy(), rotations=sc.rotations.numpy(), bounds=bounds, dL_dinvdepth_img=gD,
                       dL_dalpha_img=gA)
        return {q: b[q] for q in keys + ((["abs_" + q for q in keys] + ["n_terms"]) if bounds else [])}, dtab, dexp

    for b, dtab, dexp in _pose_map(pose_backward, range(N), workers):
        if dtab is not None:
            dtab_sum += dtab
            dexp_sum += dexp
        if gsum is None:
            gsum = {q: b[q].astype(np.float64) for q in b}
        else:
            for q in b:
                gsum[q] += b[q]
    out.update({q: (v.astype(np.float32) if q != "n_terms" else v.astype(np.int64)) for q, v in gsum.items()})
    out["dL_dcrf_table"] = dtab_sum.astype(np.float32)
    out["dL_dexposure"] = float(dexp_sum)
    return out


GRAD_KEYS = [("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"),
             ("shs", "dL_dshs"), ("scales", "dL_dscales"), ("rotations", "dL_drots")]


# The gradient contract (profiles/r02_parity_table.json, scripts/parity_table.py): on identical decisions the HIP path
# and the fp32 C oracle are equally far from the float64 autograd truth (relative L2 2-5e-6, 99.9th percentile 2-7e-4,
# worst element up to 1e-2 of max(|x|, 1e-3 RMS) -- the fp32 conditioning of the T / (1 - alpha) recurrences), and
# within a few 1e-4 of each other.  Bars below = those measurements with headroom, not round numbers.
STRICT = dict(frac_tol=1e-2, max_tol=1e-2, l2_tol=1e-5)  # measured: frac <= 6e-3, max <= 3e-3, l2 <= 1e-6 (HIP vs C)
# ... tensors of >= 5000 rows (Gaussians): the bar the measurements allow there (round 6, the whole suite
# with HS_PARITY_REPORT=1: worst fraction beyond 1e-4 9.7e-4, worst element 5.8e-3 -- 100 000 Gaussians at 800 x 800 --,
# relative L2 <= 3.2e-6).  A few thousand elements and more give the fraction its meaning; below that the two-element
# escape of assert_grads_close and the wider STRICT stay.
STRICT_LARGE = dict(frac_tol=2e-3, max_tol=6e-3, l2_tol=5e-6)
LARGE_ROWS = 5000
# Rows (Gaussians) that leave the strict bar -- ONLY those reached by a pixel on which the two implementations
# demonstrably decided differently (decision_masks: contributor count or transmittance differs, which must itself lie
# inside the oracle's threshold guard band), or by a pixel within rounding distance of a CRF knot (the interval, hence
# the slope dL/dH is multiplied with, is the one decision no output reveals).  One flipped contribution is at most
# alpha = 1/255 of a pixel term (a skip) or T < 1e-2 of one (a termination), a neighbouring CRF slope a few per cent of
# one: bounded per element by 10 x max(|ref|, 1e-3 RMS) -- i.e. 1e-2 of the tensor's RMS for elements below the floor --
# and together by the L2 share of the tensor they may change (measured on the MI355X over the fixed tests and ~5000
# configurations of the sweep: worst element 6.8 -- a termination flip, T < 1e-2 of a pixel term against the floor, in a
# "deep" scene of faint layers whose opacity gradients are large --, L2 1.1e-3 -- clouds of a few hundred Gaussians, where
# the rows of one flipped pixel are a large part of the tensor).  No bound on the fraction WITHIN those rows (a flipped pixel changes every Gaussian along
# it), but the rows themselves must stay few: `min_strict`.
AT_RISK = dict(frac_tol=1.0, max_tol=10.0, l2_tol=5e-3)


def assert_grads_close(got: dict, ref: dict, keys=GRAD_KEYS, frac_tol=None, max_tol=None, l2_tol=None, what="",
                       at_risk=None, min_strict=None):
    """Gradient parity against the oracle.  Per tensor: the fraction of elements beyond 1e-4 relative (floor 1e-3 *
    tensor RMS) <= frac_tol, the worst element <= max_tol, relative L2 <= l2_tol (defaults: STRICT).  `at_risk`: bool
    [P] (decision_masks()["rows"]) -- those Gaussians (rows) are held to AT_RISK instead, all others to the strict
    bar; without it every row is strict.  `min_strict`: the share of rows that must be on the strict bar."""
    def bar_for(rows_total):
        b = dict(STRICT_LARGE if rows_total >= LARGE_ROWS else STRICT)
        for k, v in (("frac_tol", frac_tol), ("max_tol", max_tol), ("l2_tol", l2_tol)):
            if v is not None:
                b[k] = v
        return b
    report = {}
    if at_risk is not None:
        report["strict_share"] = 1.0 - float(at_risk.mean()) if at_risk.size else 1.0
        if min_strict is not None:
            assert report["strict_share"] >= min_strict, (what, "rows on the strict bar", report["strict_share"])
    if os.environ.get("HS_PARITY_REPORT") and at_risk is not None:
        print("SHARE", what, os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], round(report["strict_share"], 4), "min_strict", min_strict, flush=True)
    for gk, rk in keys:
        r = np.asarray(ref[rk])
        g = np.asarray(got["d_" + gk]).reshape(r.shape)
        floor = grad_floor(r)
        bar = bar_for(r.shape[0] if r.ndim else 1)
        parts = [("", slice(None), bar)]
        if at_risk is not None and at_risk.any() and r.shape[0] == at_risk.shape[0]:
            parts = [("[clear]", ~at_risk, bar), ("[at risk]", at_risk, AT_RISK)]
        for tag, rows, b in parts:
            rr, gg = r[rows], g[rows]
            if rr.size == 0:
                continue
            mx, frac = rel_err(gg, rr, floor)
            d2 = ((gg.astype(np.float64) - rr) ** 2).reshape(rr.shape[0], -1).sum(axis=1)
            # The L2 bar judges the FULL tensor.  One exception, narrowly: a Gaussian that covers the whole frame sums
            # thousands of random-sign pixel terms, and an fp32 sum of n such terms is off by ~1e-7 sqrt(n) of their
            # magnitude -- 1e-4 of the row, which then IS the tensor's L2 error when the row is also its largest (sweep seed
            # 24 case 9: radius 2738 px, 1.2e-4 on that row, one-list and two-group kernel alike).  Only THAT case is
            # excused: the row holding more than half of the squared error must be the largest row of the reference and
            # must itself be within 3e-4 of its own norm (a wrong slot or plane for one entry is a per-cent error of the
            # row, not 1e-4) -- then the L2 bar judges the rest; any other single-row error stays in the L2.
            if d2.size > 1 and d2.max() > 0.5 * d2.sum():
                k = int(d2.argmax())
                n2 = (rr.astype(np.float64) ** 2).reshape(rr.shape[0], -1).sum(axis=1)
                if k == int(n2.argmax()) and d2[k] <= (3e-4 ** 2) * n2[k]:
                    if os.environ.get("HS_PARITY_REPORT"):
                        print("L2_EXEMPTION", what, gk + tag, os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], flush=True)
                    d2 = np.delete(d2, k)
            l2 = float(np.sqrt(d2.sum()) / max(np.linalg.norm(r.astype(np.float64)), 1e-30))
            report[gk + tag] = (mx, frac, l2)
            # the fraction bound always admits two elements (tensors of a few dozen entries: P down to 1 in the sweep)
            frac_ok = frac <= max(b["frac_tol"], 2.0 / rr.size)
            # ... and the L2 bar of a tensor of n elements is no tighter than 1e-4 / sqrt(n): for a handful of elements the
            # relative L2 IS the relative error of single fp32 sums (n = 1: one Gaussian's gradient, hundreds of terms)
            l2_ok = l2 <= max(b["l2_tol"], 1e-4 / np.sqrt(rr.size))
            assert frac_ok and mx <= b["max_tol"] and l2_ok, (what, gk + tag, mx, frac, l2)
    if os.environ.get("HS_PARITY_REPORT"):
        print("PARITY", what, {k: (tuple(float(f"{x:.3g}") for x in v) if isinstance(v, tuple) else round(v, 4))
                               for k, v in report.items()}, flush=True)
    return report


def crf_region(sc: S.Scene, u32):
    """Region of the piecewise-linear CRF a log-exposure u (float32 array) falls into, with exactly the fp32 operations of
    the kernels and the oracle (a15: s = (u - umin) / (umax - umin) * (K - 1)): -1 below the table, K - 1 above it
    (slope zero there), else the interval index min(floor(s), K - 2)."""
    K = sc.crf_table.shape[1]
    umin, umax = np.float32(sc.crf_range[0]), np.float32(sc.crf_range[1])
    sv = (np.asarray(u32, np.float32) - umin) / (umax - umin) * np.float32(K - 1)
    idx = np.minimum(np.floor(sv), K - 2).astype(np.int64)
    idx = np.where(sv > 0, idx, -1)
    return np.where(sv >= K - 1, K - 1, idx)


def crf_interval_risk(sc: S.Scene, hdr_got, hdr_ref, ulps=4):
    """bool [H,W]: pixels whose CRF interval -- hence the slope dL/dH is multiplied with, a piecewise-constant decision
    like the alpha / T thresholds -- is not provably the same in both implementations.  The interval is a monotone fp32
    function of u = ln(H dt); the two sides differ (i) in H (observable: both radiance images are compared here) and
    (ii) in ln() itself (v_log_f32 * ln 2 on the GPU, glibc logf in the oracle: within ~2 ulp of each other, NOT
    observable -- the CRF is continuous across a knot, no output reveals the interval).  So: at risk = the region of
    u(H_hip) differs from that of u(H_oracle), or either u lies within `ulps` ulp of a region boundary (evaluated with
    the kernels' own fp32 arithmetic, crf_region).  About 1e-4 of the pixels -- a quarter of the fixed 2e-4-knot band
    of round 2."""
    dt = np.float32(float(sc.exposure))

    def u_of(h):
        x = np.asarray(h, np.float32) * dt
        return np.log(np.maximum(x, np.float32(1e-8)))

    def ambiguous(u):
        step = np.spacing(np.abs(u)).astype(np.float32) * np.float32(ulps)
        return crf_region(sc, u + step) != crf_region(sc, u - step)

    ug, ur = u_of(hdr_got), u_of(hdr_ref)
    return ((crf_region(sc, ug) != crf_region(sc, ur)) | ambiguous(ug) | ambiguous(ur)).any(axis=0)


def oracle_risk(O, sc: S.Scene, fwds, cams=None, guard_alpha=1e-5, guard_T=5e-5, workers=1, conditioned=None):
    """Union over the poses of oracle.threshold_risk: (pix_risk [N,H,W], gauss_risk [P]) -- the guard band of the frame:
    where another fp32 implementation MAY decide differently.  Which rows actually leave the strict gradient bar is
    decided by decision_masks (where it DID).
    conditioned=k: the band widened by k 2^-24 M per (pixel, entry) (oracle.threshold_risk(conditioned=k)), and a third
    result: dict(T_tol [N,H,W], color_tol [N,3,H,W], max_M, power_c) -- the per-pixel bounds under identical decisions."""
    cams = cams or [sc.camera]
    pix, gs = [], None
    if conditioned is not None:
        rs = _pose_map(lambda cf: O.threshold_risk(oracle_camera(O, sc, cf[0]), cf[1], guard_alpha, guard_T,
                                                   conditioned=conditioned), zip(cams, fwds), workers)
        for r in rs:
            gs = r["gauss_risk"] if gs is None else (gs | r["gauss_risk"])
        tol = dict(T_tol=np.stack([r["T_tol"] for r in rs]), color_tol=np.stack([r["color_tol"] for r in rs]),
                   max_M=max(r["max_M"] for r in rs), power_c=max(r["power_c"] for r in rs))
        return np.stack([r["pix_risk"] for r in rs]), gs, tol
    for r in _pose_map(lambda cf: O.threshold_risk(oracle_camera(O, sc, cf[0]), cf[1], guard_alpha, guard_T),
                       zip(cams, fwds), workers):
        pix.append(r["pix_risk"])
        gs = r["gauss_risk"] if gs is None else (gs | r["gauss_risk"])
    return np.stack(pix), gs


# A pixel whose T_tol (oracle.threshold_risk(conditioned=k): the relative difference identical decisions may leave in final_T)
# exceeds this cannot be classified: ONE flipped contributor moves T by at least 1/255 = 3.9e-3, so the threshold that tells
# a flip from rounding, 2e-3 + T_tol, has to stay below that.
T_TOL_CLASSIFIABLE = 1.5e-3


def decision_masks(O, sc: S.Scene, fwds, st, cams=None, crf_got=None, crf_ref=None, what="", workers=1, conditioned=None):
    """Where the HIP path (`st`: inspect_state as numpy) and the oracle (`fwds`: one forward dict per pose) took
    different decisions, and which gradient rows that excuses.
      differs [N,H,W]  pixels whose contributor count differs or whose final transmittance is off by more than 2e-3
                       relative (identical decisions leave T within ~2e-4: fp32 products of (1 - alpha <= 0.99); ONE
                       skipped or extra contributor changes it by >= 1/255).  Asserted to lie inside the oracle's
                       threshold guard band (pix_risk): a difference anywhere else is a bug, not rounding.
      rows [P]         Gaussians on the tile lists of those pixels that either implementation may have blended there
                       (oracle.pixel_reach(whole_list=True)), plus -- crf_got / crf_ref: lists of the radiance images
                       the CRF is applied to, per pose or ONE mean image -- the oracle's contributors of the pixels
                       whose CRF interval is not provably the same (crf_interval_risk).
    Everything else is held to the STRICT gradient bar.
    conditioned=k (ill-conditioned footprints -- needles, discs seen edge-on; None: everything above, unchanged): the band is
    the conditioned one, the transmittance test becomes |dT| > (2e-3 + T_tol) |T| with the pixel's own T_tol, and the pixels
    whose T_tol exceeds T_TOL_CLASSIFIABLE -- where that test can no longer tell a flip from rounding -- are set aside up
    front: `unclassifiable` [N,H,W] / `n_unclassifiable`, part of `excluded`, not of `differs` (a differing contributor
    COUNT is still observable on them and must lie inside the band like any other).  Also returned: T_tol, color_tol."""
    cams = cams or [sc.camera]
    tol = None
    if conditioned is not None:
        pix_risk, _, tol = oracle_risk(O, sc, fwds, cams, workers=workers, conditioned=conditioned)
        unclass = tol["T_tol"] > T_TOL_CLASSIFIABLE
    else:
        pix_risk, _ = oracle_risk(O, sc, fwds, cams, workers=workers)
    P = fwds[0]["radii"].shape[0]
    rows = np.zeros(P, bool)
    differs = np.zeros_like(pix_risk)
    for k, (cam, f) in enumerate(zip(cams, fwds)):
        nc = np.asarray(st["n_contrib"][k]).astype(np.int64) & 0xFFFFFFFF
        Tg, Tr = np.asarray(st["final_T"][k], np.float64), np.asarray(f["final_T"], np.float64)
        if tol is not None:
            count = nc != f["n_contrib"].astype(np.int64)
            d = count | ((np.abs(Tg - Tr) > (2e-3 + tol["T_tol"][k]) * np.abs(Tr)) & ~unclass[k])
            out = d & ~pix_risk[k]
            assert not out.any(), (what, "pose", k, "a decision differs OUTSIDE the conditioned guard band", int(out.sum()),
                                   [tuple(int(v) for v in yx) for yx in np.argwhere(out)[:8]])
            d = d & ~unclass[k]
            differs[k] = d
            if d.any():
                rows |= O.pixel_reach(oracle_camera(O, sc, cam), f, d, whole_list=True, conditioned=conditioned)
            continue
        d = (nc != f["n_contrib"].astype(np.int64)) | (np.abs(Tg - Tr) > 2e-3 * np.abs(Tr))
        assert not (d & ~pix_risk[k]).any(), (what, "pose", k, "a decision differs OUTSIDE the guard band", int((d & ~pix_risk[k]).sum()))
        differs[k] = d
        if d.any():
            rows |= O.pixel_reach(oracle_camera(O, sc, cam), f, d, whole_list=True)
    n_knot = 0
    knot = np.zeros_like(differs)
    if crf_ref is not None:
        per_pose = len(crf_ref) == len(fwds)
        for k, (cam, f) in enumerate(zip(cams, fwds)):
            j = k if per_pose else 0
            m = crf_interval_risk(sc, crf_got[j], crf_ref[j])
            knot[k] = m
            n_knot += int(m.sum())
            if m.any():
                rows |= O.pixel_reach(oracle_camera(O, sc, cam), f, m)
    # excluded [H,W]: the pixels of the FRAME (any pose) on which a decision differed or a CRF interval is not provably the
    # same -- a backward whose dL is zero there (both sides) involves identical decisions only: masked_backward_pass
    if tol is not None:
        return dict(pix_risk=pix_risk, differs=differs, knot=knot, rows=rows, n_differ=int(differs.sum()), n_knot_pixels=n_knot,
                    excluded=differs.any(axis=0) | knot.any(axis=0) | unclass.any(axis=0), unclassifiable=unclass,
                    n_unclassifiable=int(unclass.sum()), T_tol=tol["T_tol"], color_tol=tol["color_tol"], max_M=tol["max_M"],
                    k=float(conditioned))
    return dict(pix_risk=pix_risk, differs=differs, knot=knot, rows=rows, n_differ=int(differs.sum()), n_knot_pixels=n_knot,
                excluded=differs.any(axis=0) | knot.any(axis=0))


def check_image_conditioned(got, ref, masks, tol, what, pose=0, floor=1e-2):
    """check_image for ill-conditioned footprints (masks = decision_masks(conditioned=k)): off the pixels of this pose where a
    decision differed or that cannot be classified, EVERY value within 1e-4 max(|ref|, floor) + tol -- `tol` [H,W] or [3,H,W],
    the oracle's own per-pixel bound under identical decisions (masks["color_tol"][pose] for the colour,
    masks["T_tol"][pose] * |final_T| for the transmittance).  Returns the largest excess over the 1e-4 term in units of tol."""
    off = masks["differs"][pose] | masks["unclassifiable"][pose]
    got, ref, tol = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(tol, np.float64)
    excess = np.abs(got - ref) - 1e-4 * np.maximum(np.abs(ref), floor)
    bad = (excess > tol) & ~(off[None] if got.ndim == 3 else off)
    assert not bad.any(), (what, "values beyond 1e-4 max(|ref|, floor) + the conditioned bound", int(bad.sum()),
                           float((excess - tol)[bad].max()))
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where((excess > 0) & ~(off[None] if got.ndim == 3 else off), excess / tol, 0.0)
    return float(np.nan_to_num(share, posinf=np.inf).max())


def crf_grads_given_decisions(O, sc: S.Scene, masks, ref_imgs, got_imgs, dL_ldr=None):
    """Oracle d(crf_table), d(exposure) of the 'ldr' blur domain (or a single pose) GIVEN the decisions the HIP path took:
    the oracle's tone-map backward run on its own radiance images, except on the pixels where a compositing decision
    demonstrably differed (masks["differs"], already confined to the guard band), where the HIP path's radiance stands
    in.  One flipped contribution moves a pixel's log-exposure by up to a third of a knot interval and with it ~|dL| of
    weight between two table entries -- 1e-2 of a knot's sum at full size, where 8000 pixels meet in a knot -- which is a
    property of the decision, not of the table-gradient kernel this comparison is about."""
    N = len(ref_imgs)
    dL = (sc.dL_dimage.numpy() if dL_ldr is None else dL_ldr) / N
    dt, tab, (umin, umax) = float(sc.exposure), sc.crf_table.numpy(), sc.crf_range
    dtab, dexp = np.zeros_like(tab, dtype=np.float64), 0.0
    for k in range(N):
        h = np.where(masks["differs"][k][None], np.asarray(got_imgs[k], np.float32), np.asarray(ref_imgs[k], np.float32))
        _, t, e = O.tonemap_bwd(np.ascontiguousarray(h), dt, tab, umin, umax, dL)
        dtab += t
        dexp += e
    return dtab.astype(np.float32), float(dexp)


def guarded_scene(O, P, W, H, deg, seed=0, hdr=False, cams_fn=None, tries=2000, **kw):
    """First scene with seed >= `seed` whose frame(s) have NO pixel inside the threshold guard band (SURVEY.md 7.4-3:
    fixtures are reject-sampled so that every fp32 implementation takes identical skip / termination decisions)."""
    for s_ in range(seed, seed + tries):
        sc = S.make_scene(P, W, H, deg, seed=s_, hdr=hdr, **kw)
        cams = cams_fn(W, H) if cams_fn else [sc.camera]
        ok = True
        for cam in cams:
            f, _ = run_oracle(O, sc, cam=cam, backward=False)
            if O.threshold_risk(oracle_camera(O, sc, cam), f, 2e-5, 1e-4)["n_risky_pixels"]:
                ok = False
                break
        if ok:
            return sc, s_
    raise RuntimeError("no guard-banded seed found")


# ---------------------------------------------------------------------------------------------------------------------
# Closing the allowances.  (a) A second backward with dL ZEROED on the pixels where a decision
# demonstrably differed and on the CRF-knot pixels, on both sides: every term of every gradient then comes from a pixel on
# which HIP path and oracle took identical decisions, so NO row is excused -- every Gaussian is held to the strict bar.
# (b) A bound per ELEMENT instead of "at most x % of the elements beyond 1e-4": the oracle returns, next to every
# gradient element, S = sum w |term| (O.backward(bounds=True): every per-pixel term with the differences inside it replaced
# by sums of absolute values and weighted by w = 4 + the number of T / (1 - alpha) steps the replay took before it -- each
# step costs T an ulp, and T multiplies the term --, carried through the linear a11 / a12 by |Jacobian|).  An fp32
# evaluation of the same sum in any order, with v_exp_f32 / v_rcp_f32 in place of expf / a division, stays within
#       |hip - ref| <= 1e-4 |ref| + C_BOUND * 2^-24 * S
# -- one constant for every tensor, size and configuration; ZERO elements outside.  (The form VERDICT r4 suggested,
# c 2^-24 sqrt(n) sum |term| without the depth weight, needs c > 200 at c2 and grows with the length of the tile lists: a
# Gaussian seen by a handful of pixels deep inside long lists has a small n and terms whose T went through a hundred
# divisions.)  C_BOUND is measured, not derived: profiles/r05_parity_table.json records the largest
# (|hip - ref| - 1e-4 |ref|) / (2^-24 S) of every frame.
# ---------------------------------------------------------------------------------------------------------------------
C_BOUND = 8.0


def assert_grads_bounded(got: dict, ref: dict, keys=GRAD_KEYS, c=C_BOUND, what="", rows=None, conditioned=None):
    """Per-element bound |hip - ref| <= 1e-4 |ref| + c 2^-24 sum w|term| on EVERY element of every tensor; `ref` comes
    from run_oracle / run_oracle_hdr(bounds=True).  `rows`: bool [P] -- only those Gaussians are held to it (the clear rows
    of a first pass, ~decision_masks()["rows"]: every pixel they were blended on took identical decisions on both sides).
    Returns {tensor: (n_outside, c_needed)}.
    conditioned=k (`ref` from O.backward(bounds=True, conditioned=True)): the bound gains k 2^-24 cond, cond = the same
    magnitudes weighted by M_i + T_units(pixel) -- |hip - ref| <= 1e-4 |ref| + c 2^-24 abs + k 2^-24 cond; returns
    {tensor: (n_outside, c_needed, k_needed)}, each constant the one its term would need with the other at its set value."""
    if conditioned is not None:
        return _assert_grads_bounded_conditioned(got, ref, keys, c, float(conditioned), what, rows)
    rep = {}
    for gk, rk in keys:
        r = np.asarray(ref[rk], np.float64)
        g = np.asarray(got["d_" + gk], np.float64).reshape(r.shape)
        S = np.asarray(ref["abs_" + rk], np.float64).reshape(r.shape)
        if rows is not None:
            r, g, S = r[rows], g[rows], S[rows]
        unit = 2.0 ** -24 * S
        excess = np.abs(g - r) - 1e-4 * np.abs(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            need = np.where(excess > 0, excess / unit, 0.0)
        need = np.where(np.isfinite(need), need, np.where(excess > 0, np.inf, 0.0))
        n_out = int((excess > c * unit).sum())
        rep[gk] = (n_out, float(need.max()) if need.size else 0.0)
    if os.environ.get("HS_PARITY_REPORT"):
        print("BOUND", what, {k: (v[0], round(v[1], 2)) for k, v in rep.items()}, flush=True)
    bad = {k: v for k, v in rep.items() if v[0]}
    assert not bad, (what, "elements outside 1e-4 |ref| + c 2^-24 sum w|term|, c =", c, bad)
    return rep


def _assert_grads_bounded_conditioned(got, ref, keys, c, k, what, rows):
    def needed(excess, unit):
        with np.errstate(divide="ignore", invalid="ignore"):
            need = np.where(excess > 0, excess / unit, 0.0)
        need = np.where(np.isfinite(need), need, np.where(excess > 0, np.inf, 0.0))
        return float(need.max()) if need.size else 0.0
    rep = {}
    for gk, rk in keys:
        r = np.asarray(ref[rk], np.float64)
        g = np.asarray(got["d_" + gk], np.float64).reshape(r.shape)
        S = np.asarray(ref["abs_" + rk], np.float64).reshape(r.shape)
        Sc = np.asarray(ref["cond_" + rk], np.float64).reshape(r.shape)
        if rows is not None:
            r, g, S, Sc = r[rows], g[rows], S[rows], Sc[rows]
        ua, uc = 2.0 ** -24 * S, 2.0 ** -24 * Sc
        excess = np.abs(g - r) - 1e-4 * np.abs(r)
        rep[gk] = (int((excess > c * ua + k * uc).sum()), needed(excess - k * uc, ua), needed(excess - c * ua, uc))
    if os.environ.get("HS_PARITY_REPORT"):
        print("BOUND_COND", what, {q: (v[0], round(v[1], 2), round(v[2], 2)) for q, v in rep.items()}, flush=True)
    bad = {q: v for q, v in rep.items() if v[0]}
    assert not bad, (what, "elements outside 1e-4 |ref| + c 2^-24 abs + k 2^-24 cond, c, k =", c, k, bad)
    return rep


def crf_grad_bound(sc: S.Scene, ref_imgs, dL_ldr, c=6.0):
    """Per-entry bound of d(crf_table) [3,K]: `ref_imgs` are the radiance images the CRF is applied to -- one per pose in the
    'ldr' blur domain (each takes dL / N), the ONE mean image in the 'hdr' domain or for a single pose (it takes dL).
    1e-4 |ref| is added by the caller;
    this is what the two implementations may differ by on identical decisions,
        c * (sigma_q sqrt(n_k) + delta_f sqrt(sum g^2)_k),
    n_k / (sum g^2)_k over the (pixel, pose) terms that touch entry k (a pixel between knots i, i + 1 adds (1 - f) g and
    f g to them): sigma_q = q / sqrt(12) with q = 2^-18 max|g| -- the kernel adds its terms as fixed point with a step of
    at most 2^-18 of the block's largest |g| (render.hip, crf_grad_kernel: 19 bits below a power of two >= max|g|) --
    and delta_f = 4 ulp of the log-exposure u times (K - 1) / (umax - umin): v_log_f32 * ln 2 against glibc logf moves a
    pixel's interval weight f by that much.  c = 6: a six-sigma statistical bound on a sum of independent roundings."""
    N = len(ref_imgs)
    K = sc.crf_table.shape[1]
    umin, umax = float(sc.crf_range[0]), float(sc.crf_range[1])
    dt = np.float32(float(sc.exposure))
    g = np.asarray(dL_ldr, np.float64) / N
    gmax = float(np.abs(g).max())
    q = 2.0 ** -18 * gmax
    delta_f = 4 * 2.0 ** -24 * max(abs(umin), abs(umax)) * (K - 1) / (umax - umin)
    n_k = np.zeros((3, K)); s2_k = np.zeros((3, K))
    for h in ref_imgs:
        u = np.log(np.maximum(np.asarray(h, np.float32) * dt, np.float32(1e-8)))
        reg = crf_region(sc, u)
        for ch in range(3):
            inside = (reg[ch] >= 0) & (reg[ch] <= K - 2)
            idx = reg[ch][inside].ravel()
            w = g[ch][inside].ravel() ** 2
            for off in (0, 1):
                n_k[ch] += np.bincount(idx + off, minlength=K)[:K]
                s2_k[ch] += np.bincount(idx + off, weights=w, minlength=K)[:K]
    return c * (q / np.sqrt(12.0) * np.sqrt(n_k) + delta_f * np.sqrt(s2_k))


def run_oracle_poses(O, sc: S.Scene, cameras, dL, fwds, radiance_activation="relu_shift", bounds=False, workers=1,
                     use_cov_precomp=None, use_colors_precomp=None, conditioned=False, dL_invdepth=None, dL_alpha=None):
    """Backward of the non-HDR N-pose frame (the linear-radiance blur: the output is the mean of the per-pose renders) with
    the C oracle: sum over the poses, in pose order, of backward(dL / N) given each pose's forward in `fwds`; with
    `bounds`, the abs_* magnitudes (and n_terms) are summed alongside.  `dL_invdepth` / `dL_alpha` [H,W]: the inverse-depth
    and accumulated-opacity images are means over the poses too, so each pose takes 1 / N of those as well."""
    N = len(cameras)
    dLn = (np.asarray(dL, np.float32) / np.float32(N)).astype(np.float32)
    share = lambda g: None if g is None else (np.asarray(g, np.float32) / np.float32(N)).astype(np.float32)
    kw = dict(dL_dinvdepth_img=share(dL_invdepth), dL_dalpha_img=share(dL_alpha))
    if use_colors_precomp is not None:
        kw["colors_precomp"] = use_colors_precomp.numpy()
    else:
        kw["shs"] = sc.shs.numpy()
    if use_cov_precomp is not None:
        kw["cov3D_precomp"] = use_cov_precomp.numpy()
    else:
        kw.update(scales=sc.scales.numpy(), rotations=sc.rotations.numpy())

    def one(k):
        ocam = oracle_camera(O, sc, cameras[k], radiance_activation)
        if conditioned:   # (the cond_* magnitudes of O.backward(conditioned=True), summed over the poses like abs_*)
            b = O.backward(ocam, fwds[k], dLn, sc.means3D.numpy(), bounds=bounds, conditioned=True, **kw)
        else:
            b = O.backward(ocam, fwds[k], dLn, sc.means3D.numpy(), bounds=bounds, **kw)
        return {q: v for q, v in b.items() if q.startswith(("dL_d", "abs_dL_d", "cond_dL_d", "n_terms")) and isinstance(v, np.ndarray)}

    acc = None
    for b in _pose_map(one, range(N), workers):
        if acc is None:
            acc = {q: v.astype(np.float64 if q != "n_terms" else np.int64) for q, v in b.items()}
        else:
            for q in acc:
                acc[q] += b[q]
    return {q: (v.astype(np.float32) if q != "n_terms" else v) for q, v in acc.items()}


def masked_backward_pass(O, sc: S.Scene, masks, fwds, cameras=None, hdr=True, blur_domain="ldr", workers=1, what="",
                         radiance_activation="relu_shift", use_cov_precomp=None, use_colors_precomp=None, conditioned=False,
                         invdepth_grad=None, alpha_grad=None):
    """The second backward of VERDICT r4 next #2: dL zeroed on masks["excluded"] on BOTH sides (the HIP path renders and
    differentiates the frame again with the masked dL, the oracle reuses its forwards).  Returns (got, ref, dL_masked);
    the caller holds EVERY row to its bar (no at_risk) and every element to assert_grads_bounded.  Frames: HDR (one or N
    poses, either blur domain), and linear radiance of one pose (precomputed colours / covariances allowed) or of N poses
    (the mean of the per-pose renders: the oracle reference is sum_k backward(dL / N)).
    `invdepth_grad` / `alpha_grad` [H,W]: gradients on the inverse-depth / accumulated-opacity outputs, zeroed on
    masks["excluded"] on both sides like the colour's."""
    keep = (~masks["excluded"]).astype(np.float32)
    dLm = np.asarray(sc.dL_dimage.numpy(), np.float32) * keep[None]
    gD = None if invdepth_grad is None else np.asarray(invdepth_grad, np.float32) * keep
    gA = None if alpha_grad is None else np.asarray(alpha_grad, np.float32) * keep
    got = run_hip(sc, cameras=cameras, hdr=hdr, blur_domain=blur_domain, dL_image=dLm, radiance_activation=radiance_activation,
                  use_cov_precomp=use_cov_precomp, use_colors_precomp=use_colors_precomp, invdepth_grad=gD, alpha_grad=gA)
    if hdr:
        assert use_cov_precomp is None and use_colors_precomp is None and not conditioned
        ref = run_oracle_hdr(O, sc, cameras, blur_domain, dL_ldr=dLm, workers=workers, fwds=fwds, bounds=True,
                             radiance_activation=radiance_activation, dL_invdepth=gD, dL_alpha=gA)
    else:
        ref = run_oracle_poses(O, sc, cameras or [sc.camera], dLm, fwds, radiance_activation, bounds=True, workers=workers,
                               use_cov_precomp=use_cov_precomp, use_colors_precomp=use_colors_precomp, conditioned=conditioned,
                               dL_invdepth=gD, dL_alpha=gA)
    return got, ref, dLm


# ---------------------------------------------------------------------------------------------------------------------
# Ill-conditioned footprints (tests/test_anisotropy.py on the CPU, tests/test_anisotropy_gpu.py): synthetic.anisotropic_scene
# (kind, ratio, fraction, seed), 3000 Gaussians at 240 x 160, SH degree 1.  A scene is usable only if the oracle ALONE says
# so -- conditioned band <= ANISO_BAND_CAP of the pixels, unclassifiable pixels <= ANISO_UNCLASSIFIABLE_CAP (conditions on
# the scene, asserted by test_anisotropy.py; never raised) -- so the two free choices were made by rule, before any GPU run:
# the seed is the first one, counted from 0, at which the scene holds both caps (C: seed 0 has 1.8e-2 unclassifiable pixels,
# a handful of opaque 500 px needles crossing the frame centre); E's fraction was halved from 0.02, where every seed 0-5
# misses the cap (1.1e-2 - 2.8e-2), to 0.01, which keeps a radius of 1104 px.
# ---------------------------------------------------------------------------------------------------------------------
ANISO_SCENES = {"A": ("needle", 10.0, 1.0, 0), "B": ("needle", 30.0, 1.0, 0), "C": ("needle", 100.0, 0.25, 1),
                "D": ("disc", 1000.0, 0.25, 0), "E": ("needle", 1000.0, 0.01, 0)}
ANISO_BAND_CAP = 5e-3
ANISO_UNCLASSIFIABLE_CAP = 1e-2
