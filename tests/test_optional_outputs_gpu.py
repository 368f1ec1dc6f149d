"""The rasterizer's optional outputs -- expected inverse depth (return_invdepth: the DEPTH instantiation of both render
kernels, ten sums per entry in 208-byte LDS records) and accumulated opacity (return_alpha) -- and the gradients that flow back
through them, against the C oracle under the per-element error model the colour gradients are held to
(helpers.assert_grads_bounded at helpers.C_BOUND, zero elements outside).

Every case makes four checks (_hold):
  decisions      helpers.decision_masks: every difference inside the oracle's guard band;
  images         out_invdepth against the oracle's invdepth, out_alpha against 1 - final_T (both: mean over the poses), off
                 the pixels where a decision differed, within 1e-4 max(|ref|, 1e-3);
  gradients      the first pass on its clear rows, the masked pass (all three upstream gradients zeroed on the excluded
                 pixels, both sides) on every row and every element;
  instantiation  the same frame without the optional outputs: n_contrib, final_T and the colour image bit for bit.
Caps (conditions on the scene, met by the choice of seed on the CPU, never widened): clear rows >= one half, excluded pixels
<= 1 % of the frame in the fixed cases.

With HS_PARITY_REPORT=1 the largest constant any element needed goes to profiles/optional_outputs_parity.json, per case and
tensor.

Not here: n_frames > 1.  GaussianRasterizer and hs_backward refuse the optional outputs together with frames (ValueError /
HS_ERR: "per-image outputs", tests/test_frame_batch.py asserts the refusal), so there is no such launch to test.
"""
import json
import os

import numpy as np
import pytest
import torch

import helpers as Hh
from casualhdrsplat_amd import synthetic as S
from test_gpu_parity import SWEEP_BAR, assert_image_close, check_image, check_structure, environment, u32
from test_render_bwd_tile_wave import block_scene, deep_tile_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PARITY = {}
MIN_CLEAR = 0.5          # clear rows of the first pass (test_render_bwd_tile_wave.py: min_clear)
MAX_EXCLUDED = 0.01      # pixels the masked pass leaves out, fixed cases
PRECOMP_KEYS = [("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"),
                ("colors_precomp", "dL_dcolors_precomp"), ("cov3D_precomp", "dL_dcov3D")]


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    if os.environ.get("HS_PARITY_REPORT") and _PARITY:
        with open(os.path.join(ROOT, "profiles", "optional_outputs_parity.json"), "w") as fh:
            json.dump(dict(bound="|hip - ref| <= 1e-4 |ref| + C 2^-24 S; the largest C any element needs, per case and tensor "
                                 "(C_BOUND = 8): first_pass on the clear rows, masked on every row; images: the largest "
                                 "|hip - ref| / max(|ref|, 1e-3) off the pixels where a decision differed (bar 1e-4)",
                           cases=_PARITY), fh, indent=1, sort_keys=True)
            fh.write("\n")


def upstream(H, W, seed, invdepth=True, alpha=True):
    """(dL/d inverse depth, dL/d accumulated opacity) [H,W]: N(0, 1) x 5 and x 3, or None for an output that is off."""
    gen = torch.Generator().manual_seed(seed)
    gD = (torch.randn(H, W, generator=gen) * 5).numpy()
    gA = (torch.randn(H, W, generator=gen) * 3).numpy()
    return (gD if invdepth else None), (gA if alpha else None)


def _image_err(got, ref, off):
    e = np.abs(np.asarray(got, np.float64) - ref) / np.maximum(np.abs(ref), 1e-3)
    return float(e[~off].max()) if (~off).any() else 0.0


def _hold(O, sc, name, cams=None, hdr=False, dom="ldr", act="relu_shift", gD=None, gA=None, pre=None, keys=Hh.GRAD_KEYS,
          capacity_slack=None, sweep=False):
    """The four checks of this file on one frame: linear radiance of one pose (precomputed inputs allowed) or of the mean of
    N poses, or HDR + CRF in either blur domain.  `sweep`: also the structure, per-pose image and SWEEP_BAR checks of
    test_gpu_parity._sweep_case_vs_oracle, and no cap on the excluded pixels.  `capacity_slack`: fixed-capacity binning with
    room for the frame's pairs plus that many (None: the synchronous mode).  Returns what the case went through."""
    pre = pre or {}
    poses = cams or [sc.camera]
    N, P = len(poses), sc.means3D.shape[0]
    opt = dict(dL_invdepth=gD, dL_alpha=gA)
    fs = [Hh.run_oracle(O, sc, cam=c, backward=False, radiance_activation=act, **pre)[0] for c in poses]
    if hdr:
        r = Hh.run_oracle_hdr(O, sc, cams, dom, radiance_activation=act, fwds=fs, bounds=True, **opt)
    else:
        r = Hh.run_oracle_poses(O, sc, poses, sc.dL_dimage.numpy(), fs, act, bounds=True, **pre, **opt)
    capacity = None if capacity_slack is None else sum(f["R"] for f in fs) + capacity_slack
    run = dict(cameras=cams, hdr=hdr, blur_domain=dom, capacity=capacity, radiance_activation=act, **pre)
    g = Hh.run_hip(sc, invdepth_grad=gD, alpha_grad=gA, **run)
    st = g["state"]

    # 1. decisions
    crf = {}
    if hdr:
        one = dom == "hdr" or N == 1
        crf = dict(crf_got=[g["hdr"]] if one else list(st["pose_hdr"][:N]),
                   crf_ref=[r["hdr"]] if one else [f["color"] for f in fs])
    m = Hh.decision_masks(O, sc, fs, st, cams, what=name, **crf)
    clear = ~m["rows"]
    assert clear.mean() >= MIN_CLEAR, (name, "clear rows", float(clear.mean()))
    if not sweep:
        assert m["excluded"].mean() <= MAX_EXCLUDED, (name, "excluded pixels", float(m["excluded"].mean()))
    rec = _PARITY[name] = dict(clear_rows=round(float(clear.mean()), 4), excluded_pixels=int(m["excluded"].sum()),
                               contributors_max=int(max(f["n_contrib"].max() for f in fs)))
    if sweep:
        Rtot = sum(f["R"] for f in fs)
        assert st["num_rendered"] == Rtot, name
        for k, f in enumerate(fs):
            check_structure(st, f, pose=k, P=P)
            check_image(st["pose_hdr"][k] if (hdr or N > 1) else g["color"], f["color"], m, name, pose=k)
        pl = np.concatenate([f["point_list"].astype(np.int64) + k * P for k, f in enumerate(fs)])
        assert np.array_equal(u32(st["point_list"][:Rtot]), pl), name
        assert np.array_equal(g["radii"], np.max(np.stack([f["radii"] for f in fs]), axis=0)), name
        if N == 1 and not hdr:
            assert np.array_equal(u32(st["offsets"]), u32(fs[0]["offsets"])), name
            assert np.array_equal(u32(st["ranges"]), u32(fs[0]["ranges"])), name
        if hdr:
            assert_image_close(g["hdr"], r["hdr"], name)
            assert_image_close(g["color"], r["ldr"], name)
        elif N > 1:
            assert_image_close(g["color"], np.mean(np.stack([f["color"] for f in fs]), axis=0, dtype=np.float64), name)

    # 2. the two images: both are means over the poses of the frame
    off = m["differs"].any(axis=0)
    refs = dict(invdepth=np.mean(np.stack([f["invdepth"] for f in fs]), axis=0, dtype=np.float64),
                alpha=1.0 - np.mean(np.stack([f["final_T"] for f in fs]), axis=0, dtype=np.float64))
    for k, up in (("invdepth", gD), ("alpha", gA)):
        if up is not None:
            assert g[k].shape == refs[k].shape and (sweep or np.abs(refs[k]).max() > 0), (name, k)
            rec[k + "_image"] = e = _image_err(g[k], refs[k], off)
            print(name, k, "image: worst |hip - ref| / max(|ref|, 1e-3)", e, flush=True)
            assert e <= 1e-4, (name, k, "image beyond 1e-4 max(|ref|, 1e-3) where no decision differs", e)

    # 3. gradients: the first pass on its clear rows, the masked pass on every row
    if sweep:
        Hh.assert_grads_close(g, r, keys=keys, what=name, at_risk=m["rows"], **SWEEP_BAR)
    rep = Hh.assert_grads_bounded(g, r, keys=keys, what=name + " clear rows", rows=clear)
    rec["first_pass"] = {k: round(v[1], 4) for k, v in rep.items()}
    g2, r2, dLm = Hh.masked_backward_pass(O, sc, m, fs, cameras=cams, hdr=hdr, blur_domain=dom, radiance_activation=act,
                                          invdepth_grad=gD, alpha_grad=gA, what=name, **pre)
    if sweep:
        Hh.assert_grads_close(g2, r2, keys=keys, what=name + " masked", **SWEEP_BAR)
    rep = Hh.assert_grads_bounded(g2, r2, keys=keys, what=name + " masked")
    rec["masked"] = {k: round(v[1], 4) for k, v in rep.items()}
    print(name, rec, flush=True)
    if hdr:   # d_crf_table / d_exposure as the sweep holds them (test_gpu_parity._masked_pass, crf_rel = 2e-4)
        tab = np.asarray(r2["dL_dcrf_table"], np.float64)
        err = np.abs(np.asarray(g2["d_crf_table"], np.float64) - tab)
        imgs = [r2["hdr"]] if dom == "hdr" else [f["color"] for f in fs]
        bound = 1e-4 * np.abs(tab) + Hh.crf_grad_bound(sc, imgs, dLm)
        assert not (err > bound).any(), (name, "d_crf_table entries outside the stated bound", int((err > bound).sum()))
        rms = float(np.sqrt((tab ** 2).mean()))
        rel = float((err / np.maximum(np.abs(tab), rms)).max())
        assert rel <= 2e-4, (name, "d_crf_table", rel)
        assert float(g2["d_exposure"]) == pytest.approx(r2["dL_dexposure"], rel=1e-4, abs=1e-4 * float(np.abs(dLm).sum()) * 1e-3)

    # 4. the instantiation with the optional outputs against the plain frame's.  (Only a frame with inverse depth runs the
    # DEPTH kernels: with the opacity output alone both launches are the plain instantiation, and this compares two runs of it.)
    g0 = Hh.run_hip(sc, **run)
    s0 = g0["state"]
    assert np.array_equal(u32(st["n_contrib"]), u32(s0["n_contrib"])), (name, "n_contrib differs from the plain frame's")
    for what, a, b in (("final_T", st["final_T"], s0["final_T"]), ("color", g["color"], g0["color"])) + \
            ((("hdr", g["hdr"], g0["hdr"]),) if hdr else ()):
        same = Hh.bits(a) == Hh.bits(b)
        assert same.all(), (name, what, "differs in bits from the plain frame's", int((~same).sum()),
                            float(np.abs(np.asarray(a, np.float64) - b).max()))
    return dict(g=g, g0=g0, r=r, fs=fs, m=m, clear=clear)


# ---- (a) one tile, seven batches of 48 records of 208 bytes and a partial one, both outputs ----

def test_deep_tile_both_outputs(oracle):
    sc = deep_tile_scene()
    gD, gA = upstream(16, 16, 21)
    c = _hold(oracle, sc, "a_deep_tile", gD=gD, gA=gA)
    n = int(c["fs"][0]["n_contrib"].max())
    assert n > 6 * 48 and n % 48, n


# ---- (b) tiles cut off in both directions ----

def test_partial_tiles_inverse_depth(oracle):
    sc = S.make_scene(2000, 37, 23, 2, seed=5)
    gD, _ = upstream(23, 37, 22, alpha=False)
    _hold(oracle, sc, "b_partial_tiles", gD=gD)


# ---- (c) one lane group at a time: the tenth sum stored through each plane in turn ----

@pytest.mark.parametrize("g,w", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_one_block_at_a_time_inverse_depth(oracle, g, w):
    sc = block_scene(g, w)
    gD, _ = upstream(16, 16, 23 + 2 * g + w, alpha=False)
    c = _hold(oracle, sc, f"c_block_g{g}_w{w}", gD=gD)
    nc = np.asarray(c["fs"][0]["n_contrib"]).reshape(16, 16)
    inside = np.zeros((16, 16), bool)
    inside[8 * w:8 * w + 8, 8 * g:8 * g + 8] = True
    assert (nc[~inside] == 0).all() and (nc[inside] > 0).sum() >= 16, (g, w)
    assert float(np.abs(c["g"]["d_means3D"]).sum()) > 0


# ---- (d) 20 tiles: one of them through the backward's queue, both outputs, antialiasing ----

D_SEED = 0     # (the first seed, counted from 0, whose frame holds both caps by the oracle's guard band alone)


def queue_scene():
    sc = S.make_scene(1500, 80, 64, 1, seed=D_SEED)
    sc.antialias = True
    return sc


def test_tile_queue_both_outputs_antialiased(oracle):
    sc = queue_scene()
    gD, gA = upstream(64, 80, 24)
    _hold(oracle, sc, "d_queue_antialias", gD=gD, gA=gA)     # 20 tiles: 8 % of them, one tile, goes through the queue


# ---- (e) HDR + CRF, two poses: the DEPTH instantiation and the CRF tail in one launch ----

def hdr_scene():
    return S.make_scene(1500, 48, 32, 1, seed=12, hdr=True), S.blur_poses(48, 32, 2, step=0.03)


@pytest.mark.parametrize("dom", ["ldr", "hdr"])
def test_hdr_crf_two_poses_both_outputs(oracle, dom):
    sc, cams = hdr_scene()
    gD, gA = upstream(32, 48, 25)
    _hold(oracle, sc, f"e_hdr_crf_{dom}", cams=cams, hdr=True, dom=dom, gD=gD, gA=gA)


@pytest.mark.parametrize("dom", ["ldr", "hdr"])
def test_hdr_crf_fused_backward_equals_staged_with_both_outputs(dom):
    """The CRF-table / exposure gradients of the fused backward (their first stage rides in the tail workgroups of the DEPTH
    render backward, whose staging area they borrow) equal those of the staged calls bit for bit.  And the other way round:
    the per-Gaussian gradients of the fused backward equal those of a backward without the CRF stage (render + preprocess),
    in which no tail workgroup shares the launch."""
    from casualhdrsplat_amd import GaussianRasterizer
    from casualhdrsplat_amd import _lib as L
    from casualhdrsplat_amd.rasterizer import replay_backward
    sc, cams = hdr_scene()
    P = sc.means3D.shape[0]
    gD, gA = (torch.from_numpy(x).cuda() for x in upstream(32, 48, 25))
    rs, expo, crf = Hh.settings_from_scene(sc, "cuda", cams, hdr=True, blur_domain=dom, requires_grad=True)
    lv = [getattr(sc, k).cuda().requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")]
    out = GaussianRasterizer(rs, return_alpha=True, return_invdepth=True)(
        lv[0], torch.zeros(P, 3, device="cuda", requires_grad=True), lv[1], shs=lv[2], scales=lv[3], rotations=lv[4])
    assert len(out) == 5
    dL = sc.dL_dimage.cuda()
    kw = dict(grad_alpha=gA, grad_invdepth=gD)

    def tensors(g):
        return {k: v.detach().cpu().numpy().copy() for k, v in g.items()
                if isinstance(v, torch.Tensor) and not k.startswith("_") and k != "view_colors"}

    fused = tensors(replay_backward(out[0], dL, **kw))
    no_crf = tensors(replay_backward(out[0], dL, L.HS_BWD_RENDER | L.HS_BWD_PREPROCESS, **kw))
    replay_backward(out[0], dL, L.HS_BWD_RENDER, **kw)
    staged = tensors(replay_backward(out[0], dL, L.HS_BWD_CRF, **kw))
    assert np.abs(fused["crf_table"]).max() > 0 and float(np.abs(fused["exposure"]).max()) > 0
    for k in ("exposure", "crf_table"):
        assert np.array_equal(Hh.bits(fused[k]), Hh.bits(staged[k])), k
    for k in ("means3D", "opacities", "shs", "scales", "rotations", "means2D"):
        assert np.abs(fused[k]).max() > 0 and np.array_equal(Hh.bits(fused[k]), Hh.bits(no_crf[k])), k
    assert not np.abs(no_crf["crf_table"]).any() and not np.abs(no_crf["exposure"]).any()    # (that call left the CRF stage out)
    # ... and the optional gradients reach the replay: without them the geometry differs
    plain = tensors(replay_backward(out[0], dL))
    assert not np.array_equal(Hh.bits(plain["means3D"]), Hh.bits(fused["means3D"]))
    assert np.array_equal(Hh.bits(plain["crf_table"]), Hh.bits(fused["crf_table"]))


# ---- (g) the upstream gradient on ONE optional output, the colour's all zero ----

@pytest.mark.parametrize("which", ["invdepth", "alpha"])
def test_gradient_on_one_output_only(oracle, which):
    sc = queue_scene()
    sc.dL_dimage = torch.zeros_like(sc.dL_dimage)
    gD, gA = upstream(64, 80, 26, invdepth=which == "invdepth", alpha=which == "alpha")
    c = _hold(oracle, sc, f"g_only_{which}", gD=gD, gA=gA)
    g = c["g"]
    assert not Hh.bits(g["d_shs"]).any(), "d_shs must be zero in every bit"
    for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
        assert float(np.abs(g["d_" + k][c["clear"]]).sum()) > 0, (which, k)


# ---- (h) the randomized sweep's configurations with the optional outputs ----

SWEEP_SEED = 2027    # (the first seed after the existing sweep's whose twelve cases all hold the clear-rows cap by the
                     #  oracle's guard band alone; it draws HDR and linear frames, 1-3 poses, and all three output sets)
SWEEP_CASES = 12


def test_randomized_configurations_with_optional_outputs(oracle):
    """helpers.sweep_case from a seed of this test's own, then helpers.optional_outputs_case: which of the two outputs carry
    a gradient.  Structure, images and gradients as the sweep of test_gpu_parity.py holds them, plus the four checks of this
    file.  Failures are collected over all cases."""
    rng = np.random.default_rng(SWEEP_SEED)
    failures, seen = [], set()
    for case in range(SWEEP_CASES):
        c = Hh.sweep_case(rng, case)
        o = Hh.optional_outputs_case(rng, c)
        seen.add(o["which"])
        pre, keys = {}, Hh.GRAD_KEYS
        single = not (c["hdr"] or c["n_poses"] > 1)
        if c["precomp"] and single:
            f0 = Hh.run_oracle(oracle, c["sc"], backward=False)[0]
            pre = dict(use_colors_precomp=c["colors"], use_cov_precomp=torch.from_numpy(f0["cov3D"].copy()))
            keys = PRECOMP_KEYS
        # (as the existing sweep: even cases bin with a fixed capacity just above the frame's pairs -- HDR frames and the
        #  single-pose linear frame; odd cases, and the linear frame of several poses, in the synchronous mode)
        slack = None if case % 2 else (7 if c["hdr"] else 1 if single else None)
        try:
            with environment(HS_TILE_SORT=(None, "radix", "hier")[case % 3], HS_DEPTH_SORT="lsd" if case % 4 == 3 else None):
                _hold(oracle, c["sc"], f"h_case{case:02d}", cams=c["cams"], hdr=c["hdr"], dom=c["dom"], act=c["act"],
                      gD=o["invdepth_grad"], gA=o["alpha_grad"], pre=pre, keys=keys, capacity_slack=slack, sweep=True)
        except AssertionError as e:
            failures.append(f"{o['what']}: {e}")
            if os.environ.get("HS_PARITY_REPORT"):
                print("SWEEP FAILED", failures[-1], flush=True)
    assert seen == {"invdepth", "alpha", "invdepth+alpha"}, seen
    assert not failures, f"{len(failures)} failing case(s):\n" + "\n".join(failures)
