"""GPU checks of the per-Gaussian feature compositing (features.hip through features.composite_features) against the float64
restatement of its definition (tests/features_reference.py), against the rasterizer itself and against itself.

Bound, per element:  |hip - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S  with helpers.C_BOUND (8) as it stands; forward: S_out[c, p]
= sum of w |f| (4 + contributors composited at the pixel); backward: S_grad[g, c] = sum of w |dL| (4 + contributors composited
before the entry at that pixel).  With HS_PARITY_REPORT=1 in the environment the largest observed
(|hip - ref| - 1e-4 |ref|) / (2^-24 S) of every case goes to profiles/features_parity.json.
"""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import features_reference as R
import helpers as Hh
import poison
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES = "casualhdrsplat_amd.features"
C_ALL = 19                 # the widest case: every narrower one takes its first columns (channels do not mix)
_PARITY = {}


def _leaves(sc, grad=True, **replace):
    t = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=sc.scales,
             rotations=sc.rotations)
    t.update(replace)
    return {k: v.detach().clone().to(DEV).requires_grad_(grad) for k, v in t.items() if v is not None}


def _forward(sc, cameras=None, n_frames=1, grad=True, leaves=None, **rast_kw):
    """One forward of the scene; returns (what composite_features takes, the rasterizer, the outputs, the leaves)."""
    from casualhdrsplat_amd import GaussianRasterizer
    rs, _, _ = Hh.settings_from_scene(sc, DEV, cameras)
    if n_frames > 1:
        rs = rs._replace(n_frames=n_frames)
    rast = GaussianRasterizer(rs, **rast_kw)
    lv = leaves if leaves is not None else _leaves(sc, grad)
    a = dict(lv)
    with torch.enable_grad() if grad else torch.no_grad():
        out = rast(a.pop("means3D"), a.pop("means2D"), a.pop("opacities"), **a)
    return (out[0] if grad else rast), rast, out, lv


def _dev(x, grad=False):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).requires_grad_(grad)


def _run(handle, feat, dL=None):
    """composite_features on `handle`; returns (out, dL_dfeatures or None) as numpy."""
    from casualhdrsplat_amd import composite_features
    f = _dev(feat, grad=dL is not None)
    out = composite_features(handle, f)
    g = None
    if dL is not None:
        g, = torch.autograd.grad(out, f, _dev(dL).reshape(out.shape))
        g = g.cpu().numpy()
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), g


def _inputs(P, H, W, seed, n_poses=1):
    """features N(0, 1) with an all-ones channel (1) and a x 50 channel (2); dL N(0, 1)"""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((P, C_ALL))
    feat[:, 1] = 1.0
    feat[:, 2] *= 50.0
    return feat.astype(np.float32), rng.standard_normal((n_poses, C_ALL, H, W)).astype(np.float32)


def _hold_to_the_bound(name, out, grad, ref, C, keep=None, factor=1.0):
    """out [C, H, W] and grad [P, C] against the first C channels of the float64 restatement `ref`; `keep` [H, W]: the pixels
    of the forward comparison."""
    keep = np.ones(ref["out"].shape[1:], bool) if keep is None else keep
    c_out = R.needed_constant(out[:, keep], ref["out"][:C][:, keep], ref["S_out"][:C][:, keep])
    c_grad = R.needed_constant(grad, ref["grad"][:, :C], ref["S_grad"][:, :C])
    _PARITY[name] = dict(out=round(c_out, 4), dL_dfeatures=round(c_grad, 4), contributors_max=int(ref["count"].max()),
                         pixels_compared=int(keep.sum()))
    print(f"features parity {name}: C needed {c_out:.3f} (out) {c_grad:.3f} (dL_dfeatures)", flush=True)
    assert c_out <= factor * Hh.C_BOUND and c_grad <= factor * Hh.C_BOUND, (name, c_out, c_grad)


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    if os.environ.get("HS_PARITY_REPORT") and _PARITY:
        with open(os.path.join(ROOT, "profiles", "features_parity.json"), "w") as fh:
            json.dump(dict(bound="|hip - ref| <= 1e-4 |ref| + C 2^-24 S; the largest C any element needs, per case (C_BOUND = 8; "
                                 "the rasterizer cases compare two fp32 results: twice the bound)", cases=_PARITY),
                      fh, indent=1, sort_keys=True)
            fh.write("\n")


# ---- 1. guarded scenes: no pixel in the threshold band, every fp32 implementation decides alike ----

GUARDED = {"a": (1000, 128, 128, 3), "b": (600, 104, 72, 1)}


@pytest.fixture(scope="module")
def guarded(oracle):
    out = {}
    for k, (P, W, H, deg) in GUARDED.items():
        sc, seed = Hh.guarded_scene(oracle, P, W, H, deg)
        f, _ = Hh.run_oracle(oracle, sc, backward=False)
        feat, dL = _inputs(P, H, W, 31)
        out[k] = dict(sc=sc, f=f, feat=feat, dL=dL[0], ref=R.composite(f, W, H, feat, dL[0]), seed=seed)
    assert out["b"]["seed"] == 0
    return out


@pytest.mark.parametrize("C", (1, 4, 7, 19))
@pytest.mark.parametrize("which", tuple(GUARDED))
def test_guarded_scene_against_the_restatement(guarded, which, C):
    g = guarded[which]
    handle, _, _, _ = _forward(g["sc"])
    out, grad = _run(handle, g["feat"][:, :C], g["dL"][:C])
    assert out.shape == (1, C) + g["dL"].shape[1:] and grad.shape == (GUARDED[which][0], C)
    _hold_to_the_bound(f"guarded_{which}_C{C}", out[0], grad, g["ref"], C)
    if C > 1:   # the all-ones channel is the accumulated opacity
        from casualhdrsplat_amd import inspect_state
        T = inspect_state(handle)["final_T"][0].double().cpu().numpy()
        assert np.abs(out[0, 1] - (1.0 - T)).max() <= 1e-5


# ---- 2. long lists, batch boundaries, early termination ----

LONG = {"deep": (6000, 64, 64, 0), "rows": (3000, 48, 40, 1)}


@pytest.mark.parametrize("which", tuple(LONG))
def test_long_lists_and_early_termination(oracle, which):
    """Tile lists of thousands of entries (many staging batches), pixels that terminate after hundreds of contributors: the
    pixels where the two sides demonstrably decided differently, or may have, are left out of the forward comparison and
    carry no upstream gradient."""
    from casualhdrsplat_amd import inspect_state
    P, W, H, deg = LONG[which]
    C = 7
    sc = S.make_scene(P, W, H, deg, seed=0)
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    lens = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).max()
    assert lens > 1500 and int(f["n_contrib"].max()) > 128, (lens, int(f["n_contrib"].max()))
    handle, _, _, _ = _forward(sc)
    st = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in inspect_state(handle).items()}
    m = Hh.decision_masks(oracle, sc, [f], st, what=which)
    share = float(m["excluded"].mean())
    print(f"{which}: excluded share {share:.4f}, band {float(m['pix_risk'].mean()):.4f}, longest list {lens}", flush=True)
    assert share <= 0.01, (which, share)
    keep = ~m["excluded"]
    feat, dL = _inputs(P, H, W, 32)
    feat, dL = feat[:, :C], dL[0, :C] * keep[None]
    out, grad = _run(handle, feat, dL)
    _hold_to_the_bound(f"long_{which}", out[0], grad, R.composite(f, W, H, feat, dL), C, keep=keep)


# ---- 3. against the rasterizer itself ----

def test_compositing_the_colours_gives_the_rendered_image_and_its_colour_gradient(guarded):
    """One pose, LDR, a black background: the rendered image IS the compositing of the three colour channels, and the
    gradient of colors_precomp (the identity under every radiance activation: preprocess.hip stores it as it is) IS
    dL_dfeatures.  Each side is within the bound of float64: twice the bound between them."""
    from casualhdrsplat_amd import inspect_state
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    sc = dataclasses.replace(g["sc"], bg=torch.zeros(3))
    dL = g["dL"][:3]
    handle, _, outs, _ = _forward(sc)
    rgb = inspect_state(handle)["rgb"].detach().cpu().numpy()
    assert rgb.shape == (P, 3)
    rgb[outs[1].cpu().numpy() == 0] = 0.0      # (a culled Gaussian is on nobody's list, and its record was never written)
    img = outs[0].detach().cpu().numpy()
    out, _ = _run(handle, rgb)
    ref = R.composite(g["f"], W, H, rgb, dL)
    c_img = R.needed_constant(out[0], img, ref["S_out"])
    print(f"features vs rasterizer: C needed {c_img:.3f} (image)", flush=True)
    assert np.abs(img).max() > 0.1 and c_img <= 2 * Hh.C_BOUND, c_img
    # non-negative colours as a leaf
    col = np.abs(g["feat"][:, :3])
    lv = _leaves(sc, shs=None)
    lv["colors_precomp"] = _dev(col, grad=True)
    handle, _, outs, _ = _forward(sc, leaves=lv)
    (outs[0] * _dev(dL)).sum().backward()
    out, grad = _run(handle, col, dL)
    refc = R.composite(g["f"], W, H, col, dL)
    c_fwd = R.needed_constant(out[0], outs[0].detach().cpu().numpy(), refc["S_out"])
    c_bwd = R.needed_constant(grad, lv["colors_precomp"].grad.cpu().numpy(), refc["S_grad"])
    _PARITY["rasterizer_b"] = dict(image_from_rgb=round(c_img, 4), image_from_colors_precomp=round(c_fwd, 4),
                                   colors_precomp_grad=round(c_bwd, 4))
    print(f"features vs rasterizer (colors_precomp): C needed {c_fwd:.3f} (image) {c_bwd:.3f} (gradient)", flush=True)
    assert np.abs(grad).max() > 0.1 and c_fwd <= 2 * Hh.C_BOUND and c_bwd <= 2 * Hh.C_BOUND, (c_fwd, c_bwd)


# ---- 4. poses and frames ----

@pytest.fixture(scope="module")
def posed():
    P, W, H, C = 1500, 72, 56, 7
    sc, cams = S.make_scene(P, W, H, 1, seed=3), S.blur_poses(W, H, 4, step=0.03)
    feat, dL = _inputs(P, H, W, 33, n_poses=4)
    feat, dL = feat[:, :C], dL[:, :C]
    single = [_run(_forward(sc, cameras=[c])[0], feat, dL[k]) for k, c in enumerate(cams)]
    return sc, cams, feat, dL, single


def _fold(grads):
    s = torch.zeros(grads[0].shape, dtype=torch.float32)
    for g in grads:
        s = s + torch.as_tensor(g)
    return s.numpy()


def test_one_call_over_three_poses_is_three_single_pose_calls(posed):
    sc, cams, feat, dL, single = posed
    handle, _, _, _ = _forward(sc, cameras=cams[:3])
    out, grad = _run(handle, feat, dL[:3])
    assert out.shape[0] == 3 and np.abs(out).max() > 1 and (np.abs(grad).sum(axis=1) > 0).sum() > 100
    for k in range(3):
        assert poison.bytes_of(out[k]) == poison.bytes_of(single[k][0][0]), k
    assert poison.bytes_of(grad) == poison.bytes_of(_fold([single[k][1] for k in range(3)]))


def test_two_frames_of_two_poses_are_four_single_pose_calls(posed):
    sc, cams, feat, dL, single = posed
    handle, _, _, _ = _forward(sc, cameras=cams, n_frames=2)
    out, grad = _run(handle, feat, dL)
    assert out.shape[0] == 4
    for k in range(4):        # pose k of frame f at f * N + k
        assert poison.bytes_of(out[k]) == poison.bytes_of(single[k][0][0]), k
    assert poison.bytes_of(grad) == poison.bytes_of(_fold([s[1] for s in single]))


# ---- 5. autograd ----

def test_autograd_reaches_the_features_and_only_them(guarded):
    from casualhdrsplat_amd import composite_features, features
    from casualhdrsplat_amd.rasterizer import _state_of
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    C = 7
    feat_np, dL_np = g["feat"][:, :C], g["dL"][:C]
    handle, _, _, lv = _forward(g["sc"])
    f = _dev(feat_np, grad=True)
    out = composite_features(handle, f)
    assert out.requires_grad and tuple(out.shape) == (1, C, H, W)
    got, = torch.autograd.grad(out, f, _dev(dL_np)[None], retain_graph=True)
    explicit = features._features_backward(_state_of(handle), C, _dev(dL_np)[None].contiguous())
    assert poison.bytes_of(got) == poison.bytes_of(explicit) and got.abs().max() > 0.1
    # the geometry gets nothing through these channels
    geo = torch.autograd.grad(out.sum(), [lv[k] for k in ("means3D", "opacities", "scales", "rotations", "shs")], allow_unused=True)
    assert all(x is None for x in geo)
    # features that ask for no gradient give an output that carries none
    plain = composite_features(handle, _dev(feat_np))
    assert not plain.requires_grad and plain.grad_fn is None and poison.bytes_of(plain) == poison.bytes_of(out)


def test_backward_works_after_a_second_forward_of_the_same_rasterizer(posed):
    from casualhdrsplat_amd import composite_features
    sc, cams, feat, dL, single = posed
    rast, _, _, lv = _forward(sc, cameras=[cams[0]], grad=False, keep_state=True)
    f = _dev(feat, grad=True)
    out = composite_features(rast, f)
    with torch.no_grad():     # the rasterizer moves on to another view (and another state)
        a = dict(_leaves(sc, grad=False))
        rs2, _, _ = Hh.settings_from_scene(sc, DEV, [cams[3]])
        rast.raster_settings = rs2
        rast(a.pop("means3D"), a.pop("means2D"), a.pop("opacities"), **a)
    other = composite_features(rast, f)
    grad, = torch.autograd.grad(out, f, _dev(dL[0])[None])
    torch.cuda.synchronize()
    assert poison.bytes_of(out) == poison.bytes_of(single[0][0]) and poison.bytes_of(grad) == poison.bytes_of(single[0][1])
    assert poison.bytes_of(other) == poison.bytes_of(single[3][0])


# ---- 6. every element is written; nothing leaks ----

def _under_every_pattern(monkeypatch, handle, feat, dL):
    """(out, dL_dfeatures) of a call whose output tensors and workspace held zeros -- after asserting that the other
    patterns give the same bits."""
    from casualhdrsplat_amd import features
    results = {}
    for pattern in ("zero", "ff", "nan", "a5", "random"):
        features._WORKSPACES.clear()
        with poison.poisoned(monkeypatch, pattern) as session:
            results[pattern] = _run(handle, feat, dL)
        fills = session.require(FEATURES, roles=("feature_workspace#0",), at_least=3)     # out, dL_dfeatures, the workspace
        assert {f.nbytes for f in fills} >= {4 * results[pattern][0].size, 4 * results[pattern][1].size}
    features._WORKSPACES.clear()
    zero = results["zero"]
    for pattern, got in results.items():
        assert poison.bytes_of(got[0]) == poison.bytes_of(zero[0]) and poison.bytes_of(got[1]) == poison.bytes_of(zero[1]), pattern
    return zero


def test_results_do_not_depend_on_what_the_buffers_held(guarded, monkeypatch):
    from casualhdrsplat_amd import ContributionStats, accumulate_contributions, inspect_state
    C = 7
    g = guarded["b"]
    full = _under_every_pattern(monkeypatch, _forward(g["sc"])[0], g["feat"][:, :C], g["dL"][:C])
    assert np.abs(full[0]).max() > 1 and np.abs(full[1]).max() > 0.1
    # a frame with empty tiles, and with Gaussians that are on lists but too faint to be composited anywhere
    P, W, H = 24, 104, 72
    sc = S.make_scene(P, W, H, 1, seed=5)
    sc.opacities[::4] = 0.002
    handle, _, _, _ = _forward(sc)
    st = inspect_state(handle)
    ranges = st["ranges"].cpu().numpy()
    untouched = st["n_contrib"][0].cpu().numpy() == 0
    assert (ranges[:, 0] == ranges[:, 1]).any() and untouched.any() and not untouched.all()
    feat, dL = _inputs(P, H, W, 34)
    feat, dL = feat[:, :C], dL[0, :C]
    zero = _under_every_pattern(monkeypatch, handle, feat, dL)
    assert poison.bytes_of(zero[0][0][:, untouched]) == bytes(4 * C * int(untouched.sum()))        # +0 where nothing reaches
    # ... and the cached workspace, as an earlier call of another gradient left it, is as good as a fresh one
    _run(handle, feat, -3.0 * dL)
    again = _run(handle, feat, dL)
    assert poison.bytes_of(again[0]) == poison.bytes_of(zero[0]) and poison.bytes_of(again[1]) == poison.bytes_of(zero[1])
    # a Gaussian composited nowhere reaches no pixel, whatever its features hold; it gets +0
    stats = ContributionStats(P, DEV)
    accumulate_contributions(handle, stats)
    unseen = (stats.pixel_count == 0).cpu().numpy()
    assert unseen.any() and not unseen.all()
    zeroed, nans = feat.copy(), feat.copy()
    zeroed[unseen], nans[unseen] = 0.0, np.nan
    assert poison.bytes_of(_run(handle, nans)[0]) == poison.bytes_of(_run(handle, zeroed)[0])
    assert poison.bytes_of(zero[1][unseen]) == bytes(4 * C * int(unseen.sum()))
    # a non-finite gradient at a pixel nothing reaches stays there
    yx = np.argwhere(untouched)[0]
    dL_nan = dL.copy()
    dL_nan[:, yx[0], yx[1]] = np.nan
    assert poison.bytes_of(_run(handle, feat, dL_nan)[1]) == poison.bytes_of(zero[1])


# ---- 7. other modes ----

def test_an_overflowed_frame_gives_zeros_and_its_replay_gives_the_plain_call(guarded):
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    C = 7
    feat, dL = g["feat"][:, :C], g["dL"][:C]
    plain = _run(_forward(g["sc"])[0], feat, dL)
    assert poison.bytes_of(_run(_forward(g["sc"])[0], feat, dL)[1]) == poison.bytes_of(plain[1])     # two runs, the same bits
    # sync-free mode, capacity far below the frame's pairs: with grad nobody looks at the counters before the backward
    handle, rast, _, _ = _forward(g["sc"], capacity=256, keep_state=True)
    out, grad = _run(handle, feat, dL)
    assert poison.bytes_of(out) == bytes(4 * out.size) and poison.bytes_of(grad) == bytes(4 * grad.size)
    # under no_grad the rasterizer grows the capacity and renders the frame again by itself
    a = _leaves(g["sc"], grad=False)
    with torch.no_grad():
        rast(a.pop("means3D"), a.pop("means2D"), a.pop("opacities"), **a)
    assert rast.overflow_replays >= 1 and int(rast.capacity) > 256
    again = _run(rast, feat, dL)
    assert poison.bytes_of(again[0]) == poison.bytes_of(plain[0]) and poison.bytes_of(again[1]) == poison.bytes_of(plain[1])


def test_raw_parameterization_and_a_kept_state_give_the_plain_arrays(guarded):
    from casualhdrsplat_amd import inspect_state
    g = guarded["b"]
    sc = g["sc"]
    C = 4
    feat, dL = g["feat"][:, :C], g["dL"][:C]
    x = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))
    l = torch.log(sc.scales)
    q = sc.rotations * 1.7
    raw_handle, _, _, _ = _forward(sc, grad=False, leaves=_leaves(sc, grad=False, opacities=x, scales=l, rotations=q),
                                   parameterization="raw", keep_state=True)
    raw = _run(raw_handle, feat, dL)
    st = inspect_state(raw_handle)
    acts = {k: st[k].detach().clone() for k in ("opacities", "scales", "rotations")}
    plain_handle, _, _, _ = _forward(sc, leaves=_leaves(sc, **acts))
    plain = _run(plain_handle, feat, dL)
    assert poison.bytes_of(raw[0]) == poison.bytes_of(plain[0]) and poison.bytes_of(raw[1]) == poison.bytes_of(plain[1])
    assert np.abs(raw[0]).max() > 1 and np.abs(raw[1]).max() > 0.1
