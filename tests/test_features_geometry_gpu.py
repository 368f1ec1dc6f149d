"""GPU checks of the geometry gradients through the composited feature channels (featgeo.hip through
features.composite_features(..., geometry=...)) against the C oracle's truth (tests/test_features_geometry.py, oracle_truth:
ceil(C / 3) colors_precomp backwards over a black background, gradients and bounds summed), against the rasterizer's own
backward and against itself.

Bound, per element of dL_dmeans3D, dL_dopacities, dL_dscales, dL_drotations: helpers.assert_grads_bounded with C_BOUND (8) as
it stands -- |hip - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S, S the oracle's sum of w |term| summed over the triples.  With
HS_PARITY_REPORT=1 in the environment the largest constant any element needs goes to profiles/features_geometry_parity.json,
per case.
"""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import helpers as Hh
import poison
import test_features_geometry as TG
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES = "casualhdrsplat_amd.features"
KEYS = ("means3D", "opacities", "scales", "rotations")
K_PASS = 16                # channels per pass of the replay (featgeo.hip, kGeoPass)
C_ALL = 2 * K_PASS + 1     # three passes; every narrower case takes its first columns
_PARITY = {}
_TRUTHS = {}               # oracle_truth's cache: full triples are shared between the cases of a scene


def _black(sc):
    sc = copy.copy(sc)
    sc.bg = torch.zeros(3)
    return sc


def _leaves(sc, grad=True, **replace):
    t = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=sc.scales,
             rotations=sc.rotations)
    t.update(replace)
    return {k: v.detach().clone().to(DEV).requires_grad_(grad) for k, v in t.items() if v is not None}


def _forward(sc, cameras=None, n_frames=1, leaves=None, **rast_kw):
    """One forward with grad; returns (the outputs, the rasterizer, the leaves)."""
    from casualhdrsplat_amd import GaussianRasterizer
    rs, _, _ = Hh.settings_from_scene(sc, DEV, cameras)
    if n_frames > 1:
        rs = rs._replace(n_frames=n_frames)
    rast = GaussianRasterizer(rs, **rast_kw)
    lv = leaves if leaves is not None else _leaves(sc)
    a = dict(lv)
    out = rast(a.pop("means3D"), a.pop("means2D"), a.pop("opacities"), **a)
    return out, rast, lv


def _dev(x, grad=False):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).requires_grad_(grad)


def _geo(lv):
    return {k: lv[k] for k in KEYS}


def _grads(out0, lv, feat, dL, geometry=True):
    """composite_features on the forward behind out0 and its backward under dL; {out, d_features, d_<key>} as numpy."""
    from casualhdrsplat_amd import composite_features
    f = _dev(feat, grad=True)
    out = composite_features(out0, f, geometry=_geo(lv) if geometry else None)
    wrt = [f] + ([lv[k] for k in KEYS] if geometry else [])
    g = torch.autograd.grad(out, wrt, _dev(dL).reshape(out.shape))
    torch.cuda.synchronize()
    res = dict(out=out.detach().cpu().numpy(), d_features=g[0].cpu().numpy())
    for k, t in zip(KEYS, g[1:]):
        assert t.shape == lv[k].shape, k
        res["d_" + k] = t.cpu().numpy()
    return res


def _run(sc, feat, dL, cameras=None, n_frames=1, **rast_kw):
    out, _, lv = _forward(sc, cameras, n_frames, **rast_kw)
    return _grads(out[0], lv, feat, dL)


def _same_bits(a, b, keys=KEYS):
    for k in keys:
        assert poison.bytes_of(a["d_" + k]) == poison.bytes_of(b["d_" + k]), k


def _hold_to_the_bound(name, got, ref, rows=None):
    rep = Hh.assert_grads_bounded(got, ref, keys=TG.GEO_KEYS, what=name, rows=rows)
    _PARITY[name] = {k: round(v[1], 4) for k, v in rep.items()}
    print(f"features geometry parity {name}: C needed {_PARITY[name]}", flush=True)
    for k in KEYS:      # the gradients are there
        assert np.abs(got["d_" + k]).max() > 1e-3, (name, k)


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    if os.environ.get("HS_PARITY_REPORT") and _PARITY:
        with open(os.path.join(ROOT, "profiles", "features_geometry_parity.json"), "w") as fh:
            json.dump(dict(bound="|hip - ref| <= 1e-4 |ref| + C 2^-24 S; the largest C any element needs, per case and tensor "
                                 "(C_BOUND = 8; the rasterizer case compares two fp32 results: twice the bound)", cases=_PARITY),
                      fh, indent=1, sort_keys=True)
            fh.write("\n")


# ---- 1. guarded scenes: no pixel in the threshold band, every fp32 implementation decides alike ----

GUARDED = {"a": (1000, 128, 128, 3), "b": (600, 104, 72, 1)}


@pytest.fixture(scope="module")
def guarded(oracle):
    out = {}
    for k, (P, W, H, deg) in GUARDED.items():
        sc, seed = Hh.guarded_scene(oracle, P, W, H, deg)
        feat, dL = TG.geometry_inputs(P, H, W, 51, C_ALL)
        out[k] = dict(sc=_black(sc), feat=feat, dL=dL, seed=seed)
    assert out["b"]["seed"] == 0
    return out


# C: one channel; the colours' three; C % 4 != 0; exactly one pass; one pass and a channel; three passes
@pytest.mark.parametrize("C_", (1, 3, 6, K_PASS, K_PASS + 1, C_ALL))
@pytest.mark.parametrize("which", tuple(GUARDED))
def test_guarded_scene_against_the_truth(oracle, guarded, which, C_):
    g = guarded[which]
    feat, dL = g["feat"][:, :C_], g["dL"][:, :C_]
    got = _run(g["sc"], feat, dL)
    ref = TG.oracle_truth(oracle, g["sc"], feat, dL, cache=_TRUTHS, tag="guarded_" + which)
    _hold_to_the_bound(f"guarded_{which}_C{C_}", got, ref)


# ---- 2. long lists, batch boundaries, early termination ----

LONG = {"deep": (6000, 64, 64, 0), "rows": (3000, 48, 40, 1)}


@pytest.mark.parametrize("which", tuple(LONG))
def test_long_lists_and_early_termination(oracle, which):
    """Tile lists of thousands of entries (dozens of staging batches), pixels that end after more than 128 contributors: the
    pixels where the two sides demonstrably decided differently, or may have, carry no upstream gradient."""
    from casualhdrsplat_amd import inspect_state
    P, W, H, deg = LONG[which]
    C_ = K_PASS + 1
    sc = _black(S.make_scene(P, W, H, deg, seed=0))
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    lens = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).max()
    assert lens > 1500 and int(f["n_contrib"].max()) > 128, (lens, int(f["n_contrib"].max()))
    out, _, lv = _forward(sc)
    st = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in inspect_state(out[0]).items()}
    m = Hh.decision_masks(oracle, sc, [f], st, what=which)
    share = float(m["excluded"].mean())
    assert share <= 0.01, (which, share)
    feat, dL = TG.geometry_inputs(P, H, W, 52, C_)
    dL = dL * (~m["excluded"])[None, None]
    got = _grads(out[0], lv, feat, dL)
    _hold_to_the_bound(f"long_{which}", got, TG.oracle_truth(oracle, sc, feat, dL))


# ---- 3. against the rasterizer itself ----

def test_three_channels_give_the_rasterizers_own_geometry_gradients(oracle, guarded):
    """C = 3, a black background, LDR, one pose: the image of a colors_precomp forward IS the compositing of the colours, so
    the geometry gradients of (image * dL).sum() ARE the new path's under the same dL.  Each side is within the bound of the
    truth: twice the bound between them."""
    g = guarded["b"]
    sc = g["sc"]
    col, dL = np.abs(g["feat"][:, :3]), g["dL"][:, :3]
    lv = _leaves(sc, shs=None)
    lv["colors_precomp"] = _dev(col, grad=True)
    out, _, _ = _forward(sc, leaves=lv)
    own = torch.autograd.grad(out[0], [lv[k] for k in KEYS], _dev(dL[0]), retain_graph=True)
    got = _grads(out[0], lv, col, dL)
    ref = TG.oracle_truth(oracle, sc, col, dL)
    need = {}
    for (k, rk), a in zip(TG.GEO_KEYS, own):
        a = a.cpu().numpy().astype(np.float64).reshape(ref[rk].shape)
        b = got["d_" + k].astype(np.float64).reshape(ref[rk].shape)
        excess = np.abs(a - b) - 2e-4 * np.abs(ref[rk])
        unit = 2.0 ** -24 * ref["abs_" + rk]
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.where(excess > 0, excess / unit, 0.0)
        need[k] = float(np.nan_to_num(n, nan=np.inf).max())
        assert np.abs(a).max() > 1e-2 and np.abs(b).max() > 1e-2, k      # not trivially small
    _PARITY["rasterizer_b"] = {k: round(v, 4) for k, v in need.items()}
    print(f"features geometry vs rasterizer: C needed {need}", flush=True)
    assert all(v <= 2 * Hh.C_BOUND for v in need.values()), need


# ---- 4. poses and frames ----

POSED = (500, 72, 56, 1, 394)      # (P, W, H, SH degree, the first seed whose four poses are all outside the guard band)


@pytest.fixture(scope="module")
def posed(oracle):
    P, W, H, deg, seed0 = POSED
    poses = lambda w, h: S.blur_poses(w, h, 4, step=0.03)
    sc, seed = Hh.guarded_scene(oracle, P, W, H, deg, seed=seed0, cams_fn=poses)
    assert seed == seed0
    feat, dL = TG.geometry_inputs(P, H, W, 53, 7, n_poses=4)
    return _black(sc), poses(W, H), feat, dL


def test_one_call_over_three_poses(oracle, posed):
    sc, cams, feat, dL = posed
    got = _run(sc, feat, dL[:3], cameras=cams[:3])
    assert got["out"].shape[0] == 3
    _hold_to_the_bound("poses_3", got, TG.oracle_truth(oracle, sc, feat, dL[:3], cams[:3], cache=_TRUTHS, tag="posed"))


def test_two_frames_of_two_poses(oracle, posed):
    sc, cams, feat, dL = posed
    got = _run(sc, feat, dL, cameras=cams, n_frames=2)
    assert got["out"].shape[0] == 4
    _hold_to_the_bound("frames_2x2", got, TG.oracle_truth(oracle, sc, feat, dL, cams, cache=_TRUTHS, tag="posed"))


# ---- 5. autograd ----

def _both_losses(sc, feat, dL, w_img):
    from casualhdrsplat_amd import composite_features
    out, _, lv = _forward(sc)
    f = _dev(feat, grad=True)
    feat_out = composite_features(out[0], f, geometry=_geo(lv))
    return (out[0] * w_img).sum(), (feat_out * _dev(dL).reshape(feat_out.shape)).sum(), lv, f


def test_the_two_losses_add_on_every_leaf_and_the_order_does_not_matter(guarded):
    g = guarded["b"]
    C_ = 7
    feat, dL = g["feat"][:, :C_], g["dL"][:, :C_]
    w_img = _dev(np.random.default_rng(54).standard_normal((3, 72, 104)))
    wrt = lambda lv: [lv[k] for k in KEYS]
    # the rasterizer's backward first (its node frees its saved tensors), then the features'
    img, fl, lv, f = _both_losses(g["sc"], feat, dL, w_img)
    g_img = torch.autograd.grad(img, wrt(lv))
    g_feat = torch.autograd.grad(fl, wrt(lv) + [f])
    # the other way round, on a forward of its own: the same bits (the two share no pair flags)
    img, fl, lv2, f2 = _both_losses(g["sc"], feat, dL, w_img)
    h_feat = torch.autograd.grad(fl, wrt(lv2) + [f2])
    h_img = torch.autograd.grad(img, wrt(lv2))
    for k, a, b, c, d in zip(KEYS + ("features",), g_feat, h_feat, g_img + (None,), h_img + (None,)):
        assert poison.bytes_of(a) == poison.bytes_of(b) and a.abs().max() > 1e-3, k
        assert c is None or (poison.bytes_of(c) == poison.bytes_of(d) and c.abs().max() > 1e-3), k
    # one backward of the sum leaves, on each leaf, exactly the sum of the two
    img, fl, lv3, f3 = _both_losses(g["sc"], feat, dL, w_img)
    (img + fl).backward()
    for k, a, b in zip(KEYS, g_img, g_feat):
        assert poison.bytes_of(lv3[k].grad) == poison.bytes_of(a + b), k
    assert poison.bytes_of(f3.grad) == poison.bytes_of(g_feat[4])
    # dL_dfeatures and the output are what the call without `geometry` gives
    out, _, lv4 = _forward(g["sc"])
    plain = _grads(out[0], lv4, feat, dL, geometry=False)
    with_geo = _grads(out[0], lv4, feat, dL)
    assert poison.bytes_of(plain["d_features"]) == poison.bytes_of(with_geo["d_features"]) == poison.bytes_of(g_feat[4])
    assert poison.bytes_of(plain["out"]) == poison.bytes_of(with_geo["out"])


# ---- 6. parameterization="raw", with and without filter_3D; antialiasing ----

@pytest.mark.parametrize("filtered", (False, True))
def test_raw_parameterization_is_the_activated_result_pushed_through_the_activations(guarded, filtered):
    from casualhdrsplat_amd import _lib as L
    g = guarded["b"]
    sc = g["sc"]
    P = GUARDED["b"][0]
    C_ = 5
    feat, dL = g["feat"][:, :C_], g["dL"][:, :C_]
    x = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))
    l = torch.log(sc.scales)
    q = sc.rotations * 1.7
    filt = torch.full((P,), 0.02, device=DEV) if filtered else None
    kw = dict(parameterization="raw", **(dict(filter_3D=filt) if filtered else {}))
    out, _, lv = _forward(sc, leaves=_leaves(sc, opacities=x, scales=l, rotations=q), **kw)
    raw = _grads(out[0], lv, feat, dL)
    saved = out[0].grad_fn.saved_tensors
    acts = dict(opacities=saved[1].detach().clone(), scales=saved[4].detach().clone(), rotations=saved[5].detach().clone())
    out2, _, lv2 = _forward(sc, leaves=_leaves(sc, **acts))
    act = _grads(out2[0], lv2, feat, dL)
    assert poison.bytes_of(raw["out"]) == poison.bytes_of(act["out"])
    assert poison.bytes_of(raw["d_means3D"]) == poison.bytes_of(act["d_means3D"])
    assert poison.bytes_of(raw["d_features"]) == poison.bytes_of(act["d_features"])
    # the activated rows through hs_activate_backward / hs_smoothing_apply_backward, in place, as _launch_backward's to_stored
    rows = {k: _dev(act["d_" + k]) for k in ("opacities", "scales", "rotations")}
    b = L.hs_activate_args()
    b.P = P
    b.rotations_raw = lv["rotations"].data_ptr()
    b.opacities, b.scales, b.rotations = (lv2[k].data_ptr() for k in ("opacities", "scales", "rotations"))
    b.dL_dopacities, b.dL_dscales, b.dL_drotations = (rows[k].data_ptr() for k in ("opacities", "scales", "rotations"))
    b.g_begin, b.g_end = 0, P
    if filtered:
        b.dL_dopacities, b.dL_dscales = None, None
    stream = torch.cuda.current_stream().cuda_stream
    L.check(L.load().hs_activate_backward(C.byref(b), stream), "hs_activate_backward")
    if filtered:
        s = L.hs_smoothing_apply_args()
        s.P = P
        s.opacity_raw, s.scales_raw, s.filter = lv["opacities"].data_ptr(), lv["scales"].data_ptr(), filt.data_ptr()
        s.dL_dopacities, s.dL_dscales = rows["opacities"].data_ptr(), rows["scales"].data_ptr()
        s.g_begin, s.g_end = 0, P
        L.check(L.load().hs_smoothing_apply_backward(C.byref(s), stream), "hs_smoothing_apply_backward")
    torch.cuda.synchronize()
    for k in ("opacities", "scales", "rotations"):
        assert poison.bytes_of(raw["d_" + k]) == poison.bytes_of(rows[k]), k
        assert poison.bytes_of(raw["d_" + k]) != poison.bytes_of(act["d_" + k]) and np.abs(raw["d_" + k]).max() > 1e-3, k


AA = (600, 104, 72, 1, 16)         # the first seed whose ANTIALIASED frame has no pixel inside the guard band


def test_an_antialiased_forward_is_held_to_the_truth(oracle):
    P, W, H, deg, seed = AA
    sc = _black(S.make_scene(P, W, H, deg, seed=seed))
    sc.antialias = True
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    assert not oracle.threshold_risk(Hh.oracle_camera(oracle, sc), f, 2e-5, 1e-4)["n_risky_pixels"]
    feat, dL = TG.geometry_inputs(P, H, W, 55, 7)
    _hold_to_the_bound("antialias", _run(sc, feat, dL), TG.oracle_truth(oracle, sc, feat, dL))


# ---- 7. reproducibility and robustness ----

def test_results_do_not_depend_on_what_the_buffers_held(guarded, monkeypatch):
    from casualhdrsplat_amd import features
    g = guarded["b"]
    C_ = K_PASS + 3          # two passes: the second adds to the records of the first
    feat, dL = g["feat"][:, :C_], g["dL"][:, :C_]
    out, _, lv = _forward(g["sc"])
    results = {}
    for pattern in ("zero", "ff", "nan", "a5", "random"):
        features._GEOMETRY_WORKSPACES.clear()
        features._WORKSPACES.clear()
        with poison.poisoned(monkeypatch, pattern) as session:
            results[pattern] = _grads(out[0], lv, feat, dL)
        fills = session.require(FEATURES, roles=("geometry_workspace#0", "feature_workspace#0"), at_least=7)
        assert {f.nbytes for f in fills} >= {4 * results[pattern]["d_" + k].size for k in KEYS}
    features._GEOMETRY_WORKSPACES.clear()
    for pattern, got in results.items():
        _same_bits(got, results["zero"], KEYS + ("features",))
    # twice the same bits, from a forward of its own; and the cached workspace, as a call under another gradient and another
    # C left it, is as good as a fresh one
    again = _run(g["sc"], feat, dL)
    _same_bits(again, results["zero"], KEYS + ("features",))
    _grads(out[0], lv, g["feat"][:, :3], -3.0 * g["dL"][:, :3])
    _same_bits(_grads(out[0], lv, feat, dL), results["zero"])
    # a frame with empty tiles and with Gaussians that are on lists but composited nowhere
    P, W, H = 24, 104, 72
    sc = _black(S.make_scene(P, W, H, 1, seed=5))
    sc.opacities[::4] = 0.002
    f2, d2 = TG.geometry_inputs(P, H, W, 56, 5)
    out, _, lv = _forward(sc)
    sparse = {}
    for pattern in ("zero", "nan", "random"):
        features._GEOMETRY_WORKSPACES.clear()
        with poison.poisoned(monkeypatch, pattern):
            sparse[pattern] = _grads(out[0], lv, f2, d2)
        _same_bits(sparse[pattern], sparse["zero"])
    features._GEOMETRY_WORKSPACES.clear()
    assert all(np.isfinite(sparse["zero"]["d_" + k]).all() for k in KEYS) and np.abs(sparse["zero"]["d_means3D"]).max() > 1e-3


def test_an_overflowed_frame_gives_zeros_and_full_capacity_gives_the_plain_call(guarded):
    g = guarded["b"]
    C_ = 7
    feat, dL = g["feat"][:, :C_], g["dL"][:, :C_]
    plain = _run(g["sc"], feat, dL)
    # sync-free mode, capacity far below the frame's pairs: with grad nobody looks at the counters before the backward
    over = _run(g["sc"], feat, dL, capacity=256)
    for k in KEYS + ("features",):
        assert poison.bytes_of(over["d_" + k]) == bytes(4 * over["d_" + k].size), k
    # the same mode with room for every pair
    full = _run(g["sc"], feat, dL, capacity=1 << 18)
    assert poison.bytes_of(full["out"]) == poison.bytes_of(plain["out"])
    _same_bits(full, plain, KEYS + ("features",))
