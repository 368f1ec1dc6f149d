"""GPU checks of the depth-distortion loss (distort.hip through distortion.distortion_loss) against the float64 truth of
tests/distortion_reference.py (the numpy restatement on the C oracle's forward, its rows projected through the Jacobians of
oracle.torch_rasterizer.preprocess; test_distortion.py pins that truth without a GPU), against the rasterizer's own inverse
depth image and against itself.

Bound, per element of the map, the moment and dL_dmeans3D, dL_dopacities, dL_dscales, dL_drotations:
|hip - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S with helpers.C_BOUND (8) as it stands and S built by the rule stated at the top of
distortion_reference.py.  With HS_PARITY_REPORT=1 in the environment the largest constant any element needs goes to
profiles/distortion_parity.json, per case and tensor.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import distortion_reference as DR
import helpers as Hh
import poison
import test_distortion as TD

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTORTION = "casualhdrsplat_amd.distortion"
KEYS = ("means3D", "opacities", "scales", "rotations")
_PARITY = {}
_TRUTHS = {}


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


def _grads(out0, lv, gammas, state=True):
    """distortion_loss on the forward behind out0 and its backward under gammas; {out, moment, n_contrib, d_<key>} as numpy."""
    from casualhdrsplat_amd import distortion_loss, inspect_state
    dmap = distortion_loss(out0, _geo(lv))
    assert dmap.requires_grad and dmap.dtype == torch.float32
    moment = dmap.grad_fn.moment
    g = torch.autograd.grad(dmap, [lv[k] for k in KEYS], _dev(gammas).reshape(dmap.shape))
    torch.cuda.synchronize()
    res = dict(out=dmap.detach().cpu().numpy(), moment=moment.cpu().numpy())
    if state:       # (inspect_state raises for an overflowed frame)
        res["n_contrib"] = inspect_state(out0)["n_contrib"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    for k, t in zip(KEYS, g):
        assert t.shape == lv[k].shape, k
        res["d_" + k] = t.cpu().numpy()
    return res


def _run(sc, gammas, cameras=None, n_frames=1, state=True, **rast_kw):
    out, _, lv = _forward(sc, cameras, n_frames, **rast_kw)
    return _grads(out[0], lv, gammas, state)


def _truth(oracle, name, gammas=None, poses=None):
    c = TD.case(oracle, name)
    key = (name, poses)
    if gammas is not None or key not in _TRUTHS:
        idx = list(range(len(c["cams"]))) if poses is None else list(poses)
        g = c["gammas"][idx] if gammas is None else gammas
        t = DR.truth([c["fwds"][k] for k in idx], [c["cams"][k] for k in idx], g, c["sc"])
        if gammas is not None:
            return t
        _TRUTHS[key] = t
    return _TRUTHS[key]


def _same_bits(a, b, keys=KEYS + ("out", "moment")):
    for k in keys:
        ka = k if k in ("out", "moment") else "d_" + k
        assert poison.bytes_of(a[ka]) == poison.bytes_of(b[ka]), k


def _hold_to_the_bound(name, got, ref, pixels=None):
    """the map and the moment (on `pixels` [H, W] bool, default all), and the four gradients"""
    assert got["out"].shape == ref["out"].shape
    m = np.ones(ref["out"].shape[1:], bool) if pixels is None else pixels
    need = dict(out=TD.needed(got["out"][:, m], ref["out"][:, m], ref["S_out"][:, m]),
                moment=TD.needed(got["moment"][:, m], ref["moment"][:, m], ref["S_moment"][:, m]))
    print(f"distortion parity {name}: map / moment need {need}", flush=True)
    assert all(v <= Hh.C_BOUND for v in need.values()), (name, need)
    rep = Hh.assert_grads_bounded(got, ref, keys=DR.GEO_KEYS, what=name)
    need.update({k: v[1] for k, v in rep.items()})
    _PARITY[name] = {k: round(v, 4) for k, v in need.items()}
    print(f"distortion parity {name}: C needed {_PARITY[name]}", flush=True)
    assert (got["out"][:, m] >= 0).all()
    return need


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    if os.environ.get("HS_PARITY_REPORT") and _PARITY:
        with open(os.path.join(ROOT, "profiles", "distortion_parity.json"), "w") as fh:
            json.dump(dict(bound="|hip - ref| <= 1e-4 |ref| + C 2^-24 S; the largest C any element needs, per case and tensor "
                                 "(C_BOUND = 8; invdepth compares two fp32 results: twice the bound)", cases=_PARITY),
                      fh, indent=1, sort_keys=True)
            fh.write("\n")


# ---- 1. guarded scenes: no pixel in the threshold band, every fp32 implementation decides alike ----

@pytest.mark.parametrize("which", tuple(TD.GUARDED))
def test_guarded_scene_against_the_truth(oracle, which):
    c = TD.case(oracle, which)
    got = _run(c["sc"], c["gammas"])
    ref = _truth(oracle, which)
    assert (got["n_contrib"] == ref["n_contrib"]).all()          # the forward decided as the reference does
    _hold_to_the_bound("guarded_" + which, got, ref)
    assert got["out"].max() > 1e-2
    for k in KEYS:      # the gradients are there
        assert np.abs(got["d_" + k]).max() > 1e-3, k


# ---- 2. long lists, batch boundaries, early termination ----

@pytest.mark.parametrize("which", tuple(TD.LONG))
def test_long_lists_and_early_termination(oracle, which):
    """Tile lists of thousands of entries (dozens of staging batches), pixels that end after more than 128 contributors: the
    pixels where the two sides demonstrably decided differently, or may have, carry no upstream gradient and are left out
    of the map comparison."""
    from casualhdrsplat_amd import inspect_state
    c = TD.case(oracle, which)
    sc, f = c["sc"], c["fwds"][0]
    lens = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).max()
    assert lens > 1500 and int(f["n_contrib"].max()) > 128, (lens, int(f["n_contrib"].max()))
    out, _, lv = _forward(sc)
    st = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in inspect_state(out[0]).items()}
    m = Hh.decision_masks(oracle, sc, [f], st, what=which)
    share = float(m["excluded"].mean())
    assert share <= 0.01, (which, share)
    gammas = c["gammas"] * (~m["excluded"])[None]
    got = _grads(out[0], lv, gammas)
    _hold_to_the_bound("long_" + which, got, _truth(oracle, which, gammas=gammas), pixels=~m["excluded"])
    for k in KEYS:
        assert np.abs(got["d_" + k]).max() > 1e-3, k


# ---- 3. cross-checks inside the library ----

def test_the_moment_is_the_rasterizers_own_inverse_depth_image(oracle):
    """Two fp32 evaluations of sum w / z, each within the bound of the truth: twice the bound between them."""
    from casualhdrsplat_amd import distortion_loss
    c = TD.case(oracle, "b")
    out, _, lv = _forward(c["sc"], return_invdepth=True)
    dmap = distortion_loss(out[0], _geo(lv))
    own = out[-1].detach().cpu().numpy()
    moment = dmap.grad_fn.moment.cpu().numpy()[0]
    ref = _truth(oracle, "b")
    assert own.shape == moment.shape and own.max() > 0.1
    excess = np.abs(own.astype(np.float64) - moment) - 2e-4 * np.abs(ref["moment"][0])
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(excess > 0, excess / (2.0 ** -24 * ref["S_moment"][0]), 0.0)
    need = float(np.nan_to_num(need, nan=np.inf).max())
    _PARITY["invdepth_b"] = dict(moment=round(need, 4))
    assert need <= 2 * Hh.C_BOUND, need


def test_one_depth_plane_gives_a_zero_map(oracle):
    """Every Gaussian on one view-space depth: the map is zero within the bound (the fp32 depths differ by ulps), while the
    moment is the accumulated opacity over that depth."""
    from casualhdrsplat_amd import inspect_state
    c = TD.case(oracle, "plane")
    out, _, lv = _forward(c["sc"])
    st = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in inspect_state(out[0]).items()}
    keep = ~Hh.decision_masks(oracle, c["sc"], c["fwds"], st, what="plane")["excluded"]
    got = _grads(out[0], lv, c["gammas"])
    ref = _truth(oracle, "plane")
    z0 = TD.PLANE[5]
    assert ref["S_out"].max() > 1.0 and np.abs(got["moment"][0] * z0 - (1 - st["final_T"][0]))[keep].max() < 1e-4
    need = TD.needed(got["out"][0][keep], np.zeros(int(keep.sum())), ref["S_out"][0][keep])
    _PARITY["plane"] = dict(out=round(need, 4))
    assert need <= Hh.C_BOUND, need


def test_opacity_gradient_is_the_adjoint_of_the_map(oracle):
    """For a random direction delta on the opacities, sum(gamma * map) at opacity +- eps delta differs by 2 eps <grad, delta>
    within the summed bound of the map and of the gradient.  The map is discontinuous in the opacities wherever an entry
    crosses the 1 / 255 threshold at a pixel, and ONE such flip moves sum(gamma * map) by up to 1e-3 on this scene: eps has
    to be small enough that no decision flips (1e-6: verified by equal n_contrib on the GPU, and by equal contributor counts
    at every pixel in the reference), which leaves a difference of 1e-6 -- far inside the summed bound (0.1).  The test
    can therefore fail only on a gross error; both numbers are printed and recorded."""
    import copy
    from casualhdrsplat_amd import distortion_loss, inspect_state
    c = TD.case(oracle, "b")
    sc, gam = c["sc"], c["gammas"]
    ref = _truth(oracle, "b")
    base = _run(sc, gam)
    delta = np.random.default_rng(71).standard_normal(tuple(sc.opacities.shape))
    eps = ADJOINT_EPS
    ops = [(sc.opacities.double() + sign * eps * torch.as_tensor(delta)).float() for sign in (1.0, -1.0)]
    delta = ((ops[0].double() - ops[1].double()) / (2 * eps)).numpy()        # the step the float32 opacities really take
    count0 = DR.distortion(c["fwds"][0], c["W"], c["H"])["count"]
    val = []
    for op in ops:
        assert float(op.min()) > 0 and float(op.max()) < 1
        moved = copy.copy(sc)
        moved.opacities = op
        f, _ = Hh.run_oracle(oracle, moved, backward=False)
        assert (DR.distortion(f, c["W"], c["H"])["count"] == count0).all()      # no decision flips in the reference ...
        out, _, _ = _forward(sc, leaves=_leaves(sc, opacities=op))
        assert (inspect_state(out[0])["n_contrib"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF == base["n_contrib"]).all()
        val.append(float((distortion_loss(out[0]).double().cpu().numpy() * gam).sum()))
    fd = 0.5 * (val[0] - val[1])
    g = base["d_opacities"].astype(np.float64)
    lin = eps * float((g * delta.reshape(g.shape)).sum())
    unit = Hh.C_BOUND * 2.0 ** -24
    tol = float((np.abs(gam) * (1e-4 * np.abs(ref["out"]) + unit * ref["S_out"])).sum())
    tol += eps * float((np.abs(delta.reshape(g.shape)) * (1e-4 * np.abs(ref["dL_dopacity"]) + unit * ref["abs_dL_dopacity"])).sum())
    print(f"adjoint: difference {fd:.6e}, eps <grad, delta> {lin:.6e}, summed bound {tol:.3e}", flush=True)
    _PARITY["adjoint_b"] = dict(difference=float(f"{fd:.4e}"), eps_grad_delta=float(f"{lin:.4e}"), summed_bound=float(f"{tol:.4e}"))
    assert lin != 0 and abs(fd - lin) <= tol, (fd, lin, tol)


ADJOINT_EPS = 1e-6


# ---- 4. poses and frames ----

def test_one_call_over_three_poses(oracle):
    c = TD.case(oracle, "posed")
    got = _run(c["sc"], c["gammas"][:3], cameras=c["cams"][:3])
    assert got["out"].shape[0] == 3
    _hold_to_the_bound("poses_3", got, _truth(oracle, "posed", poses=(0, 1, 2)))
    # each pose's map is that of a call on that pose alone
    for k in range(3):
        out, _, _ = _forward(c["sc"], cameras=c["cams"][k:k + 1])
        from casualhdrsplat_amd import distortion_loss
        alone = distortion_loss(out[0])
        assert poison.bytes_of(alone[0]) == poison.bytes_of(got["out"][k]), k


def test_two_frames_of_two_poses(oracle):
    c = TD.case(oracle, "posed")
    got = _run(c["sc"], c["gammas"], cameras=c["cams"], n_frames=2)
    assert got["out"].shape[0] == 4
    _hold_to_the_bound("frames_2x2", got, _truth(oracle, "posed"))


# ---- 5. autograd ----

def _both_losses(sc, gam, w_img, rast=None):
    from casualhdrsplat_amd import distortion_loss
    out, rast, lv = _forward(sc)
    dmap = distortion_loss(out[0], _geo(lv))
    return (out[0] * w_img).sum(), (dmap * _dev(gam).reshape(dmap.shape)).sum(), lv, dmap, out, rast


def test_the_two_losses_add_on_every_leaf_and_the_order_does_not_matter(oracle):
    from casualhdrsplat_amd import distortion_loss
    c = TD.case(oracle, "b")
    sc, gam = c["sc"], c["gammas"]
    w_img = _dev(np.random.default_rng(72).standard_normal((3, c["H"], c["W"])))
    wrt = lambda lv: [lv[k] for k in KEYS]
    # the rasterizer's backward first (its node frees its saved tensors), then the distortion's
    img, dl, lv, dmap, _, _ = _both_losses(sc, gam, w_img)
    g_img = torch.autograd.grad(img, wrt(lv))
    g_dist = torch.autograd.grad(dl, wrt(lv))
    # the other way round, on a forward of its own: the same bits (the two share no pair flags)
    img, dl, lv2, _, _, _ = _both_losses(sc, gam, w_img)
    h_dist = torch.autograd.grad(dl, wrt(lv2))
    h_img = torch.autograd.grad(img, wrt(lv2))
    for k, a, b, p, q in zip(KEYS, g_dist, h_dist, g_img, h_img):
        assert poison.bytes_of(a) == poison.bytes_of(b) and a.abs().max() > 1e-3, k
        assert poison.bytes_of(p) == poison.bytes_of(q) and p.abs().max() > 1e-3, k
    # one backward of the sum leaves, on each leaf, exactly the sum of the two
    img, dl, lv3, _, out, rast = _both_losses(sc, gam, w_img)
    # ... and it works after a second forward of the same rasterizer: the node holds the state of ITS forward
    other = _leaves(sc, grad=False)
    with torch.no_grad():
        rast(other["means3D"] + 0.05, other["means2D"], other["opacities"] * 0.5, shs=other["shs"], scales=other["scales"],
             rotations=other["rotations"])
    (img + dl).backward()
    for k, a, b in zip(KEYS, g_img, g_dist):
        assert poison.bytes_of(lv3[k].grad) == poison.bytes_of(a + b), k
    # the evaluation form: the same map bits, no gradient
    out, _, lv4 = _forward(sc)
    plain = distortion_loss(out[0])
    assert plain.requires_grad is False and plain.grad_fn is None
    assert poison.bytes_of(plain) == poison.bytes_of(dmap) == poison.bytes_of(distortion_loss(out[0], _geo(lv4)))


def test_keep_state_rasterizer_after_a_no_grad_forward_gives_the_same_map(oracle):
    from casualhdrsplat_amd import GaussianRasterizer, distortion_loss
    c = TD.case(oracle, "b")
    sc = c["sc"]
    out, _, _ = _forward(sc)
    want = distortion_loss(out[0])
    rs, _, _ = Hh.settings_from_scene(sc, DEV)
    rast = GaussianRasterizer(rs, keep_state=True)
    lv = _leaves(sc, grad=False)
    with torch.no_grad():
        rast(lv["means3D"], lv["means2D"], lv["opacities"], shs=lv["shs"], scales=lv["scales"], rotations=lv["rotations"])
    got = distortion_loss(rast)
    assert not got.requires_grad and poison.bytes_of(got) == poison.bytes_of(want)
    with pytest.raises(ValueError, match="keep_state rasterizer"):
        distortion_loss(rast, _geo(lv))


# ---- 6. parameterization="raw", with and without filter_3D; antialiasing ----

@pytest.mark.parametrize("filtered", (False, True))
def test_raw_parameterization_is_the_activated_result_pushed_through_the_activations(oracle, filtered):
    from casualhdrsplat_amd import _lib as L
    c = TD.case(oracle, "b")
    sc, gam = c["sc"], c["gammas"]
    P = TD.GUARDED["b"][0]
    x = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))
    l = torch.log(sc.scales)
    q = sc.rotations * 1.7
    filt = torch.full((P,), 0.02, device=DEV) if filtered else None
    kw = dict(parameterization="raw", **(dict(filter_3D=filt) if filtered else {}))
    out, _, lv = _forward(sc, leaves=_leaves(sc, opacities=x, scales=l, rotations=q), **kw)
    raw = _grads(out[0], lv, gam)
    saved = out[0].grad_fn.saved_tensors
    acts = dict(opacities=saved[1].detach().clone(), scales=saved[4].detach().clone(), rotations=saved[5].detach().clone())
    out2, _, lv2 = _forward(sc, leaves=_leaves(sc, **acts))
    act = _grads(out2[0], lv2, gam)
    _same_bits(raw, act, ("out", "moment", "means3D"))
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


def test_an_antialiased_forward_is_held_to_the_truth(oracle):
    c = TD.case(oracle, "aa")
    f = c["fwds"][0]
    assert not oracle.threshold_risk(Hh.oracle_camera(oracle, c["sc"]), f, 2e-5, 1e-4)["n_risky_pixels"]
    got = _run(c["sc"], c["gammas"])
    ref = _truth(oracle, "aa")
    assert (got["n_contrib"] == ref["n_contrib"]).all()
    _hold_to_the_bound("antialias", got, ref)


# ---- 7. reproducibility and robustness ----

def test_results_do_not_depend_on_what_the_buffers_held(oracle, monkeypatch):
    from casualhdrsplat_amd import distortion
    c = TD.case(oracle, "b")
    sc, gam = c["sc"], c["gammas"]
    out, _, lv = _forward(sc)
    results = {}
    for pattern in ("zero", "ff", "nan", "a5", "random"):
        distortion._WORKSPACES.clear()
        with poison.poisoned(monkeypatch, pattern) as session:
            results[pattern] = _grads(out[0], lv, gam)
        fills = session.require(DISTORTION, roles=("distortion_workspace#0", "_distortion_forward#0", "_distortion_forward#1"),
                                at_least=7)
        assert {f.nbytes for f in fills} >= {4 * results[pattern]["d_" + k].size for k in KEYS} | {4 * gam.size}
    distortion._WORKSPACES.clear()
    for pattern, got in results.items():
        _same_bits(got, results["zero"])
    # twice the same bits, from a forward of its own
    _same_bits(_run(sc, gam), results["zero"])
    # a cached workspace left by a call of other dims (the cache is keyed by dims: make the one of THESE dims hold its bytes)
    p = TD.case(oracle, "plane")
    _run(p["sc"], p["gammas"])
    other = next(ws for key, ws in distortion._WORKSPACES.items() if ws.numel())
    st = out[0].grad_fn.st
    mine = distortion.distortion_workspace(st.dims, st.geom.device)
    poison.fill_(mine, "stale", stale=other)
    _same_bits(_grads(out[0], lv, gam), results["zero"])
    # ... and one left by a call under another gradient
    _grads(out[0], lv, -3.0 * gam)
    _same_bits(_grads(out[0], lv, gam), results["zero"])
    # a frame with empty tiles and with Gaussians that are on lists but composited nowhere
    from casualhdrsplat_amd import synthetic as S
    P, W, H = 24, 104, 72
    sc = S.make_scene(P, W, H, 1, seed=5)
    sc.opacities[::4] = 0.002
    g2 = np.random.default_rng(73).standard_normal((1, H, W)).astype(np.float32)
    out, _, lv = _forward(sc)
    sparse = {}
    for pattern in ("zero", "nan", "random"):
        distortion._WORKSPACES.clear()
        with poison.poisoned(monkeypatch, pattern):
            sparse[pattern] = _grads(out[0], lv, g2)
        _same_bits(sparse[pattern], sparse["zero"])
    distortion._WORKSPACES.clear()
    assert all(np.isfinite(sparse["zero"]["d_" + k]).all() for k in KEYS) and np.abs(sparse["zero"]["d_means3D"]).max() > 1e-4
    empty = sparse["zero"]["n_contrib"][0] == 0
    assert empty.any() and not sparse["zero"]["out"][0][empty].any() and not np.signbit(sparse["zero"]["out"]).any()


def test_an_overflowed_frame_gives_zeros_and_full_capacity_gives_the_plain_call(oracle):
    c = TD.case(oracle, "b")
    sc, gam = c["sc"], c["gammas"]
    plain = _run(sc, gam)
    # sync-free mode, capacity far below the frame's pairs: with grad nobody looks at the counters before the backward
    over = _run(sc, gam, state=False, capacity=256)
    for k in ("out", "moment") + tuple("d_" + k for k in KEYS):
        assert poison.bytes_of(over[k]) == bytes(4 * over[k].size), k
    # the same mode with room for every pair
    _same_bits(_run(sc, gam, capacity=1 << 18), plain)
