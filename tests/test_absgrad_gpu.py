"""GPU checks of the absolute screen-gradient statistic (absgrad.hip through importance.accumulate_abs_gradients and through
the backward of a GaussianRasterizer given a DensifyStats(absgrad=True)) against the float64 restatement of its definition
(tests/absgrad_reference.py) and against itself.

Bound, per Gaussian:  |hip - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S  with helpers.C_BOUND (8) as it stands and S the
restatement's magnitude sums (every signed quantity replaced by its magnitude, each term weighted by 4 + the contributors of
its pixel, through the square root).  With HS_PARITY_REPORT=1 in the environment the largest observed
(|hip - ref| - 1e-4 |ref|) / (2^-24 S) of every case goes to profiles/absgrad_parity.json.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import absgrad_reference as R
import densify_reference as DR
import helpers as Hh
import poison
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPORTANCE = "casualhdrsplat_amd.importance"
_PARITY = {}


def _leaves(sc, grad=True, **replace):
    t = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=sc.scales,
             rotations=sc.rotations)
    t.update(replace)
    return {k: v.detach().clone().to(DEV).requires_grad_(grad) for k, v in t.items()}


def _forward(sc, cameras=None, n_frames=1, hdr=False, blur_domain="ldr", exposures=None, leaves=None, settings=None, **rast_kw):
    """One forward of the scene with grad; returns (the outputs, the rasterizer, the leaves)."""
    from casualhdrsplat_amd import GaussianRasterizer
    rs, _, _ = Hh.settings_from_scene(sc, DEV, cameras, hdr=hdr, blur_domain=blur_domain)
    if n_frames > 1:
        rs = rs._replace(n_frames=n_frames)
    if exposures is not None:
        rs = rs._replace(exposure=torch.tensor(list(exposures) if n_frames > 1 else float(exposures[0]), device=DEV))
    if settings:
        rs = rs._replace(**settings)
    rast = GaussianRasterizer(rs, **rast_kw)
    lv = leaves if leaves is not None else _leaves(sc)
    a = dict(lv)
    out = rast(a.pop("means3D"), a.pop("means2D"), a.pop("opacities"), **a)
    return out, rast, lv


def _t(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(DEV)


def _accumulate(handle, dL, P=None, target=None, **kw):
    from casualhdrsplat_amd import accumulate_abs_gradients
    target = target if target is not None else torch.zeros(P, dtype=torch.float32, device=DEV)
    accumulate_abs_gradients(handle, _t(dL), target, **{k: _t(v) for k, v in kw.items()})
    return target


def _np(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _state(handle):
    from casualhdrsplat_amd import inspect_state
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in inspect_state(handle).items()}


def _hold_to_the_bound(name, got, frames):
    """abs_grad_accum of a call on a zeroed array against the float64 restatement (`frames`: one R.statistic per frame)."""
    want = R.accumulate(np.zeros_like(frames[0]["a"]), frames)
    S_ = sum(fr["S"] for fr in frames)
    hit = np.zeros_like(frames[0]["hit"])
    for fr in frames:
        hit |= fr["hit"]
    c = R.needed_constant(got, want, S_)
    rel = float((np.abs(got - want)[hit] / np.maximum(want[hit], 1e-300)).max())
    _PARITY[name] = dict(C_needed=round(c, 4), max_relative_difference=float(f"{rel:.3e}"), gaussians_reached=int(hit.sum()), pairs=int(sum(fr.get("pairs", 0) for fr in frames)))
    print(f"absgrad parity {name}: C needed {c:.3f}, largest relative difference {rel:.2e}, Gaussians with a term {int(hit.sum())}", flush=True)
    assert hit.sum() > 50 and (want[hit] > 0).any()
    assert not got[~hit].any(), (name, "a Gaussian without a term received something")
    assert c <= Hh.C_BOUND, (name, c)


def _frame_stat(poses):
    st = R.statistic(poses)
    st["pairs"] = sum(p["pairs"] for p in poses)
    return st


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    if os.environ.get("HS_PARITY_REPORT") and _PARITY:
        with open(os.path.join(ROOT, "profiles", "absgrad_parity.json"), "w") as fh:
            json.dump(dict(bound="|hip - ref| <= 1e-4 |ref| + C 2^-24 S; the largest C any Gaussian needs, per case (C_BOUND = 8)",
                           cases=_PARITY), fh, indent=1, sort_keys=True)
            fh.write("\n")


# ---- 1. guarded scenes: no pixel in the threshold band, every fp32 implementation decides alike ----

GUARDED = {"a": (1000, 128, 128, 3), "b": (600, 104, 72, 1)}


@pytest.fixture(scope="module")
def guarded(oracle):
    out = {}
    for k, (P, W, H, deg) in GUARDED.items():
        sc, seed = Hh.guarded_scene(oracle, P, W, H, deg)
        f, _ = Hh.run_oracle(oracle, sc, backward=False)
        dL = sc.dL_dimage.numpy()
        out[k] = dict(sc=sc, f=f, dL=dL, ref=R.abs_gradients(f, W, H, dL, sc.bg.numpy()), seed=seed)
    assert out["b"]["seed"] == 0
    return out


@pytest.mark.parametrize("which", tuple(GUARDED))
def test_guarded_scene_against_the_restatement(guarded, which):
    g = guarded[which]
    P, W, H, _ = GUARDED[which]
    out, _, _ = _forward(g["sc"])
    got = _np(_accumulate(out[0], g["dL"], P))
    _hold_to_the_bound(f"guarded_{which}_ldr", got, [_frame_stat([g["ref"]])])


def _crf_masked(oracle, sc, fwds, out, cams, blur_domain, what):
    """decision_masks of an HDR frame (compositing decisions and CRF intervals), from the forward's own images."""
    st = _state(out[0])
    N = len(fwds)
    if blur_domain == "ldr" or N == 1:
        crf_got = [st["pose_hdr"][k] for k in range(N)] if N > 1 else [_np(out[2])]
        crf_ref = [f["color"] for f in fwds]
    else:
        crf_got = [_np(out[2])]
        crf_ref = [np.mean(np.stack([f["color"] for f in fwds]), axis=0, dtype=np.float64).astype(np.float32)]
    m = Hh.decision_masks(oracle, sc, fwds, st, cams=cams, crf_got=crf_got, crf_ref=crf_ref, what=what)
    share = float(m["excluded"].mean())
    print(f"{what}: excluded share {share:.4f}", flush=True)
    return m, share


def test_guarded_scene_hdr_and_crf_against_the_restatement(oracle):
    """The HDR + CRF path at 104 x 72: dL/dH is the oracle's tone-map under float64 autograd; dL is zeroed on the pixels whose
    CRF interval is not provably the same on both sides (helpers.crf_interval_risk: the slope is a decision)."""
    from oracle import torch_rasterizer as T
    P, W, H, deg = GUARDED["b"]
    sc, _ = Hh.guarded_scene(oracle, P, W, H, deg, hdr=True)
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    out, _, _ = _forward(sc, hdr=True)
    m, share = _crf_masked(oracle, sc, [f], out, None, "ldr", "guarded_b_hdr")
    assert share <= 0.01
    rng = np.random.default_rng(11)
    dL = sc.dL_dimage.numpy() * (~m["excluded"])[None]
    dL_hdr = (rng.standard_normal((3, H, W)) * 0.1).astype(np.float32) * (~m["excluded"])[None]
    got = _np(_accumulate(out[0], dL, P, dL_dout_hdr=dL_hdr))
    dH = R.hdr_pose_gradients(T, sc, [f], dL, dL_hdr=dL_hdr)
    _hold_to_the_bound("guarded_b_hdr_crf", got, [_frame_stat([R.abs_gradients(f, W, H, dH[0], sc.bg.numpy())])])


# ---- 2. long lists, batch boundaries, early termination ----

LONG = {"deep": (6000, 64, 64, 0), "rows": (3000, 48, 40, 1)}


@pytest.mark.parametrize("which", tuple(LONG))
def test_long_lists_and_early_termination(oracle, which):
    """Tile lists of thousands of entries (many staging batches), pixels that terminate after hundreds of contributors: dL is
    zero, on both sides, on the pixels where the two sides demonstrably decided differently."""
    P, W, H, deg = LONG[which]
    sc = S.make_scene(P, W, H, deg, seed=0)
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    lens = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).max()
    assert lens > 1500 and int(f["n_contrib"].max()) > 128, (lens, int(f["n_contrib"].max()))
    out, _, _ = _forward(sc)
    m = Hh.decision_masks(oracle, sc, [f], _state(out[0]), what=which)
    share = float(m["excluded"].mean())
    print(f"{which}: excluded share {share:.4f}, band {float(m['pix_risk'].mean()):.4f}, longest list {lens}", flush=True)
    assert share <= 0.01, (which, share)
    dL = sc.dL_dimage.numpy() * (~m["excluded"])[None]
    got = _np(_accumulate(out[0], dL, P))
    _hold_to_the_bound(f"long_{which}", got, [_frame_stat([R.abs_gradients(f, W, H, dL, sc.bg.numpy())])])


# ---- 3. poses and frames ----

@pytest.fixture(scope="module")
def posed(oracle):
    P, W, H = 1500, 72, 56
    sc = S.make_scene(P, W, H, 1, seed=3, hdr=True)
    cams = S.blur_poses(W, H, 4, step=0.03)
    fwds = [Hh.run_oracle(oracle, sc, cam=c, backward=False)[0] for c in cams]
    return sc, cams, fwds, (P, W, H)


@pytest.mark.parametrize("blur_domain", ("ldr", "hdr"))
def test_one_call_over_three_poses_against_the_restatement(oracle, posed, blur_domain):
    from oracle import torch_rasterizer as T
    sc, cams, fwds, (P, W, H) = posed
    cams, fwds = cams[:3], fwds[:3]
    out, _, _ = _forward(sc, cameras=cams, hdr=True, blur_domain=blur_domain)
    m, share = _crf_masked(oracle, sc, fwds, out, cams, blur_domain, f"posed_{blur_domain}")
    assert share <= 0.05
    dL = sc.dL_dimage.numpy() * (~m["excluded"])[None]
    got = _np(_accumulate(out[0], dL, P))
    dH = R.hdr_pose_gradients(T, sc, fwds, dL, blur_domain=blur_domain)
    poses = [R.abs_gradients(f, W, H, dH[k], sc.bg.numpy()) for k, f in enumerate(fwds)]
    _hold_to_the_bound(f"three_poses_blur_{blur_domain}", got, [_frame_stat(poses)])


@pytest.mark.parametrize("hdr", (False, True))
def test_two_frames_of_two_poses_are_two_calls(posed, hdr):
    sc, cams, _, (P, W, H) = posed
    rng = np.random.default_rng(4)
    dL = rng.standard_normal((2, 3, H, W)).astype(np.float32)
    dLh = rng.standard_normal((2, 3, H, W)).astype(np.float32) * 0.1 if hdr else None
    expo = (0.5, 1.25)
    kw = dict(hdr=True, blur_domain="hdr") if hdr else {}
    out, _, _ = _forward(sc, cameras=cams, n_frames=2, exposures=expo if hdr else None, **kw)
    both = _np(_accumulate(out[0], dL, P, **(dict(dL_dout_hdr=dLh) if hdr else {})))
    acc = torch.zeros(P, dtype=torch.float32, device=DEV)
    for fr in range(2):
        o1, _, _ = _forward(sc, cameras=cams[2 * fr:2 * fr + 2], exposures=expo[fr:fr + 1] if hdr else None, **kw)
        _accumulate(o1[0], dL[fr], target=acc, **(dict(dL_dout_hdr=dLh[fr]) if hdr else {}))
    assert poison.bytes_of(both) == poison.bytes_of(_np(acc))
    assert (both > 0).sum() > 100
    # the gradient image is per frame: the other way round it is another result
    assert poison.bytes_of(both) != poison.bytes_of(_np(_accumulate(out[0], dL[::-1].copy(), P, **(dict(dL_dout_hdr=dLh) if hdr else {}))))
    with pytest.raises(ValueError, match="dL_dout must have shape"):
        _accumulate(out[0], dL[0], P)
    with pytest.raises(ValueError, match="per-image gradients"):
        _accumulate(out[0], dL, P, dL_dout_alpha=np.zeros((H, W), np.float32))


# ---- 4. wiring ----

def _step(sc, dL, absgrad, **fw):
    """One forward + backward through autograd with a DensifyStats; returns (stats, gradients by leaf, outputs)."""
    from casualhdrsplat_amd import DensifyStats
    P = sc.means3D.shape[0]
    stats = DensifyStats(P, DEV, absgrad=absgrad)
    out, rast, lv = _forward(sc, densify_stats=stats, **fw)
    (out[0] * _t(dL)).sum().backward()
    torch.cuda.synchronize()
    return stats, {k: v.grad.detach().clone() for k, v in lv.items() if v.grad is not None}, out


def test_the_hooked_backward_is_the_standalone_call_and_changes_nothing_else(guarded):
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    with_abs, grads_a, out = _step(g["sc"], g["dL"], True)
    without, grads_b, _ = _step(g["sc"], g["dL"], False)
    assert without.abs_grad_accum is None
    alone = _accumulate(out[0], g["dL"], P)
    assert poison.bytes_of(with_abs.abs_grad_accum) == poison.bytes_of(alone) and (_np(alone) > 0).sum() > 300
    for name in ("grad_accum", "denom", "max_radii"):
        assert poison.bytes_of(getattr(with_abs, name)) == poison.bytes_of(getattr(without, name)), name
    assert set(grads_a) == set(grads_b) and len(grads_a) >= 6
    for k in grads_a:
        assert poison.bytes_of(grads_a[k]) == poison.bytes_of(grads_b[k]), k
    # the statistic is the larger one, and mean_abs_grad divides by the shared denominator
    assert (_np(with_abs.abs_grad_accum) >= _np(with_abs.grad_accum) * (1 - 1e-5)).all()
    assert poison.bytes_of(with_abs.mean_abs_grad()) == poison.bytes_of(with_abs.abs_grad_accum / with_abs.denom.clamp_min(1.0))
    # a second backward accumulates
    out2, rast2, lv2 = _forward(g["sc"], densify_stats=with_abs)
    (out2[0] * _t(g["dL"])).sum().backward()
    assert poison.bytes_of(with_abs.abs_grad_accum) == poison.bytes_of(alone + alone)
    # a statistics object of another size is refused
    from casualhdrsplat_amd import DensifyStats
    bad = DensifyStats(P, DEV, absgrad=True)
    bad.abs_grad_accum = torch.zeros(P + 1, device=DEV)
    out3, _, _ = _forward(g["sc"], densify_stats=bad)
    with pytest.raises(ValueError, match="abs_grad_accum must be"):
        (out3[0] * _t(g["dL"])).sum().backward()


def test_raw_parameterization_gives_the_same_array(guarded):
    from casualhdrsplat_amd import inspect_state
    g = guarded["b"]
    sc = g["sc"]
    x = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))
    raw_stats, _, raw_out = _step(sc, g["dL"], True, leaves=_leaves(sc, opacities=x, scales=torch.log(sc.scales), rotations=sc.rotations * 1.7),
                                  parameterization="raw")
    st = inspect_state(raw_out[0])
    acts = {k: st[k].detach().clone() for k in ("opacities", "scales", "rotations")}
    plain_stats, _, _ = _step(sc, g["dL"], True, leaves=_leaves(sc, **acts))
    assert poison.bytes_of(raw_stats.abs_grad_accum) == poison.bytes_of(plain_stats.abs_grad_accum)
    assert (_np(raw_stats.abs_grad_accum) > 0).sum() > 300


# ---- 5. robustness ----

def test_twice_the_same_bits_accumulation_and_untouched_gaussians(guarded):
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    sc = copy.copy(g["sc"])
    sc.means3D = sc.means3D.clone()
    sc.means3D[:7, 2] = -sc.means3D[:7, 2]            # seven Gaussians behind the camera: on no tile's list
    out, _, _ = _forward(sc)
    first = _accumulate(out[0], g["dL"], P)
    again = _accumulate(out[0], g["dL"], P)
    assert poison.bytes_of(first) == poison.bytes_of(again) and (_np(first) > 0).sum() > 300
    twice = _accumulate(out[0], g["dL"], target=first.clone())
    assert poison.bytes_of(twice) == poison.bytes_of(first + first)        # the same increment: x + x is exact
    held = torch.empty(P, dtype=torch.float32, device=DEV)
    poison.fill_(held, "a5")
    before = _np(held).copy()
    after = _np(_accumulate(out[0], g["dL"], target=held))
    untouched = _np(first) == 0
    assert untouched[:7].all() and poison.bytes_of(after[untouched]) == poison.bytes_of(before[untouched])
    assert poison.bytes_of(after[~untouched]) == poison.bytes_of((before + _np(first))[~untouched])
    nan = torch.empty(P, dtype=torch.float32, device=DEV)
    poison.fill_(nan, "ff")                                                 # a NaN with a payload
    assert poison.bytes_of(_np(_accumulate(out[0], g["dL"], target=nan))[:7]) == b"\xff" * 28


def test_result_does_not_depend_on_what_the_workspace_held(guarded, monkeypatch):
    from casualhdrsplat_amd import importance
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    out, _, _ = _forward(g["sc"])
    results = {}
    for pattern in ("zero", "ff", "nan", "a5", "one", "random"):
        importance._ABS_WORKSPACES.clear()
        target = torch.zeros(P, dtype=torch.float32, device=DEV)
        with poison.poisoned(monkeypatch, pattern) as session:
            results[pattern] = _np(_accumulate(out[0], g["dL"], target=target))
        fills = session.require(IMPORTANCE, roles=("abs_gradient_workspace#0",))
        assert fills[0].nbytes >= 8 * P
    importance._ABS_WORKSPACES.clear()
    for pattern, got in results.items():
        assert poison.bytes_of(got) == poison.bytes_of(results["zero"]), pattern
    # ... and the cached workspace, as an earlier call under another gradient left it, is as good as a fresh one
    _accumulate(out[0], -3.0 * g["dL"], P)
    assert poison.bytes_of(_np(_accumulate(out[0], g["dL"], P))) == poison.bytes_of(results["zero"])


def test_an_overflowed_frame_adds_nothing_and_its_replay_adds_what_a_plain_call_adds(guarded):
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    plain = _np(_accumulate(_forward(g["sc"])[0][0], g["dL"], P))
    # sync-free mode, capacity far below the frame's pairs: with grad nobody looks at the counters before the backward
    out, rast, _ = _forward(g["sc"], capacity=256, keep_state=True)
    held = torch.full((P,), 1.5, dtype=torch.float32, device=DEV)
    assert poison.bytes_of(_np(_accumulate(out[0], g["dL"], target=held))) == poison.bytes_of(np.full(P, 1.5, np.float32))
    # under no_grad the rasterizer grows the capacity and renders the frame again by itself
    a = _leaves(g["sc"], grad=False)
    with torch.no_grad():
        rast(a.pop("means3D"), a.pop("means2D"), a.pop("opacities"), **a)
    assert rast.overflow_replays >= 1 and int(rast.capacity) > 256
    assert poison.bytes_of(plain) == poison.bytes_of(_np(_accumulate(rast, g["dL"], P)))


# ---- 6. optional gradients ----

def test_alpha_and_inverse_depth_gradients_together(guarded):
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    sc = copy.copy(g["sc"])
    sc.bg = torch.tensor([0.3, 0.1, 0.6])             # (the background colour changes no decision)
    rng = np.random.default_rng(7)
    dA = rng.standard_normal((H, W)).astype(np.float32)
    dD = rng.standard_normal((H, W)).astype(np.float32)
    out, _, lv = _forward(sc, return_alpha=True, return_invdepth=True)
    got = _np(_accumulate(out[0], g["dL"], P, dL_dout_alpha=dA, dL_dout_invdepth=dD))
    ref = R.abs_gradients(g["f"], W, H, g["dL"], sc.bg.numpy(), dL_alpha=dA, dL_invdepth=dD)
    _hold_to_the_bound("guarded_b_alpha_invdepth", got, [_frame_stat([ref])])
    assert poison.bytes_of(got) != poison.bytes_of(_np(_accumulate(out[0], g["dL"], P)))
    # ... and through autograd: the hooked backward hands the same three gradients over
    from casualhdrsplat_amd import DensifyStats
    stats = DensifyStats(P, DEV, absgrad=True)
    out2, _, _ = _forward(sc, return_alpha=True, return_invdepth=True, densify_stats=stats)
    assert len(out2) == 4
    ((out2[0] * _t(g["dL"])).sum() + (out2[2] * _t(dA)).sum() + (out2[3] * _t(dD)).sum()).backward()
    assert poison.bytes_of(_np(stats.abs_grad_accum)) == poison.bytes_of(got)


# ---- 7. policy ----

def test_densify_and_prune_selects_by_the_absolute_statistic():
    from casualhdrsplat_amd import DensifyStats, GaussianAdam, cloud_param_groups, densify_and_prune
    P = 10007
    case = DR.make_case(P, 4, seed=DR.case_seed(P, 4))
    rng = np.random.default_rng(9)
    absg = (np.nan_to_num(case["grad_accum"], nan=1e-4)[rng.permutation(P)] * 3.0).astype(np.float32)
    absg[case["denom"] == 0] = 0.0

    def run(absgrad, with_array=True):
        t = {k: torch.tensor(v, device=DEV).requires_grad_(True) for k, v in case["cloud"].items()}
        opt = GaussianAdam(cloud_param_groups(*[t[k] for k in DR.NAMES]), eps=1e-15)
        opt.prepare()
        stats = DensifyStats(P, DEV, absgrad=with_array)
        stats.grad_accum.copy_(torch.tensor(case["grad_accum"]))
        stats.denom.copy_(torch.tensor(case["denom"]))
        stats.max_radii.copy_(torch.tensor(case["max_radii"]))
        if with_array:
            stats.abs_grad_accum.copy_(torch.tensor(absg))
        mean_abs = _np(stats.mean_abs_grad()) if with_array else None
        res = densify_and_prune(opt, stats, noise=torch.tensor(case["noise"], device=DEV), absgrad=absgrad, **case["policy"])
        assert stats.abs_grad_accum is None or (tuple(stats.abs_grad_accum.shape) == (res.counts["P_out"],) and not stats.abs_grad_accum.any())
        return res, mean_abs

    th = DR.thresholds(**case["policy"])
    res_abs, mean_abs = run(True)
    c = case["cloud"]
    _, row_map, counts = DR.plan(mean_abs, np.ones(P, np.float32), case["max_radii"], c["opacities"], c["scales"], th)
    assert np.array_equal(res_abs.row_map.cpu().numpy().view(np.uint32), row_map)
    assert [res_abs.counts[k] for k in ("P_out", "survivors", "clones", "children")] == counts[:4]
    # ... the same rows as the accumulated array over the shared denominator, and other rows than the signed statistic selects
    _, row_map2, _ = DR.plan(absg, case["denom"], case["max_radii"], c["opacities"], c["scales"], th)
    assert np.array_equal(row_map, row_map2)
    res_signed, _ = run(False)
    _, row_map_signed, _ = DR.plan(case["grad_accum"], case["denom"], case["max_radii"], c["opacities"], c["scales"], th)
    assert np.array_equal(res_signed.row_map.cpu().numpy().view(np.uint32), row_map_signed)
    assert not np.array_equal(row_map, row_map_signed)
    with pytest.raises(ValueError, match="absgrad=True needs stats.abs_grad_accum"):
        run(True, with_array=False)
