"""GPU checks of the blending-weight statistics (contrib.hip through importance.accumulate_contributions) against the
float64 restatement of their definition (tests/contribution_reference.py) and against themselves.

Bound, per Gaussian:  |hip - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S  for weight_sum, with helpers.C_BOUND (8) as it stands and
S = sum of |e| w (4 + contributors composited before the entry at that pixel); for weight_max the same with the S of the
single largest term; pixel_count is exact.  With HS_PARITY_REPORT=1 in the environment the largest observed
(|hip - ref| - 1e-4 |ref|) / (2^-24 S) of every case goes to profiles/contribution_parity.json.
"""
import json
import os

import numpy as np
import pytest
import torch

import contribution_reference as R
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


def _forward(sc, cameras=None, n_frames=1, grad=True, leaves=None, **rast_kw):
    """One forward of the scene; returns (what accumulate_contributions takes, the rasterizer, the outputs)."""
    from casualhdrsplat_amd import GaussianRasterizer
    rs, _, _ = Hh.settings_from_scene(sc, DEV, cameras)
    if n_frames > 1:
        rs = rs._replace(n_frames=n_frames)
    rast = GaussianRasterizer(rs, **rast_kw)
    a = dict(leaves if leaves is not None else _leaves(sc, grad))
    with torch.enable_grad() if grad else torch.no_grad():
        out = rast(a.pop("means3D"), a.pop("means2D"), a.pop("opacities"), **a)
    return (out[0] if grad else rast), rast, out


def _stats(P, fill=None):
    from casualhdrsplat_amd import ContributionStats
    st = ContributionStats(P, DEV)
    if fill is not None:
        st.weight_sum.fill_(fill[0]); st.weight_max.fill_(fill[1]); st.pixel_count.fill_(fill[2])
    return st


def _arrays(st):
    torch.cuda.synchronize()
    return st.weight_sum.cpu().numpy(), st.weight_max.cpu().numpy(), st.pixel_count.cpu().numpy()


def _same(a, b):
    return all(poison.bytes_of(x) == poison.bytes_of(y) for x, y in zip(a, b))


def _accumulate(handle, P, pixel_weight=None, stats=None):
    from casualhdrsplat_amd import accumulate_contributions
    stats = stats if stats is not None else _stats(P)
    pw = None if pixel_weight is None else torch.as_tensor(np.asarray(pixel_weight, np.float32)).to(DEV)
    accumulate_contributions(handle, stats, pw)
    return stats


def _hold_to_the_bound(name, got, ref):
    """weight_sum, weight_max, pixel_count of a call on zeroed statistics against the float64 restatement `ref`."""
    ws, wm, pc = got
    want = R.accumulate((np.zeros_like(ref["sum"]), np.zeros_like(ref["sum"]), np.zeros_like(ref["count"])), ref)
    c_sum = R.needed_constant(ws, want[0], ref["S"])
    c_max = R.needed_constant(wm, want[1], ref["S_max"])
    n_count = int((pc.astype(np.int64) != want[2]).sum())
    _PARITY[name] = dict(weight_sum=round(c_sum, 4), weight_max=round(c_max, 4), pixel_count_mismatches=n_count,
                         gaussians_reached=int((ref["count"] > 0).sum()), pairs=int(ref["pairs"]))
    print(f"contribution parity {name}: C needed {c_sum:.3f} (sum) {c_max:.3f} (max), count mismatches {n_count}", flush=True)
    assert n_count == 0, (name, "pixel_count differs", n_count, np.nonzero(pc.astype(np.int64) != want[2])[0][:8])
    assert c_sum <= Hh.C_BOUND and c_max <= Hh.C_BOUND, (name, c_sum, c_max)


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    if os.environ.get("HS_PARITY_REPORT") and _PARITY:
        with open(os.path.join(ROOT, "profiles", "contribution_parity.json"), "w") as fh:
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
        e = np.random.default_rng(17).random((H, W)).astype(np.float32)
        e.reshape(-1)[np.random.default_rng(18).permutation(H * W)[:H * W // 3]] = 0.0     # a third exactly 0
        out[k] = dict(sc=sc, f=f, e=e, ref=R.contributions(f, W, H), ref_e=R.contributions(f, W, H, pixel_weight=e), seed=seed)
    assert out["b"]["seed"] == 0
    return out


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("which", tuple(GUARDED))
def test_guarded_scene_against_the_restatement(guarded, which, weighted):
    g = guarded[which]
    P, W, H, _ = GUARDED[which]
    handle, _, _ = _forward(g["sc"])
    st = _accumulate(handle, P, g["e"] if weighted else None)
    _hold_to_the_bound(f"guarded_{which}_{'weighted' if weighted else 'plain'}", _arrays(st), g["ref_e"] if weighted else g["ref"])


# ---- 2. long lists, batch boundaries, early termination ----

LONG = {"deep": (6000, 64, 64, 0), "rows": (3000, 48, 40, 1)}


@pytest.mark.parametrize("which", tuple(LONG))
def test_long_lists_and_early_termination(oracle, which):
    """Tile lists of thousands of entries (many staging batches), pixels that terminate after hundreds of contributors: the
    pixels where the two sides demonstrably decided differently, or may have, weigh 0 on both sides."""
    from casualhdrsplat_amd import inspect_state
    P, W, H, deg = LONG[which]
    sc = S.make_scene(P, W, H, deg, seed=0)
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    lens = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).max()
    assert lens > 1500 and int(f["n_contrib"].max()) > 128, (lens, int(f["n_contrib"].max()))
    handle, _, _ = _forward(sc)
    st = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in inspect_state(handle).items()}
    m = Hh.decision_masks(oracle, sc, [f], st, what=which)
    share = float(m["excluded"].mean())
    print(f"{which}: excluded share {share:.4f}, band {float(m['pix_risk'].mean()):.4f}, longest list {lens}", flush=True)
    assert share <= 0.01, (which, share)
    e = (~m["excluded"]).astype(np.float32)
    got = _arrays(_accumulate(handle, P, e))
    _hold_to_the_bound(f"long_{which}", got, R.contributions(f, W, H, pixel_weight=e))


# ---- 3. poses and frames ----

@pytest.fixture(scope="module")
def posed():
    P, W, H = 1500, 72, 56
    return S.make_scene(P, W, H, 1, seed=3), S.blur_poses(W, H, 4, step=0.03), (P, W, H)


def test_one_call_over_three_poses_is_three_single_pose_calls(posed):
    sc, cams, (P, W, H) = posed
    e = np.random.default_rng(2).random((H, W)).astype(np.float32)
    for pw in (None, e):
        handle, _, _ = _forward(sc, cameras=cams[:3])
        one = _arrays(_accumulate(handle, P, pw))
        st = _stats(P)
        for c in cams[:3]:
            h1, _, _ = _forward(sc, cameras=[c])
            _accumulate(h1, P, pw, stats=st)
        assert _same(one, _arrays(st))
        assert one[2].sum() > 1000 and (one[0] > 0).sum() > 100


def test_two_frames_of_two_poses_are_two_calls(posed):
    sc, cams, (P, W, H) = posed
    e = np.random.default_rng(4).random((2, H, W)).astype(np.float32)
    e[1].reshape(-1)[::5] = 0.0
    handle, _, _ = _forward(sc, cameras=cams, n_frames=2)
    both = _arrays(_accumulate(handle, P, e))
    st = _stats(P)
    for fr in range(2):
        h1, _, _ = _forward(sc, cameras=cams[2 * fr:2 * fr + 2])
        _accumulate(h1, P, e[fr], stats=st)
    assert _same(both, _arrays(st))
    # the weight image is per frame: the other way round it is another result
    st2 = _stats(P)
    _accumulate(handle, P, e[::-1].copy(), stats=st2)
    assert not _same(both, _arrays(st2))
    with pytest.raises(ValueError, match="pixel_weight must have shape"):
        _accumulate(handle, P, e[0])


# ---- 4. accumulation and the compositing identity on the device ----

def test_a_second_call_accumulates_and_the_sum_is_the_accumulated_opacity(guarded):
    from casualhdrsplat_amd import inspect_state
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    handle, _, _ = _forward(g["sc"])
    st = _accumulate(handle, P)
    first = _arrays(st)
    second = _arrays(_accumulate(handle, P, stats=st))
    assert np.array_equal(second[2], 2 * first[2]) and first[2].sum() > 10000
    assert poison.bytes_of(second[1]) == poison.bytes_of(first[1])
    assert poison.bytes_of(second[0]) == poison.bytes_of(first[0] + first[0])     # the same increment: x + x is exact
    # statistics that hold something: the maximum starts from it, sum and count add to it
    held = _arrays(_accumulate(handle, P, stats=_stats(P, (1.5, 0.25, 7))))
    assert poison.bytes_of(held[1]) == poison.bytes_of(np.maximum(first[1], np.float32(0.25)))
    assert np.array_equal(held[2], first[2] + 7)
    assert poison.bytes_of(held[0]) == poison.bytes_of(np.float32(1.5) + first[0])
    # sum_g weight_sum = sum_p (1 - final_T)
    T = inspect_state(handle)["final_T"].double().cpu().numpy()
    lhs, rhs = first[0].astype(np.float64).sum(), (1.0 - T).sum()
    assert abs(lhs - rhs) <= 1e-4 * rhs, (lhs, rhs)
    # an all-zero weight image leaves the three arrays untouched, bit for bit
    st0 = _stats(P, (-0.0, -3.0, 5))
    before = _arrays(st0)
    assert _same(before, _arrays(_accumulate(handle, P, np.zeros((H, W), np.float32), stats=st0)))


# ---- 5. the workspace's contents do not matter ----

def test_result_does_not_depend_on_what_the_workspace_held(guarded, monkeypatch):
    from casualhdrsplat_amd import importance
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    handle, _, _ = _forward(g["sc"])
    results = {}
    for pattern in ("zero", "ff", "nan", "a5", "one", "random"):
        importance._WORKSPACES.clear()
        with poison.poisoned(monkeypatch, pattern) as session:
            results[pattern] = _arrays(_accumulate(handle, P, g["e"]))
        fills = session.require(IMPORTANCE, roles=("contribution_workspace#0",))
        assert fills[0].nbytes >= 16 * P
    importance._WORKSPACES.clear()
    for pattern, got in results.items():
        assert _same(got, results["zero"]), pattern
    # ... and the cached workspace, as an earlier call of other weights left it, is as good as a fresh one
    _accumulate(handle, P)
    assert _same(_arrays(_accumulate(handle, P, g["e"])), results["zero"])


# ---- 6. other modes ----

def test_an_overflowed_frame_adds_nothing_and_its_replay_adds_what_a_plain_call_adds(guarded):
    g = guarded["b"]
    P, W, H, _ = GUARDED["b"]
    plain = _arrays(_accumulate(_forward(g["sc"])[0], P, g["e"]))
    # sync-free mode, capacity far below the frame's pairs: with grad nobody looks at the counters before the backward
    handle, rast, _ = _forward(g["sc"], capacity=256, keep_state=True)
    st = _stats(P, (1.5, 0.25, 7))
    before = _arrays(st)
    assert _same(before, _arrays(_accumulate(handle, P, g["e"], stats=st)))
    # under no_grad the rasterizer grows the capacity and renders the frame again by itself
    a = _leaves(g["sc"], grad=False)
    with torch.no_grad():
        rast(a.pop("means3D"), a.pop("means2D"), a.pop("opacities"), **a)
    assert rast.overflow_replays >= 1 and int(rast.capacity) > 256
    assert _same(plain, _arrays(_accumulate(rast, P, g["e"])))


def test_raw_parameterization_and_a_kept_state_give_the_plain_arrays(guarded):
    from casualhdrsplat_amd import inspect_state
    g = guarded["b"]
    sc = g["sc"]
    P, W, H, _ = GUARDED["b"]
    x = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))
    l = torch.log(sc.scales)
    q = sc.rotations * 1.7
    raw_handle, _, _ = _forward(sc, grad=False, leaves=_leaves(sc, grad=False, opacities=x, scales=l, rotations=q),
                                parameterization="raw", keep_state=True)
    raw = _arrays(_accumulate(raw_handle, P, g["e"]))
    st = inspect_state(raw_handle)
    acts = {k: st[k].detach().clone() for k in ("opacities", "scales", "rotations")}
    plain_handle, _, _ = _forward(sc, leaves=_leaves(sc, **acts))
    assert _same(raw, _arrays(_accumulate(plain_handle, P, g["e"])))
    assert raw[2].sum() > 5000
