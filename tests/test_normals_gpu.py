"""GPU checks of the depth-normal consistency term and of the per-Gaussian normal (normals.hip through the C ABI and through
normals.normal_consistency_loss / normals.gaussian_normals) against the float64 truth of tests/normals_reference.py
(test_normals.py pins that truth without a GPU), and against themselves.

Bound, per element of the loss map, the depth-normal map, dL_dnormals, dL_dinvdepth, dL_dalpha, the per-Gaussian normals and
dL_drotations: |hip - truth| <= 1e-4 |truth| + C_BOUND 2^-24 mag with helpers.C_BOUND (8) as it stands and mag built by the
rule stated at the top of normals_reference.py; the elements the definition makes zero are exactly zero.  With
HS_PARITY_REPORT=1 in the environment the largest constant any element needs goes to
profiles/normal_consistency_parity.json, per case and tensor, next to what the float32 restatement needs.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as Hh
import normals_reference as NR
import poison
import test_normals as TN

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096          # bytes handed over as the (empty) workspace: the calls must leave them alone
_PARITY = {}


def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _abi(c, pattern="nan", want=NR.KEYS, drop=()):
    """hs_normal_consistency + hs_normal_consistency_backward on case `c` with every output and the guard zone filled with
    `pattern` first; `want`: the outputs asked for, `drop`: the optional inputs left out.  {key: numpy}; asserts that the inputs
    and the guard zone are unwritten."""
    from casualhdrsplat_amd import _lib as L
    lib = L.load()
    B, H, W = c["shape"]
    names = ("invdepth", "alpha", "normals", "weight", "rot", "g")
    host = {k: (None if k in drop else c[k]) for k in names}
    t = {k: _dev(v) for k, v in host.items()}
    shapes = dict(out=(B, H, W), depth_normals=(B, 3, H, W), d_normals=(B, 3, H, W), d_invdepth=(B, H, W), d_alpha=(B, H, W))
    if t["alpha"] is None:
        want = tuple(k for k in want if k != "d_alpha")
    outs = {k: poison.fill_(torch.empty(shapes[k], dtype=torch.float32, device=DEV), pattern, seed=i) for i, k in enumerate(want)}
    guard = poison.fill_(torch.empty(GUARD, dtype=torch.uint8, device=DEV), pattern, seed=9)
    before = poison.bytes_of(guard)
    assert lib.hs_normal_consistency_workspace_bytes(B, H, W) == 0
    a = L.hs_normal_consistency_args()
    a.B, a.H, a.W, a.fx, a.fy = B, H, W, c["fx"], c["fy"]
    a.invdepth, a.alpha, a.normals, a.weight, a.cam_to_world = (_ptr(t[k]) for k in ("invdepth", "alpha", "normals", "weight", "rot"))
    a.out, a.depth_normals = _ptr(outs.get("out")), _ptr(outs.get("depth_normals"))
    a.dL_dout = _ptr(t["g"])
    a.dL_dnormals, a.dL_dinvdepth, a.dL_dalpha = (_ptr(outs.get(k)) for k in ("d_normals", "d_invdepth", "d_alpha"))
    a.workspace = guard.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    if a.out or a.depth_normals:
        L.check(lib.hs_normal_consistency(C.byref(a), stream), "hs_normal_consistency")
    L.check(lib.hs_normal_consistency_backward(C.byref(a), stream), "hs_normal_consistency_backward")
    torch.cuda.synchronize()
    for k in names:
        if host[k] is not None:
            assert poison.bytes_of(t[k]) == poison.bytes_of(host[k]), k
    assert poison.bytes_of(guard) == before
    return {k: v.cpu().numpy() for k, v in outs.items()}


def _hold(name, got, truth, mag, keys):
    need = {}
    for k in keys:
        assert got[k].shape == truth[k].shape and np.isfinite(got[k]).all(), (name, k)
        assert not got[k][truth[k] == 0].any(), (name, k)                # exact zeros where the definition puts them
        need[k] = NR.needed(got[k], truth[k], mag[k])
    print(f"normal consistency parity {name}: C needed {need}", flush=True)
    assert all(v <= Hh.C_BOUND for v in need.values()), (name, need)
    return need


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    if os.environ.get("HS_PARITY_REPORT") and _PARITY:
        with open(os.path.join(ROOT, "profiles", "normal_consistency_parity.json"), "w") as fh:
            json.dump(dict(bound="|x - truth| <= 1e-4 |truth| + C 2^-24 mag; c_needed: the largest C any element of the HIP result "
                                 "needs, float32_restatement: what the numpy float32 restatement needs (C_BOUND = 8)",
                           cases=_PARITY), fh, indent=1, sort_keys=True)
            fh.write("\n")


# ---- 1. the image-space term through the C ABI ----

@pytest.mark.parametrize("name", tuple(TN.SHAPES))
def test_the_term_and_its_gradients_against_the_truth(name):
    c = TN.case(name)
    truth, mag = TN.reference(name)
    got = _abi(c, "nan")
    keys = tuple(k for k in NR.KEYS if k in got)
    need = _hold(name, got, truth, mag, keys)
    f32 = NR.closed_form(*TN.ref_args(c), dtype=np.float32)
    _PARITY[name] = dict(c_needed={k: round(v, 4) for k, v in need.items()},
                         float32_restatement={k: round(NR.needed(f32[k], truth[k], mag[k]), 4) for k in keys})
    off = ~truth["interior"]
    assert not got["out"][off].any() and not got["depth_normals"][np.broadcast_to(off[:, None], got["depth_normals"].shape)].any()
    assert not got["d_invdepth"][~truth["valid"]].any()
    if min(c["shape"][1:]) < 3:
        assert all(not v.any() for v in got.values())
    else:
        n = np.linalg.norm(got["depth_normals"], axis=1)[truth["interior"]]
        assert np.abs(n - 1).max() < 1e-5 and np.abs(got["d_invdepth"]).max() > 1e-3
    # the same bits whatever the outputs held, and on a second run
    for pattern in ("ff", "random"):
        again = _abi(c, pattern)
        for k in keys:
            assert poison.bytes_of(again[k]) == poison.bytes_of(got[k]), (name, pattern, k)


@pytest.mark.parametrize("drop", (("alpha",), ("weight",), ("rot",), ("alpha", "weight", "rot")))
def test_each_optional_input_absent(drop):
    c = dict(TN.case("holes"))
    for k in drop:
        c[k] = None
    truth, mag = NR.truth(*TN.ref_args(c)), NR.magnitudes(*TN.ref_args(c))
    got = _abi(TN.case("holes"), "a5", drop=drop)
    assert ("d_alpha" in got) == ("alpha" not in drop)
    _PARITY["holes_without_" + "_".join(drop)] = dict(c_needed={k: round(v, 4) for k, v in _hold(str(drop), got, truth, mag, tuple(got)).items()})
    if "alpha" in drop:       # the alpha holes of the case are no holes now
        assert truth["interior"][0, 10, 30] and got["out"][0, 10, 30] != 0


def test_each_optional_output_absent():
    c = TN.case("holes")
    full = _abi(c, "nan")
    for k in NR.KEYS:
        alone = _abi(c, "ff", want=(k,))
        assert tuple(alone) == (k,) and poison.bytes_of(alone[k]) == poison.bytes_of(full[k]), k
    for pair in (("d_invdepth", "d_alpha"), ("d_normals", "d_alpha"), ("out", "d_invdepth")):
        got = _abi(c, "random", want=pair)
        for k in pair:
            assert poison.bytes_of(got[k]) == poison.bytes_of(full[k]), pair


# ---- 2. the autograd wrapper ----

def _wrapper(c, single=False, **kw):
    from casualhdrsplat_amd import normal_consistency_loss
    pick = (lambda x: x[0]) if single else (lambda x: x)
    leaves = {k: pick(_dev(c[k])).clone().requires_grad_(True) for k in ("invdepth", "normals", "alpha") if c[k] is not None}
    res = normal_consistency_loss(leaves["invdepth"], leaves["normals"], c["fx"], c["fy"], alpha=leaves.get("alpha"),
                                  weight=None if c["weight"] is None else pick(_dev(c["weight"])),
                                  cam_to_world=None if c["rot"] is None else pick(_dev(c["rot"])), **kw)
    return res, leaves


@pytest.mark.parametrize("name", ("holes", "strip", "tile_plus_one"))
def test_the_wrappers_gradients_are_the_abis_bits(name, monkeypatch):
    c = TN.case(name)
    want = _abi(c, "nan")
    with poison.poisoned(monkeypatch, "nan") as session:
        (out, dn), leaves = _wrapper(c, return_depth_normals=True)
        assert out.requires_grad and not dn.requires_grad
        out.backward(_dev(c["g"]))
        torch.cuda.synchronize()
    session.require("casualhdrsplat_amd.normals", at_least=4)
    assert poison.bytes_of(out) == poison.bytes_of(want["out"]) and poison.bytes_of(dn) == poison.bytes_of(want["depth_normals"])
    for k, key in (("invdepth", "d_invdepth"), ("normals", "d_normals"), ("alpha", "d_alpha")):
        if k in leaves:
            assert poison.bytes_of(leaves[k].grad) == poison.bytes_of(want[key]), k
    # a gradient asked for the normals alone, without the depth-normal map: the same bits
    out2, leaves2 = _wrapper(c)
    assert poison.bytes_of(out2) == poison.bytes_of(want["out"])
    g = torch.autograd.grad(out2, leaves2["normals"], _dev(c["g"]))[0]
    assert poison.bytes_of(g) == poison.bytes_of(want["d_normals"])
    # weight and cam_to_world are constants even when they require grad
    from casualhdrsplat_amd import normal_consistency_loss
    if c["weight"] is not None:
        w = _dev(c["weight"]).requires_grad_(True)
        o = normal_consistency_loss(_dev(c["invdepth"]).requires_grad_(True), _dev(c["normals"]), c["fx"], c["fy"], weight=w)
        o.sum().backward()
        assert w.grad is None


def test_a_single_frame_without_the_batch_axis():
    c = dict(TN.case("example"))
    want = _abi(c, "nan")
    (out, dn), leaves = _wrapper(c, single=True, return_depth_normals=True)
    assert out.shape == c["shape"][1:] and dn.shape == (3,) + c["shape"][1:]
    out.backward(_dev(c["g"])[0])
    assert poison.bytes_of(out) == poison.bytes_of(want["out"][0]) and poison.bytes_of(dn) == poison.bytes_of(want["depth_normals"][0])
    assert poison.bytes_of(leaves["invdepth"].grad) == poison.bytes_of(want["d_invdepth"][0])
    assert poison.bytes_of(leaves["alpha"].grad) == poison.bytes_of(want["d_alpha"][0])
    assert poison.bytes_of(leaves["normals"].grad) == poison.bytes_of(want["d_normals"][0])


# ---- 3. the per-Gaussian normal ----

@pytest.mark.parametrize("P", TN.GN_SIZES)
def test_gaussian_normals_against_the_truth(P, monkeypatch):
    from casualhdrsplat_amd import _lib as L
    from casualhdrsplat_amd import gaussian_normals
    lib = L.load()
    c = TN.gn_case(P)
    truth = NR.gaussian_normals(*TN.gn_args(c))
    mag = NR.gaussian_normals(*TN.gn_args(c), mode="mag")
    f32 = NR.gaussian_normals(*TN.gn_args(c), mode=np.float32)
    results = []
    for pattern in ("nan", "ff"):
        t = {k: _dev(c[k]) for k in ("rotations", "scales", "means3D", "campos", "g")}
        n = poison.fill_(torch.empty((P, 3), dtype=torch.float32, device=DEV), pattern)
        dq = poison.fill_(torch.empty((P, 4), dtype=torch.float32, device=DEV), pattern, seed=1)
        a = L.hs_gaussian_normals_args()
        a.P = P
        a.rotations, a.scales, a.means3D, a.campos = (t[k].data_ptr() for k in ("rotations", "scales", "means3D", "campos"))
        a.normals, a.dL_dnormals, a.dL_drotations = n.data_ptr(), t["g"].data_ptr(), dq.data_ptr()
        stream = torch.cuda.current_stream().cuda_stream
        L.check(lib.hs_gaussian_normals(C.byref(a), stream), "hs_gaussian_normals")
        L.check(lib.hs_gaussian_normals_backward(C.byref(a), stream), "hs_gaussian_normals_backward")
        torch.cuda.synchronize()
        for k in t:
            assert poison.bytes_of(t[k]) == poison.bytes_of(c[k]), k
        results.append(dict(normals=n.cpu().numpy(), d_rotations=dq.cpu().numpy()))
    got = results[0]
    for k in got:
        assert poison.bytes_of(got[k]) == poison.bytes_of(results[1][k]), k
    need = _hold(f"gaussian_normals_{P}", got, truth, mag, ("normals", "d_rotations"))
    _PARITY[f"gaussian_normals_{P}"] = dict(c_needed={k: round(v, 4) for k, v in need.items()},
                                            float32_restatement={k: round(NR.needed(f32[k], truth[k], mag[k]), 4) for k in need})
    assert (np.sign((got["normals"] * (c["campos"] - c["means3D"])).sum(1))[truth["live"]] >= 0).all()
    if P > 10:
        assert not got["normals"][5].any() and not got["d_rotations"][5].any()
    if P > 100:     # a NaN or infinite component, a sum of squares that overflows or underflows: zeros, as |q| = 0
        dead = [5, 11, 12, 13, 14]
        assert not truth["live"][dead].any() and not got["normals"][dead].any() and not got["d_rotations"][dead].any()
    # the wrapper: the same bits, the gradient on the rotations alone
    with poison.poisoned(monkeypatch, "nan") as session:
        leaves = [_dev(c[k]).requires_grad_(True) for k in ("rotations", "scales", "means3D", "campos")]
        n = gaussian_normals(*leaves)
        n.backward(_dev(c["g"]))
        torch.cuda.synchronize()
    session.require("casualhdrsplat_amd.normals", at_least=2)
    assert poison.bytes_of(n) == poison.bytes_of(got["normals"]) and poison.bytes_of(leaves[0].grad) == poison.bytes_of(got["d_rotations"])
    assert all(l.grad is None for l in leaves[1:])
    # the stored log-scales name the same axis
    logs = gaussian_normals(_dev(c["rotations"]), _dev(np.log(c["scales"])), _dev(c["means3D"]), _dev(c["campos"]))
    assert poison.bytes_of(logs) == poison.bytes_of(got["normals"])


# ---- 4. the path it completes ----

CHAIN = (2000, 64, 48)
KEYS = ("means3D", "opacities", "scales", "rotations")


def _chain_forward(sc, lv):
    """the forward of the documented path; (colour, alpha, invdepth, composited normals, the map, what the map was given)"""
    from casualhdrsplat_amd import GaussianRasterizer, composite_features, gaussian_normals, normal_consistency_loss
    rs, _, _ = Hh.settings_from_scene(sc, DEV)
    rast = GaussianRasterizer(rs, return_alpha=True, return_invdepth=True)
    color, radii, alpha, invd = rast(lv["means3D"], lv["means2D"], lv["opacities"], shs=lv["shs"], scales=lv["scales"],
                                     rotations=lv["rotations"])
    geo = {k: lv[k] for k in KEYS}
    n = gaussian_normals(lv["rotations"], lv["scales"], lv["means3D"], rs.campos)
    N = composite_features(color, n, geometry=geo)[0]
    cam = sc.camera
    fx, fy = cam.W / (2.0 * cam.tanfovx), cam.H / (2.0 * cam.tanfovy)
    rot = rs.viewmatrix[:3, :3].contiguous()
    term = normal_consistency_loss(invd, N, fx, fy, alpha=alpha, weight=alpha.detach(), cam_to_world=rot)
    return color, alpha, invd, N, term, dict(fx=fx, fy=fy, rot=rot)


def _chain_leaves(sc):
    t = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=sc.scales,
             rotations=sc.rotations)
    return {k: v.detach().clone().to(DEV).requires_grad_(True) for k, v in t.items()}


def test_the_chain_adds_to_the_rasterizers_gradients(oracle):
    """One backward() of image loss + term against the rasterizer-only gradients plus the ABI's dL_dinvdepth, dL_dalpha,
    dL_dnormals pushed through the rasterizer's and composite_features' backwards by hand.  The two sides push the same
    upstream images through the same kernels; they differ in where the three images are added (inside one rasterizer backward,
    or across two and a tensor sum), so they are two fp32 evaluations of the same sums, held to the contract as it stands:
    |a - b| <= 1e-4 |b| + C_BOUND 2^-24 S, S = the oracle's sum of |terms| of the rasterizer backward under the colour and
    inverse-depth gradients plus that of the accumulated opacity (a colour channel that is 1 for every Gaussian) under
    dL_dalpha.  The path through the composited normals is the same kernels on the same bits on both sides."""
    from casualhdrsplat_amd import _lib as L
    from casualhdrsplat_amd import synthetic as S
    P, W, H = CHAIN
    sc = S.make_scene(P, W, H, 1, seed=3)
    rng = np.random.default_rng(81)
    w_img = _dev(rng.standard_normal((3, H, W)).astype(np.float32))
    gam = _dev((rng.random((H, W)) / (H * W)).astype(np.float32) * 50.0)
    wrt = lambda lv: [lv[k] for k in KEYS]
    # one backward of the sum
    lv = _chain_leaves(sc)
    color, alpha, invd, N, term, extra = _chain_forward(sc, lv)
    assert term.shape == (H, W) and float(term.detach().abs().max()) > 1e-3
    ((color * w_img).sum() + (term * gam).sum()).backward()
    total = [lv[k].grad.detach().cpu().numpy().astype(np.float64) for k in KEYS]
    # by hand: the ABI's three gradients ...
    lib = L.load()
    outs = [poison.fill_(torch.empty_like(t), "nan") for t in (N, invd, alpha)]
    weight = alpha.detach().clone()
    a = L.hs_normal_consistency_args()
    a.B, a.H, a.W, a.fx, a.fy = 1, H, W, extra["fx"], extra["fy"]
    a.invdepth, a.alpha, a.normals, a.weight, a.cam_to_world = (t.data_ptr() for t in (invd, alpha, N, weight, extra["rot"]))
    a.dL_dout = gam.data_ptr()
    a.dL_dnormals, a.dL_dinvdepth, a.dL_dalpha = (t.data_ptr() for t in outs)
    L.check(lib.hs_normal_consistency_backward(C.byref(a), torch.cuda.current_stream().cuda_stream), "hs_normal_consistency_backward")
    dN, dinv, dalpha = outs
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in outs)
    by_hand = {}
    for order in ("rasterizer_first", "term_first"):
        lv2 = _chain_leaves(sc)
        color2, alpha2, invd2, N2, _, _ = _chain_forward(sc, lv2)
        for x, y in ((color2, color), (alpha2, alpha), (invd2, invd), (N2, N)):
            assert poison.bytes_of(x) == poison.bytes_of(y)
        img = lambda: torch.autograd.grad((color2 * w_img).sum(), wrt(lv2), retain_graph=True)
        chain = lambda: torch.autograd.grad([invd2, alpha2, N2], wrt(lv2), [dinv, dalpha, dN], retain_graph=True)
        if order == "rasterizer_first":
            g_r, g_c = img(), chain()
        else:
            g_c, g_r = chain(), img()
        by_hand[order] = [(p + q).cpu().numpy().astype(np.float64) for p, q in zip(g_r, g_c)]
        by_hand[order + "_parts"] = [(p.cpu().numpy(), q.cpu().numpy()) for p, q in zip(g_r, g_c)]
    for p, q in zip(by_hand["rasterizer_first_parts"], by_hand["term_first_parts"]):
        assert poison.bytes_of(p[0]) == poison.bytes_of(q[0]) and poison.bytes_of(p[1]) == poison.bytes_of(q[1])
    # S: the oracle's magnitudes of the rasterizer backward under (w_img, dinv), and of the alpha image under dalpha
    f, b1 = Hh.run_oracle(oracle, sc, dL=None, backward=False)
    ocam = Hh.oracle_camera(oracle, sc)
    kw = dict(scales=sc.scales.numpy(), rotations=sc.rotations.numpy())
    b1 = oracle.backward(ocam, f, w_img.cpu().numpy(), sc.means3D.numpy(), shs=sc.shs.numpy(), dL_dinvdepth_img=dinv.cpu().numpy(),
                         bounds=True, **kw)
    ones = np.ones((P, 3), np.float32)
    f1 = oracle.forward(ocam, sc.means3D.numpy(), sc.opacities.numpy(), colors_precomp=ones, **kw)
    d_a = np.zeros((3, H, W), np.float32)
    d_a[0] = dalpha.cpu().numpy()
    b2 = oracle.backward(ocam, f1, d_a, sc.means3D.numpy(), colors_precomp=ones, bounds=True, **kw)
    names = dict(means3D="dL_dmeans3D", opacities="dL_dopacity", scales="dL_dscales", rotations="dL_drots")
    worst = {}
    for i, k in enumerate(KEYS):
        S_ = (np.asarray(b1["abs_" + names[k]], np.float64) + np.asarray(b2["abs_" + names[k]], np.float64)).reshape(total[i].shape)
        ref = by_hand["rasterizer_first"][i]
        assert np.abs(ref).max() > 1e-3 and np.abs(by_hand["rasterizer_first_parts"][i][1]).max() > 1e-6, k
        excess = np.abs(total[i] - ref) - 1e-4 * np.abs(ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[k] = float(np.where(excess > 0, excess / (2.0 ** -24 * S_), 0.0).max())
    print(f"normal consistency chain: C needed {worst}", flush=True)
    _PARITY["chain"] = dict(c_needed={k: round(v, 4) for k, v in worst.items()})
    assert all(v <= Hh.C_BOUND for v in worst.values()), worst


def test_a_captured_step_replays_bit_for_bit():
    """forward + backward of both entry points captured in torch.cuda.graph, replayed after the inputs changed"""
    from casualhdrsplat_amd import gaussian_normals, normal_consistency_loss
    c = TN.case("holes")
    g = TN.gn_case(1000)

    def inputs(shift, scale):      # (the holes move with the rest)
        return dict(invdepth=np.roll(c["invdepth"], shift, axis=2) * np.float32(scale), normals=np.roll(c["normals"], shift, axis=3),
                    alpha=np.roll(c["alpha"], shift, axis=1), q=np.roll(g["rotations"], shift, axis=0))

    first, second = inputs(0, 1.0), inputs(3, 1.25)
    static = {k: _dev(v).clone().requires_grad_(True) for k, v in first.items()}
    const = dict(weight=_dev(c["weight"]), rot=_dev(c["rot"]), gam=_dev(c["g"]), scales=_dev(g["scales"]), means=_dev(g["means3D"]),
                 campos=_dev(g["campos"]), gq=_dev(g["g"]))

    def step(t):
        for v in t.values():
            v.grad = None
        out, dn = normal_consistency_loss(t["invdepth"], t["normals"], c["fx"], c["fy"], alpha=t["alpha"], weight=const["weight"],
                                          cam_to_world=const["rot"], return_depth_normals=True)
        n = gaussian_normals(t["q"], const["scales"], const["means"], const["campos"])
        torch.autograd.backward([out, n], [const["gam"], const["gq"]])
        return out, dn, n

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    for v in static.values():
        v.grad = None
    with torch.cuda.graph(graph):
        captured = step(static)
    grads = {k: v.grad for k, v in static.items()}
    for values in (second, first):
        with torch.no_grad():
            for k, v in values.items():
                static[k].copy_(_dev(v))
        graph.replay()
        torch.cuda.synchronize()
        eager_in = {k: _dev(v).clone().requires_grad_(True) for k, v in values.items()}
        eager = step(eager_in)
        for x, y in zip(captured, eager):
            assert poison.bytes_of(x) == poison.bytes_of(y)
        for k in static:
            assert poison.bytes_of(grads[k]) == poison.bytes_of(eager_in[k].grad), k
        assert float(grads["invdepth"].abs().max()) > 1e-3


def test_the_example_trains_with_the_term():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "--steps", "20", "--normal", "0.05"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = next(l for l in out.stdout.splitlines() if l.startswith("loss "))
    first, last = (float(x) for x in line.split(";")[0].replace("loss", "").split("->"))
    assert np.isfinite(first) and np.isfinite(last) and last < first, line
    term = next(l for l in out.stdout.splitlines() if l.startswith("mean normal-consistency map"))
    assert all(np.isfinite(float(x)) for x in term.split("map")[1].split("(")[0].split("->")), term
