"""The fused L1 + D-SSIM loss (casualhdrsplat_amd.losses) on the MI355X: held to fp64 autograd through the published
formulation (tests/loss_reference.py) at least as closely as that formulation in fp32 is; bitwise deterministic; linear in
the upstream gradient; bitwise the eager step inside a captured GraphedStep; and it trains the example."""
import os
import sys

import pytest
import torch

import helpers as Hh
import loss_reference as R
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

SMALL = [(1, 1, 1), (3, 5, 7), (3, 28, 161), (3, 37, 129), (2, 3, 50, 70), (1, 64, 64)]
LARGE = [(3, 800, 800), (3, 1080, 1920)]
CONTENTS = ["random", "rendered", "flat", "hdr"]

_rendered_cache = {}


def _rendered(H, W):
    """A rasterizer-rendered LDR image [3, H, W] (rendered at >= 32 x 32 and cropped)."""
    key = (H, W)
    if key not in _rendered_cache:
        RH, RW = max(H, 32), max(W, 32)
        sc = S.make_scene(min(100000, max(2000, RH * RW // 16)), RW, RH, 1, seed=5)
        img = torch.as_tensor(Hh.run_hip(sc, backward=False)["color"])
        _rendered_cache[key] = img[:, :H, :W].contiguous()
    return _rendered_cache[key]


def _content(kind, shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    H, W = shape[-2], shape[-1]
    planes = 1
    for s in shape[:-2]:
        planes *= s

    def rnd(*sz):
        return torch.rand(*sz, generator=g)

    def nrm(*sz):
        return torch.randn(*sz, generator=g)

    if kind == "random":
        x, y = rnd(shape), rnd(shape)
    elif kind == "rendered":
        img = _rendered(H, W)
        x = torch.stack([img[i % 3] * (1.0 + 0.1 * (i // 3)) for i in range(planes)]).reshape(shape)
        y = (x + 0.03 * nrm(shape)).clamp(0, 1)
    elif kind == "flat":      # sigma = e - m^2 cancels almost entirely
        x = 0.5 + 1e-3 * nrm(shape)
        y = 0.5 + 1e-3 * nrm(shape)
    elif kind == "hdr":
        x = 20.0 * rnd(shape)
        y = (x * (1.0 + 0.2 * nrm(shape))).clamp(0, 20)
    else:
        raise ValueError(kind)
    return x.float().contiguous(), y.float().contiguous()


def _fused(x, y, lam, k=1.0):
    from casualhdrsplat_amd import photometric_loss
    xx = x.cuda().requires_grad_(True)
    loss = photometric_loss(xx, y.cuda(), lam)
    if k == 1.0:
        loss.backward()
    else:
        (k * loss).backward()
    return loss.detach(), xx.grad


def _check_parity(x, y, lam):
    L64, g64 = R.loss_and_grad(x, y, lam, torch.float64)
    L32, g32 = R.loss_and_grad(x, y, lam, torch.float32)
    loss, g = _fused(x, y, lam)
    L, g = float(loss.cpu()), g.cpu().double()
    g32 = g32.double()
    e_loss, t_loss = abs(L - L64), abs(L32 - L64)
    n64 = float(g64.norm())
    rel = float((g - g64).norm()) / max(n64, 1e-300)
    t_rel = float((g32 - g64).norm()) / max(n64, 1e-300)
    worst, t_worst = float((g - g64).abs().max()), float((g32 - g64).abs().max())
    gmax = float(g64.abs().max())
    rep = dict(L=L, L64=L64, e_loss=e_loss, t_loss=t_loss, rel=rel, t_rel=t_rel, worst=worst, t_worst=t_worst, gmax=gmax)
    assert e_loss <= max(2 * t_loss, 2e-6), rep
    assert rel <= max(2 * t_rel, 1e-6), rep
    assert worst <= max(2 * t_worst, 1e-5 * gmax), rep


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient_are_at_least_as_close_to_fp64_as_the_fp32_formulation(shape, kind, lam):
    x, y = _content(kind, shape, seed=len(shape) * 7 + shape[-1])
    _check_parity(x, y, lam)


@pytest.mark.parametrize("shape", LARGE, ids=lambda s: "x".join(map(str, s)))
def test_rendered_frames_at_c2_and_c3_size_against_fp64(shape):
    x, y = _content("rendered", shape, seed=3)
    _check_parity(x, y, 0.2)


def test_two_calls_give_the_same_bits():
    x, y = _content("rendered", (3, 240, 320), seed=4)
    l1, g1 = _fused(x, y, 0.2)
    l2, g2 = _fused(x, y, 0.2)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_gradient_is_linear_in_the_upstream_gradient_and_pure_l1_at_lambda_0():
    x, y = _content("random", (2, 3, 45, 77), seed=6)
    _, base = _fused(x, y, 0.2)
    for k in (3.0, -0.37, 1e-3):
        _, gk = _fused(x, y, 0.2, k=k)
        want = k * base
        ulp = torch.finfo(torch.float32).eps * want.abs() + torch.finfo(torch.float32).tiny
        assert bool(((gk - want).abs() <= ulp).all()), k
    _, g0 = _fused(x, y, 0.0)
    N = x.numel()
    want = torch.sign(x - y).cuda() / N
    assert bool(((g0 - want).abs() <= torch.finfo(torch.float32).eps * want.abs()).all())


def test_terms_and_ssim_agree_with_the_loss():
    from casualhdrsplat_amd import photometric_loss, ssim
    x, y = _content("rendered", (3, 64, 96), seed=8)
    xc, yc = x.cuda(), y.cuda()
    loss, (l1, s) = photometric_loss(xc, yc, 0.2, return_terms=True)
    assert not l1.requires_grad and not s.requires_grad
    assert abs(float(loss) - (0.8 * float(l1) + 0.2 * (1 - float(s)))) < 1e-6
    assert abs(float(l1) - float((x - y).abs().double().mean())) < 1e-7
    with torch.no_grad():
        s2 = ssim(xc, yc)
    assert abs(float(s2) - float(s)) < 1e-6
    s64 = float(R.ssim_map(x, y).mean())
    assert abs(float(s2) - s64) < 1e-5
    xx = xc.clone().requires_grad_(True)
    ssim(xx, yc).backward()
    _, g64 = R.loss_and_grad(x, y, 1.0)
    assert float((xx.grad.cpu().double() + g64).norm() / g64.norm()) < 1e-4    # d ssim = - d (1 - ssim)


def test_captured_step_with_the_loss_replays_the_eager_bits():
    """Rasterizer forward + photometric_loss + backward, captured once (graphs.GraphedStep) at c2 size: the loss scalar and
    every parameter gradient are bitwise the eager step's, on every replay, also after in-place parameter updates."""
    from casualhdrsplat_amd import GaussianRasterizer, photometric_loss
    from casualhdrsplat_amd.graphs import GraphedStep
    sc = S.make_scene(100000, 800, 800, 3, seed=12)
    rs, _, _ = Hh.settings_from_scene(sc, "cuda")
    names = ("means3D", "opacities", "shs", "scales", "rotations")
    leaf = {k: getattr(sc, k).cuda().requires_grad_(True) for k in names}
    m2 = torch.zeros(100000, 3, device="cuda", requires_grad=True)
    plist = list(leaf.values()) + [m2]
    target = torch.as_tensor(Hh.run_hip(sc, backward=False)["color"]).cuda()
    target = (target + 0.05 * torch.randn(target.shape, generator=torch.Generator().manual_seed(1)).cuda()).clamp(0, 1)
    R_ = Hh.run_hip(sc)["state"]["num_rendered"]
    with torch.no_grad():
        leaf["opacities"].mul_(0.9)

    def make_step(rast):
        def step():
            for p in plist:
                p.grad = None
            out = rast(leaf["means3D"], m2, leaf["opacities"], shs=leaf["shs"], scales=leaf["scales"], rotations=leaf["rotations"])
            loss = photometric_loss(out[0], target, 0.2)
            loss.backward()
            return loss.detach()
        return step

    eager = make_step(GaussianRasterizer(rs, capacity=R_ + 20000))
    rast_g = GaussianRasterizer(rs, capacity=R_ + 20000)
    g = GraphedStep(make_step(rast_g), [rast_g], params=plist)
    for rep in range(4):
        if rep:
            with torch.no_grad():
                leaf["means3D"].add_(0.002 * torch.randn_like(leaf["means3D"]))
                leaf["opacities"].mul_(0.98)
        loss_g = g.step()
        got = [loss_g.clone()] + [t.clone() for t in g.grads]
        assert g.check_overflow()[0] > 0
        loss_e = eager()
        want = [loss_e] + [p.grad for p in plist]
        assert float(loss_e) > 0
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (rep, i)


def test_example_trains_with_the_fused_loss():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic as T
    r = T.run(steps=30, quiet=True, lambda_dssim=0.2)
    f, l = r["first"], r["last"]
    assert l["loss"] < f["loss"] and l["psnr"] > f["psnr"], (f, l)
