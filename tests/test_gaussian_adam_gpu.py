"""The fused Adam step (casualhdrsplat_amd.optim.GaussianAdam, adam.hip) on the MI355X: bit for bit the numpy restatement
(tests/adam_reference.py) -- dense, column groups, sparse, unaligned gradient views, subnormal / overflowing squares --,
as close to fp64 Adam as fp32 torch is, deterministic, interchangeable with torch.optim.Adam's state, bitwise the eager
steps inside a captured graph, and it trains the example."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import adam_reference as R
import helpers as Hh
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _special_grads(rng, shape, step):
    """Gradients with exact zeros, magnitudes whose squares are subnormal (1e-20) or underflow (1e-30), and 1e30-scale
    values whose squares overflow."""
    g = (10.0 ** rng.uniform(-6.0, 0.0, size=shape) * rng.standard_normal(shape)).astype(np.float32)
    u = rng.random(shape)
    g[u < 0.05] = 0.0
    g[(u >= 0.05) & (u < 0.08)] *= np.float32(1e-20)
    g[(u >= 0.08) & (u < 0.10)] *= np.float32(1e-30)
    if step % 3 == 1:
        g[(u >= 0.10) & (u < 0.11)] *= np.float32(1e30)
    return g


class Cloud:
    """Parameters of a cloud of P Gaussians (row widths 3, 1, 48, 3, 4) and a dense 7-vector, on the GPU with their
    gradients as VIEWS of one flat buffer that starts 4 bytes past an aligned address, and the same values in numpy with
    the reference's state."""
    SHAPES = (("means3D", (3,)), ("opacities", (1,)), ("shs", (16, 3)), ("scales", (3,)), ("rotations", (4,)))

    def __init__(self, P, seed=0, eps=1e-15):
        from casualhdrsplat_amd import GaussianAdam, cloud_param_groups
        self.rng = np.random.default_rng(seed)
        self.P = P
        self.np = {k: self.rng.standard_normal((P,) + s).astype(np.float32) for k, s in self.SHAPES}
        self.np["extra"] = self.rng.standard_normal((7,)).astype(np.float32)
        self.names = [k for k, _ in self.SHAPES] + ["extra"]
        self.t = {k: torch.tensor(self.np[k], device=DEV).requires_grad_(True) for k in self.names}
        total = sum(self.np[k].size for k in self.names)
        self.flat = torch.zeros(total + 1, device=DEV)
        off = 1                                         # (4-byte aligned, not 16: P * width is odd for P = 10 007, too)
        for k in self.names:
            n = self.np[k].size
            self.t[k].grad = self.flat[off:off + n].view(self.np[k].shape)
            off += n
        groups = cloud_param_groups(*[self.t[k] for k, _ in self.SHAPES]) + [dict(params=[self.t["extra"]], lr=3e-3, eps=1e-8)]
        self.opt = GaussianAdam(groups, eps=eps)
        # the reference: one hyper row per (group, tensor) pair in the optimizer's order; its arrays seen as [rows, width]
        self.cols = [("means3D", 0, 3), ("opacities", 0, 1), ("shs", 0, 3), ("shs", 3, 48), ("scales", 0, 3), ("rotations", 0, 4),
                     ("extra", 0, 1)]
        self.ref = R.AdamReference(len(self.cols))
        self.m = {k: np.zeros_like(v) for k, v in self.np.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.np.items()}

    def hyper(self):
        return [(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])) for g in self.opt.param_groups]

    def step(self, step, visibility=None, vis_np=None, grads=None):
        grads = grads or {k: _special_grads(self.rng, self.np[k].shape, step) for k in self.names}
        for k in self.names:
            self.t[k].grad.copy_(torch.tensor(grads[k]))
        self.opt.step(visibility=visibility)
        d = self.ref.tick(self.hyper())
        for i, (k, a, b) in enumerate(self.cols):
            rows = self.np[k].shape[0] if k != "extra" else self.np[k].size
            view = lambda x: x.reshape(rows, -1)[:, a:b]           # noqa: E731  (views: updated in place)
            R.update(view(self.np[k]), view(grads[k]), view(self.m[k]), view(self.v[k]), d[i], None if k == "extra" else vis_np)
        return grads

    def assert_bits(self, what=""):
        for k in self.names:
            st = self.opt.state[self.t[k]]
            for name, got, want in (("param", self.t[k], self.np[k]), ("exp_avg", st["exp_avg"], self.m[k]),
                                    ("exp_avg_sq", st["exp_avg_sq"], self.v[k])):
                g = got.detach().cpu().numpy()
                if not R.same_bits(g, want):
                    bad = ~((g.view(np.uint32) == want.view(np.uint32)) | (np.isnan(g) & np.isnan(want)))
                    i = tuple(int(x[0]) for x in np.nonzero(bad))
                    raise AssertionError(f"{what}: {k}.{name} differs in {int(bad.sum())} of {bad.size} elements; first at {i}: "
                                         f"got {g[i]!r} ({g.view(np.uint32)[i]:#x}), reference {want[i]!r} ({want.view(np.uint32)[i]:#x})")


@pytest.mark.parametrize("P", [10007, 262144])
def test_twenty_dense_steps_are_the_reference_bit_for_bit(P):
    """Parameters, exp_avg, exp_avg_sq after every one of 20 steps: row widths 1, 3, 4, 48, the SH tensor as two column
    groups with two learning rates, a dense group, gradients that are 4-byte aligned views of one flat buffer, a learning
    rate change at step 7, zeros / subnormal and underflowing squares / overflowing squares.  No tolerance."""
    c = Cloud(P, seed=P % 97)
    saw_inf = False
    for step in range(20):
        if step == 7:
            c.opt.param_groups[3]["lr"] = 7e-4
            c.opt.param_groups[0]["lr"] *= 0.5
        c.step(step)
        c.assert_bits(f"P={P} step {step}")
        saw_inf = saw_inf or bool(np.isinf(c.v["shs"]).any())
    assert saw_inf and c.opt._read_t() == 20           # (inf where the reference has inf: the case was exercised)
    assert float(c.opt.state_dict()["state"][0]["step"]) == 20.0


@pytest.mark.parametrize("kind", ["radii", "bool"])
@pytest.mark.parametrize("fraction", [0.0, 0.3, 1.0])
def test_sparse_steps_skip_invisible_rows_entirely(kind, fraction):
    P = 10007
    c, dense = Cloud(P, seed=3), Cloud(P, seed=3)
    for step in range(2):                                   # (moments and parameters away from their start values)
        g = c.step(step)
        dense.step(step, grads=g)
    rng = np.random.default_rng(11)
    for step in range(2, 5):
        vis_np = rng.random(P) < fraction if 0.0 < fraction < 1.0 else np.full(P, fraction == 1.0)
        if kind == "radii":
            vis = torch.tensor(np.where(vis_np, rng.integers(1, 40, P), 0).astype(np.int32), device=DEV)
        else:
            vis = torch.tensor(vis_np, device=DEV)
        before = {k: [x.clone() for x in (c.t[k].detach(), c.opt.state[c.t[k]]["exp_avg"], c.opt.state[c.t[k]]["exp_avg_sq"])]
                  for k in c.names}
        g = c.step(step, visibility=vis, vis_np=vis_np)
        dense.step(step, grads=g)
        c.assert_bits(f"{kind} fraction {fraction} step {step}")           # visible rows: the reference; invisible: untouched there too
        hidden = torch.tensor(~vis_np, device=DEV)
        for k in c.names[:-1]:
            now = (c.t[k].detach(), c.opt.state[c.t[k]]["exp_avg"], c.opt.state[c.t[k]]["exp_avg_sq"])
            for a, b in zip(before[k], now):
                assert torch.equal(a[hidden].view(torch.int32), b[hidden].view(torch.int32)), k
        assert not torch.equal(before["extra"][0], c.t["extra"].detach())   # (the dense group moves whatever the mask says)
        if fraction == 1.0:
            for k in c.names:
                assert torch.equal(c.t[k].detach().view(torch.int32), dense.t[k].detach().view(torch.int32)), k
    if fraction == 0.0:
        assert torch.equal(before["shs"][0], c.t["shs"].detach())


def test_wrong_mask_length_and_dtype_raise_on_the_gpu_too():
    c = Cloud(1000, seed=1)
    c.step(0)
    with pytest.raises(ValueError, match="length 999"):
        c.opt.step(visibility=torch.zeros(999, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError, match="int32 radii or a bool"):
        c.opt.step(visibility=torch.zeros(1000, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c.opt.step(visibility=torch.zeros(1000, dtype=torch.bool))
    c.assert_bits("after refused calls")


def _run_pinned(make_opt, p0, grads, dtype=torch.float32, device=DEV):
    p = torch.tensor(p0, dtype=dtype, device=device).requires_grad_(True)
    opt = make_opt(p)
    for g in grads:
        p.grad = torch.tensor(g, dtype=dtype, device=device)
        opt.step()
    return p, opt


def _errors(p, truth):
    e = p.detach().double().cpu().numpy() - truth
    return float(np.abs(e).max()), float(np.sqrt(np.mean(e ** 2)))


def test_fifty_steps_are_as_close_to_fp64_adam_as_fp32_torch_is():
    """The pinned case of tests/test_gaussian_adam.py on the GPU: error against torch.optim.Adam in float64 at most 1.5 x
    the error of torch.optim.Adam in float32 (max and RMS over the elements)."""
    from casualhdrsplat_amd import GaussianAdam
    p0, grads = R.pinned_case()
    lr, b1, b2, eps = R.PINNED_HYPER
    kw = dict(lr=lr, betas=(b1, b2), eps=eps)
    truth = _run_pinned(lambda p: torch.optim.Adam([p], **kw), p0, grads, torch.float64, "cpu")[0].detach().numpy()
    t32, _ = _run_pinned(lambda p: torch.optim.Adam([p], **kw), p0, grads, torch.float32, "cpu")
    ours, _ = _run_pinned(lambda p: GaussianAdam([dict(params=[p], per_gaussian=True)], **kw), p0, grads)
    (mx, rms), (mx32, rms32) = _errors(ours, truth), _errors(t32, truth)
    print(f"max error: fused {mx:.3e}, torch fp32 {mx32:.3e} (ratio {mx / mx32:.4f}); RMS {rms:.3e} / {rms32:.3e} (ratio {rms / rms32:.4f})")
    assert mx <= 1.5 * mx32 and rms <= 1.5 * rms32, ((mx, mx32), (rms, rms32))


def test_two_runs_give_identical_bits():
    outs = []
    for _ in range(2):
        c = Cloud(50000, seed=5)
        rng = np.random.default_rng(2)
        for step in range(6):
            vis_np = rng.random(c.P) < 0.5 if step % 2 else None
            c.step(step, visibility=None if vis_np is None else torch.tensor(vis_np, device=DEV), vis_np=vis_np)
        outs.append([x.clone() for k in c.names for x in (c.t[k].detach(), c.opt.state[c.t[k]]["exp_avg"], c.opt.state[c.t[k]]["exp_avg_sq"])])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_state_loaded_from_torch_adam_continues_within_the_same_bar():
    """torch.optim.Adam (float32) runs 5 steps; its state_dict goes into a GaussianAdam on the GPU; both run 5 more.  Held,
    against float64 torch over all 10 steps, to 1.5 x the error of the float32 torch run (the products beta^t are rebuilt
    with pow on load, so the continuation equals an uninterrupted run to rounding only)."""
    from casualhdrsplat_amd import GaussianAdam
    p0, grads = R.pinned_case(seed=4, rows=5000, cols=12, steps=10)
    lr, b1, b2, eps = R.PINNED_HYPER
    kw = dict(lr=lr, betas=(b1, b2), eps=eps)
    truth = _run_pinned(lambda p: torch.optim.Adam([p], **kw), p0, grads, torch.float64, "cpu")[0].detach().numpy()
    p, topt = _run_pinned(lambda p: torch.optim.Adam([p], **kw), p0, grads[:5], torch.float32, "cpu")
    q = p.detach().to(DEV).requires_grad_(True)
    ours = GaussianAdam([q], **kw)
    ours.load_state_dict(topt.state_dict())
    assert ours._read_t() == 5 and ours.state[q]["exp_avg"].device == q.device
    assert torch.equal(ours.state[q]["exp_avg"].cpu(), topt.state[p]["exp_avg"])
    for g in grads[5:]:
        p.grad = torch.tensor(g)
        q.grad = torch.tensor(g, device=DEV)
        topt.step()
        ours.step()
    (mx, rms), (mx32, rms32) = _errors(q, truth), _errors(p, truth)
    print(f"max error: fused {mx:.3e}, torch fp32 {mx32:.3e} (ratio {mx / mx32:.4f}); RMS {rms:.3e} / {rms32:.3e} (ratio {rms / rms32:.4f})")
    assert mx <= 1.5 * mx32 and rms <= 1.5 * rms32, ((mx, mx32), (rms, rms32))
    sd = ours.state_dict()
    assert float(sd["state"][0]["step"]) == 10.0 and sd["state"][0]["exp_avg"].shape == q.shape
    topt.load_state_dict(sd)                     # ... and back


def test_captured_enqueue_replays_the_eager_steps_bit_for_bit():
    """enqueue() -- two kernels, nothing else -- recorded once with torch.cuda.graph (one stream, a linear chain) and replayed
    10 times with new gradients copied into the static tensors and a learning-rate change between replays 4 and 5 equals 10
    eager steps: step count, bias corrections and learning rates are read on the device."""
    from casualhdrsplat_amd import GaussianAdam
    P = 30011
    rng = np.random.default_rng(8)
    init = {"shs": rng.standard_normal((P, 16, 3)).astype(np.float32), "opac": rng.standard_normal((P, 1)).astype(np.float32),
            "expo": rng.standard_normal((5,)).astype(np.float32)}

    def make():
        t = {k: torch.tensor(v, device=DEV).requires_grad_(True) for k, v in init.items()}
        for v in t.values():
            v.grad = torch.zeros_like(v)
        opt = GaussianAdam([dict(params=[t["shs"]], lr=2.5e-3, columns=(0, 3), per_gaussian=True),
                            dict(params=[t["shs"]], lr=1.25e-4, columns=(3, 48), per_gaussian=True),
                            dict(params=[t["opac"]], lr=5e-2, per_gaussian=True), dict(params=[t["expo"]], lr=1e-2)], eps=1e-15)
        vis = torch.zeros(P, dtype=torch.int32, device=DEV)
        return t, opt, vis

    te, eager, vis_e = make()
    tg, graphed, vis_g = make()
    graphed.prepare()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        graphed.enqueue(vis_g)
    assert graphed._read_t() == 0                       # (recording runs nothing)
    for rep in range(10):
        if rep == 5:
            eager.set_lr(1e-3, group=0)
            graphed.set_lr(1e-3, group=0)
        radii = torch.tensor(np.where(rng.random(P) < 0.6, 3, 0).astype(np.int32), device=DEV)
        vis_e.copy_(radii)
        vis_g.copy_(radii)
        for k in init:
            g = torch.tensor(_special_grads(rng, init[k].shape, rep), device=DEV)
            te[k].grad.copy_(g)
            tg[k].grad.copy_(g)
        eager.step(visibility=vis_e)
        graph.replay()
        for k in init:
            for a, b in ((te[k], tg[k]), (eager.state[te[k]]["exp_avg"], graphed.state[tg[k]]["exp_avg"]),
                         (eager.state[te[k]]["exp_avg_sq"], graphed.state[tg[k]]["exp_avg_sq"])):
                assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), (rep, k)
    assert graphed._read_t() == 10 == eager._read_t()
    assert not torch.equal(tg["shs"].detach().cpu(), torch.tensor(init["shs"]))


def _example():
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("graph", [False, True])
def test_training_example_with_the_fused_optimizer(graph):
    """examples/train_synthetic.py with fused_adam=True, held to the thresholds tests/test_image_formation.py holds the
    torch.optim.Adam run to (same arguments)."""
    r = _example().run(P=5000, W=192, H=128, frames=3, virtual=4, steps=120, seed=3, quiet=True, graph=graph, fused_adam=True)
    f, l = r["first"], r["last"]
    assert abs(f["loss"] - 0.05) < 0.05 and all(0 <= h["loss"] < 1.0 for h in r["history"])
    assert l["loss"] < 0.5 * f["loss"], (f, l)
    assert l["psnr"] > f["psnr"] + 3.0, (f, l)
    assert l["exposure_log_err"] < 0.5 * f["exposure_log_err"], (f, l)
    assert all(torch.isfinite(torch.tensor([h["loss"] for h in r["history"]])))


def test_a_step_from_the_rasterizers_radii_leaves_unseen_gaussians_untouched():
    """rasterizer -> photometric_loss -> backward -> GaussianAdam.step(visibility=radii) on a small scene: every Gaussian
    with radii == 0 keeps the bits of all five tensors and of their moments; the seen ones move."""
    from casualhdrsplat_amd import GaussianAdam, GaussianRasterizer, cloud_param_groups, photometric_loss
    P = 4000
    sc = S.make_scene(P, 160, 120, 3, seed=21)
    rs, _, _ = Hh.settings_from_scene(sc, DEV)
    names = ("means3D", "opacities", "shs", "scales", "rotations")
    leaf = {k: getattr(sc, k).to(DEV).clone() for k in names}
    with torch.no_grad():
        leaf["means3D"][: P // 4] = sc.camera.campos.to(DEV)          # a quarter of the cloud inside the near plane: never seen
    leaf = {k: v.requires_grad_(True) for k, v in leaf.items()}
    m2 = torch.zeros(P, 3, device=DEV, requires_grad=True)
    opt = GaussianAdam(cloud_param_groups(*[leaf[k] for k in names]), eps=1e-15)
    rast = GaussianRasterizer(rs)
    target = torch.rand(3, 120, 160, device=DEV)
    for it in range(3):
        for v in leaf.values():
            v.grad = None
        out = rast(leaf["means3D"], m2, leaf["opacities"], shs=leaf["shs"], scales=leaf["scales"], rotations=leaf["rotations"])
        image, radii = out[0], out[1]
        photometric_loss(image, target, 0.2).backward()
        before = {k: v.detach().clone() for k, v in leaf.items()}
        moments = {k: [x.clone() for x in (opt.state[v].get("exp_avg"), opt.state[v].get("exp_avg_sq")) if x is not None]
                   for k, v in leaf.items()}
        opt.step(visibility=radii)
        unseen, seen = radii == 0, radii > 0
        assert int(unseen.sum()) >= P // 4 and int(seen.sum()) > P // 10
        for k, v in leaf.items():
            assert torch.equal(before[k][unseen].view(torch.int32), v.detach()[unseen].view(torch.int32)), k
            st = opt.state[v]
            for old, new in zip(moments[k], (st["exp_avg"], st["exp_avg_sq"])):
                assert torch.equal(old[unseen].view(torch.int32), new[unseen].view(torch.int32)), k
            if it == 0:
                assert not st["exp_avg"][unseen].any() and not st["exp_avg_sq"][unseen].any()
        assert not torch.equal(before["shs"][seen], leaf["shs"].detach()[seen])
        assert not torch.equal(before["opacities"][seen], leaf["opacities"].detach()[seen])
