"""GPU parity on ill-conditioned footprints (run with -m gpu on an MI355X): needles and discs with axis ratios of 10 to 1000
(synthetic.anisotropic_scene, helpers.ANISO_SCENES A-E; every other scene of the suite stays below e) against the oracle
under its conditioned guard band -- the instrument tests/test_anisotropy.py pins on the CPU.

What these footprints reach that nothing else does: render.hip's block_may_touch, whose own cancelling quadratic culls per
8 x 8 block with a fixed 0.05 log2 margin (a wrongly culled contributor is a decision that differs OUTSIDE the band: the
first thing asserted); tile lists most of whose entries contribute nothing (a needle's square rect covers tiles it never
touches), feeding the forward's pair_act / tile_work records and the backward's per-lane-group taker lists; the quaternion /
scale chain of preprocess_bwd and activate_bwd at strongly unequal scales.

Per scene: structure bit for bit; every differing decision inside the conditioned band, on at most 1e-3 of the frame;
colour and final_T off the excluded pixels within 1e-4 max(|ref|, 1e-2) + the oracle's per-pixel bound; the masked pass
(dL zeroed on the excluded pixels, both sides, no row excused) with every element inside
    |hip - ref| <= 1e-4 |ref| + C_BOUND 2^-24 abs + k 2^-24 cond .
profiles/anisotropy_parity.json (scripts/anisotropy_parity.py) records each scene's figures.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import activation_reference as R
import helpers as Hh
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIFFER_CAP = 1e-3           # pixels with a differing decision, share of the frame (as test_frame_batch_gpu.py)


def u32(a):
    return np.asarray(a).astype(np.int64) & 0xFFFFFFFF


@contextlib.contextmanager
def environment(**kv):
    """os.environ[k] = v for the forwards inside (the Python host reads the sort switches at every forward)."""
    was = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in was.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _scene(name):
    return S.anisotropic_scene(*Hh.ANISO_SCENES[name])


@functools.lru_cache(maxsize=None)
def _oracle_forward(name):
    """The oracle's frame of a scene, computed once and shared (read only) by the tests that need it."""
    from oracle import c_oracle as O
    O.build()
    sc = _scene(name)
    return sc, Hh.run_oracle(O, sc, backward=False)[0]


def scene_parity(oracle, name, tile_sort=None):
    """One scene through the HIP path (optionally under a tile sort switch) against the oracle: every assertion of this
    module's header; returns the scene's record for profiles/anisotropy_parity.json."""
    k = oracle.K_COND
    sc, f = _oracle_forward(name)
    with environment(**({"HS_TILE_SORT": tile_sort} if tile_sort else {})):
        g = Hh.run_hip(sc)
    st = g["state"]
    if tile_sort:
        assert int(st["tile_sort"]) == {"radix": 0, "count": 1, "hier": 2}[tile_sort], (name, tile_sort, st["tile_sort"])
    R_ = f["R"]
    P = f["radii"].shape[0]
    npix = sc.camera.W * sc.camera.H
    # structure, bit for bit
    assert st["num_rendered"] == R_, name
    for q in ("depths", "xy", "conic_opacity"):
        assert np.array_equal(Hh.bits(st[q][:P]), Hh.bits(f[q])), (name, q)
    assert np.array_equal(st["radii"][:P], f["radii"]) and np.array_equal(g["radii"], f["radii"]), name
    assert np.array_equal(u32(st["tiles_touched"][:P]), u32(f["tiles_touched"])), name
    assert np.abs(st["rgb"][:P] - f["rgb"]).max() <= 1e-6 * max(1.0, np.abs(f["rgb"]).max()), name
    assert np.array_equal(u32(st["offsets"]), u32(f["offsets"])), name
    assert np.array_equal(u32(st["point_list"][:R_]), u32(f["point_list"])), name
    assert np.array_equal(u32(st["ranges"]), u32(f["ranges"])), name
    # decisions: confined to the conditioned band (asserted inside), few
    m = Hh.decision_masks(oracle, sc, [f], st, what=f"scene {name}", conditioned=k)
    kind, ratio, fraction, seed = Hh.ANISO_SCENES[name]
    rec = dict(kind=kind, ratio=ratio, fraction=fraction, seed=seed, R=int(R_), largest_radius=int(f["radii"].max()), largest_M=float(m["max_M"]),
               band_share=float(m["pix_risk"].mean()), unclassifiable_share=m["n_unclassifiable"] / npix,
               pixels_with_a_differing_decision=m["n_differ"])
    print(f"scene {name}" + (f" [{tile_sort}]" if tile_sort else ""), rec, flush=True)
    assert m["pix_risk"].mean() <= Hh.ANISO_BAND_CAP and m["n_unclassifiable"] <= Hh.ANISO_UNCLASSIFIABLE_CAP * npix, name
    assert m["n_differ"] <= DIFFER_CAP * npix, (name, "pixels with a differing decision", m["n_differ"])
    # images: inside the per-pixel bounds off the excluded pixels
    rec["color_share_of_bound"] = Hh.check_image_conditioned(g["color"], f["color"], m, m["color_tol"][0], f"scene {name} color")
    rec["final_T_share_of_bound"] = Hh.check_image_conditioned(
        st["final_T"][0], f["final_T"], m, m["T_tol"][0] * np.abs(f["final_T"].astype(np.float64)), f"scene {name} final_T")
    # the masked pass: no row excused, both bound terms, zero elements outside
    with environment(**({"HS_TILE_SORT": tile_sort} if tile_sort else {})):
        g2, b2, _ = Hh.masked_backward_pass(oracle, sc, m, [f], hdr=False, what=f"scene {name}", conditioned=True)
    rep = Hh.assert_grads_bounded(g2, b2, what=f"scene {name} masked", conditioned=k)
    assert all(float(np.abs(g2["d_" + gk]).sum()) > 0 for gk, _ in Hh.GRAD_KEYS), name
    rec["c_needed_abs"] = {q: round(v[1], 3) for q, v in rep.items()}
    rec["c_needed_cond"] = {q: round(v[2], 3) for q, v in rep.items()}
    return rec


@pytest.mark.parametrize("name", sorted(Hh.ANISO_SCENES))
def test_anisotropic_scene_vs_oracle(oracle, name):
    scene_parity(oracle, name)


@pytest.mark.parametrize("tile_sort", ["radix", "hier"])
def test_long_idle_tile_lists_under_the_other_tile_sorts(oracle, tile_sort):
    """Scene C (500 px needles: rects of hundreds of tiles, most of which the needle never touches) through the radix and
    the hierarchical tile sort: the same structure, decisions, images and gradients hold."""
    scene_parity(oracle, "C", tile_sort=tile_sort)


def test_two_backwards_of_scene_c_give_the_same_bits():
    sc = _scene("C")
    a, b = Hh.run_hip(sc), Hh.run_hip(sc)
    assert np.array_equal(Hh.bits(a["color"]), Hh.bits(b["color"]))
    for gk, _ in Hh.GRAD_KEYS:
        assert float(np.abs(a["d_" + gk]).sum()) > 0
        assert np.array_equal(Hh.bits(a["d_" + gk]), Hh.bits(b["d_" + gk])), gk


def test_raw_parameters_of_scene_b_against_the_two_call_path():
    """Scene B (every Gaussian a needle of ratio up to 30) through parameterization="raw" against the default rasterizer fed
    the activated tensors the library produced, as test_raw_parameters_gpu.py does on well-rounded clouds: outputs and
    the gradients the conversion does not touch bit for bit; the stored-space gradients of opacity, scales and rotations --
    activate_bwd's quaternion / scale chain at strongly unequal scales -- the bits of the numpy restatement of the chain rule
    applied to the two-call path's gradients, and within the bars of float64."""
    from casualhdrsplat_amd import GaussianRasterizer, inspect_state
    sc = _scene("B")
    P = sc.means3D.shape[0]
    gen = torch.Generator().manual_seed(77)
    x = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))
    l = torch.log(sc.scales)
    q = sc.rotations * torch.exp(torch.empty(P, 1).uniform_(-2.0, 2.0, generator=gen))
    assert float((l.max(dim=1).values - l.min(dim=1).values).max()) > np.log(25.0)      # the unequal scales this is about
    res, acts = {}, None
    for how in ("raw", "activated"):
        rs, _, _ = Hh.settings_from_scene(sc, DEV)
        opac, scales, rots = (x, l, q) if how == "raw" else acts
        leaf = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=opac, shs=sc.shs, scales=scales,
                    rotations=rots)
        leaf = {n: v.detach().clone().to(DEV).requires_grad_(True) for n, v in leaf.items()}
        args = dict(leaf)
        out = GaussianRasterizer(rs, parameterization=how)(args.pop("means3D"), args.pop("means2D"), args.pop("opacities"), **args)
        if how == "raw":
            st = inspect_state(out[0])
            acts = tuple(st[n].detach().clone().cpu() for n in ("opacities", "scales", "rotations"))
        (out[0] * sc.dL_dimage.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        res[how] = dict(out=[o.detach().cpu() for o in out], grads={n: v.grad.detach().cpu() for n, v in leaf.items()})
    for a, b in zip(res["raw"]["out"], res["activated"]["out"]):
        assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    assert int((res["raw"]["out"][1] > 0).sum()) > 2000
    gr, gt = res["raw"]["grads"], res["activated"]["grads"]
    converted = ("opacities", "scales", "rotations")
    for n in gr:
        if n not in converted:
            assert float(gr[n].abs().sum()) > 0 or n == "means2D"
            assert torch.equal(gr[n].view(torch.int32), gt[n].view(torch.int32)), n
    act = tuple(t.numpy() for t in acts)
    g = tuple(gt[n].numpy() for n in converted)
    got = tuple(gr[n].numpy() for n in converted)
    assert all(np.isfinite(t).all() and float(np.abs(t).sum()) > 0 for t in got)
    c = R.backward_constants(g, act, q.numpy(), got)
    for n, v in c.items():
        print(f"scene B raw: {n} c = {v:.4f} (bar {R.BARS[n]})")
        assert v <= R.BARS[n], (n, v)
    want = R.backward(g[0], act[0], g[1], act[1], g[2], act[2], q.numpy())
    for a, b in zip(got, want):
        assert R.same_bits(a, b)
