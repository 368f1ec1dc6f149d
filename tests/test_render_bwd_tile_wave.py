"""Render backward, one wave per tile (four pixels per lane, the four DPP rows of the wave as lane groups): the cases in
which that form can go wrong, each against the C oracle under the project's own per-element error model
(helpers.assert_grads_bounded at its default constant, on the rows whose pixels took identical decisions on both sides).

  * one 16 x 16 tile with a few hundred faint Gaussians: several staging batches and a partial last one;
  * a 37 x 23 frame: tiles cut off in both directions;
  * all Gaussians inside ONE 8 x 8 block of a 16 x 16 frame: one lane group (one plane 2g + w of the entry records) works
    while the other three walk sentinels;
  * HDR + CRF with two poses at 48 x 32: the CRF-table / exposure gradients of the fused backward (whose first stage rides
    at the end of the render backward's launch) equal those of the staged calls bit for bit;
  * the inverse-depth output (the kernel's DEPTH instantiation: ten sums per entry instead of nine);
  * two backward calls on one forward give the same bits in every tensor.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import helpers as Hh
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

NAMES = ("means3D", "opacities", "shs", "scales", "rotations")


def _vs_oracle(O, sc, what, min_clear=0.5):
    """Gradients of the single-pose linear frame against the oracle's, every element of every clear row inside the bound."""
    f, _ = Hh.run_oracle(O, sc, backward=False)
    g = Hh.run_hip(sc)
    m = Hh.decision_masks(O, sc, [f], g["state"], what=what)
    r = Hh.run_oracle_poses(O, sc, [sc.camera], sc.dL_dimage.numpy(), [f], bounds=True)
    clear = ~m["rows"]
    assert clear.mean() >= min_clear, (what, "clear rows", float(clear.mean()))
    rep = Hh.assert_grads_bounded(g, r, what=what, rows=clear)
    print(what, "n_contrib max", int(f["n_contrib"].max()), "clear rows", int(clear.sum()), "of", clear.size,
          {k: round(v[1], 2) for k, v in rep.items()}, flush=True)
    for k, rk in Hh.GRAD_KEYS:
        assert float(np.abs(g["d_" + k][clear]).sum()) > 0, (what, k)
    return g, f


def deep_tile_scene():
    """307 faint Gaussians on one 16 x 16 tile: no pixel terminates early, the tile's list is walked to its end (a prime
    number of entries: the last batch is partial at every batch size)."""
    sc = S.make_scene(307, 16, 16, 1, seed=3)
    sc.opacities *= 0.05
    return sc


def test_single_tile_many_batches(oracle):
    sc = deep_tile_scene()
    g, f = _vs_oracle(oracle, sc, "one tile, 307 faint Gaussians")
    n = int(f["n_contrib"].max())
    # several batches and a partial last one, whatever the batch size between 32 and 64 is
    assert n > 3 * 64 and all(n % kb for kb in range(32, 65)), n


def test_partial_tiles(oracle):
    sc = S.make_scene(2000, 37, 23, 2, seed=5)
    _vs_oracle(oracle, sc, "37 x 23, 2000 Gaussians")


def block_scene(g, w):
    """24 small Gaussians whose centres lie well inside the 8 x 8 block (g, w) of a 16 x 16 frame."""
    sc = S.make_scene(24, 16, 16, 1, seed=40 + 2 * g + w)
    gen = torch.Generator().manual_seed(7 + 2 * g + w)
    u = torch.rand(3, 24, generator=gen, dtype=torch.float64)
    S._retarget(sc, torch.arange(24), 8 * g + 3.0 + 2.0 * u[0], 8 * w + 3.0 + 2.0 * u[1], 3.0 + 4.0 * u[2],
                torch.full((24,), 0.3, dtype=torch.float64))
    return sc


@pytest.mark.parametrize("g,w", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_one_block_at_a_time(oracle, g, w):
    sc = block_scene(g, w)
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    nc = np.asarray(f["n_contrib"]).reshape(16, 16)
    inside = np.zeros((16, 16), bool)
    inside[8 * w:8 * w + 8, 8 * g:8 * g + 8] = True
    # (checked on the CPU before the scene is used: only this block takes anything)
    assert (nc[~inside] == 0).all() and (nc[inside] > 0).sum() >= 16, (g, w, nc)
    _vs_oracle(oracle, sc, f"block g={g} w={w}")


@pytest.fixture(scope="module")
def hdr_two_poses():
    """One HDR + CRF forward of two poses at 48 x 32, kept for the replays of the two tests below."""
    from casualhdrsplat_amd import GaussianRasterizer
    P, W, H = 1500, 48, 32
    sc = S.make_scene(P, W, H, 1, seed=12, hdr=True)
    cams = S.blur_poses(W, H, 2, step=0.03)
    rs, expo, crf = Hh.settings_from_scene(sc, "cuda", cams, hdr=True, requires_grad=True)
    leaves = [getattr(sc, k).cuda().requires_grad_(True) for k in NAMES]
    out = GaussianRasterizer(rs)(leaves[0], torch.zeros(P, 3, device="cuda", requires_grad=True), leaves[1],
                                 shs=leaves[2], scales=leaves[3], rotations=leaves[4])
    return out, sc.dL_dimage.cuda(), (leaves, expo, crf)


def _tensors(g):
    return {k: v.detach().cpu().numpy().copy() for k, v in g.items()
            if isinstance(v, torch.Tensor) and not k.startswith("_") and k != "view_colors"}


def test_crf_gradients_fused_equal_staged(hdr_two_poses):
    from casualhdrsplat_amd import _lib as L
    from casualhdrsplat_amd.rasterizer import replay_backward
    out, dL, _ = hdr_two_poses
    fused = _tensors(replay_backward(out[0], dL))
    replay_backward(out[0], dL, L.HS_BWD_RENDER)
    staged = _tensors(replay_backward(out[0], dL, L.HS_BWD_CRF))
    assert np.abs(fused["crf_table"]).max() > 0 and float(np.abs(fused["exposure"]).max()) > 0
    for k in ("exposure", "crf_table"):
        assert np.array_equal(Hh.bits(fused[k]), Hh.bits(staged[k])), k


def test_two_backwards_give_the_same_bits(hdr_two_poses):
    from casualhdrsplat_amd.rasterizer import replay_backward
    out, dL, _ = hdr_two_poses
    a = _tensors(replay_backward(out[0], dL))
    b = _tensors(replay_backward(out[0], dL))
    assert len(a) >= 8 and np.abs(a["means3D"]).max() > 0
    for k in a:
        assert np.array_equal(Hh.bits(a[k]), Hh.bits(b[k])), k


def test_inverse_depth_instantiation(oracle):
    """return_invdepth with an upstream gradient on it: the backward's DEPTH instantiation, against the oracle's backward
    with dL/d(inverse depth)."""
    from casualhdrsplat_amd import GaussianRasterizer, inspect_state
    P, W, H = 600, 40, 40
    sc = S.make_scene(P, W, H, 1, seed=23)
    gD = (torch.randn(H, W, generator=torch.Generator().manual_seed(4)) * 5).float()
    rs, _, _ = Hh.settings_from_scene(sc, "cuda")
    leaf = {k: getattr(sc, k).cuda().requires_grad_(True) for k in NAMES}
    leaf["means2D"] = torch.zeros(P, 3, device="cuda", requires_grad=True)
    out = GaussianRasterizer(rs, return_invdepth=True)(leaf["means3D"], leaf["means2D"], leaf["opacities"], shs=leaf["shs"],
                                                       scales=leaf["scales"], rotations=leaf["rotations"])
    assert len(out) == 3 and out[2].shape == (H, W)
    st = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in inspect_state(out[0]).items()}
    ((out[0] * sc.dL_dimage.cuda()).sum() + (out[2] * gD.cuda()).sum()).backward()
    got = {"d_" + k: v.grad.cpu().numpy() for k, v in leaf.items()}
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    m = Hh.decision_masks(oracle, sc, [f], st, what="invdepth")
    r = oracle.backward(Hh.oracle_camera(oracle, sc), f, sc.dL_dimage.numpy(), sc.means3D.numpy(), shs=sc.shs.numpy(),
                        scales=sc.scales.numpy(), rotations=sc.rotations.numpy(), dL_dinvdepth_img=gD.numpy(), bounds=True)
    clear = ~m["rows"]
    assert clear.mean() >= 0.5
    rep = Hh.assert_grads_bounded(got, r, what="invdepth 40 x 40", rows=clear)
    print("invdepth", {k: round(v[1], 2) for k, v in rep.items()}, flush=True)
    # the depth term reaches the gradients: without it they differ
    r0 = Hh.run_oracle_poses(oracle, sc, [sc.camera], sc.dL_dimage.numpy(), [f])
    assert np.abs(r["dL_dmeans3D"] - r0["dL_dmeans3D"]).max() > 1e-3 * np.abs(r0["dL_dmeans3D"]).max()
