"""The bilateral-grid correction (casualhdrsplat_amd.bilagrid, bilagrid.hip) on the MI355X against tests/bilagrid_reference.py:
the slice and its gradient to the image BIT FOR BIT the float32 restatement, the gradient to the grids against the float64
truth inside the project's gradient contract (1e-4 |truth| + 8 2^-24 sum|term|; no fixed point is used, so
no quantisation term; the two shapes this file adds to the issue's five have lattices finer than the pixels and take the
conditioning term bilagrid_reference.grid_bound_sparse derives on top), exact zeros for unused grids, reproducible bits
whatever the workspace held, optional outputs, the autograd wrappers against the ABI's bits and through the rasterizer and
the loss, the total variation, a captured graph replayed after the image and the grid ids changed, a fit from the identity, and examples/train_synthetic.py --bilagrid.
Every output and workspace is filled with a pattern of tests/poison.py before each call."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import bilagrid_reference as R
import helpers as Hh
import poison
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
GUARD = 512        # bytes of pattern behind the workspace that must stay

# (F, H, W | G, L, Y, X), ids: the issue's five, then a grid finer than the pixel tile (its cells do not fit the LDS stage: the
# kernel reads the grid from memory; L = 16 takes the widest instantiation of the gather) and a mix of staged and unstaged tiles
SHAPES = [((1, 37, 70, 1, 5, 3, 4), [0]), ((3, 40, 72, 4, 4, 3, 4), [2, 0, 2]), ((2, 33, 65, 2, 1, 1, 1), [0, 1]),
          ((1, 16, 64, 1, 2, 2, 2), [0]), ((2, 208, 320, 3, 8, 16, 16), [1, 0]),
          ((1, 16, 64, 1, 16, 64, 64), [0]), ((1, 40, 130, 2, 3, 9, 64), [1])]
N_ISSUE = 5        # the first five are held to the plain contract
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{s[3]}x{s[4]}x{s[5]}x{s[6]}" for s, _ in SHAPES]


@functools.lru_cache(maxsize=None)
def reference(i):
    """Case i with its references, computed once and shared (read only)."""
    shape, ids = SHAPES[i]
    case = R.make_case(*shape, ids=ids, seed=i)
    case["out"] = R.slice_forward(case["image"], case["grids"], ids)
    case["d_image"] = R.slice_backward_image(case["image"], case["grids"], ids, case["d_out"])
    case["d_grids"], case["mag"], cond = R.slice_backward_grids(case["image"], case["grids"], ids, case["d_out"], with_cond=True)
    case["bound"] = R.grid_bound(case["d_grids"], case["mag"]) if i < N_ISSUE else R.grid_bound_sparse(case["d_grids"], case["mag"], cond)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _dev(x, dtype=None):
    return torch.from_numpy(np.array(x, order="C", copy=True)).to(DEV) if dtype is None else torch.tensor(list(x), dtype=dtype, device=DEV)


def _poisoned(shape, dtype, pattern, seed=0):
    return poison.fill_(torch.empty(shape, dtype=dtype, device=DEV), pattern, seed=seed)


def _args(case, image, grids, ids):
    from casualhdrsplat_amd import _lib as L
    a = L.hs_bilagrid_args()
    a.F, a.H, a.W, a.G, a.L, a.Y, a.X = case["shape"]
    a.image, a.grids, a.grid_ids = image.data_ptr(), grids.data_ptr(), ids.data_ptr()
    return a


def abi_forward(case, ids=None, pattern="nan"):
    from casualhdrsplat_amd import _lib as L
    lib = L.load()
    image, grids = _dev(case["image"]), _dev(case["grids"])
    idt = _dev(case["ids"] if ids is None else ids, torch.int32)
    out = _poisoned(image.shape, torch.float32, pattern)
    a = _args(case, image, grids, idt)
    a.out = out.data_ptr()
    L.check(lib.hs_bilagrid_slice(C.byref(a), torch.cuda.current_stream().cuda_stream), "hs_bilagrid_slice")
    torch.cuda.synchronize()
    assert same_bits(image.cpu().numpy(), case["image"]) and same_bits(grids.cpu().numpy(), case["grids"]), "an input was written"
    return out.cpu().numpy()


def abi_backward(case, ids=None, pattern="nan", want_image=True, want_grids=True):
    """hs_bilagrid_slice_backward with both outputs and the workspace filled with `pattern`; returns (dL_dimage, dL_dgrids) as
    the call left them (a skipped output: the pattern)."""
    from casualhdrsplat_amd import _lib as L
    lib = L.load()
    image, grids, d_out = _dev(case["image"]), _dev(case["grids"]), _dev(case["d_out"])
    idt = _dev(case["ids"] if ids is None else ids, torch.int32)
    nbytes = lib.hs_bilagrid_workspace_bytes(*case["shape"])
    assert nbytes == R.workspace_bytes(*case["shape"]) > 0
    ws = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    poison.fill_(ws[:nbytes], pattern, seed=7)
    before = ws.clone()
    d_image = _poisoned(image.shape, torch.float32, pattern, seed=1)
    d_grids = _poisoned(grids.shape, torch.float32, pattern, seed=2)
    keep = (d_image.clone(), d_grids.clone())
    a = _args(case, image, grids, idt)
    a.dL_dout = d_out.data_ptr()
    a.dL_dimage = d_image.data_ptr() if want_image else None
    a.dL_dgrids = d_grids.data_ptr() if want_grids else None
    a.workspace = ws.data_ptr() if want_grids else None
    L.check(lib.hs_bilagrid_slice_backward(C.byref(a), torch.cuda.current_stream().cuda_stream), "hs_bilagrid_slice_backward")
    torch.cuda.synchronize()
    assert torch.equal(ws[nbytes:], before[nbytes:]), "written behind the workspace"
    if not want_grids:
        assert torch.equal(ws, before), "the workspace was written although no grid gradient was asked for"
        assert poison.bytes_of(d_grids) == poison.bytes_of(keep[1]), "a skipped dL_dgrids was written"
    if not want_image:
        assert poison.bytes_of(d_image) == poison.bytes_of(keep[0]), "a skipped dL_dimage was written"
    return d_image.cpu().numpy(), d_grids.cpu().numpy()


def hold_grids(got, case, what):
    """Every element of dL_dgrids inside 1e-4 |truth| + 8 2^-24 sum|term| (the case's bound); prints the worst use of it."""
    truth, bound = case["d_grids"], case["bound"]
    assert got.dtype == np.float32 and np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - truth)
    used = float((err / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
    print(f"{what}: worst |error| / bound = {used:.4f}, worst |error| = {err.max():.3e}")
    assert (err <= bound).all(), (what, used, int((err > bound).sum()))
    assert not got[bound == 0].any(), f"{what}: an element without terms is not exactly zero"
    return used


# ---- 1. forward ----

@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_forward_is_the_float32_restatement_bit_for_bit(i):
    case = reference(i)
    z = R.luma(case["image"].transpose(1, 0, 2, 3), np.float32)
    assert (z < 0).any() and (z > 1).any() and (z == 0).any()           # both clamps occur, and pixels sit exactly on one
    got = abi_forward(case)
    diff = got.view(np.uint32) != case["out"].view(np.uint32)
    print(f"{IDS[i]}: {int(diff.sum())} of {diff.size} elements differ from the restatement")
    assert same_bits(got, case["out"]), (IDS[i], int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert same_bits(abi_forward(case, pattern="ff"), got)


@pytest.mark.parametrize("i", [1, 4], ids=[IDS[1], IDS[4]])
def test_ids_outside_the_grids_are_the_identity_bit_for_bit(i):
    case = dict(reference(i))
    F, G = case["shape"][0], case["shape"][3]
    image = case["image"].copy()
    image.view(np.uint32)[0, 0, 1, :3] = (0x7FC12345, 0x80000000, 0x00000001)        # a NaN payload, -0.0, a denormal
    case["image"] = image
    ids = ([-1, G] * F)[:F]
    assert same_bits(abi_forward(case, ids=ids), image)
    d_image, d_grids = abi_backward(case, ids=ids)
    assert same_bits(d_image, case["d_out"]) and not d_grids.any() and same_bits(d_grids, np.zeros_like(d_grids))


# ---- 2. backward ----

@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_backward_image_bits_and_grid_gradient_inside_the_contract(i):
    case = reference(i)
    d_image, d_grids = abi_backward(case)
    diff = d_image.view(np.uint32) != case["d_image"].view(np.uint32)
    print(f"{IDS[i]}: {int(diff.sum())} of {diff.size} elements of dL_dimage differ from the restatement")
    assert same_bits(d_image, case["d_image"]), (IDS[i], int(diff.sum()), np.argwhere(diff)[:4].tolist())
    hold_grids(d_grids, case, IDS[i])
    G = case["shape"][3]
    for g in range(G):
        if g not in case["ids"]:
            assert same_bits(d_grids[g], np.zeros_like(d_grids[g])), f"unused grid {g} is not exactly zero"
        else:
            assert d_grids[g].any()
    # a second run over a workspace and outputs poisoned differently: the same bits
    again = abi_backward(case, pattern="random")
    assert same_bits(again[0], d_image) and same_bits(again[1], d_grids)
    again = abi_backward(case, pattern="zero")
    assert same_bits(again[0], d_image) and same_bits(again[1], d_grids)
    # a NULL output skips only that output
    only_image = abi_backward(case, want_grids=False)
    assert same_bits(only_image[0], d_image)
    only_grids = abi_backward(case, want_image=False, pattern="a5")
    assert same_bits(only_grids[1], d_grids)


def test_a_duplicate_id_is_summed_and_identity_frames_add_nothing():
    case = reference(1)                                           # ids [2, 0, 2]
    _, d_grids = abi_backward(case)
    # the two frames of grid 2 alone, and each alone: the sum is the sum (to rounding), never one of them
    sub = lambda fr: dict(case, image=case["image"][fr], d_out=case["d_out"][fr], shape=(len(fr),) + case["shape"][1:])   # noqa: E731
    a = abi_backward(sub([0]), ids=[2])[1][2].astype(np.float64)
    b = abi_backward(sub([2]), ids=[2])[1][2].astype(np.float64)
    both = d_grids[2].astype(np.float64)
    assert np.abs(both - (a + b)).max() <= 2.0 ** -23 * np.abs(a + b).max() + 1e-12
    assert np.abs(both - a).max() > 1e-3 and np.abs(both - b).max() > 1e-3
    # the middle frame without a grid: grids 2's bits stay (the same terms in the same order), grid 0 gets exact zeros
    d_image, skipped = abi_backward(case, ids=[2, -1, 2])
    assert same_bits(skipped[2], d_grids[2]) and same_bits(skipped[0], np.zeros_like(skipped[0]))
    assert same_bits(d_image[1], case["d_out"][1]) and same_bits(d_image[0], case["d_image"][0])
    # ... and the bits of a call that never saw that frame
    two = abi_backward(sub([0, 2]), ids=[2, 2])[1]
    assert same_bits(two[2], d_grids[2])


# ---- 3. autograd ----

def test_module_gradients_are_the_abis_bits(monkeypatch):
    from casualhdrsplat_amd import BilateralGrid
    case = reference(1)
    _, _, _, G, L, Y, X = case["shape"]
    m = BilateralGrid(G, grid_X=X, grid_Y=Y, grid_W=L, device=DEV)
    assert same_bits(m.grids.detach().cpu().numpy(), R.identity(G, L, Y, X))
    with torch.no_grad():
        m.grids.copy_(_dev(case["grids"]))
    image = _dev(case["image"]).requires_grad_(True)
    with poison.poisoned(monkeypatch, "nan") as session:
        out = m(image, case["ids"])
        out.backward(_dev(case["d_out"]))
    session.require("casualhdrsplat_amd.bilagrid", at_least=4)           # out, dL_dimage, the workspace, dL_dgrids
    want_image, want_grids = abi_backward(case)
    assert same_bits(out.detach().cpu().numpy(), case["out"])
    assert same_bits(image.grad.cpu().numpy(), want_image) and same_bits(m.grids.grad.cpu().numpy(), want_grids)
    # ids as a device tensor, one [3, H, W] frame, and only the grids asking for a gradient
    one = _dev(case["image"][0])
    m.grids.grad = None
    out1 = m(one, torch.tensor([2], dtype=torch.int32, device=DEV))
    assert out1.shape == one.shape and same_bits(out1.detach().cpu().numpy(), case["out"][0])
    out1.backward(_dev(case["d_out"][0]))
    sub = dict(case, image=case["image"][:1], d_out=case["d_out"][:1], shape=(1,) + case["shape"][1:])
    assert same_bits(m.grids.grad.cpu().numpy(), abi_backward(sub, ids=[2])[1])
    with torch.no_grad():
        assert same_bits(m(one, -1).cpu().numpy(), case["image"][0])


def test_render_slice_loss_gives_the_rasterizer_the_abis_gradient():
    """GaussianRasterizer -> slice_image -> photometric_loss: the leaves' gradients are bit for bit those of a rasterizer
    backward fed the ABI's dL_dimage (of the loss's gradient) directly."""
    from casualhdrsplat_amd import GaussianRasterizer, photometric_loss, slice_image
    P, W, H = 600, 72, 40
    sc = S.make_scene(P, W, H, 1, seed=5)
    rs, _, _ = Hh.settings_from_scene(sc, DEV)
    names = ("means3D", "opacities", "shs", "scales", "rotations")
    grids_np = reference(1)["grids"]
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)).to(DEV)

    def render():
        leaf = {k: getattr(sc, k).clone().to(DEV).requires_grad_(True) for k in names}
        m2 = torch.zeros(P, 3, device=DEV, requires_grad=True)
        out = GaussianRasterizer(rs)(leaf["means3D"], m2, leaf["opacities"], shs=leaf["shs"], scales=leaf["scales"],
                                     rotations=leaf["rotations"])
        return leaf, out[0]

    leaf, image = render()
    grids = _dev(grids_np).requires_grad_(True)
    sliced = slice_image(image, grids, 3)
    photometric_loss(sliced, target, 0.2).backward()
    # the same chain by hand: the loss's gradient at the sliced image, through the ABI, into a second rasterizer's backward
    leaf2, image2 = render()
    assert torch.equal(image2, image)
    s2 = sliced.detach().clone().requires_grad_(True)
    photometric_loss(s2, target, 0.2).backward()
    case = dict(image=image.detach().cpu().numpy()[None], grids=grids_np, d_out=s2.grad.cpu().numpy()[None], ids=[3],
                shape=(1, H, W) + grids_np.shape[:1] + grids_np.shape[2:])
    d_image, d_grids = abi_backward(case)
    assert np.abs(d_image).sum() > 0
    image2.backward(_dev(d_image[0]))
    for k in names:
        assert leaf[k].grad is not None and torch.equal(leaf[k].grad, leaf2[k].grad), k
        assert bool(torch.isfinite(leaf[k].grad).all())
    assert float(leaf["shs"].grad.abs().sum()) > 0
    assert same_bits(grids.grad.cpu().numpy(), d_grids)


# ---- 4. total variation ----

def abi_tv(grids_np, upstream=None, pattern="nan"):
    from casualhdrsplat_amd import _lib as L
    lib = L.load()
    grids = _dev(grids_np)
    a = L.hs_bilagrid_tv_args()
    a.G, _, a.L, a.Y, a.X = grids_np.shape
    a.grids = grids.data_ptr()
    ws = torch.full((L.HS_BILAGRID_TV_WORKSPACE_BYTES + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    poison.fill_(ws[:L.HS_BILAGRID_TV_WORKSPACE_BYTES], pattern, seed=4)
    out = _poisoned((1,), torch.float32, pattern)
    a.tv, a.workspace = out.data_ptr(), ws.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    L.check(lib.hs_bilagrid_tv(C.byref(a), stream), "hs_bilagrid_tv")
    grad = None
    if upstream is not None:
        up = torch.tensor([upstream], dtype=torch.float32, device=DEV)
        grad = _poisoned(grids.shape, torch.float32, pattern, seed=5)
        a.dL_dtv, a.dL_dgrids = up.data_ptr(), grad.data_ptr()
        L.check(lib.hs_bilagrid_tv_backward(C.byref(a), stream), "hs_bilagrid_tv_backward")
        grad = grad.cpu().numpy()
    torch.cuda.synchronize()
    assert (ws[L.HS_BILAGRID_TV_WORKSPACE_BYTES:] == 0x5A).all(), "written behind the workspace"
    return float(out.cpu().numpy()[0]), grad


@pytest.mark.parametrize("shape", [(1, 8, 16, 16), (5, 4, 3, 4), (5, 1, 3, 4), (1, 5, 7, 1), (5, 16, 64, 64), (2, 1, 1, 1)])
def test_tv_value_and_gradient_against_float64(shape):
    from casualhdrsplat_amd import tv_loss
    G, L, Y, X = shape
    g = (R.identity(G, L, Y, X) + 0.3 * np.random.default_rng(2).standard_normal((G, 12, L, Y, X))).astype(np.float32)
    want, want_grad = R.tv(g)
    got, grad = abi_tv(g, upstream=0.37)
    print(f"{shape}: tv {got!r} against {want!r}; relative error {abs(got - want) / max(want, 1e-300):.2e}")
    assert abs(got - want) <= 1e-6 * want
    assert np.abs(grad - 0.37 * want_grad).max() <= 1e-6 * np.abs(0.37 * want_grad).max()
    for pattern in ("ff", "random"):
        again, grad2 = abi_tv(g, upstream=0.37, pattern=pattern)
        assert again == got and same_bits(grad2, grad)
    assert abi_tv(R.identity(G, L, Y, X), upstream=1.0)[0] == 0.0
    assert not abi_tv(R.identity(G, L, Y, X), upstream=1.0)[1].any()
    # the wrapper: a 0-dim device tensor with the ABI's bits, 10 tv gives 10 times the gradient of tv
    t = _dev(g).requires_grad_(True)
    v = tv_loss(t)
    assert v.dim() == 0 and v.device.type == "cuda" and float(v.detach()) == got
    (10.0 * v).backward()
    if want > 0:
        assert np.abs(t.grad.cpu().numpy() - 10.0 * want_grad).max() <= 1e-6 * np.abs(10.0 * want_grad).max()
    else:
        assert not t.grad.any()


# ---- 5. capture ----

def test_captured_slice_and_backward_follow_the_image_and_the_ids():
    """slice_image + its backward inside ONE torch.cuda.graph (a single chain of kernels: no parallel branches), replayed
    after the image and the CONTENTS of grid_ids changed: bit for bit the eager results."""
    from casualhdrsplat_amd import slice_image
    case = reference(1)
    G = case["shape"][3]
    image = _dev(case["image"]).requires_grad_(True)
    grids = _dev(case["grids"]).requires_grad_(True)
    ids = torch.tensor(case["ids"], dtype=torch.int32, device=DEV)
    d_out = _dev(case["d_out"])

    def step():
        out = slice_image(image, grids, ids)
        gi, gg = torch.autograd.grad(out, [image, grids], d_out)
        return out.detach(), gi, gg

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    rng = np.random.default_rng(9)
    for rep, new_ids in enumerate(([2, 0, 2], [1, 3, -1], [0, G, 0])):
        if rep:
            with torch.no_grad():
                image.copy_(_dev(rng.uniform(-0.2, 1.3, size=case["image"].shape).astype(np.float32)))
                ids.copy_(torch.tensor(new_ids, dtype=torch.int32, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static]
        want = step()
        for k, (a, b) in enumerate(zip(got, want)):
            assert poison.bytes_of(a) == poison.bytes_of(b), (rep, k)
        now = dict(case, image=image.detach().cpu().numpy(), ids=new_ids)
        assert same_bits(got[0].cpu().numpy(), R.slice_forward(now["image"], case["grids"], new_ids))
        used = [g for g in range(G) if g in new_ids]
        assert all(bool(got[2][g].any()) for g in used) and not any(bool(got[2][g].any()) for g in range(G) if g not in used)


# ---- 6. fit ----

def test_grids_fit_a_known_correction_from_the_identity():
    """200 steps of torch.optim.Adam(lr=1e-2) on mean|slice(image, g) - slice(image, g_true)| from the identity: 48 x 64 image,
    grid L, Y, X = 4, 3, 4, g_true = identity + 0.15 randn, seed 0.  Ends at <= 0.1 of the initial loss (the torch CPU
    formulation went 0.0748 -> 0.0016, i.e. 0.022)."""
    from casualhdrsplat_amd import BilateralGrid, slice_image
    torch.manual_seed(0)
    image = torch.rand(3, 48, 64).to(DEV)
    m = BilateralGrid(1, grid_X=4, grid_Y=3, grid_W=4, device=DEV)
    g_true = (m.grids.detach().cpu() + 0.15 * torch.randn(1, 12, 4, 3, 4)).to(DEV)
    with torch.no_grad():
        target = slice_image(image, g_true, 0)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    losses = []
    for _ in range(200):
        opt.zero_grad(set_to_none=True)
        loss = (m(image, 0) - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad():
        losses.append((m(image, 0) - target).abs().mean())
    first, last = float(losses[0]), float(losses[-1])
    print(f"fit: {first:.4f} -> {last:.4f}, ratio {last / first:.4f}")
    assert np.isfinite(last) and first > 0.01
    assert last <= 0.1 * first, (first, last)


# ---- 7. the example ----

def _example():
    spec = importlib.util.spec_from_file_location("train_synthetic_bilagrid", os.path.join(ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("batch_frames", [False, True])
def test_example_trains_with_the_bilateral_grids(batch_frames):
    """30 steps of the example with bilagrid=True at the size the other example tests use: every entry finite, the loss (the
    total-variation term included) lower than at step 0, the grids moved off the identity.  The process-wide depth sort
    setting is put back whatever the run's frames made of it: later tests of the suite start where they started before."""
    from casualhdrsplat_amd import _lib as L
    depth_sort = L.load().hs_depth_sort(-1)
    try:
        r = _example().run(P=3000, W=96, H=64, frames=2, virtual=3, steps=30, quiet=True, bilagrid=True, batch_frames=batch_frames)
    finally:
        L.load().hs_depth_sort(depth_sort)
    f, l = r["first"], r["last"]
    print(f"batch_frames={batch_frames}: loss {f['loss']:.5f} -> {l['loss']:.5f}, PSNR {f['psnr']:.3f} -> {l['psnr']:.3f} dB, "
          f"tv {f['tv']:.3e} -> {l['tv']:.3e}")
    assert all(np.isfinite(float(v)) for h in r["history"] for v in h.values())
    assert l["loss"] < f["loss"], (f, l)
    assert f["tv"] == 0.0 and l["tv"] > 0.0                       # the grids start at the identity and moved
    assert bool(torch.isfinite(r["grids"]).all()) and tuple(r["grids"].shape) == (2, 12, 8, 16, 16)


def test_bilagrid_refuses_a_captured_step():
    with pytest.raises(ValueError, match="--bilagrid"):
        _example().run(P=100, W=32, H=32, frames=2, virtual=2, steps=1, bilagrid=True, graph=True, quiet=True)
