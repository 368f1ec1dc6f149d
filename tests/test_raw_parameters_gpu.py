"""GPU checks of the stored parameterisation (activate.hip; GaussianRasterizer(..., parameterization="raw")): the activated
tensors and the converted gradients against float64 within the bars of tests/activation_reference.py (and bit for bit where no
expf enters), the "raw" path against the two-call path (the default rasterizer fed the activated tensors the library
produced) bit for bit, where the gradients live, chunks, capture, a densification, and the training example."""
import ctypes as C
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import activation_reference as R
import helpers as Hh
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = -12345.5          # what rows beyond P hold before and after


def _np(t):
    return t.detach().cpu().numpy()


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _within_bars(c, what):
    for k, v in c.items():
        print(f"{what}: {k} c = {v:.4f} (bar {R.BARS[k]})")
    for k, v in c.items():
        assert v <= R.BARS[k], (what, k, v)


# ---- 1. the kernels through the ABI ----

def _abi_inputs(P, seed):
    x, l, q, g = R.inputs(P, seed)
    x = x[:P].copy()
    if P >= 16:
        x[1:1 + len(R.SPECIAL_LOGITS)] = R.SPECIAL_LOGITS
        q[3] = 0.0                      # a zero quaternion: the clamp
        q[4] = q[4] * np.float32(1e-16) # |q| < 1e-12: the clamp, not zero
    return x, l, q, (g["opacities"][:P].copy(), g["scales"], g["rotations"])


def _carve(arr, offset):
    """`arr` inside a larger PATTERN-filled device buffer, `offset` floats behind a 16-byte aligned address; returns
    (the whole buffer, the view)."""
    n = arr.size
    full = torch.full((n + 64,), PATTERN, dtype=torch.float32, device=DEV)
    assert full.data_ptr() % 16 == 0
    view = full[16 + offset:16 + offset + n]
    view.copy_(torch.from_numpy(arr.reshape(-1)))
    return full, view


def _untouched(full, view_offset, n, lo=0, hi=None):
    """Everything of `full` outside elements [lo, hi) of the view still holds PATTERN."""
    hi = n if hi is None else hi
    a = 16 + view_offset
    return bool((full[:a + lo] == PATTERN).all()) and bool((full[a + hi:] == PATTERN).all())


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("P", [1, 10007, 262144, 1_000_000])
def test_activated_tensors_and_converted_gradients_through_the_abi(P, offset):
    """hs_activate / hs_activate_backward on P rows, the pointers 16-byte aligned or one float off: every activated tensor
    within the bars of float64, the normalised quaternions and -- given the activated values -- the converted gradients equal
    to the numpy restatement bit for bit, the special rows (zero quaternion, |x| = 100) finite, nothing outside the rows asked
    for touched (the forward: beyond P; the backward: outside [g_begin, g_end)), two runs the same bits."""
    from casualhdrsplat_amd import _lib
    L = _lib.load()
    x, l, q, g = _abi_inputs(P, seed=P % 89 + offset)
    stream = torch.cuda.current_stream().cuda_stream
    raw = [_carve(a, offset) for a in (x, l, q)]
    act = [_carve(np.full(a.shape, PATTERN, np.float32), offset) for a in (x, l, q)]
    a = _lib.hs_activate_args()
    a.P = P
    a.opacity_raw, a.scales_raw, a.rotations_raw = (v.data_ptr() for _, v in raw)
    a.opacities, a.scales, a.rotations = (v.data_ptr() for _, v in act)
    _lib.check(L.hs_activate(C.byref(a), stream), "hs_activate")
    torch.cuda.synchronize()
    got = [_np(v).reshape(s.shape) for (_, v), s in zip(act, (x, l, q))]
    assert all(np.isfinite(t).all() for t in got)
    for (full, _), s in zip(act, (x, l, q)):
        assert _untouched(full, offset, s.size)
    for (full, v), s in zip(raw, (x, l, q)):                      # the stored tensors are read only
        assert _untouched(full, offset, s.size) and np.array_equal(_np(v), s.reshape(-1))
    _within_bars(R.forward_constants(x, l, q, got), f"P={P} offset={offset}")
    assert R.same_bits(got[2], R.activate(q=q)[2])                # no expf in the normalisation: the restatement's bits
    if P >= 16:
        o = got[0][1:1 + len(R.SPECIAL_LOGITS)]
        assert o[6] == 1.0 and o[7] == 0.0 and o[8] == 0.5 and 0 < o[5] < 2.0 ** -126
        assert np.array_equal(got[2][3], [0, 0, 0, 0])
    first = [t.copy() for t in got]
    for _, v in act:
        v.fill_(PATTERN)
    _lib.check(L.hs_activate(C.byref(a), stream), "hs_activate")
    torch.cuda.synchronize()
    assert all(R.same_bits(_np(v).reshape(f.shape), f) for (_, v), f in zip(act, first))

    # backward, in place, rows [g0, g1): once a part, once everything
    for g0, g1 in ((P // 3, P - P // 5), (0, P)):
        grads = [_carve(t, offset) for t in g]
        a.g_begin, a.g_end = g0, g1
        a.dL_dopacities, a.dL_dscales, a.dL_drotations = (v.data_ptr() for _, v in grads)
        _lib.check(L.hs_activate_backward(C.byref(a), stream), "hs_activate_backward")
        torch.cuda.synchronize()
        out = [_np(v).reshape(t.shape) for (_, v), t in zip(grads, g)]
        want = R.backward(g[0], got[0], g[1], got[1], g[2], got[2], q)
        for (full, _), t, o_, w, cols in zip(grads, g, out, want, (1, 3, 4)):
            assert _untouched(full, offset, t.size)
            assert R.same_bits(o_[g0:g1], w[g0:g1])                                   # IEEE arithmetic only: the same bits
            assert R.same_bits(o_[:g0], t[:g0]) and R.same_bits(o_[g1:], t[g1:])     # rows outside the range keep g
        if (g0, g1) == (0, P):
            assert all(np.isfinite(o_).all() for o_ in out)
            _within_bars(R.backward_constants(g, got, q, out), f"P={P} offset={offset} backward")
            if P >= 16:
                assert R.same_bits(out[2][3:5], g[2][3:5] / np.float32(1e-12))       # the clamp rule: g / eps
    # an empty range and P = 0 launch nothing
    a.g_begin = a.g_end = P // 2
    assert L.hs_activate_backward(C.byref(a), stream) == 0
    a.P = a.g_begin = a.g_end = 0
    assert L.hs_activate(C.byref(a), stream) == 0 and L.hs_activate_backward(C.byref(a), stream) == 0


# ---- 2 / 3. the "raw" rasterizer against the two-call path ----

def _stored_of(sc, seed):
    """Stored tensors whose activations are (up to rounding) the scene's: logit, log, randomly rescaled quaternions -- with a
    saturated pair of logits and, with scales / rotations, a zero and a tiny quaternion (the clamp)."""
    gen = torch.Generator().manual_seed(seed)
    P = sc.means3D.shape[0]
    x = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))
    x[0], x[1] = 30.0, -30.0
    l = torch.log(sc.scales)
    q = sc.rotations * torch.exp(torch.empty(P, 1).uniform_(-2.0, 2.0, generator=gen))
    q[2] = 0.0
    q[3] = q[3] * 1e-16
    return x, l, q


def _cov3d(scales, rotations):
    q = torch.nn.functional.normalize(rotations.double())
    w, x, y, z = q.unbind(1)
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                      2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = Rm * scales.double()[:, None, :]
    Sg = M @ M.transpose(1, 2)
    return torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).float().contiguous()


CASES = ("ldr_deg3", "hdr_crf_4_free_poses", "antialias_invdepth", "cov3d_raw_opacity", "colors_precomp")


@functools.lru_cache(maxsize=None)
def _case(name):
    """Both paths of one case: {"raw": ..., "two": ...} with outputs, gradients and the tensors involved."""
    from casualhdrsplat_amd import GaussianRasterizer, inspect_state
    P, W, H = 3000, 160, 120
    seed = CASES.index(name) + 40
    hdr, cams, rkw, deg = False, None, {}, 3
    if name == "hdr_crf_4_free_poses":
        hdr, deg = True, 2
        base = S.random_camera(W, H, 7)
        sc = S.make_scene(P, W, H, deg, seed=seed, hdr=True, place_in=base)
        cams = S.perturbed_poses(base, 4, seed=2, rot_step_deg=1.0, step=0.02)
        rkw = dict(return_alpha=True)
    else:
        sc = S.make_scene(P, W, H, 1 if name in ("cov3d_raw_opacity", "colors_precomp") else deg, seed=seed)
    if name == "antialias_invdepth":
        sc.antialias = True
        rkw = dict(return_invdepth=True, return_alpha=True)
    x, l, q = _stored_of(sc, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    cols = torch.rand(P, 3, generator=gen) if name == "colors_precomp" else None
    cov = _cov3d(sc.scales, sc.rotations) if name == "cov3d_raw_opacity" else None
    # upstream gradients of the optional outputs, in the order they are returned: HDR image, alpha, inverse depth
    dL_extra = [torch.randn(*shape, generator=gen) for on, shape in ((hdr, (3, H, W)), (rkw.get("return_alpha"), (H, W)),
                                                                      (rkw.get("return_invdepth"), (H, W))) if on]

    def run(how, opac, scales, rots):
        rs, expo, crf = Hh.settings_from_scene(sc, DEV, cams, hdr=hdr, requires_grad=True)
        pose = []
        if cams is not None:
            rs = rs._replace(viewmatrices=rs.viewmatrices.clone().requires_grad_(True),
                             projmatrices=rs.projmatrices.clone().requires_grad_(True),
                             camposes=rs.camposes.clone().requires_grad_(True))
            pose = [rs.viewmatrices, rs.projmatrices, rs.camposes]
        leaf = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=opac)
        leaf["colors_precomp" if cols is not None else "shs"] = cols if cols is not None else sc.shs
        if cov is not None:
            leaf["cov3D_precomp"] = cov
        else:
            leaf.update(scales=scales, rotations=rots)
        leaf = {k: v.detach().clone().to(DEV).requires_grad_(True) for k, v in leaf.items()}
        rast = GaussianRasterizer(rs, parameterization=how, **rkw)
        return rs, expo, crf, pose, leaf, rast

    res = {}
    acts = None
    for how in ("raw", "activated"):
        opac, scales, rots = (x, l, q) if how == "raw" else acts
        rs, expo, crf, pose, leaf, rast = run(how, opac, scales, rots)
        args = dict(leaf)
        out = rast(args.pop("means3D"), args.pop("means2D"), args.pop("opacities"), **args)
        if how == "raw":
            st = inspect_state(out[0])
            acts = tuple(None if st[k] is None else st[k].detach().clone().cpu() for k in ("opacities", "scales", "rotations"))
        loss = (out[0] * sc.dL_dimage.to(DEV)).sum()
        assert len(out) == 2 + len(dL_extra)
        for o_, dL in zip(out[2:], dL_extra):
            assert o_.shape == dL.shape
            loss = loss + (o_ * dL.to(DEV)).sum()
        loss.backward()
        torch.cuda.synchronize()
        extra = dict(exposure=expo, crf_table=crf, viewmatrices=pose[0], projmatrices=pose[1], camposes=pose[2]) if pose else \
            (dict(exposure=expo, crf_table=crf) if hdr else {})
        res["raw" if how == "raw" else "two"] = dict(
            out=[o_.detach().clone() for o_ in out], leaf=leaf,
            grads={k: v.grad.detach().clone() for k, v in dict(leaf, **extra).items()})
    res["stored"], res["activated"] = (x, l, q), acts
    return res


@pytest.mark.parametrize("name", CASES)
def test_forward_equals_the_two_call_path_bit_for_bit(name):
    """One render with "raw", one with the default rasterizer fed the activated tensors the library produced: the image,
    radii, the HDR image, alpha, inverse depth are bit-identical (alpha and its gradient ride on the HDR and the antialiasing case); the activated tensors are within the bars of float64."""
    r = _case(name)
    assert len(r["raw"]["out"]) == len(r["two"]["out"]) == {"hdr_crf_4_free_poses": 4, "antialias_invdepth": 4}.get(name, 2)
    for a, b in zip(r["raw"]["out"], r["two"]["out"]):
        assert _bits_equal(a, b)
    assert float(r["raw"]["out"][0].abs().sum()) > 0 and int((r["raw"]["out"][1] > 0).sum()) > 500
    x, l, q = r["stored"]
    act = r["activated"]
    only_opacity = name == "cov3d_raw_opacity"
    assert (act[1] is None and act[2] is None) == only_opacity
    got = (_np(act[0]), None if only_opacity else _np(act[1]), None if only_opacity else _np(act[2]))
    _within_bars(R.forward_constants(_np(x), None if only_opacity else _np(l), None if only_opacity else _np(q), got), name)
    assert all(np.isfinite(t).all() for t in got if t is not None)


@pytest.mark.parametrize("name", CASES)
def test_gradients_against_the_two_call_path(name):
    """Everything the conversion does not touch -- means3D, shs / colors_precomp, means2D, cov3D_precomp, exposure, crf_table,
    the pose gradients -- bit-identical to the two-call path's; the stored-space gradients of opacity, scales and rotations
    within the bars of the float64 chain rule applied to the two-call path's activated-space gradients (and the restatement's
    bits); the zero quaternion's gradient by the clamp rule."""
    r = _case(name)
    gr, gt = r["raw"]["grads"], r["two"]["grads"]
    assert set(gr) == set(gt) and float(gr["means3D"].abs().sum()) > 0
    converted = ("opacities", "scales", "rotations")
    for k in gr:
        if k not in converted:
            assert _bits_equal(gr[k], gt[k]), k
    x, l, q = (_np(t) for t in r["stored"])
    act = tuple(None if t is None else _np(t) for t in r["activated"])
    g = tuple(_np(gt[k]) if k in gt else None for k in converted)
    got = tuple(_np(gr[k]) if k in gr else None for k in converted)
    assert all(np.isfinite(t).all() for t in got if t is not None) and float(np.abs(got[0]).sum()) > 0
    _within_bars(R.backward_constants(g, act, q, got), name)
    want = R.backward(g[0], act[0], g[1], act[1], g[2], act[2], q if g[2] is not None else None)
    for a, b in zip(got, want):
        assert (a is None and b is None) or R.same_bits(a, b)
    if got[2] is not None:
        assert R.same_bits(got[2][2:4], g[2][2:4] / np.float32(1e-12))


def _raw_step(sc, stored, rast_kw, dev=DEV):
    from casualhdrsplat_amd import GaussianRasterizer
    rs, expo, crf = Hh.settings_from_scene(sc, dev, hdr=True, requires_grad=True)
    x, l, q = stored
    leaf = [t.detach().clone().to(dev).requires_grad_(True) for t in (sc.means3D, torch.zeros_like(sc.means3D), x, sc.shs, l, q)]
    rast = GaussianRasterizer(rs, **rast_kw)
    return rs, expo, crf, leaf, rast


def test_two_backwards_give_the_same_bits():
    sc = S.make_scene(3000, 160, 120, 2, seed=3, hdr=True)
    stored = _stored_of(sc, 3)
    runs = []
    for _ in range(2):
        rs, expo, crf, leaf, rast = _raw_step(sc, stored, dict(parameterization="raw"))
        out = rast(leaf[0], leaf[1], leaf[2], shs=leaf[3], scales=leaf[4], rotations=leaf[5])
        (out[0] * sc.dL_dimage.to(DEV)).sum().backward()
        runs.append([t.grad.clone() for t in leaf + [expo, crf]])
    for a, b in zip(*runs):
        assert _bits_equal(a, b)


# ---- 4. where the gradients live ----

def test_stored_tensors_are_leaves_whose_gradients_share_the_flat_buffer():
    """As test_gradients_share_one_flat_buffer: the .grads of the STORED tensors are views of the one flat buffer, in the
    unchanged layout [means3D | opacities | scales | rotations | exposure | crf_table | shs | means2D]."""
    from casualhdrsplat_amd.distributed import _shared_flat
    P = 3000
    sc = S.make_scene(P, 128, 96, 3, seed=1, hdr=True)
    rs, expo, crf, leaf, rast = _raw_step(sc, _stored_of(sc, 1), dict(parameterization="raw"))
    out = rast(leaf[0], leaf[1], leaf[2], shs=leaf[3], scales=leaf[4], rotations=leaf[5])
    torch.autograd.backward(out[0], grad_tensors=sc.dL_dimage.to(DEV))
    assert all(t.is_leaf for t in leaf)
    grads = [t.grad for t in leaf + [expo, crf]]
    assert all(g is not None for g in grads)
    flat = _shared_flat(grads)
    assert flat is not None and flat.numel() >= sum(g.numel() for g in grads)
    store = leaf[0].grad.untyped_storage().data_ptr()
    assert all(g.untyped_storage().data_ptr() == store for g in grads)
    m3, m2, op, sh, scl, rot = (t.grad for t in leaf)
    order = [m3, op, scl, rot, expo.grad, crf.grad, sh, m2]
    offs = [(g.data_ptr() - m3.data_ptr()) // 4 for g in order]
    want, at = [], 0
    for g in order:
        want.append(at)
        at += (g.numel() + 3) // 4 * 4
    assert offs == want, (offs, want)
    before = leaf[5].grad.clone()
    flat.mul_(2.0)   # what an in-place all-reduce would do
    assert torch.equal(leaf[5].grad, 2 * before)


# ---- 5. chunks ----

def test_raw_backward_in_chunks_is_bit_identical_and_leaves_the_reduce_in_flight():
    """As test_backward_in_gaussian_chunks_is_bit_identical_to_the_whole_backward, with "raw": the conversion runs per chunk,
    on exactly the chunk's rows, and 1, 3 and 4 chunks give the whole backward's bits.  With leaf stored tensors the
    rasterizer's cell shows the collectives left pending (none were waited for in backward()); the same step with torch
    activations in front of a default rasterizer waits inside backward() -- what the feature removes."""
    from casualhdrsplat_amd import DensifyStats, GaussianRasterizer
    P = 5000
    sc = S.make_scene(P, 224, 144, 3, seed=17, hdr=True)
    cams = S.blur_poses(224, 144, 3, step=0.02)
    stored = _stored_of(sc, 17)
    res = []
    for chunks in (0, 1, 3, 4):
        rs, expo, crf = Hh.settings_from_scene(sc, DEV, cams, hdr=True, requires_grad=True)
        rs = rs._replace(viewmatrices=rs.viewmatrices.clone().requires_grad_(True),
                         projmatrices=rs.projmatrices.clone().requires_grad_(True),
                         camposes=rs.camposes.clone().requires_grad_(True))
        leaf = [t.detach().clone().to(DEV).requires_grad_(True) for t in (sc.means3D, torch.zeros_like(sc.means3D), stored[0],
                                                                            sc.shs, stored[1], stored[2])]
        dens = DensifyStats(P, DEV)
        rast = GaussianRasterizer(rs, densify_stats=dens, reduce_group=True if chunks else None, reduce_chunks=chunks,
                                  parameterization="raw")
        out = rast(leaf[0], leaf[1], leaf[2], shs=leaf[3], scales=leaf[4], rotations=leaf[5])
        (out[0] * sc.dL_dimage.to(DEV)).sum().backward()
        if chunks:
            assert "reduce_pending" in rast._cell and "reduce_waited_in_backward" not in rast._cell, rast._cell
        assert rast.finish_reduce() == 0   # one rank: nothing on the wire
        res.append([t.grad.clone() for t in leaf + [expo, crf, rs.viewmatrices, rs.projmatrices, rs.camposes]] +
                   [dens.grad_accum.clone(), dens.denom.clone(), dens.max_radii.clone()])
    assert float(res[0][2].abs().sum()) > 0 and float(res[0][5].abs().sum()) > 0 and float(res[0][8].abs().sum()) > 0
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert _bits_equal(a, b)
    # the usual wiring: torch activations between the leaves and a default rasterizer -- backward() waits
    rs, expo, crf = Hh.settings_from_scene(sc, DEV, cams, hdr=True, requires_grad=True)
    leaf = [t.detach().clone().to(DEV).requires_grad_(True) for t in (sc.means3D, torch.zeros_like(sc.means3D), stored[0],
                                                                        sc.shs, stored[1], stored[2])]
    rast = GaussianRasterizer(rs, reduce_group=True, reduce_chunks=3)
    out = rast(leaf[0], leaf[1], torch.sigmoid(leaf[2]), shs=leaf[3], scales=torch.exp(leaf[4]),
               rotations=torch.nn.functional.normalize(leaf[5]))
    (out[0] * sc.dL_dimage.to(DEV)).sum().backward()
    assert "reduce_waited_in_backward" in rast._cell
    assert not _shared_store(leaf[2].grad, leaf[0].grad)      # ... and its stored-space gradients are torch's own allocations


def _shared_store(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def test_raw_backward_through_the_gather_branch_is_bit_identical_to_the_whole_backward():
    """The third branch of the backward -- defer_sh_grad with gather_group (render + segmented sum, the view gather started,
    then HS_BWD_PROJECT) -- converts behind the project call: on one rank its stored-space gradients, every other gradient
    it writes and the deferred view colours are the bits of the same deferred backward run as one launch (whose conversion
    the two-call comparisons above hold to the chain rule)."""
    from casualhdrsplat_amd import GaussianRasterizer
    P = 4000
    sc = S.make_scene(P, 192, 128, 3, seed=23, hdr=True)
    stored = _stored_of(sc, 23)
    res = []
    for kw in (dict(defer_sh_grad=True), dict(defer_sh_grad=True, gather_group=True)):
        rs, expo, crf, leaf, rast = _raw_step(sc, stored, dict(parameterization="raw", **kw))
        out = rast(leaf[0], leaf[1], leaf[2], shs=leaf[3], scales=leaf[4], rotations=leaf[5])
        (out[0] * sc.dL_dimage.to(DEV)).sum().backward()
        assert leaf[3].grad is None and rast.deferred.get("view_colors") is not None      # the SH gradient is deferred
        res.append([t.grad.clone() for t in (leaf[0], leaf[1], leaf[2], leaf[4], leaf[5], expo, crf)] + [rast.deferred["view_colors"].clone()])
        assert all(_shared_store(t.grad, leaf[0].grad) for t in (leaf[2], leaf[4], leaf[5]))
    assert all(float(g.abs().sum()) > 0 for g in res[0])
    for a, b in zip(*res):
        assert _bits_equal(a, b)


# ---- 6. capture ----

def test_captured_raw_step_with_loss_and_adam_replays_the_eager_steps_bit_for_bit():
    """GraphedStep over forward ("raw") + photometric_loss + backward + GaussianAdam.enqueue(visibility=radii): two warm-up
    steps and five replays leave the parameters of seven eager steps, bit for bit."""
    from casualhdrsplat_amd import GaussianAdam, GaussianRasterizer, cloud_param_groups, photometric_loss
    from casualhdrsplat_amd.graphs import GraphedStep
    P, W, H = 4000, 160, 120
    sc = S.make_scene(P, W, H, 1, seed=4)
    stored = _stored_of(sc, 4)
    rs, _, _ = Hh.settings_from_scene(sc, DEV)
    with torch.no_grad():
        target = GaussianRasterizer(rs)(sc.means3D.to(DEV), torch.zeros(P, 3, device=DEV), sc.opacities.to(DEV), shs=sc.shs.to(DEV),
                                        scales=sc.scales.to(DEV), rotations=sc.rotations.to(DEV))[0].clone()

    def make():
        gen = torch.Generator().manual_seed(9)
        start = (sc.means3D, stored[0] + 0.3 * torch.randn(stored[0].shape, generator=gen), sc.shs * 0.8, stored[1] + 0.1, stored[2])
        leaf = [t.detach().clone().to(DEV).contiguous().requires_grad_(True) for t in start]
        opt = GaussianAdam(cloud_param_groups(*leaf, spatial_lr_scale=1.0), eps=1e-15)
        opt.prepare()
        rast = GaussianRasterizer(rs, capacity=60 * P, parameterization="raw")
        m2 = torch.zeros(P, 3, device=DEV, requires_grad=True)

        def fn():
            for t in leaf + [m2]:
                t.grad = None
            out = rast(leaf[0], m2, leaf[1], shs=leaf[2], scales=leaf[3], rotations=leaf[4])
            loss = photometric_loss(out[0], target, 0.2)
            loss.backward()
            opt.enqueue(visibility=out[1])
            return loss.detach()

        return leaf, opt, rast, fn

    leaf_e, opt_e, _, fn_e = make()
    losses = [float(fn_e()) for _ in range(7)]
    leaf_g, opt_g, rast_g, fn_g = make()
    step = GraphedStep(fn_g, [rast_g], warmup=2, params=leaf_g)
    for _ in range(5):
        step.step()
    step.check_overflow()
    torch.cuda.synchronize()
    assert opt_e._read_t() == 7 == opt_g._read_t()
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    for a, b in zip(leaf_e, leaf_g):
        assert _bits_equal(a.detach(), b.detach())
    assert not torch.equal(leaf_g[1].detach().cpu(), stored[0])
    assert all(_shared_store(g, step.grads[0]) for g in step.grads)      # the captured gradients: one flat buffer


# ---- 7. through a densification ----

def test_raw_steps_through_a_densification_accumulate_the_two_call_paths_statistics():
    """A few "raw" steps with DensifyStats, densify_and_prune, more steps: shapes follow P_out, every loss is finite, and on
    every step the statistics equal, bit for bit, those the two-call path accumulates on the same parameters (means2D's
    gradient is not touched by the conversion)."""
    from casualhdrsplat_amd import (DensifyStats, GaussianAdam, GaussianRasterizer, cloud_param_groups, densify_and_prune,
                                    inspect_state, photometric_loss)
    names = ("means3D", "opacities", "shs", "scales", "rotations")
    W, H = 160, 120
    sc = S.make_scene(4000, W, H, 1, seed=4)
    rs, _, _ = Hh.settings_from_scene(sc, DEV)
    stored = _stored_of(sc, 4)
    with torch.no_grad():
        target = GaussianRasterizer(rs)(sc.means3D.to(DEV), torch.zeros(4000, 3, device=DEV), sc.opacities.to(DEV), shs=sc.shs.to(DEV),
                                        scales=sc.scales.to(DEV), rotations=sc.rotations.to(DEV))[0].clone()
    sub = slice(0, None, 4)
    leaf = dict(zip(names, (sc.means3D[sub], stored[0][sub], sc.shs[sub], stored[1][sub], stored[2][sub])))
    leaf = {k: v.detach().clone().to(DEV).contiguous().requires_grad_(True) for k, v in leaf.items()}
    P0 = leaf["means3D"].shape[0]
    extent = float(sc.means3D.std(dim=0).norm())
    opt = GaussianAdam(cloud_param_groups(*[leaf[k] for k in names], spatial_lr_scale=extent), eps=1e-15)
    stats, twin = DensifyStats(P0, DEV), DensifyStats(P0, DEV)
    losses = []

    def train_step():
        rast = GaussianRasterizer(rs, densify_stats=stats, parameterization="raw")
        for v in leaf.values():
            v.grad = None
        m2 = torch.zeros_like(leaf["means3D"], requires_grad=True)
        o = rast(leaf["means3D"], m2, leaf["opacities"], shs=leaf["shs"], scales=leaf["scales"], rotations=leaf["rotations"])
        act = inspect_state(o[0])
        loss = photometric_loss(o[0], target, 0.2)
        loss.backward()
        # the two-call path on the same parameters: the default rasterizer on the activated tensors the library produced
        t = [leaf["means3D"].detach().clone().requires_grad_(True), torch.zeros_like(m2, requires_grad=True),
             act["opacities"].detach().clone().requires_grad_(True), leaf["shs"].detach().clone().requires_grad_(True),
             act["scales"].detach().clone().requires_grad_(True), act["rotations"].detach().clone().requires_grad_(True)]
        o2 = GaussianRasterizer(rs, densify_stats=twin)(t[0], t[1], t[2], shs=t[3], scales=t[4], rotations=t[5])
        photometric_loss(o2[0], target, 0.2).backward()
        assert _bits_equal(m2.grad, t[1].grad)
        for a, b in ((stats.grad_accum, twin.grad_accum), (stats.denom, twin.denom), (stats.max_radii, twin.max_radii)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        opt.step(visibility=o[1])
        losses.append(float(loss.detach()))

    for _ in range(6):
        train_step()
    seen = stats.denom > 0
    assert int(seen.sum()) > P0 // 4
    g_med = float(stats.mean_grad()[seen].median())
    s_med = float(torch.exp(leaf["scales"].detach()).max(dim=1).values.median())
    res = densify_and_prune(opt, stats, extent=extent, grad_threshold=g_med, percent_dense=s_med / extent, min_opacity=0.005,
                            generator=torch.Generator(device=DEV).manual_seed(1))
    leaf = dict(res.params)
    P1 = res.counts["P_out"]
    print(f"P {P0} -> {P1}: {res.counts}")
    assert P1 != P0 and all(leaf[k].shape[0] == P1 and leaf[k].is_leaf for k in names) and stats.denom.shape == (P1,)
    twin.resize(P1)
    for _ in range(6):
        train_step()
    print("losses:", " ".join(f"{v:.5f}" for v in losses))
    assert all(math.isfinite(v) for v in losses) and int((stats.denom > 0).sum()) > 0
    assert all(leaf[k].grad.shape == leaf[k].shape for k in names)


# ---- 8. the example ----

def test_training_example_raw_against_the_torch_wiring():
    """examples/train_synthetic.py, 60 steps at its test size, seeds 0, 1, 2, --fused-adam with and without --raw: each --raw
    run ends below its starting loss, and per seed its final PSNR differs from the torch wiring's by no more than the
    largest difference between two torch-wiring seeds (the wirings differ by expf rounding: less than a seed does)."""
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    runs = {}
    for seed in (0, 1, 2):
        for raw in (False, True):
            r = mod.run(P=5000, W=192, H=128, frames=3, virtual=4, steps=60, seed=seed, quiet=True, fused_adam=True, raw=raw)
            runs[seed, raw] = r
    torch_psnr = [runs[s, False]["last"]["psnr"] for s in (0, 1, 2)]
    spread = max(torch_psnr) - min(torch_psnr)
    for seed in (0, 1, 2):
        a, b = runs[seed, False]["last"]["psnr"], runs[seed, True]["last"]["psnr"]
        print(f"seed {seed}: final PSNR torch wiring {a:.4f} dB, raw {b:.4f} dB (difference {abs(a - b):.4f}; seed spread {spread:.4f})")
    for seed in (0, 1, 2):
        r = runs[seed, True]
        assert r["last"]["loss"] < r["first"]["loss"], (seed, r["first"], r["last"])
        assert all(math.isfinite(h["loss"]) for h in r["history"])
        assert abs(runs[seed, False]["last"]["psnr"] - r["last"]["psnr"]) <= spread, (seed, torch_psnr, r["last"]["psnr"])
