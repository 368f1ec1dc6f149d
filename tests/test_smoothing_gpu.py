"""GPU checks of the 3D smoothing filter (smoothing.hip; smoothing.py; GaussianRasterizer(..., filter_3D=...)): the filter and
the views against the numpy restatement of tests/smoothing_reference.py bit for bit, the activations with the filter and their
chain rule against float64 within that module's bars (and bit for bit given the device's own expf), the "raw" rasterizer with a
filter against the default rasterizer fed what hs_smoothing_apply wrote, the formation's filter, the training example and the
fused PLY."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import helpers as Hh
import poison
import smoothing_reference as R
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = -12345.5          # what rows beyond P hold before and after
IPATTERN = -77              # ... of n_views


def _np(t):
    return t.detach().cpu().numpy()


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the filter ----

@functools.lru_cache(maxsize=None)
def filter_scene(P, n_cams, looking_away=False):
    """(xyz [P, 3], views [C, 16], intrinsics [C, 4]) float32 on the host: a free camera (synthetic.random_camera) and
    C poses around it that rotate up to 20 degrees about every axis (synthetic.perturbed_poses), every camera with its own
    (fx, fy, W, H); points drawn in the first camera's frame from a region wider than its frustum and reaching behind it.
    looking_away: every point behind every camera."""
    W, H = 72, 40
    base = S.random_camera(W, H, seed=11 + n_cams)
    cams = S.perturbed_poses(base, n_cams, seed=n_cams, rot_step_deg=20.0 / max(n_cams, 1), step=0.5 / max(n_cams, 1))
    views = np.stack([c.viewmatrix.numpy().reshape(16) for c in cams]).astype(np.float32) if n_cams else np.zeros((0, 16), np.float32)
    k = np.arange(n_cams, dtype=np.float64)
    fx0 = W / (2 * base.tanfovx)
    intr = np.stack([fx0 * (1.0 + 0.3 * k / max(n_cams, 1)), fx0 * (1.1 - 0.2 * k / max(n_cams, 1)), W + k % 7, H + k % 5],
                    axis=1).astype(np.float32).reshape(n_cams, 4)
    rng = np.random.default_rng(1000 * P + n_cams)
    z = rng.uniform(-12.0, -1.0, P) if looking_away else rng.uniform(-2.0, 10.0, P)
    if P >= 3 and not looking_away:
        z[:3] = (5.0, -4.0, 0.1)                                   # in front, behind, inside the near plane
    v = np.stack([rng.uniform(-1.6, 1.6, P) * np.abs(z) * base.tanfovx, rng.uniform(-1.6, 1.6, P) * np.abs(z) * base.tanfovy, z], axis=1)
    if P >= 3 and not looking_away:
        v[0, :2] = 0.0                                             # on the first camera's axis: every camera sees it
    w2c = S.camera_w2c(base).numpy()
    xyz = ((v - w2c[:3, 3]) @ w2c[:3, :3]).astype(np.float32)      # x_w = R^T (x_v - t)
    return xyz, views, intr


def filter_run(xyz, views, intr, want_views=True, fill=None, offset=0):
    """hs_smoothing_filter through ctypes: outputs padded with a pattern that must stay, the workspace filled with 0xA5 (or
    the poison pattern `fill`) and followed by bytes that must stay.  Returns (filter [P], n_views [P] or None)."""
    from casualhdrsplat_amd import _lib as L
    lib = L.load()
    P, n_cams = xyz.shape[0], views.shape[0]
    nbytes = lib.hs_smoothing_filter_workspace_bytes(P)
    assert nbytes == (8 * min((P + 255) // 256, 2048) + 255) // 256 * 256
    ws = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    if fill is not None and nbytes:
        poison.fill_(ws[:nbytes], fill, seed=3)
    out = torch.full((P + 64 + offset,), PATTERN, dtype=torch.float32, device=DEV)
    nv = torch.full((P + 64 + offset,), IPATTERN, dtype=torch.int32, device=DEV)
    d_xyz = torch.from_numpy(xyz).to(DEV).contiguous()
    d_views = torch.from_numpy(views).to(DEV).contiguous()
    d_intr = torch.from_numpy(intr).to(DEV).contiguous()
    a = L.hs_smoothing_filter_args()
    a.P, a.C = P, n_cams
    a.xyz = d_xyz.data_ptr() if P else None
    a.viewmatrices, a.intrinsics = (d_views.data_ptr(), d_intr.data_ptr()) if n_cams else (None, None)
    a.filter, a.workspace = out[offset:].data_ptr(), ws.data_ptr()
    a.n_views = nv[offset:].data_ptr() if want_views else None
    L.check(lib.hs_smoothing_filter(C.byref(a), _stream()), "hs_smoothing_filter")
    torch.cuda.synchronize()
    assert (ws[nbytes:].cpu().numpy() == 0xA5).all(), "written behind the workspace"
    o, n = out.cpu().numpy(), nv.cpu().numpy()
    assert (o[:offset] == PATTERN).all() and (o[offset + P:] == PATTERN).all(), "filter written outside rows [0, P)"
    assert (n[:offset] == IPATTERN).all() and (n[offset + P:] == IPATTERN).all(), "n_views written outside rows [0, P)"
    if not want_views:
        assert (n == IPATTERN).all()
    if P == 0:
        assert (ws.cpu().numpy() == 0xA5).all(), "P == 0 launches nothing"
    return o[offset:offset + P].copy(), (n[offset:offset + P].copy() if want_views else None)


@pytest.mark.parametrize("n_cams", [1, 7, R.CAM_CHUNK + 1])
@pytest.mark.parametrize("P", [1, 255, 1000, 4097])
def test_filter_and_views_equal_the_restatement_bit_for_bit(P, n_cams):
    """Every P x C: filter and n_views equal the numpy restatement bit for bit (cameras that differ in pose and in all four
    intrinsics; C = 65 is one more than the kernel stages at a time), rows beyond P and bytes beyond the workspace stay, a
    second run and a run without n_views give the same bits, output pointers 4 bytes off a 16-byte boundary too.  Asserted
    on the host first: from P = 255 on each scene holds a Gaussian no camera sees and one every camera sees, and -- where
    there is more than one camera; with one the kind does not exist -- one that some cameras see."""
    xyz, views, intr = filter_scene(P, n_cams)
    want, n_want = R.filter_3d(xyz, views, intr)
    if P >= 255:
        kinds = [(n_want == 0).sum(), (n_want == n_cams).sum(), ((n_want > 0) & (n_want < n_cams)).sum()]
        print(f"P={P} C={n_cams}: seen by none / all / some = {kinds}")
        assert kinds[0] > 0 and kinds[1] > 0 and (kinds[2] > 0 or n_cams == 1), kinds
        assert n_want[0] == n_cams and n_want[1] == 0
    assert np.isfinite(want).all() and (want > 0).all() == bool((n_want > 0).any())
    got, n_got = filter_run(xyz, views, intr)
    assert np.array_equal(n_got, n_want)
    assert R.same_bits(got, want)
    again, _ = filter_run(xyz, views, intr, want_views=False, offset=1)
    assert R.same_bits(again, got)


def test_filter_cases_with_a_fixed_answer():
    """All cameras looking away: zeros and no views.  C == 0: zeros.  P == 0: nothing is launched (the workspace keeps its bytes)."""
    xyz, views, intr = filter_scene(1000, 7, looking_away=True)
    got, n = filter_run(xyz, views, intr)
    assert (n == 0).all() and R.same_bits(got, np.zeros(1000, np.float32)) and (R.filter_3d(xyz, views, intr)[0] == 0).all()
    got, n = filter_run(xyz, views[:0], intr[:0])
    assert (n == 0).all() and R.same_bits(got, np.zeros(1000, np.float32))
    got, n = filter_run(xyz[:0], views, intr)
    assert got.shape == (0,) and n.shape == (0,)
    # one Gaussian seen by one camera only: the others take its distance
    xyz, views, intr = filter_scene(255, 7)
    want, n_want = R.filter_3d(xyz[:3], views[:1], intr[:1])
    assert n_want.tolist() == [1, 0, 0] and want[1] == want[0] == want[2]
    got, n = filter_run(xyz[:3], views[:1], intr[:1])
    assert R.same_bits(got, want) and n.tolist() == [1, 0, 0]


def test_filter_does_not_depend_on_what_the_workspace_held():
    """Every workspace word is written before it is read: a workspace filled with each of tests/poison.py's patterns gives the
    bits of the 0xA5 one -- one workgroup's words (P = 255), several (4097), and the strided grid's 2048 (600 000)."""
    for P, n_cams in ((255, 7), (4097, R.CAM_CHUNK + 1), (600_000, 3)):
        xyz, views, intr = filter_scene(P, n_cams)
        want, n_want = filter_run(xyz, views, intr)
        if P > 524288:                       # more rows than 2048 workgroups hold: the restatement once, here
            ref, n_ref = R.filter_3d(xyz, views, intr)
            assert R.same_bits(want, ref) and np.array_equal(n_want, n_ref)
        for pattern in tuple(poison.FIXED) + ("random",):
            got, n_got = filter_run(xyz, views, intr, fill=pattern)
            assert R.same_bits(got, want) and np.array_equal(n_got, n_want), (P, pattern)


def test_compute_filter_3d_python(monkeypatch):
    """The Python front end: [C, 4, 4] and [F, N, 4, 4] cameras, scalar and per-camera intrinsics (lists and tensors), the
    views on request, an empty cloud -- equal to the restatement bit for bit, with its scratch poisoned."""
    from casualhdrsplat_amd import compute_filter_3D
    xyz, views, intr = filter_scene(1000, 6)
    want, n_want = R.filter_3d(xyz, views, intr)
    d_xyz, d_views = torch.from_numpy(xyz).to(DEV), torch.from_numpy(views).to(DEV)
    with poison.poisoned(monkeypatch, "nan") as session:
        f, n = compute_filter_3D(d_xyz, d_views.reshape(6, 4, 4), intr[:, 0].tolist(), torch.from_numpy(intr[:, 1]),
                                 torch.from_numpy(intr[:, 2]).to(DEV), intr[:, 3].tolist(), return_views=True)
        torch.cuda.synchronize()
    session.require("casualhdrsplat_amd.smoothing", at_least=3)
    assert f.dtype == torch.float32 and f.shape == (1000,) and n.dtype == torch.int32 and not f.requires_grad
    assert R.same_bits(_np(f), want) and np.array_equal(_np(n), n_want)
    # scalars, frames of poses
    same = np.tile(np.array([[40.0, 41.0, 72.0, 40.0]], np.float32), (6, 1))
    f2 = compute_filter_3D(d_xyz.requires_grad_(True), d_views.reshape(2, 3, 4, 4), 40.0, 41.0, 72, 40)
    assert isinstance(f2, torch.Tensor) and not f2.requires_grad and R.same_bits(_np(f2), R.filter_3d(xyz, views, same)[0])
    assert compute_filter_3D(d_xyz[:0].detach(), d_views, 40.0, 41.0, 72, 40).shape == (0,)
    z = compute_filter_3D(d_xyz.detach(), d_views[:0].reshape(0, 4, 4), 40.0, 41.0, 72, 40)
    assert z.shape == (1000,) and not bool(z.any())


# ---- 2. applying it ----

ROWS = 4099


@functools.lru_cache(maxsize=None)
def apply_case():
    """4099 rows: the measurement's distributions with the special logits, f = 0 rows (every 16th, and some more), a row
    whose three v are zero (l = -inf, f = 0), one with a single zero v, one with s = 0 under a filter."""
    x, l, f, g_o, g_s = R.inputs(ROWS - len(R.SPECIAL_LOGITS), seed=7)
    assert x.shape == (ROWS,) and (x[-9:] == np.array(R.SPECIAL_LOGITS, np.float32)).all()
    f[-9:-5] = 0.0
    l[5], f[5] = -np.inf, 0.0
    l[6, 1], f[6] = -np.inf, 0.0
    l[7, 2] = -np.inf
    assert f[0] == 0 and f[16] == 0 and f[7] > 0
    return x, l, f, g_o, g_s


def _device_activations(x, l):
    """(o, s) as hs_activate computes them on the device: the expf the smoothing kernels share."""
    from casualhdrsplat_amd import _lib as L
    dx, dl = torch.from_numpy(x).to(DEV), torch.from_numpy(l).to(DEV).contiguous()
    o, s = torch.empty_like(dx), torch.empty_like(dl)
    a = L.hs_activate_args()
    a.P = x.shape[0]
    a.opacity_raw, a.scales_raw, a.opacities, a.scales = dx.data_ptr(), dl.data_ptr(), o.data_ptr(), s.data_ptr()
    L.check(L.load().hs_activate(C.byref(a), _stream()), "hs_activate")
    torch.cuda.synchronize()
    return _np(o), _np(s)


def _carve(arr, offset):
    """`arr` inside a larger PATTERN-filled device buffer, `offset` floats behind a 16-byte aligned address."""
    n = arr.size
    full = torch.full((n + 64,), PATTERN, dtype=torch.float32, device=DEV)
    assert full.data_ptr() % 16 == 0
    view = full[16 + offset:16 + offset + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)))
    return full, view


def _untouched(full, offset, n):
    a = 16 + offset
    return bool((full[:a] == PATTERN).all()) and bool((full[a + n:] == PATTERN).all())


def apply_run(offset, chunks=None, backward=True):
    """hs_smoothing_apply and, over `chunks` of rows (default: one call over all), hs_smoothing_apply_backward on apply_case();
    every array carved `offset` floats off a 16-byte boundary.  Returns (o', s', d_o, d_s) as numpy."""
    from casualhdrsplat_amd import _lib as L
    lib = L.load()
    x, l, f, g_o, g_s = apply_case()
    ins = [_carve(t, offset) for t in (x, l, f)]
    outs = [_carve(np.full(t.shape, PATTERN, np.float32), offset) for t in (x, l)]
    a = L.hs_smoothing_apply_args()
    a.P = ROWS
    a.opacity_raw, a.scales_raw, a.filter = (v.data_ptr() for _, v in ins)
    a.opacities, a.scales = (v.data_ptr() for _, v in outs)
    L.check(lib.hs_smoothing_apply(C.byref(a), _stream()), "hs_smoothing_apply")
    torch.cuda.synchronize()
    for (full, v), t in zip(ins, (x, l, f)):
        assert _untouched(full, offset, t.size) and poison.bytes_of(v) == t.tobytes(), "the stored values are read only"
    for (full, _), t in zip(outs, (x, l)):
        assert _untouched(full, offset, t.size)
    res = [_np(outs[0][1]).copy(), _np(outs[1][1]).reshape(ROWS, 3).copy()]
    if not backward:
        return res
    grads = [_carve(t, offset) for t in (g_o, g_s)]
    a.opacities, a.scales = None, None                                    # (the backward reads neither)
    a.dL_dopacities, a.dL_dscales = (v.data_ptr() for _, v in grads)
    done = np.zeros(ROWS, bool)
    for g0, g1 in (chunks or [(0, ROWS)]):
        a.g_begin, a.g_end = g0, g1
        L.check(lib.hs_smoothing_apply_backward(C.byref(a), _stream()), "hs_smoothing_apply_backward")
        torch.cuda.synchronize()
        done[g0:g1] = True
        d_o, d_s = _np(grads[0][1]), _np(grads[1][1]).reshape(ROWS, 3)
        assert R.same_bits(d_o[~done], g_o[~done]) and R.same_bits(d_s[~done], g_s[~done]), "rows outside the range were written"
    for (full, _), t in zip(grads, (g_o, g_s)):
        assert _untouched(full, offset, t.size)
    return res + [_np(grads[0][1]).copy(), _np(grads[1][1]).reshape(ROWS, 3).copy()]


def _within_bars(c, what):
    for k, v in c.items():
        print(f"{what}: {k} c = {v:.4f} (bar {R.BARS[k]})")
    for k, v in c.items():
        assert v <= R.BARS[k], (what, k, v)


def test_apply_forward_and_backward_against_float64_and_the_restatement():
    """4099 rows with the special logits, f = 0 rows and v = 0 rows: s', o' and the two gradients within the bars of float64;
    given the device's own sigmoid and exp (hs_activate's: the same expf) every value equals the restatement bit for bit; the
    special rows are what the rules say; nothing outside the arrays is written."""
    x, l, f, g_o, g_s = apply_case()
    oc, sp, d_o, d_s = apply_run(0)
    assert all(np.isfinite(t).all() for t in (oc, sp, d_o, d_s))
    _within_bars(R.forward_constants(x, l, f, oc, sp), "forward")
    o_dev, s_dev = _device_activations(x, l)
    fwd = R.apply(x, l, f, o=o_dev, s=s_dev)
    assert R.same_bits(oc, fwd["oc"]) and R.same_bits(sp, fwd["sp"])
    want = R.backward(g_o, g_s, fwd)
    assert R.same_bits(d_o, want[0]) and R.same_bits(d_s, want[1])
    _within_bars(R.backward_constants(g_o, g_s, fwd, d_o, d_s), "backward")
    # f = 0 rows: hs_activate's values and hs_activate_backward's gradients, bit for bit
    z = f == 0
    z[5:8] = False                                                        # (the rows with l = -inf are looked at below)
    assert z.sum() > 250 and R.same_bits(sp[z], s_dev[z]) and R.same_bits(oc[z], o_dev[z])
    assert R.same_bits(d_s[z], g_s[z] * s_dev[z]) and R.same_bits(d_o[z], (g_o[z] * o_dev[z]) * (np.float32(1) - o_dev[z]))
    # v = 0: r = 1, t = 0 -- the opacity passes, the scale is 0 and its gradient 0 (not NaN)
    assert (sp[5] == 0).all() and oc[5] == o_dev[5] and (d_s[5] == 0).all()
    assert sp[6, 1] == 0 and oc[6] == o_dev[6] and d_s[6, 1] == 0
    assert sp[7, 2] == f[7] and oc[7] == 0 and d_o[7] == 0               # s = 0 under a filter: the filter's ball, no opacity
    assert oc[-3] == fwd["c"][-3] and oc[-2] == 0.0                       # x = 100, -100


def test_apply_pointers_four_bytes_off_give_the_same_values():
    a, b = apply_run(0), apply_run(1)
    for u, v in zip(a, b):
        assert R.same_bits(u, v)
    for off in (2, 3):
        for u, v in zip(a[:2], apply_run(off, backward=False)):
            assert R.same_bits(u, v)


def test_apply_backward_in_chunks_equals_one_call():
    """[0, 1000), [1000, 1001), [1001, 4099) -- a chunk that ends on a group of four rows, one row alone, a chunk that starts
    inside a group -- equal one call bit for bit, on 16-byte and on 4-byte aligned arrays; rows outside a call's range keep
    their bits (apply_run asserts it after every call)."""
    chunks = [(0, 1000), (1000, 1001), (1001, ROWS)]
    for offset in (0, 1):
        whole, parts = apply_run(offset), apply_run(offset, chunks=chunks)
        for u, v in zip(whole, parts):
            assert R.same_bits(u, v)
    rev = apply_run(0, chunks=chunks[::-1] + [(37, 37)])                # any order; an empty range is a no-op
    for u, v in zip(apply_run(0), rev):
        assert R.same_bits(u, v)


# ---- 3. the rasterizer ----

@functools.lru_cache(maxsize=None)
def raster_case():
    """2000 Gaussians, 72 x 40, SH 1, HDR, two poses: the "raw" rasterizer with a filter, the default one fed what
    hs_smoothing_apply wrote, the "raw" one with a filter of zeros and the "raw" one without."""
    from casualhdrsplat_amd import GaussianRasterizer, apply_filter_3D, compute_filter_3D, inspect_state
    P, W, H = 2000, 72, 40
    base = S.random_camera(W, H, 5)
    sc = S.make_scene(P, W, H, 1, seed=31, hdr=True, place_in=base)
    cams = S.perturbed_poses(base, 2, seed=1, rot_step_deg=1.0, step=0.02)
    gen = torch.Generator().manual_seed(9)
    x = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))
    x[0], x[1] = 30.0, -30.0
    l = torch.log(sc.scales)
    q = sc.rotations * torch.exp(torch.empty(P, 1).uniform_(-2.0, 2.0, generator=gen))
    views = torch.stack([c.viewmatrix for c in cams]).to(DEV)
    filt = compute_filter_3D(sc.means3D.to(DEV), views, W / (2 * base.tanfovx), H / (2 * base.tanfovy), W, H)
    filt[::10] = 0.0
    dL_hdr = torch.randn(3, H, W, generator=gen).to(DEV)
    stored = dict(opacities=x, scales=l, rotations=q)

    def run(how, params, filter_3D=None):
        rs, expo, crf = Hh.settings_from_scene(sc, DEV, cams, hdr=True, requires_grad=True)
        leaf = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), shs=sc.shs, **params)
        leaf = {k: v.detach().clone().to(DEV).requires_grad_(True) for k, v in leaf.items()}
        rast = GaussianRasterizer(rs, parameterization=how, filter_3D=filter_3D)
        args = dict(leaf)
        out = rast(args.pop("means3D"), args.pop("means2D"), args.pop("opacities"), **args)
        kept = inspect_state(out[0])
        kept = {k: kept[k].detach().clone() for k in ("opacities", "scales", "rotations")}
        ((out[0] * sc.dL_dimage.to(DEV)).sum() + (out[2] * dL_hdr).sum()).backward()
        torch.cuda.synchronize()
        grads = {k: v.grad.detach().clone() for k, v in dict(leaf, exposure=expo, crf_table=crf).items()}
        return dict(out=[o.detach().clone() for o in out], grads=grads, kept=kept)

    res = dict(filtered=run("raw", stored, filt))
    op, scl = apply_filter_3D(x.to(DEV), l.to(DEV), filt)
    res["applied"] = (op, scl)
    res["two"] = run("activated", dict(opacities=op, scales=scl, rotations=res["filtered"]["kept"]["rotations"]))
    res["zeros"] = run("raw", stored, torch.zeros(P, 1, device=DEV))
    res["plain"] = run("raw", stored)
    res["stored"], res["filter"] = (x, l, q), filt
    return res


def test_rasterizer_with_a_filter_equals_the_two_call_path_bit_for_bit():
    """Images (LDR and HDR) and radii of the "raw" rasterizer with filter_3D are bit-identical to the default rasterizer's on
    the tensors hs_smoothing_apply wrote; the tensors its pipeline ran on ARE those; s' and o' are within the bars."""
    r = raster_case()
    a, b = r["filtered"], r["two"]
    assert len(a["out"]) == len(b["out"]) == 3
    for u, v in zip(a["out"], b["out"]):
        assert _bits_equal(u, v)
    assert float(a["out"][0].abs().sum()) > 0 and int((a["out"][1] > 0).sum()) > 500
    op, scl = r["applied"]
    assert _bits_equal(a["kept"]["opacities"], op) and _bits_equal(a["kept"]["scales"], scl)
    x, l, _ = r["stored"]
    _within_bars(R.forward_constants(_np(x), _np(l), _np(r["filter"]), _np(op), _np(scl)), "rasterizer forward")
    # the filter changed what was rendered, and only through those two tensors
    assert not _bits_equal(a["out"][0], r["plain"]["out"][0])
    assert _bits_equal(a["kept"]["rotations"], r["plain"]["kept"]["rotations"])


def test_rasterizer_gradients_are_the_two_call_gradients_pushed_through_the_chain_rule():
    """The stored-tensor gradients equal, bit for bit, the default rasterizer's gradients pushed through
    hs_smoothing_apply_backward (and the rotations' through hs_activate_backward), and lie within the bars of the float64
    chain rule applied to those activated-space gradients; every other gradient is bit-identical."""
    from casualhdrsplat_amd import _lib as L
    r = raster_case()
    gr, gt = r["filtered"]["grads"], r["two"]["grads"]
    assert set(gr) == set(gt) and float(gr["means3D"].abs().sum()) > 0
    for k in gr:
        if k not in ("opacities", "scales", "rotations"):
            assert _bits_equal(gr[k], gt[k]), k
    x, l, q = (t.to(DEV).contiguous() for t in r["stored"])
    g_o, g_s, g_q = (gt[k].clone() for k in ("opacities", "scales", "rotations"))
    P = x.shape[0]
    a = L.hs_smoothing_apply_args()
    a.P, a.g_begin, a.g_end = P, 0, P
    a.opacity_raw, a.scales_raw, a.filter = x.data_ptr(), l.data_ptr(), r["filter"].data_ptr()
    a.dL_dopacities, a.dL_dscales = g_o.data_ptr(), g_s.data_ptr()
    L.check(L.load().hs_smoothing_apply_backward(C.byref(a), _stream()), "hs_smoothing_apply_backward")
    b = L.hs_activate_args()
    b.P, b.g_begin, b.g_end = P, 0, P
    b.rotations_raw, b.rotations, b.dL_drotations = q.data_ptr(), r["two"]["kept"]["rotations"].data_ptr(), g_q.data_ptr()
    L.check(L.load().hs_activate_backward(C.byref(b), _stream()), "hs_activate_backward")
    torch.cuda.synchronize()
    assert _bits_equal(gr["opacities"], g_o) and _bits_equal(gr["scales"], g_s) and _bits_equal(gr["rotations"], g_q)
    assert float(g_o.abs().sum()) > 0 and float(g_s.abs().sum()) > 0 and bool(torch.isfinite(g_s).all())
    xs, ls = _np(r["stored"][0]).reshape(-1), _np(r["stored"][1])
    o_dev, s_dev = _device_activations(xs, ls)
    fwd = R.apply(xs, ls, _np(r["filter"]), o=o_dev, s=s_dev)
    assert R.same_bits(fwd["oc"], _np(r["applied"][0]).reshape(-1))      # the forward values the bars start from are the device's
    _within_bars(R.backward_constants(_np(gt["opacities"]), _np(gt["scales"]), fwd, _np(gr["opacities"]), _np(gr["scales"])),
                 "rasterizer backward")


def test_a_filter_of_zeros_is_the_rasterizer_without_a_filter_bit_for_bit():
    r = raster_case()
    a, b = r["zeros"], r["plain"]
    for u, v in zip(a["out"], b["out"]):
        assert _bits_equal(u, v)
    assert set(a["grads"]) == set(b["grads"])
    for k in a["grads"]:
        assert _bits_equal(a["grads"][k], b["grads"][k]), k
    for k in a["kept"]:
        assert _bits_equal(a["kept"][k], b["kept"][k]), k


def test_rasterizer_filter_errors_on_the_device():
    from casualhdrsplat_amd import GaussianRasterizer
    P, W, H = 100, 40, 24
    sc = S.make_scene(P, W, H, 1, seed=3)
    rs, _, _ = Hh.settings_from_scene(sc, DEV)
    t = dict(means3D=sc.means3D, opacities=torch.logit(sc.opacities.clamp(1e-3, 1 - 1e-3)), shs=sc.shs, scales=sc.scales.log(),
             rotations=sc.rotations)
    t = {k: v.to(DEV) for k, v in t.items()}
    good = torch.full((P,), 0.01, device=DEV)

    def call(rast, **kw):
        return rast(t["means3D"], torch.zeros_like(t["means3D"]), t["opacities"], shs=t["shs"],
                    **(kw or dict(scales=t["scales"], rotations=t["rotations"])))

    with pytest.raises(ValueError, match="needs parameterization='raw'"):
        GaussianRasterizer(rs, filter_3D=good)
    rast = GaussianRasterizer(rs)
    rast.filter_3D = good
    with pytest.raises(ValueError, match="needs parameterization='raw'"):
        call(rast)
    rast = GaussianRasterizer(rs, parameterization="raw", filter_3D=good)
    with pytest.raises(ValueError, match="cannot be combined with cov3D_precomp"):
        call(rast, cov3D_precomp=torch.zeros(P, 6, device=DEV))
    for f, text in ((good.cpu(), "lives on cpu"), (good[:-1], "must have shape"), (good.double(), "must be float32"),
                    (torch.stack([good, good], 1)[:, 0], "must be contiguous"), (good.clone().requires_grad_(True), "must not require grad")):
        rast.filter_3D = f
        with pytest.raises(ValueError, match=text):
            call(rast)
    rast.filter_3D = good.reshape(P, 1)              # swapped back: the call works, [P, 1] as well as [P]
    out = call(rast)
    rast.filter_3D = good
    assert _bits_equal(out[0], call(rast)[0])
    rast.filter_3D = None                            # and without one it is the plain "raw" rasterizer
    assert _bits_equal(call(rast)[0], call(GaussianRasterizer(rs, parameterization="raw"))[0])


# ---- 4. formation, example, PLY ----

def test_formation_filter_equals_the_restatement_on_its_own_cameras():
    from casualhdrsplat_amd.image_formation import HDRBlurFormation, ImplicitCRF, TrajectorySpline, knots_from_lookat
    W, H, frames, virtual, P = 96, 64, 3, 4, 1500
    sc = S.make_scene(P, W, H, 1, seed=4, hdr=True)
    cam = sc.camera
    model = HDRBlurFormation(TrajectorySpline(knots_from_lookat(frames + 3, radius=0.25), kind="cubic"), frames, W, H, cam.tanfovx,
                             cam.tanfovy, n_virtual=virtual, crf=ImplicitCRF(K=32), sh_degree=1, window_scale=0.6).to(DEV)
    means = sc.means3D.to(DEV).requires_grad_(True)
    f, n = model.compute_filter_3D(means, return_views=True)
    views = _np(model.cameras_all()[0]).reshape(frames * virtual, 16)
    intr = np.tile(np.array([[W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy), W, H]], np.float32), (frames * virtual, 1))
    want, n_want = R.filter_3d(_np(means), views, intr)
    assert f.shape == (P,) and not f.requires_grad and R.same_bits(_np(f), want) and np.array_equal(_np(n), n_want)
    assert (n_want == frames * virtual).sum() > P // 2 and (want > 0).all()


def _example():
    spec = importlib.util.spec_from_file_location("train_synthetic_smoothing", os.path.join(ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_training_example_with_the_filter():
    """examples/train_synthetic.py --mcmc --filter-3d at the size the --mcmc test uses: finite everywhere, the last loss below
    the first, the filter's length equal to P in every history entry -- through both grows -- and the filter positive."""
    r = _example().run(P=3000, W=96, H=64, frames=2, virtual=3, steps=80, mcmc=True, filter_3d=True, quiet=True)
    hist, f, l = r["history"], r["first"], r["last"]
    print(f"loss {f['loss']:.5f} -> {l['loss']:.5f}, PSNR {f['psnr']:.3f} -> {l['psnr']:.3f} dB, P {f['P']} -> {l['P']}")
    assert len(hist) == 81
    for h in hist:
        assert all(np.isfinite(float(v)) for v in h.values()), h
        assert h["filter_len"] == h["P"], h
    sizes = [h["P"] for h in hist]
    assert sizes[0] == 750 and sizes[-1] == 3000 and len(set(sizes)) >= 3, sorted(set(sizes))
    for k, v in r["cloud"].items():
        assert bool(torch.isfinite(v).all()) and v.shape[0] == 3000, k
    filt = r["filter_3D"]
    assert filt.shape == (3000,) and bool(torch.isfinite(filt).all()) and bool((filt > 0).all())
    assert l["loss"] < f["loss"], (f, l)


def test_fused_ply_round_trip(tmp_path):
    """save_ply(..., filter_3D=f) stores s' and o' in stored form: reading it back gives log s' and logit o'."""
    from casualhdrsplat_amd import apply_filter_3D, scene_io
    P = 500
    rng = np.random.default_rng(3)
    cloud = scene_io.init_from_points(rng.standard_normal((P, 3)), np.full((P, 3), 0.5), sh_degree=1)
    filt = torch.from_numpy(np.exp(rng.uniform(-6, -1, P)).astype(np.float32)).to(DEV)
    filt[::5] = 0.0
    path = str(tmp_path / "fused.ply")
    scene_io.save_ply(path, cloud, filter_3D=filt)
    back = scene_io.load_ply(path)
    op, scl = apply_filter_3D(cloud.opacity_logit.to(DEV).contiguous(), cloud.log_scales.to(DEV).contiguous(), filt)
    assert torch.allclose(back.log_scales.exp(), scl.cpu(), rtol=1e-6) and torch.allclose(torch.sigmoid(back.opacity_logit), op.cpu(), rtol=1e-5)
    zero = (filt == 0).cpu()
    assert torch.allclose(back.log_scales[zero], cloud.log_scales[zero], atol=1e-6)          # unfiltered rows: what was stored
    assert bool((back.log_scales[~zero] >= cloud.log_scales[~zero]).all()) and bool((back.opacity_logit[~zero] < cloud.opacity_logit[~zero]).all())
    assert torch.equal(back.means3D, cloud.means3D) and torch.equal(back.rotations, cloud.rotations) and torch.equal(back.shs, cloud.shs)
