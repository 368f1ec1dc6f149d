"""CPU checks of the depth-distortion loss (distort.hip: hs_distortion_workspace_bytes, hs_distortion, hs_distortion_backward;
distortion.distortion_loss): the C ABI (exports, struct layout, workspace arithmetic, argument validation before any HIP
call), the Python refusals, and the TRUTH the GPU tests compare with (tests/distortion_reference.py) against what follows
from the definition -- closed forms, the pairwise double sum, the shift invariance, float64 autograd of the whole loss and a
finite difference -- and its float32 mode against the bound the GPU tests hold the kernels to, on the same scenes
(`case`, shared with tests/test_distortion_gpu.py)."""
import copy
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import distortion_reference as DR
import helpers as Hh
from casualhdrsplat_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_distortion_workspace_bytes", "hs_distortion", "hs_distortion_backward")
FWD_ARGS, BWD_ARGS = "hs_distortion_args", "hs_distortion_bwd_args"
STATE = ("geom", "binning", "image")
FWD_OUT = ("out_distortion", "out_moment")
WORKSPACES = STATE + ("ws",)
ARRAYS = ("viewmatrices", "projmatrices", "camposes", "means3D", "opacities", "scales", "rotations", "moment",
          "dL_ddistortion", "dL_dmeans3D", "dL_dopacities", "dL_dscales", "dL_drotations")


# ---- the scenes of the GPU tests: name -> (scene, cameras), built once per session ----

GUARDED = {"a": (1000, 128, 128, 3), "b": (600, 104, 72, 1)}
LONG = {"deep": (6000, 64, 64, 0), "rows": (3000, 48, 40, 1)}
POSED = (500, 72, 56, 1, 394)      # test_features_geometry_gpu.py's: the first seed whose four poses are outside the guard band
AA = (600, 104, 72, 1, 16)         # ... whose ANTIALIASED frame is
PLANE = (300, 72, 56, 1, 7, 4.0)   # (P, W, H, SH degree, seed, the view-space depth every Gaussian is moved to)
_CASES = {}


def on_one_plane(sc, z0):
    """every mean moved along the camera's viewing axis onto the view-space depth z0"""
    sc = copy.copy(sc)
    V = sc.camera.viewmatrix.double()
    m = sc.means3D.double()
    pvz = m[:, 0] * V[0, 2] + m[:, 1] * V[1, 2] + m[:, 2] * V[2, 2] + V[3, 2]
    sc.means3D = (m + (z0 - pvz)[:, None] * V[:3, 2][None, :]).float()
    return sc


def case(O, name):
    """dict(sc, cams, fwds: the oracle's forward per pose, gammas [n_poses, H, W] ~ N(0, 1))"""
    if name in _CASES:
        return _CASES[name]
    cams = None
    if name in GUARDED:
        P, W, H, deg = GUARDED[name]
        sc, _ = Hh.guarded_scene(O, P, W, H, deg)
    elif name in LONG:
        P, W, H, deg = LONG[name]
        sc = S.make_scene(P, W, H, deg, seed=0)
    elif name == "posed":
        P, W, H, deg, seed0 = POSED
        poses = lambda w, h: S.blur_poses(w, h, 4, step=0.03)
        sc, seed = Hh.guarded_scene(O, P, W, H, deg, seed=seed0, cams_fn=poses)
        assert seed == seed0
        cams = poses(W, H)
    elif name == "aa":
        P, W, H, deg, seed = AA
        sc = S.make_scene(P, W, H, deg, seed=seed)
        sc.antialias = True
    elif name == "plane":
        P, W, H, deg, seed, z0 = PLANE
        sc = on_one_plane(S.make_scene(P, W, H, deg, seed=seed), z0)
    else:
        raise KeyError(name)
    cams = cams or [sc.camera]
    fwds = [Hh.run_oracle(O, sc, cam=c, backward=False)[0] for c in cams]
    seed = 60 + sorted(list(GUARDED) + list(LONG) + ["posed", "aa", "plane"]).index(name)
    gammas = np.random.default_rng(seed).standard_normal((len(cams), H, W)).astype(np.float32)
    _CASES[name] = dict(sc=sc, cams=cams, fwds=fwds, gammas=gammas, W=W, H=H)
    return _CASES[name]


def needed(got, ref, S_):
    """the largest constant any element needs in |got - ref| <= 1e-4 |ref| + C 2^-24 S"""
    got, ref, S_ = (np.asarray(x, np.float64) for x in (got, ref, S_))
    excess = np.abs(got - ref) - 1e-4 * np.abs(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(excess > 0, excess / (2.0 ** -24 * S_), 0.0)
    need = np.where(np.isfinite(need), need, np.where(excess > 0, np.inf, 0.0))
    return float(need.max()) if need.size else 0.0


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- C ABI ----

def test_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    assert FWD_ARGS in header and BWD_ARGS in header and set(NAMES) <= set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == lib.HS_VERSION == 309       # (detected by name: the version does not move)
    import casualhdrsplat_amd as pkg
    assert "distortion_loss" in pkg.__all__ and callable(pkg.distortion_loss)


@pytest.mark.parametrize("name,must", ((FWD_ARGS, STATE + FWD_OUT), (BWD_ARGS, WORKSPACES + ARRAYS)))
def test_structs_match_c(lib, tmp_path, name, must):
    S_ = getattr(lib, name)
    fields = [n for n, _ in S_._fields_]
    assert set(must) <= set(fields)
    lines = [f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {n}));' for n in fields]
    want = [C.sizeof(S_)] + [getattr(S_, n).offset for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want


def _dims(lib, P=1000, W=128, H=128, n_poses=1, capacity=10000, n_frames=0):
    return lib.hs_dims(P, 16, 3, W, H, n_poses, capacity, 0, n_frames)


def test_workspace_bytes_follows_the_stated_formula(lib):
    L = lib.load()
    fn = L.hs_distortion_workspace_bytes
    a256 = lambda n: (n + 255) // 256 * 256
    last = 0
    for cap in (0, 1, 15, 16, 17, 1000, 10 ** 5, 10 ** 7, (1 << 30) - 1):
        b = fn(C.byref(_dims(lib, capacity=cap, n_poses=3)))
        assert b > 0 and b % 256 == 0 and b >= last and b == a256(64 * cap) + a256(64 * 1000 * 3) + a256(cap), (cap, b)
        last = b
    last = 0
    for P, n_poses in ((0, 1), (1, 1), (3, 1), (2, 2), (1000, 1), (1000, 2), (999, 3), (10 ** 6, 1), (10 ** 6, 4)):
        b = fn(C.byref(_dims(lib, P=P, n_poses=n_poses)))
        assert b == a256(64 * 10000) + a256(64 * P * n_poses) + a256(10000) and b >= last, (P, n_poses, b)
        last = b
    assert fn(C.byref(_dims(lib, P=0, capacity=0))) == 256
    assert fn(None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    for bad in (dict(P=-1), dict(W=0), dict(n_poses=0), dict(capacity=-1), dict(capacity=1 << 30), dict(n_poses=3, n_frames=2)):
        assert fn(C.byref(_dims(lib, **bad))) == lib.HS_EINVAL, bad
        assert L.hs_last_error().startswith(b"hs_plan:"), bad


def test_the_calls_validate_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the field -- on a machine without a GPU: no HIP call is
    made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy address: validation must fail before it is dereferenced

    def call(which, struct, names, dims=None, **kw):
        a = getattr(lib, struct)()
        a.dims = dims if dims is not None else _dims(lib)
        for k in names:
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, which)(C.byref(a), None), L.hs_last_error()

    bad_dims = (dict(P=-1), dict(H=0), dict(n_poses=0), dict(capacity=1 << 30), dict(n_poses=4, n_frames=3), dict(n_frames=-1))
    # ---- the forward ----
    which = "hs_distortion"
    fwd = lambda **kw: call(which, FWD_ARGS, STATE + FWD_OUT, **kw)
    assert getattr(L, which)(None, None) == lib.HS_EINVAL and L.hs_last_error() == which.encode() + b": null args"
    rows = [(dict(**{k: None}), b"null " + k.encode()) for k in STATE + FWD_OUT]
    rows += [(dict(**{k: one + 128}), k.encode() + b" must be 256-byte aligned") for k in STATE]
    rows += [(dict(**{k: one + 2}), k.encode() + b" must be 4-byte aligned") for k in FWD_OUT]
    for kw, text in rows:
        rc, msg = fwd(**kw)
        assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and text in msg, (kw, rc, msg)
    for bad in bad_dims:
        rc, msg = fwd(dims=_dims(lib, **bad))
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_plan:"), (bad, rc, msg)
    # an empty cloud still has two planes to fill: their pointers are checked, the state's are not looked at
    rc, msg = fwd(dims=_dims(lib, P=0), out_moment=None, **{k: None for k in STATE})
    assert rc == lib.HS_EINVAL and b"null out_moment" in msg
    # ---- the backward ----
    which = "hs_distortion_backward"
    bwd = lambda **kw: call(which, BWD_ARGS, WORKSPACES + ARRAYS, **kw)
    assert getattr(L, which)(None, None) == lib.HS_EINVAL and L.hs_last_error() == which.encode() + b": null args"
    rows = [(dict(**{k: None}), b"null " + k.encode()) for k in WORKSPACES + ARRAYS]
    rows += [(dict(**{k: one + 128}), k.encode() + b" must be 256-byte aligned") for k in WORKSPACES]
    rows += [(dict(**{k: one + 2}), k.encode() + b" must be 4-byte aligned") for k in ARRAYS if k not in ("rotations", "dL_drotations")]
    rows += [(dict(**{k: one + 4}), k.encode() + b" must be 16-byte aligned") for k in ("rotations", "dL_drotations")]
    for kw, text in rows:
        rc, msg = bwd(**kw)
        assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and text in msg, (kw, rc, msg)
    # a forward with a precomputed covariance has neither scales nor rotations: refused, and the text says why
    for k in ("scales", "rotations"):
        rc, msg = bwd(**{k: None})
        assert rc == lib.HS_EINVAL and b"cov3D_precomp" in msg, (k, msg)
    for bad in bad_dims:
        rc, msg = bwd(dims=_dims(lib, **bad))
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_plan:"), (bad, rc, msg)
    # an empty cloud: a successful no-op that looks at no pointer
    assert bwd(dims=_dims(lib, P=0), **{k: None for k in WORKSPACES + ARRAYS})[0] == lib.HS_OK


# ---- Python ----

def _stand_in(P=5, has_cov=False, aux=None, deferred=None):
    """A stand-in for an output tensor of a forward with grad (5 Gaussians, on the CPU): what _check_geometry looks at."""
    from casualhdrsplat_amd import _lib
    st = types.SimpleNamespace(dims=_lib.hs_dims(P, 16, 3, 16, 16, 1, 100, 0, 0), geom=torch.zeros(1))
    m3, op, sc, ro = torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 3), torch.zeros(P, 4)
    saved = (m3, op, None, None, sc, ro, None, None, None)
    fn = types.SimpleNamespace(st=st, saved_tensors=saved, has=(True, False, not has_cov, has_cov, False, False), aux=aux,
                               deferred=deferred, raw=False, filter_3D=None)
    return types.SimpleNamespace(grad_fn=fn), dict(means3D=m3, opacities=op, scales=sc, rotations=ro)


def test_python_refusals():
    import inspect
    import casualhdrsplat_amd as pkg
    from casualhdrsplat_amd import distortion, features
    assert list(inspect.signature(pkg.distortion_loss).parameters) == ["out", "geometry"]
    assert distortion._check_geometry is features._check_geometry and callable(distortion.distortion_workspace)
    handle, geo = _stand_in()
    for bad in ({k: v for k, v in geo.items() if k != "scales"}, dict(geo, means2D=torch.zeros(5, 3)), [geo["means3D"]], {}):
        with pytest.raises(ValueError, match="distortion_loss: geometry must be a dict with exactly the keys"):
            pkg.distortion_loss(handle, geometry=bad)
    with pytest.raises(ValueError, match=r"geometry\['means3D'\] has shape \(4, 3\)"):
        pkg.distortion_loss(handle, geometry=dict(geo, means3D=torch.zeros(4, 3)))
    with pytest.raises(ValueError, match=r"geometry\['opacities'\] lives on meta"):
        pkg.distortion_loss(handle, geometry=dict(geo, opacities=torch.zeros(5, 1, device="meta")))
    with pytest.raises(TypeError, match=r"geometry\['scales'\] must be a torch.Tensor"):
        pkg.distortion_loss(handle, geometry=dict(geo, scales=np.zeros((5, 3), np.float32)))
    with pytest.raises(ValueError, match="is not the tensor the forward"):
        pkg.distortion_loss(handle, geometry=dict(geo, scales=torch.zeros(5, 3)))
    # a keep_state rasterizer after a no_grad forward: the evaluation form only
    rs = pkg.GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 3, torch.zeros(3),
                                           False, False)
    rast = pkg.GaussianRasterizer(rs, keep_state=True)
    rast._last = {"state": handle.grad_fn.st}
    with pytest.raises(ValueError, match="keep_state rasterizer"):
        pkg.distortion_loss(rast, geometry=geo)
    # something that is no forward at all
    with pytest.raises(RuntimeError, match="keep_state=True"):
        pkg.distortion_loss(torch.zeros(3, 16, 16))
    handle, geo = _stand_in(has_cov=True)
    with pytest.raises(ValueError, match="cov3Ds_precomp"):
        pkg.distortion_loss(handle, geometry=geo)
    handle, geo = _stand_in(aux={"reduce_group": True})
    with pytest.raises(ValueError, match="view-parallel"):
        pkg.distortion_loss(handle, geometry=geo)
    handle, geo = _stand_in(deferred={"gather_group": object()})
    with pytest.raises(ValueError, match="view-parallel"):
        pkg.distortion_loss(handle, geometry=geo)


# ---- the restatement against what follows from the definition ----

def _stacked(o, z, W=16, H=16, sigma=3.0):
    """len(o) isotropic Gaussians on the centre of one tile, in the order given"""
    n = len(o)
    co = np.zeros((n, 4), np.float32)
    co[:, 0] = co[:, 2] = 1.0 / sigma ** 2
    co[:, 3] = o
    return dict(xy=np.full((n, 2), 7.5, np.float32), conic_opacity=co, depths=np.asarray(z, np.float32),
                ranges=np.array([[0, n]], np.int64), point_list=np.arange(n, dtype=np.int64))


def test_two_stacked_gaussians_in_closed_form():
    o1, o2, z1, z2, sigma = 0.6, 0.8, 2.0, 3.0, 3.0
    f = _stacked([o1, o2], [z1, z2], sigma=sigma)
    gam = np.random.default_rng(2).standard_normal((16, 16))
    r = DR.distortion(f, 16, 16, gam)
    yy, xx = np.mgrid[0:16, 0:16]
    G = np.exp(-0.5 * ((xx - 7.5) ** 2 + (yy - 7.5) ** 2) * np.float64(np.float32(1.0 / sigma ** 2)))
    a1, a2 = np.float64(np.float32(o1)) * G, np.float64(np.float32(o2)) * G
    on1, on2 = a1 >= 1 / 255, a2 >= 1 / 255
    w1 = np.where(on1, a1, 0.0)
    w2 = np.where(on2, a2 * (1 - w1), 0.0)
    s1, s2 = 1 / z1, 1 / z2
    assert on1.sum() > 100 and (~on1).sum() > 0
    np.testing.assert_allclose(r["out"], 2 * w1 * w2 * (s1 - s2), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(r["moment"], w1 * s1 + w2 * s2, rtol=1e-12, atol=1e-15)
    assert (r["out"][~(on1 & on2)] == 0).all() and r["out"].max() > 0.05
    # L_p = 2 a1 a2 (1 - a1) (s1 - s2):  dL/ds of the two, the opacity rows (d alpha / d o = G)
    both = on1 & on2
    np.testing.assert_allclose(r["rows"][0, 6], (gam * 2 * w1 * w2)[both].sum(), rtol=1e-12)
    np.testing.assert_allclose(r["rows"][1, 6], -(gam * 2 * w1 * w2)[both].sum(), rtol=1e-12)
    np.testing.assert_allclose(r["rows"][0, 5], (gam * G * 2 * a2 * (1 - 2 * a1) * (s1 - s2))[both].sum(), rtol=1e-11)
    np.testing.assert_allclose(r["rows"][1, 5], (gam * G * 2 * a1 * (1 - a1) * (s1 - s2))[both].sum(), rtol=1e-11)
    # a single contributor: exactly +0 everywhere, and no gradient
    r1 = DR.distortion(_stacked([o1], [z1]), 16, 16, gam)
    assert not r1["out"].any() and not np.signbit(r1["out"]).any() and not r1["rows"].any() and r1["moment"].max() > 0.25


def test_equal_depths_give_zero():
    rng = np.random.default_rng(3)
    f = _stacked(rng.uniform(0.1, 0.9, 9), np.full(9, 2.5))
    gam = rng.standard_normal((16, 16))
    r = DR.distortion(f, 16, 16, gam)
    assert np.abs(r["out"]).max() <= 1e-15 and np.abs(r["rows"][:, :6]).max() <= 1e-13        # v = 0: alpha moves nothing ...
    assert np.abs(r["rows"][:, 6]).max() > 1e-2                                   # ... but the depths would
    q = DR.distortion(f, 16, 16, gam, dtype=np.float32)
    assert not q["out"].any()
    assert (np.abs(q["rows"] - r["rows"]) <= 1e-4 * np.abs(r["rows"]) + Hh.C_BOUND * 2.0 ** -24 * r["S_rows"]).all()


def _pixel_weights(f, W, H):
    """per pixel the (instance, w) pairs of the published rule, entry by entry -- written independently of the restatement"""
    xy, co = f["xy"].astype(np.float64), f["conic_opacity"].astype(np.float64)
    gx = (W + 15) // 16
    res = {}
    for y in range(H):
        for x in range(W):
            r0, r1 = f["ranges"][(y // 16) * gx + x // 16]
            T, lst = 1.0, []
            for g in f["point_list"][int(r0):int(r1)]:
                dx, dy = xy[g, 0] - x, xy[g, 1] - y
                power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
                if power > 0:
                    continue
                a = min(0.99, co[g, 3] * np.exp(power))
                if a < 1 / 255:
                    continue
                if T * (1 - a) < 1e-4:
                    break
                lst.append((int(g), a * T))
                T *= 1 - a
            res[(y, x)] = lst
    return res


@pytest.fixture(scope="module")
def small(oracle):
    sc = S.make_scene(80, 40, 24, 0, seed=11)
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    return sc, f


def test_the_map_is_the_pairwise_double_sum(small):
    sc, f = small
    W, H = 40, 24
    r = DR.distortion(f, W, H)
    s = 1.0 / f["depths"].astype(np.float64)
    want, mom = np.zeros((H, W)), np.zeros((H, W))
    for (y, x), lst in _pixel_weights(f, W, H).items():
        want[y, x] = sum(wi * wj * abs(s[gi] - s[gj]) for gi, wi in lst for gj, wj in lst)
        mom[y, x] = sum(wi * s[gi] for gi, wi in lst)
        assert all(s[lst[k][0]] >= s[lst[k + 1][0]] for k in range(len(lst) - 1))      # sorted by depth
    assert want.max() > 1e-2 and (r["out"] >= 0).all() and r["count"].max() > 5
    np.testing.assert_allclose(r["out"], want, rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(r["moment"], mom, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(r["moment"], f["invdepth"], rtol=1e-5, atol=1e-6)       # what the oracle composites


def test_shift_invariance(small):
    sc, f = small
    W, H = 40, 24
    gam = np.random.default_rng(4).standard_normal((H, W))
    r = DR.distortion(f, W, H, gam)
    c = 0.37
    g = dict(f, depths=1.0 / (1.0 / f["depths"].astype(np.float64) + c))
    q = DR.distortion(g, W, H, gam)
    np.testing.assert_allclose(q["out"], r["out"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(q["rows"], r["rows"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(q["moment"], r["moment"] + c * (1 - r["final_T"]), rtol=1e-10, atol=1e-14)
    assert (q["S_out"] > r["S_out"])[r["count"] > 1].all()       # the bound is not invariant: it is built from |D| + s A


def _leaves(sc, dt=torch.float64):
    return [t.to(dt).clone().requires_grad_(True) for t in (sc.means3D, sc.opacities, sc.scales, sc.rotations)]


@pytest.mark.parametrize("antialias", (False, True))
def test_the_projected_truth_is_autograd_of_the_whole_loss(antialias):
    """float64 autograd through preprocess, bin_tiles and a torch copy of the sum, against the hand-derived rows pushed
    through the seven Jacobians of preprocess"""
    sc = S.make_scene(120, 56, 40, 0, seed=5)
    W, H = 56, 40
    gam = np.random.default_rng(5).standard_normal((H, W))
    leaves = _leaves(sc)
    total, fwd, img = DR.torch_loss(DR.view_of(sc.camera), *leaves, torch.as_tensor(gam), antialias=antialias, want_map=True)
    grads = torch.autograd.grad(total, leaves)
    r = DR.distortion(fwd, W, H, gam)
    np.testing.assert_allclose(r["out"], img.numpy(), rtol=1e-10, atol=1e-15)
    got = DR.project([sc.camera], [r["rows"]], [r["S_rows"]], *[l.detach().numpy() for l in leaves], antialias=antialias)
    for (k, rk), g in zip(DR.GEO_KEYS, grads):
        g = g.numpy().reshape(got[rk].shape)
        scale = np.abs(g).max()
        assert scale > 1e-2 and np.abs(got[rk] - g).max() <= 1e-9 * scale, (k, scale, np.abs(got[rk] - g).max())
        assert (got["abs_" + rk] >= np.abs(got[rk]) * (1 - 1e-12)).all(), k      # S dominates the number it stands beside


def test_a_directional_finite_difference():
    sc = S.make_scene(120, 56, 40, 0, seed=6)
    W, H = 56, 40
    rng = np.random.default_rng(6)
    gam = rng.standard_normal((H, W))
    view = DR.view_of(sc.camera)
    base = [l.detach() for l in _leaves(sc)]
    _, fwd = DR.torch_loss(view, *base, torch.as_tensor(gam))
    r = DR.distortion(fwd, W, H, gam)
    got = DR.project([sc.camera], [r["rows"]], [r["S_rows"]], *[l.numpy() for l in base])
    delta = [torch.as_tensor(rng.standard_normal(tuple(l.shape))) * s_ for l, s_ in zip(base, (1.0, 1.0, 0.1, 1.0))]
    eps = 1e-6
    val = []
    for sign in (1.0, -1.0):
        _, f2 = DR.torch_loss(view, *[l + sign * eps * d for l, d in zip(base, delta)], torch.as_tensor(gam))
        q = DR.distortion(f2, W, H)
        assert (q["n_contrib"] == r["n_contrib"]).all() and (q["count"] == r["count"]).all()      # no decision flipped
        val.append((q["out"] * gam).sum())
    fd = (val[0] - val[1]) / (2 * eps)
    want = sum((got[rk] * d.numpy().reshape(got[rk].shape)).sum() for (_, rk), d in zip(DR.GEO_KEYS, delta))
    assert abs(want) > 1e-2 and abs(fd - want) <= 1e-6 * abs(want) + 1e-8, (fd, want)


# ---- the bound the GPU tests use is neither vacuous nor unreachable ----

@pytest.mark.parametrize("name", tuple(GUARDED) + tuple(LONG) + ("posed", "aa", "plane"))
def test_the_float32_mode_lies_inside_the_bound(oracle, name):
    """The same sums in float32 (distort.hip's order of operations, numpy's exp and division) against the float64 truth:
    inside |x - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S for the map, the moment and the four gradients -- on every scene of the GPU file."""
    c = case(oracle, name)
    sc, W, H = c["sc"], c["W"], c["H"]
    ref = DR.truth(c["fwds"], c["cams"], c["gammas"], sc)
    f32 = [DR.distortion(f, W, H, g, dtype=np.float32) for f, g in zip(c["fwds"], c["gammas"])]
    for k, f in enumerate(c["fwds"]):
        assert (ref["n_contrib"][k] == f["n_contrib"]).all()             # the restatement decides as the oracle does
    need = dict(out=needed(np.stack([r["out"] for r in f32]), ref["out"], ref["S_out"]),
                moment=needed(np.stack([r["moment"] for r in f32]), ref["moment"], ref["S_moment"]))
    got = DR.project(c["cams"], [r["rows"] for r in f32], [r["S_rows"] for r in f32], sc.means3D.numpy(), sc.opacities.numpy(),
                     sc.scales.numpy(), sc.rotations.numpy(), float(getattr(sc, "scale_modifier", 1.0)),
                     bool(getattr(sc, "antialias", False)))
    rep = Hh.assert_grads_bounded({"d_" + k: got[rk] for k, rk in DR.GEO_KEYS}, ref, keys=DR.GEO_KEYS, what=name)
    need.update({k: v[1] for k, v in rep.items()})
    assert all(v <= Hh.C_BOUND for v in need.values()), (name, need)
    if name == "plane":
        assert np.abs(ref["out"]).max() <= 1e-5 * ref["S_out"].max()      # one depth plane: the map is zero up to the depths' ulps
    else:
        assert ref["out"].max() > 1e-3
        assert all(np.abs(ref[rk]).max() > 1e-3 for _, rk in DR.GEO_KEYS)
