"""CPU checks of the geometry gradients through the composited feature channels (featgeo.hip:
hs_composite_features_geometry_workspace_bytes, hs_composite_features_geometry_backward; features.composite_features(...,
geometry=...)): the C ABI (exports, struct layout, argument validation before any HIP call), the Python refusals, and the
TRUTH the GPU tests compare with -- the C oracle's backward of ceil(C / 3) colors_precomp renders over a black background,
three feature columns at a time as the colours and the same three channels of dL_dout as the image gradient, gradients and
bounds summed over the triples (`oracle_truth`, shared with tests/test_features_geometry_gpu.py)."""
import copy
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_composite_features_geometry_workspace_bytes", "hs_composite_features_geometry_backward")
ARGS = "hs_composite_features_geometry_args"
WORKSPACES = ("geom", "binning", "image", "ws")
ARRAYS = ("viewmatrices", "projmatrices", "camposes", "means3D", "opacities", "scales", "rotations", "features", "dL_dout",
          "dL_dmeans3D", "dL_dopacities", "dL_dscales", "dL_drotations")
# the four tensors of the issue, as (key of the HIP result "d_<key>", key of the oracle's result)
GEO_KEYS = [("means3D", "dL_dmeans3D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"), ("rotations", "dL_drots")]


def oracle_truth(O, sc, feat, dL, cameras=None, cache=None, tag=None):
    """Geometry gradients of sum(out * dL) for out = the compositing of `feat` [P, C] under the scene's forward(s), from the
    C oracle: per pose and per triple of channels (the last one padded with zero columns) one colors_precomp forward over a
    black background and its backward under that triple of dL [n_poses, C, H, W] with bounds=True (run_oracle_poses with
    that one pose: no 1 / N), summed in float64 over poses and triples.  Returns {dL_dX, abs_dL_dX} for X in GEO_KEYS.
    `cache` (a dict) with `tag`: the per-(pose, triple) results are kept under (tag, pose, first column, width), so cases
    that take the first C columns of one matrix share their full triples."""
    sc = copy.copy(sc)            # (a shallow copy keeps attributes set on the instance: antialias, scale_modifier)
    sc.bg = torch.zeros(3)
    cams = list(cameras) if cameras is not None else [sc.camera]
    feat = np.asarray(feat, np.float32)
    dL = np.asarray(dL, np.float32)
    P, Cn = feat.shape
    assert dL.shape[:2] == (len(cams), Cn)
    keys = [rk for _, rk in GEO_KEYS] + ["abs_" + rk for _, rk in GEO_KEYS]
    acc = None
    for k, cam in enumerate(cams):
        for c0 in range(0, Cn, 3):
            w = min(3, Cn - c0)
            ck = (tag, k, c0, w)
            b = cache.get(ck) if cache is not None and tag is not None else None
            if b is None:
                cols = np.zeros((P, 3), np.float32)
                cols[:, :w] = feat[:, c0:c0 + w]
                d3 = np.zeros((3,) + dL.shape[2:], np.float32)
                d3[:w] = dL[k, c0:c0 + w]
                colors = torch.from_numpy(cols)
                f, _ = Hh.run_oracle(O, sc, cam=cam, backward=False, use_colors_precomp=colors)
                r = Hh.run_oracle_poses(O, sc, [cam], d3, [f], bounds=True, use_colors_precomp=colors)
                b = {q: np.asarray(r[q], np.float64) for q in keys}
                if cache is not None and tag is not None:
                    cache[ck] = b
            acc = {q: v.copy() for q, v in b.items()} if acc is None else {q: acc[q] + b[q] for q in keys}
    return acc


def geometry_inputs(P, H, W, seed, C_all, n_poses=1):
    """features N(0, 1) with an all-ones column (1) and a x 50 column (2); dL_dout N(0, 1)"""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((P, C_all))
    if C_all > 1:
        feat[:, 1] = 1.0
    if C_all > 2:
        feat[:, 2] *= 50.0
    return feat.astype(np.float32), rng.standard_normal((n_poses, C_all, H, W)).astype(np.float32)


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- C ABI ----

def test_geometry_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    assert "The outputs carry NO gradient to the geometry" not in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    assert ARGS in header and set(NAMES) <= set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == lib.HS_VERSION == 309       # (detected by name: the version does not move)


def test_geometry_struct_matches_c(lib, tmp_path):
    S_ = getattr(lib, ARGS)
    fields = [n for n, _ in S_._fields_]
    assert set(WORKSPACES + ARRAYS) <= set(fields)
    lines = [f'printf("%zu\\n", sizeof({ARGS}));'] + [f'printf("%zu\\n", offsetof({ARGS}, {n}));' for n in fields]
    want = [C.sizeof(S_)] + [getattr(S_, n).offset for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want


def _dims(lib, P=1000, W=128, H=128, n_poses=1, capacity=10000, n_frames=0):
    return lib.hs_dims(P, 16, 3, W, H, n_poses, capacity, 0, n_frames)


def test_workspace_bytes_is_a_positive_multiple_of_256_and_never_shrinks(lib):
    L = lib.load()
    fn = L.hs_composite_features_geometry_workspace_bytes
    a256 = lambda n: (n + 255) // 256 * 256
    last = 0
    for cap in (0, 1, 15, 16, 17, 1000, 10 ** 5, 10 ** 7, (1 << 30) - 1):
        b = fn(C.byref(_dims(lib, capacity=cap, n_poses=3)))
        # the formula the header states: 64-byte pair records, 64-byte rows per instance, one flag byte per pair
        assert b > 0 and b % 256 == 0 and b >= last and b == a256(64 * cap) + a256(64 * 1000 * 3) + a256(cap), (cap, b)
        last = b
    last = 0
    for P, n_poses in ((0, 1), (1, 1), (3, 1), (2, 2), (1000, 1), (1000, 2), (999, 3), (10 ** 6, 1), (10 ** 6, 4)):     # P * n_poses ascending
        b = fn(C.byref(_dims(lib, P=P, n_poses=n_poses)))
        assert b > 0 and b % 256 == 0 and b >= last, (P, n_poses, b)
        last = b
    assert fn(C.byref(_dims(lib, P=0, capacity=0))) == 256
    assert fn(None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    for bad in (dict(P=-1), dict(W=0), dict(n_poses=0), dict(capacity=-1), dict(capacity=1 << 30), dict(n_poses=3, n_frames=2)):
        assert fn(C.byref(_dims(lib, **bad))) == lib.HS_EINVAL, bad
        assert L.hs_last_error().startswith(b"hs_plan:"), bad


def test_the_call_validates_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the field -- on a machine without a GPU: no HIP call is
    made before the arguments are known to be good."""
    L = lib.load()
    which = "hs_composite_features_geometry_backward"
    one = 4096     # non-null dummy address: validation must fail before it is dereferenced

    def call(dims=None, n_channels=8, **kw):
        a = getattr(lib, ARGS)()
        a.dims = dims if dims is not None else _dims(lib)
        a.n_channels = n_channels
        for k in WORKSPACES + ARRAYS:
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, which)(C.byref(a), None), L.hs_last_error()

    assert getattr(L, which)(None, None) == lib.HS_EINVAL and L.hs_last_error() == which.encode() + b": null args"
    rows = [(dict(**{k: None}), b"null " + k.encode()) for k in WORKSPACES + ARRAYS]
    rows += [(dict(**{k: one + 128}), k.encode() + b" must be 256-byte aligned") for k in WORKSPACES]
    rows += [(dict(**{k: one + 2}), k.encode() + b" must be 4-byte aligned") for k in ARRAYS if k not in ("rotations", "dL_drotations")]
    rows += [(dict(**{k: one + 4}), k.encode() + b" must be 16-byte aligned") for k in ("rotations", "dL_drotations")]
    for kw, text in rows:
        rc, msg = call(**kw)
        assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and text in msg, (kw, rc, msg)
    # a forward with a precomputed covariance has neither scales nor rotations: refused, and the text says why
    for k in ("scales", "rotations"):
        rc, msg = call(**{k: None})
        assert rc == lib.HS_EINVAL and b"cov3D_precomp" in msg, (k, msg)
    for c in (0, -1, 513, 1 << 20):
        rc, msg = call(n_channels=c)
        assert rc == lib.HS_EINVAL and b"n_channels=%d outside [1, 512]" % c in msg, (c, rc, msg)
    for bad in (dict(P=-1), dict(H=0), dict(n_poses=0), dict(capacity=1 << 30), dict(n_poses=4, n_frames=3), dict(n_frames=-1)):
        rc, msg = call(dims=_dims(lib, **bad))
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_plan:"), (bad, rc, msg)
    # an empty cloud: a successful no-op that looks at no pointer but still refuses a bad C
    assert call(dims=_dims(lib, P=0), **{k: None for k in WORKSPACES + ARRAYS})[0] == lib.HS_OK
    assert call(dims=_dims(lib, P=0), n_channels=0)[0] == lib.HS_EINVAL


# ---- Python ----

def _stand_in(P=5, has_cov=False, aux=None, deferred=None, raw=False):
    """A stand-in for an output tensor of a forward with grad (5 Gaussians, on the CPU): what _check_geometry looks at."""
    from casualhdrsplat_amd import _lib
    st = types.SimpleNamespace(dims=_lib.hs_dims(P, 16, 3, 16, 16, 1, 100, 0, 0), geom=torch.zeros(1))
    m3, op, sc, ro = torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 3), torch.zeros(P, 4)
    saved = (m3, op, None, None, sc, ro, None, None, None)
    fn = types.SimpleNamespace(st=st, saved_tensors=saved, has=(True, False, not has_cov, has_cov, False, False), aux=aux,
                               deferred=deferred, raw=raw, filter_3D=None)
    return types.SimpleNamespace(grad_fn=fn), dict(means3D=m3, opacities=op, scales=sc, rotations=ro)


def test_python_refusals():
    import inspect
    import casualhdrsplat_amd as pkg
    from casualhdrsplat_amd import features
    assert "geometry" in inspect.signature(pkg.composite_features).parameters
    assert features.GEOMETRY_KEYS == ("means3D", "opacities", "scales", "rotations") and callable(features.geometry_workspace)
    feat = torch.zeros(5, 3)
    handle, geo = _stand_in()
    # wrong keys
    for bad in ({k: v for k, v in geo.items() if k != "scales"}, dict(geo, means2D=torch.zeros(5, 3)), [geo["means3D"]], {}):
        with pytest.raises(ValueError, match="exactly the keys"):
            pkg.composite_features(handle, feat, geometry=bad)
    # wrong shapes, wrong device, another tensor
    with pytest.raises(ValueError, match=r"geometry\['means3D'\] has shape \(4, 3\)"):
        pkg.composite_features(handle, feat, geometry=dict(geo, means3D=torch.zeros(4, 3)))
    with pytest.raises(ValueError, match=r"geometry\['rotations'\] has shape \(5, 3\)"):
        pkg.composite_features(handle, feat, geometry=dict(geo, rotations=torch.zeros(5, 3)))
    with pytest.raises(ValueError, match=r"geometry\['opacities'\] lives on meta"):
        pkg.composite_features(handle, feat, geometry=dict(geo, opacities=torch.zeros(5, 1, device="meta")))
    with pytest.raises(TypeError, match=r"geometry\['scales'\] must be a torch.Tensor"):
        pkg.composite_features(handle, feat, geometry=dict(geo, scales=np.zeros((5, 3), np.float32)))
    with pytest.raises(ValueError, match="is not the tensor the forward"):
        pkg.composite_features(handle, feat, geometry=dict(geo, scales=torch.zeros(5, 3)))
    # a keep_state rasterizer: there is no graph to send gradients into
    rs = pkg.GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 3, torch.zeros(3),
                                           False, False)
    rast = pkg.GaussianRasterizer(rs, keep_state=True)
    rast._last = {"state": handle.grad_fn.st}
    with pytest.raises(ValueError, match="keep_state rasterizer"):
        pkg.composite_features(rast, feat, geometry=geo)
    # a forward with cov3Ds_precomp, and view-parallel forwards
    handle, geo = _stand_in(has_cov=True)
    with pytest.raises(ValueError, match="cov3Ds_precomp"):
        pkg.composite_features(handle, feat, geometry=geo)
    handle, geo = _stand_in(aux={"reduce_group": True})
    with pytest.raises(ValueError, match="view-parallel"):
        pkg.composite_features(handle, feat, geometry=geo)
    handle, geo = _stand_in(deferred={"gather_group": object()})
    with pytest.raises(ValueError, match="view-parallel"):
        pkg.composite_features(handle, feat, geometry=geo)


# ---- the truth ----

def test_the_oracle_truth_runs_and_is_linear_in_the_channels(oracle):
    """The second guarded scene of the GPU tests: the truth of C = 4 (two triples, the second padded) is the sum of the four
    single-channel truths, the bounds add likewise, and the all-ones channel moves opacities."""
    P, W, H = 600, 104, 72
    sc, seed = Hh.guarded_scene(oracle, P, W, H, 1)
    assert seed == 0
    feat, dL = geometry_inputs(P, H, W, 41, 4)
    whole = oracle_truth(oracle, sc, feat, dL)
    single = [oracle_truth(oracle, sc, feat[:, c:c + 1], dL[:, c:c + 1]) for c in range(4)]
    for _, rk in GEO_KEYS:
        total = sum(s[rk] for s in single)
        scale = np.abs(whole[rk]).max()
        assert scale > 1e-3 and np.abs(whole[rk] - total).max() <= 1e-4 * scale, (rk, scale)
        assert (whole["abs_" + rk] >= 0).all() and whole["abs_" + rk].max() > 0
        assert (whole["abs_" + rk] <= sum(s["abs_" + rk] for s in single) * (1 + 1e-5) + 1e-30).all(), rk
    assert np.abs(single[1]["dL_dopacity"]).max() > 1e-3
