"""CPU checks of the per-Gaussian feature compositing (features.hip: hs_composite_features_workspace_bytes,
hs_composite_features, hs_composite_features_backward; features.py): the C ABI (exports, struct layout, argument validation
before any HIP call), the Python argument errors, and the numpy restatement the GPU tests compare with
(tests/features_reference.py) against what follows from its definition."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import features_reference as R
import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_composite_features_workspace_bytes", "hs_composite_features", "hs_composite_features_backward")
FWD_FIELDS = ("geom", "binning", "image", "features", "out")
BWD_FIELDS = ("geom", "binning", "image", "ws", "dL_dout", "dL_dfeatures")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def frame(oracle):
    """The second guarded scene of the GPU tests (600 Gaussians, 104 x 72, SH degree 1: partial tiles in both directions)
    with its oracle forward, features (N(0, 1), an all-ones channel, a x 50 channel) and an upstream gradient."""
    sc, seed = Hh.guarded_scene(oracle, 600, 104, 72, 1)
    assert seed == 0            # (tests/test_features_gpu.py counts on it)
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    rng = np.random.default_rng(21)
    feat = rng.standard_normal((600, 5))
    feat[:, 1] = 1.0
    feat[:, 2] *= 50.0
    dL = rng.standard_normal((5, 72, 104))
    return f, feat, dL, R.composite(f, 104, 72, feat, dL)


# ---- C ABI ----

def test_feature_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
        assert not re.search(r"\d", n)
    assert "hs_composite_features_args" in header and "hs_composite_features_bwd_args" in header
    assert set(NAMES) <= set(lib.EXPORTS)
    assert set(re.findall(r"\b(hs_[a-z_]+)\s*\(", header)) == set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309 == lib.HS_VERSION       # (detected by name: the version does not move)


@pytest.mark.parametrize("name", ("hs_composite_features_args", "hs_composite_features_bwd_args"))
def test_feature_structs_match_c(lib, tmp_path, name):
    S_ = getattr(lib, name)
    fields = [n for n, _ in S_._fields_]
    lines = [f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {n}));' for n in fields]
    want = [C.sizeof(S_)] + [getattr(S_, n).offset for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want


def _dims(lib, P=1000, W=128, H=128, n_poses=1, capacity=10000, n_frames=0):
    return lib.hs_dims(P, 16, 3, W, H, n_poses, capacity, 0, n_frames)


def test_workspace_bytes_is_a_positive_multiple_of_256_and_grows_with_capacity(lib):
    L = lib.load()
    last = 0
    for cap in (0, 1, 15, 16, 17, 1000, 10 ** 5, 10 ** 7, (1 << 30) - 1):
        d = _dims(lib, capacity=cap, n_poses=3)
        b = L.hs_composite_features_workspace_bytes(C.byref(d))
        assert b > 0 and b % 256 == 0 and b >= 16 * cap + 16 * 1000 * 3 and b >= last, (cap, b)
        # the formula the header states (32-byte records: eight channels per pass); it does not depend on C
        assert b == (32 * cap + 255) // 256 * 256 + (32 * 1000 * 3 + 255) // 256 * 256
        last = b
    assert L.hs_composite_features_workspace_bytes(C.byref(_dims(lib, n_poses=4))) > \
        L.hs_composite_features_workspace_bytes(C.byref(_dims(lib)))
    assert L.hs_composite_features_workspace_bytes(C.byref(_dims(lib, P=0, capacity=0))) == 256
    assert L.hs_composite_features_workspace_bytes(None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    for bad in (dict(P=-1), dict(W=0), dict(n_poses=0), dict(capacity=-1), dict(capacity=1 << 30), dict(n_poses=3, n_frames=2)):
        assert L.hs_composite_features_workspace_bytes(C.byref(_dims(lib, **bad))) == lib.HS_EINVAL, bad
        assert L.hs_last_error().startswith(b"hs_plan:"), bad


def test_feature_calls_validate_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the field -- on a machine without a GPU: no HIP call is
    made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy address: validation must fail before it is dereferenced

    def call(which, dims=None, n_channels=8, **kw):
        fwd = which == "hs_composite_features"
        a = (lib.hs_composite_features_args if fwd else lib.hs_composite_features_bwd_args)()
        a.dims = dims if dims is not None else _dims(lib)
        a.n_channels = n_channels
        for k in (FWD_FIELDS if fwd else BWD_FIELDS):
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, which)(C.byref(a), None), L.hs_last_error()

    cases = {
        "hs_composite_features": [
            (dict(geom=None), b"null geom"), (dict(binning=None), b"null binning"), (dict(image=None), b"null image"),
            (dict(features=None), b"null features"), (dict(out=None), b"null out"),
            (dict(geom=one + 16), b"geom must be 256-byte aligned"), (dict(image=one + 128), b"image must be 256-byte aligned"),
            (dict(features=one + 2), b"features must be 4-byte aligned"), (dict(out=one + 1), b"out must be 4-byte aligned")],
        "hs_composite_features_backward": [
            (dict(geom=None), b"null geom"), (dict(binning=None), b"null binning"), (dict(image=None), b"null image"),
            (dict(ws=None), b"null ws"), (dict(dL_dout=None), b"null dL_dout"), (dict(dL_dfeatures=None), b"null dL_dfeatures"),
            (dict(ws=one + 128), b"ws must be 256-byte aligned"), (dict(binning=one + 64), b"binning must be 256-byte aligned"),
            (dict(dL_dout=one + 2), b"dL_dout must be 4-byte aligned"),
            (dict(dL_dfeatures=one + 3), b"dL_dfeatures must be 4-byte aligned")]}
    for which, rows in cases.items():
        assert getattr(L, which)(None, None) == lib.HS_EINVAL and L.hs_last_error() == which.encode() + b": null args"
        for kw, text in rows:
            rc, msg = call(which, **kw)
            assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and text in msg, (which, kw, rc, msg)
        for c in (0, -1, 513, 1 << 20):
            rc, msg = call(which, n_channels=c)
            assert rc == lib.HS_EINVAL and b"n_channels=%d outside [1, 512]" % c in msg, (which, c, rc, msg)
        # dims that hs_plan refuses
        for bad in (dict(P=-1), dict(H=0), dict(n_poses=0), dict(capacity=1 << 30), dict(n_poses=4, n_frames=3), dict(n_frames=-1)):
            rc, msg = call(which, dims=_dims(lib, **bad))
            assert rc == lib.HS_EINVAL and msg.startswith(b"hs_plan:"), (which, bad, rc, msg)
    # an empty cloud: the backward is a no-op that looks at no pointer but still refuses a bad C; the forward has `out` to write
    assert call("hs_composite_features_backward", dims=_dims(lib, P=0), **{k: None for k in BWD_FIELDS})[0] == lib.HS_OK
    assert call("hs_composite_features_backward", dims=_dims(lib, P=0), n_channels=0)[0] == lib.HS_EINVAL
    rc, msg = call("hs_composite_features", dims=_dims(lib, P=0), **{k: None for k in FWD_FIELDS})
    assert rc == lib.HS_EINVAL and b"null out" in msg


# ---- Python ----

def test_python_names_and_argument_errors():
    import casualhdrsplat_amd as pkg
    from casualhdrsplat_amd import _lib, features
    assert pkg.composite_features is features.composite_features and "composite_features" in pkg.__all__
    assert callable(features.feature_workspace) and features.MAX_CHANNELS == 512
    assert "composite_features" in pkg.__doc__
    with pytest.raises(RuntimeError, match="keep_state=True"):
        pkg.composite_features(torch.zeros(3, 4, 4), torch.zeros(5, 3))     # not the output of a forward
    # the checks that come before the library is called, on a stand-in for a forward's state (5 Gaussians, on the CPU)
    st = types.SimpleNamespace(dims=_lib.hs_dims(5, 16, 3, 16, 16, 1, 100, 0, 0), geom=torch.zeros(1))
    handle = types.SimpleNamespace(grad_fn=types.SimpleNamespace(st=st))
    with pytest.raises(TypeError, match="features must be a float32"):
        pkg.composite_features(handle, torch.zeros(5, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match="features must be a float32"):
        pkg.composite_features(handle, np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError, match=r"features must have shape \[5, C\]"):
        pkg.composite_features(handle, torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"features must have shape \[5, C\]"):
        pkg.composite_features(handle, torch.zeros(5))
    with pytest.raises(ValueError, match=r"C=0 outside \[1, 512\]"):
        pkg.composite_features(handle, torch.zeros(5, 0))
    with pytest.raises(ValueError, match=r"C=513 outside \[1, 512\]"):
        pkg.composite_features(handle, torch.zeros(5, 513))
    with pytest.raises(ValueError, match="features lives on meta"):
        pkg.composite_features(handle, torch.zeros(5, 3, device="meta"))


# ---- the restatement ----

def _two_stacked(alpha):
    """Two identical Gaussians on the centre of a 16 x 16 frame: one tile, both on its list."""
    return dict(xy=np.array([[8.0, 8.0], [8.0, 8.0]], np.float32),
                conic_opacity=np.array([[0.05, 0.0, 0.05, alpha]] * 2, np.float32),
                ranges=np.array([[0, 2]], np.uint32), point_list=np.array([0, 1], np.uint32))


def test_two_stacked_gaussians_give_alpha_and_alpha_times_one_minus_alpha():
    a = 0.5
    feat = np.array([[2.0, -1.0], [3.0, 0.25]])
    dL = np.zeros((2, 16, 16))
    dL[0, 8, 8], dL[1, 8, 8] = 1.5, -2.0
    r = R.composite(_two_stacked(a), 16, 16, feat, dL)
    assert r["out"][:, 8, 8].tolist() == [a * 2.0 + a * (1 - a) * 3.0, a * -1.0 + a * (1 - a) * 0.25]
    assert r["grad"].tolist() == [[a * 1.5, a * -2.0], [a * (1 - a) * 1.5, a * (1 - a) * -2.0]]
    assert r["count"][8, 8] == 2 and r["n_contrib"][8, 8] == 2
    assert r["S_out"][:, 8, 8].tolist() == [6 * (a * 2.0 + a * (1 - a) * 3.0), 6 * (a * 1.0 + a * (1 - a) * 0.25)]
    assert r["S_grad"].tolist() == [[4 * a * 1.5, 4 * a * 2.0], [5 * a * (1 - a) * 1.5, 5 * a * (1 - a) * 2.0]]
    # an opaque pair: alpha clamps to 0.99
    r = R.composite(_two_stacked(1.0), 16, 16, feat)
    assert abs(r["out"][0, 8, 8] - (0.99 * 2.0 + 0.99 * (1 - 0.99) * 3.0)) <= 1e-15 and not r["grad"].any()


def test_an_all_ones_channel_is_the_accumulated_opacity(frame):
    f, feat, dL, r = frame
    acc = 1.0 - r["final_T"]
    assert acc.sum() > 100 and np.abs(r["out"][1] - acc).max() <= 1e-12
    # the float64 evaluation takes the oracle's decisions on a guarded frame
    assert np.array_equal(r["n_contrib"], f["n_contrib"].astype(np.int64))
    assert (r["S_out"][1] >= 4 * acc * (1 - 1e-12)).all() and int(r["count"].max()) >= 20
    assert ((r["count"] == 0) == (r["n_contrib"] == 0)).all() and not r["out"][:, r["count"] == 0].any()


def test_reference_is_linear_in_the_features_and_satisfies_the_adjoint_identity(frame):
    f, feat, dL, r = frame
    g = np.random.default_rng(22).standard_normal(feat.shape)
    r2 = R.composite(f, 104, 72, 2.0 * feat - 3.0 * g, dL)
    rg = R.composite(f, 104, 72, g)
    assert np.abs(r2["out"] - (2.0 * r["out"] - 3.0 * rg["out"])).max() <= 1e-9 * np.abs(r["out"]).max()
    assert np.array_equal(r2["grad"], r["grad"])                   # the gradient does not depend on the features
    # sum_p out dL == sum_g grad f
    lhs, rhs = (r["out"] * dL).sum(), (r["grad"] * feat).sum()
    assert abs(lhs) > 1.0 and abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    # per channel too: channels do not mix
    for c in range(feat.shape[1]):
        l, h = (r["out"][c] * dL[c]).sum(), (r["grad"][:, c] * feat[:, c]).sum()
        assert abs(l - h) <= 1e-9 * max(abs(l), abs(h), 1.0), (c, l, h)


def test_float32_evaluation_stays_inside_the_bound(frame):
    """The bound the GPU tests hold the kernels to, |x - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S, against an honest float32
    evaluation of the definition (numpy: sequential float32 products and sums, its own expf): inside, with room -- the bound
    is not one that only a float64 computation could meet."""
    f, feat, dL, r = frame
    r32 = R.composite(f, 104, 72, feat.astype(np.float32), dL.astype(np.float32), dtype=np.float32)
    assert np.array_equal(r32["n_contrib"], r["n_contrib"]) and np.array_equal(r32["count"], r["count"])
    ref = R.composite(f, 104, 72, feat.astype(np.float32), dL.astype(np.float32))
    c_out = R.needed_constant(r32["out"], ref["out"], ref["S_out"])
    c_grad = R.needed_constant(r32["grad"], ref["grad"], ref["S_grad"])
    print(f"float32 restatement: C needed {c_out:.3f} (out), {c_grad:.3f} (grad); C_BOUND = {Hh.C_BOUND}")
    assert c_out <= Hh.C_BOUND and c_grad <= Hh.C_BOUND, (c_out, c_grad)
    # ... and not by being loose: the float32 values do differ from the float64 ones
    assert (r32["out"] != ref["out"]).any() and (r32["grad"] != ref["grad"]).any()
