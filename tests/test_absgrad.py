"""CPU checks of the absolute screen-gradient statistic (absgrad.hip: hs_abs_gradient_workspace_bytes, hs_abs_gradient;
importance.accumulate_abs_gradients, DensifyStats(absgrad=True)): the C ABI (exports, struct layout, argument validation
before any HIP call), the Python names and argument errors, and the numpy restatement the GPU tests compare with
(tests/absgrad_reference.py) against the C oracle's backward, a closed form and its own float32 evaluation."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import absgrad_reference as R
import helpers as Hh
from casualhdrsplat_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_abs_gradient_workspace_bytes", "hs_abs_gradient")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def frame(oracle):
    """The second guarded scene of the GPU tests (600 Gaussians, 104 x 72, SH degree 1: partial tiles in both directions)
    with its oracle forward and backward (bounds next to every gradient element) and the float64 restatement."""
    sc, seed = Hh.guarded_scene(oracle, 600, 104, 72, 1)
    assert seed == 0            # (tests/test_absgrad_gpu.py counts on it)
    f, b = Hh.run_oracle(oracle, sc, bounds=True)
    r = R.abs_gradients(f, 104, 72, sc.dL_dimage.numpy(), sc.bg.numpy())
    return sc, f, b, r


# ---- C ABI ----

def test_abs_gradient_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    assert "hs_abs_gradient_args" in header
    assert set(NAMES) <= set(lib.EXPORTS)
    assert set(re.findall(r"\b(hs_[a-z_]+)\s*\(", header)) == set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309 == lib.HS_VERSION       # (detected by name: the version does not move)


def test_abs_gradient_struct_matches_c(lib, tmp_path):
    S_ = lib.hs_abs_gradient_args
    fields = [n for n, _ in S_._fields_]
    assert fields == ["dims", "flags", "crf_K", "crf_umin", "crf_umax", "bg", "exposure", "crf_table", "geom", "binning", "image",
                      "ws", "dL_dout_color", "dL_dout_hdr", "dL_dout_alpha", "dL_dout_invdepth", "abs_grad_accum"]
    lines = [f'printf("%zu\\n", sizeof({S_.__name__}));'] + [f'printf("%zu\\n", offsetof({S_.__name__}, {n}));' for n in fields]
    want = [C.sizeof(S_)] + [getattr(S_, n).offset for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want


def _dims(lib, P=1000, W=128, H=128, n_poses=1, capacity=10000, n_frames=0, crf_K=0):
    return lib.hs_dims(P, 16, 3, W, H, n_poses, capacity, crf_K, n_frames)


def _align(n):
    return (n + 255) // 256 * 256


def test_workspace_bytes_is_a_multiple_of_256_and_grows_with_capacity_and_poses(lib):
    L = lib.load()
    last = 0
    for cap in (0, 1, 31, 32, 33, 1000, 10 ** 5, 10 ** 7, (1 << 30) - 1):
        b = L.hs_abs_gradient_workspace_bytes(C.byref(_dims(lib, capacity=cap)))
        assert b == _align(8 * cap) + _align(8 * 1000) and b % 256 == 0 and b >= last, (cap, b)
        last = b
    assert L.hs_abs_gradient_workspace_bytes(C.byref(_dims(lib, capacity=10 ** 5))) > \
        L.hs_abs_gradient_workspace_bytes(C.byref(_dims(lib, capacity=10 ** 4)))
    # ... and with the instances: one row per (pose, Gaussian)
    assert L.hs_abs_gradient_workspace_bytes(C.byref(_dims(lib, n_poses=4))) == _align(8 * 10000) + _align(8 * 4000)
    assert L.hs_abs_gradient_workspace_bytes(C.byref(_dims(lib, P=0, capacity=0))) == 256
    assert L.hs_abs_gradient_workspace_bytes(None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    for bad in (dict(P=-1), dict(W=0), dict(n_poses=0), dict(capacity=-1), dict(capacity=1 << 30), dict(n_poses=3, n_frames=2)):
        assert L.hs_abs_gradient_workspace_bytes(C.byref(_dims(lib, **bad))) == lib.HS_EINVAL, bad
        assert L.hs_last_error().startswith(b"hs_plan:"), bad


def test_abs_gradient_validates_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the field, and the no-op succeeds -- on a machine without
    a GPU: no HIP call is made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy address: validation must fail before it is dereferenced
    required = ("bg", "geom", "binning", "image", "ws", "dL_dout_color", "abs_grad_accum")
    optional = ("exposure", "crf_table", "dL_dout_hdr", "dL_dout_alpha", "dL_dout_invdepth")

    def call(dims=None, **kw):
        a = lib.hs_abs_gradient_args()
        a.dims = dims if dims is not None else _dims(lib)
        for k in required + optional:
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.hs_abs_gradient(C.byref(a), None), L.hs_last_error()

    assert L.hs_abs_gradient(None, None) == lib.HS_EINVAL and L.hs_last_error() == b"hs_abs_gradient: null args"
    cases = [(dict(**{k: None}), b"null " + k.encode()) for k in required]
    cases += [(dict(ws=one + 128), b"ws must be 256-byte aligned"), (dict(geom=one + 16), b"geom must be 256-byte aligned"),
              (dict(binning=one + 64), b"binning must be 256-byte aligned"), (dict(image=one + 8), b"image must be 256-byte aligned"),
              (dict(abs_grad_accum=one + 2), b"abs_grad_accum must be 4-byte aligned"),
              (dict(dL_dout_color=one + 1), b"dL_dout_color must be 4-byte aligned"), (dict(bg=one + 3), b"bg must be 4-byte aligned")]
    cases += [(dict(**{k: one + 2}), k.encode() + b" must be 4-byte aligned") for k in optional]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_abs_gradient:") and text in msg, (kw, rc, msg)
    # per-image gradients with frames
    for k in ("dL_dout_alpha", "dL_dout_invdepth"):
        other = "dL_dout_invdepth" if k == "dL_dout_alpha" else "dL_dout_alpha"
        rc, msg = call(dims=_dims(lib, n_poses=4, n_frames=2), **{other: None})
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_abs_gradient:") and b"n_frames=2" in msg, (k, rc, msg)
    # HDR needs its three
    HDR = lib.HS_FLAG_HDR
    for kw in (dict(exposure=None), dict(crf_table=None), dict(crf_K=1), dict(crf_K=17)):
        base = dict(flags=HDR, crf_K=16)
        base.update(kw)
        rc, msg = call(dims=_dims(lib, crf_K=16), **base)
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_abs_gradient: HDR needs"), (kw, rc, msg)
    # dims that hs_plan refuses
    for bad in (dict(P=-1), dict(H=0), dict(n_poses=0), dict(capacity=1 << 30), dict(n_poses=4, n_frames=3), dict(n_frames=-1)):
        rc, msg = call(dims=_dims(lib, **bad))
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_plan:"), (bad, rc, msg)
    # an empty cloud is a no-op: no pointer is looked at
    assert call(dims=_dims(lib, P=0), **{k: None for k in required + optional})[0] == lib.HS_OK


# ---- Python ----

def test_python_names_and_argument_errors():
    import casualhdrsplat_amd as pkg
    from casualhdrsplat_amd import importance
    assert pkg.accumulate_abs_gradients is importance.accumulate_abs_gradients
    assert "accumulate_abs_gradients" in pkg.__all__
    with pytest.raises(RuntimeError, match="keep_state=True"):
        pkg.accumulate_abs_gradients(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4), torch.zeros(5))   # not the output of a forward
    plain = pkg.DensifyStats(5, "cpu")
    assert plain.abs_grad_accum is None
    with pytest.raises(ValueError, match="absgrad=True"):
        plain.mean_abs_grad()
    with pytest.raises(ValueError, match="absgrad=True"):
        importance._abs_target("accumulate_abs_gradients", plain, 5, torch.device("cpu"))
    with pytest.raises(TypeError, match="DensifyStats"):
        importance._abs_target("accumulate_abs_gradients", [0.0] * 5, 5, torch.device("cpu"))
    for bad in (torch.zeros(4), torch.zeros(5, dtype=torch.float64), torch.zeros(5, 1), torch.zeros(10)[::2]):
        with pytest.raises(ValueError, match=r"abs_grad_accum must be a contiguous torch.float32 \[5\]"):
            importance._abs_target("accumulate_abs_gradients", bad, 5, torch.device("cpu"))
    t = torch.zeros(5)
    assert importance._abs_target("accumulate_abs_gradients", t, 5, torch.device("cpu")) is t


def test_densify_stats_own_reset_and_resize_the_array():
    import casualhdrsplat_amd as pkg
    st = pkg.DensifyStats(5, "cpu", absgrad=True)
    assert st.abs_grad_accum.dtype == torch.float32 and tuple(st.abs_grad_accum.shape) == (5,) and not st.abs_grad_accum.any()
    assert importance_target(st) is st.abs_grad_accum
    st.abs_grad_accum += torch.arange(5.0)
    st.denom += torch.tensor([0.0, 1.0, 2.0, 4.0, 0.5])
    assert st.mean_abs_grad().tolist() == [0.0, 1.0, 1.0, 0.75, 4.0]      # abs_grad_accum / max(denom, 1)
    assert not st.grad_accum.any()                                        # its own array, not grad_accum's
    st.reset()
    assert not st.abs_grad_accum.any() and not st.denom.any()
    st.abs_grad_accum += 1
    st.resize(9)
    assert tuple(st.abs_grad_accum.shape) == (9,) and not st.abs_grad_accum.any() and st.abs_grad_accum.dtype == torch.float32
    plain = pkg.DensifyStats(5, "cpu")
    plain.reset(); plain.resize(7)
    assert plain.abs_grad_accum is None and tuple(plain.grad_accum.shape) == (7,)


def importance_target(st):
    from casualhdrsplat_amd import importance
    return importance._abs_target("test", st, int(st.denom.shape[0]), st.denom.device)


def test_densify_and_prune_takes_absgrad_and_defaults_to_the_signed_statistic():
    import inspect
    from casualhdrsplat_amd import densify
    assert inspect.signature(densify.densify_and_prune).parameters["absgrad"].default is False


# ---- the restatement ----

def test_signed_sums_are_the_oracles_mean2D_gradient(frame):
    """sum_p t_x, sum_p t_y of the restatement against dL_dmeans2D of the C oracle's backward, inside the bound every gradient
    of the library is held to (helpers.assert_grads_bounded: 1e-4 |ref| + C_BOUND 2^-24 sum w |term|, the oracle's own S)."""
    sc, f, b, r = frame
    got = {"d_means2D": np.stack([r["signed_x"], r["signed_y"], np.zeros_like(r["signed_x"])], axis=1)}
    rep = Hh.assert_grads_bounded(got, b, keys=[("means2D", "dL_dmeans2D")], what="absgrad reference, signed sums")
    print("signed sums against the C oracle: C needed", rep["means2D"][1])
    assert np.abs(b["dL_dmeans2D"][:, :2]).max() > 1e-3 and r["hit"].sum() > 300
    # the float64 evaluation takes the oracle's decisions on a guarded frame
    assert np.array_equal(r["n_contrib"], f["n_contrib"].astype(np.int64))
    assert np.abs(r["final_T"] - f["final_T"]).max() <= 2e-5


def test_the_statistic_dominates_the_signed_gradient(frame):
    sc, f, b, r = frame
    assert (r["abs_x"] >= np.abs(r["signed_x"]) * (1 - 1e-12)).all() and (r["abs_y"] >= np.abs(r["signed_y"]) * (1 - 1e-12)).all()
    st = R.statistic([r])
    assert (st["a"] >= np.hypot(r["signed_x"], r["signed_y"]) * (1 - 1e-12)).all()
    # ... and it is the point of the statistic that it is LARGER where the terms cancel: most Gaussians here
    assert (st["a"] > 1.5 * np.hypot(r["signed_x"], r["signed_y"]))[r["hit"]].mean() > 0.5
    assert ((st["a"] > 0) <= r["hit"]).all() and (st["S"] >= 4 * st["a"] * (1 - 1e-12)).all()
    before = np.full(600, 1.5)
    after = R.accumulate(before, [st, st])
    assert np.array_equal(after[~r["hit"]], before[~r["hit"]]) and np.allclose(after[r["hit"]], 1.5 + 2 * st["a"][r["hit"]])


def _isolated(sigma, o, W=48):
    """One isotropic Gaussian on a pixel centre of a W x W frame, on the list of every tile."""
    n = (W // 16) ** 2
    c = 1.0 / sigma ** 2
    return dict(xy=np.array([[W / 2.0, W / 2.0]], np.float32), conic_opacity=np.array([[c, 0.0, c, o]], np.float64),
                rgb=np.array([[0.25, 0.5, 1.0]]), depths=np.array([2.0], np.float32),
                ranges=np.stack([np.arange(n), np.arange(n) + 1], axis=1).astype(np.uint32), point_list=np.zeros(n, np.uint32)), c


def test_an_isolated_isotropic_gaussian_against_the_closed_form():
    """One Gaussian, nothing behind it but a black background, a constant dL: w = o G (c . dL), t_x = -c dx w W / 2, and
    sum_p |t_x| -> (W / 2) c o (c . dL) * integral over the disc alpha >= 1 / 255 of |x| e^(-c r^2 / 2)
                 = (W / 2) c o (c . dL) * 4 * [sqrt(pi) erf(R sqrt(a)) / (4 a^1.5) - R e^(-a R^2) / (2 a)],  a = c / 2."""
    W, sigma, o = 48, 4.0, 0.6
    f, c = _isolated(sigma, o, W)
    dL = np.ones((3, W, W)) * np.array([0.5, -0.25, 0.125])[:, None, None]
    k = 0.25 * 0.5 - 0.5 * 0.25 + 1.0 * 0.125
    r = R.abs_gradients(f, W, W, dL, np.zeros(3))
    # the same sum written out on the grid, without the walk
    yy, xx = np.meshgrid(np.arange(W), np.arange(W), indexing="ij")
    dx, dy = W / 2.0 - xx, W / 2.0 - yy
    G = np.exp(-0.5 * c * (dx * dx + dy * dy))
    on = np.minimum(0.99, o * G) >= 1.0 / 255.0
    grid_x = (np.abs(c * dx) * o * G * abs(k) * 0.5 * W)[on].sum()
    assert abs(r["abs_x"][0] - grid_x) <= 1e-12 * grid_x and abs(r["abs_y"][0] - grid_x) <= 1e-12 * grid_x
    assert abs(r["signed_x"][0]) <= 1e-12 * grid_x and abs(r["signed_y"][0]) <= 1e-12 * grid_x      # the terms cancel exactly
    assert r["pairs"] == int(on.sum()) and on.sum() < W * W
    a = 0.5 * c
    Rr = math.sqrt(2.0 * math.log(255.0 * o) / c)
    integral = 4.0 * (math.sqrt(math.pi) * math.erf(Rr * math.sqrt(a)) / (4.0 * a ** 1.5) - Rr * math.exp(-a * Rr * Rr) / (2.0 * a))
    closed = 0.5 * W * c * o * abs(k) * integral
    assert abs(r["abs_x"][0] - closed) <= 1e-2 * closed, (r["abs_x"][0], closed)
    # with a background the walk starts at q = bg . dL: w = o G (c . dL - bg . dL)
    bg = np.array([0.5, 0.25, 0.125])
    kb = k - float((bg * np.array([0.5, -0.25, 0.125])).sum())
    rb = R.abs_gradients(f, W, W, dL, bg)
    assert abs(rb["abs_x"][0] - grid_x * abs(kb) / abs(k)) <= 1e-12 * grid_x
    # dL_dalpha enters the background term with the sign flipped, dL_dinvdepth as a fourth channel
    ra = R.abs_gradients(f, W, W, dL, bg, dL_alpha=np.full((W, W), 0.5), dL_invdepth=np.full((W, W), 2.0))
    assert abs(ra["abs_x"][0] - grid_x * abs(kb + 0.5 + 2.0 / 2.0) / abs(k)) <= 1e-12 * grid_x


def test_float32_evaluation_stays_inside_the_bound(frame):
    """The bound the GPU test holds the kernel to, |x - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S, against an honest float32
    evaluation of the definition (numpy: sequential float32 operations, its own expf): inside, with room -- the bound is not
    one that only a float64 computation could meet."""
    sc, f, b, r = frame
    r32 = R.abs_gradients(f, 104, 72, sc.dL_dimage.numpy(), sc.bg.numpy(), dtype=np.float32)
    assert np.array_equal(r32["n_contrib"], r["n_contrib"]) and np.array_equal(r32["hit"], r["hit"])
    s64, s32 = R.statistic([r]), R.statistic([r32])
    c_a = R.needed_constant(s32["a"], s64["a"], s64["S"])
    c_x = R.needed_constant(r32["abs_x"], r["abs_x"], r["S_x"])
    c_y = R.needed_constant(r32["abs_y"], r["abs_y"], r["S_y"])
    print(f"float32 restatement: C needed {c_a:.3f} (statistic), {c_x:.3f} / {c_y:.3f} (x / y sums); C_BOUND = {Hh.C_BOUND}")
    assert max(c_a, c_x, c_y) <= Hh.C_BOUND, (c_a, c_x, c_y)
    # ... and not by being loose: the float32 values do differ from the float64 ones
    assert (s32["a"] != s64["a"]).any()


@pytest.mark.parametrize("which", ((3000, 48, 40, 1), (6000, 64, 64, 0)))
def test_long_list_scenes_have_a_thin_guard_band(oracle, which):
    """The two long-list scenes of the GPU tests zero dL on the pixels where a decision differed; those lie inside the
    oracle's guard band (helpers.decision_masks asserts it), so a band of at most 1 % of the frame bounds the excluded share
    from the oracle alone."""
    P, W, H, deg = which
    sc = S.make_scene(P, W, H, deg, seed=0)
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    lens = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).max()
    assert lens > 1500 and int(f["n_contrib"].max()) > 128
    pix_risk, _ = Hh.oracle_risk(oracle, sc, [f])
    print(which, "guard band share", float(pix_risk.mean()))
    assert float(pix_risk.mean()) <= 0.01
