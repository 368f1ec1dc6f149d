"""CPU checks of the 3D smoothing filter (smoothing.hip: hs_smoothing_filter_workspace_bytes, hs_smoothing_filter,
hs_smoothing_apply, hs_smoothing_apply_backward; smoothing.py; GaussianRasterizer(..., filter_3D=...)): the numpy restatement
the GPU tests compare with (tests/smoothing_reference.py) against float64 and the bars that follow from it, the C ABI (exports,
struct layout, argument validation before any HIP call), the Python argument errors, and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import activation_reference as A
import smoothing_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_smoothing_filter_workspace_bytes", "hs_smoothing_filter", "hs_smoothing_apply", "hs_smoothing_apply_backward")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- the restatement ----

def test_bars_are_twice_the_measured_constants():
    """The float32 restatement against float64 on 10^6 seeded rows (logits N(0, 3) plus the rows +-17, +-30, +-88, +-100 and
    0; log scales U(-9, 3); filters e^U(-9, 1), every 16th an exact zero): each bar the GPU tests use is twice the constant
    measured here, rounded up to a power of two.  s' and o' against the float64 forward of the stored values (o' with the
    2^-126 floor: o is denormal at x = -88); the gradients against the float64 chain rule on the float32 forward values, the
    opacity gradient relative with the floor, the scale gradient in units of |g_k s' r| + |g_o o' t|."""
    x, l, f, g_o, g_s = R.inputs()
    rows = R.ROWS + len(R.SPECIAL_LOGITS)
    assert x.shape == (rows,) and l.shape == (rows, 3) and f.shape == (rows,) and (f == 0).sum() >= rows // 16
    assert f[f > 0].min() >= np.exp(-9.01) and f.max() <= np.exp(1.01)
    fwd = R.apply(x, l, f)
    assert all(np.isfinite(a).all() for a in fwd.values())
    d_o, d_s = R.backward(g_o, g_s, fwd)
    assert np.isfinite(d_o).all() and np.isfinite(d_s).all()
    c = dict(R.forward_constants(x, l, f, fwd["oc"], fwd["sp"]), **R.backward_constants(g_o, g_s, fwd, d_o, d_s))
    assert set(c) == set(R.BARS) == set(R.MEASURED)
    for k, v in c.items():
        print(f"{k}: c = {v:.4f} (recorded {R.MEASURED[k]}, bar {R.BARS[k]})")
    for k, v in c.items():
        assert R.BARS[k] == R.bar_of(v), (k, v)
        assert abs(v - R.MEASURED[k]) <= 0.1 * R.MEASURED[k], (k, v)


def test_a_filter_of_zeros_is_the_plain_activations_bit_for_bit():
    """sqrt(s s) == s, q / q == 1, o 1 == o, and the chain rule collapses to hs_activate_backward's (g o)(1 - o) and g s:
    on 4 10^6 values with log scales in [-20, 5] (beyond them s s leaves the float32 range and the identity ends)."""
    rng = np.random.default_rng(11)
    n = 4_000_000 // 3
    x = np.concatenate([3.0 * rng.standard_normal(n - len(R.SPECIAL_LOGITS)), np.array(R.SPECIAL_LOGITS)]).astype(np.float32)
    l = rng.uniform(-20.0, 5.0, size=(n, 3)).astype(np.float32)
    o, s, _ = A.activate(x, l)
    fwd = R.apply(x, l, np.zeros(n, np.float32))
    assert R.same_bits(fwd["sp"], s) and R.same_bits(fwd["oc"], o)
    assert (fwd["r"] == 1).all() and (fwd["t"] == 0).all() and (fwd["c"] == 1).all()
    g_o, g_s = rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    g_s[::7] = -0.0                                     # a -0.0 gradient stays -0.0: nothing is added where t == 0
    want = A.backward(g_o, o, g_s, s)
    d_o, d_s = R.backward(g_o, g_s, fwd)
    assert R.same_bits(d_o, want[0]) and R.same_bits(d_s, want[1])


def test_the_v_equals_zero_rule_and_the_special_rows():
    inf = np.inf
    x = np.array([0.0, 100.0, -100.0, -88.0, 2.0], np.float32)
    l = np.array([[-inf, 0.0, 1.0], [-inf, -inf, -inf], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-inf, 0.0, 0.0]], np.float32)
    f = np.array([0.0, 0.0, 1.0, 1.0, 0.5], np.float32)
    for dtype in (np.float32, np.float64):
        w = R.apply(x, l, f, dtype)
        assert w["sp"][0, 0] == 0 and w["r"][0, 0] == 1 and w["t"][0, 0] == 0 and w["c"][0] == 1 and w["oc"][0] == 0.5
        assert (w["sp"][1] == 0).all() and w["oc"][1] == 1.0
        assert (w["oc"][2] == 0.0 if dtype is np.float32 else 0 < w["oc"][2] < 1e-43) and np.allclose(w["sp"][2], np.sqrt(2.0)) and np.allclose(w["c"][2], 0.5 ** 1.5)
        # s = 0 under a filter: the Gaussian is the filter's ball and carries no opacity
        assert w["sp"][4, 0] == 0.5 and w["r"][4, 0] == 0 and w["t"][4, 0] == 1 and w["oc"][4] == 0
        d_o, d_s = R.backward(np.ones(5), np.ones((5, 3)), w, dtype)
        assert np.isfinite(d_o).all() and np.isfinite(d_s).all() and d_s[0, 0] == 0 and (d_s[1] == 0).all()
    assert 0 < R.apply(x, l, f)["oc"][3] < 2.0 ** -126            # denormal: what the floor of the opacity bar is for


def test_reference_backward_is_the_derivative_of_the_forward():
    """Central differences of the float64 forward, contracted with g, against the float64 chain rule (on float64 forward
    values): a wrong formula does not pass; a rounding order does.  And the per-axis form equals the published one."""
    rng = np.random.default_rng(5)
    n = 64
    x, l = rng.normal(0, 2, n), rng.uniform(-4, 2, (n, 3))
    f = np.exp(rng.uniform(-4, 1, n))
    g_o, g_s = rng.standard_normal(n), rng.standard_normal((n, 3))
    D = np.float64
    fwd = R.apply(x, l, f, D)
    d_o, d_s = R.backward(g_o, g_s, fwd, D)

    def loss(x_, l_):
        w = R.apply(x_, l_, f, D)
        return w["oc"] * g_o + (w["sp"] * g_s).sum(axis=1)

    h = 1e-6
    assert np.allclose(d_o, (loss(x + h, l) - loss(x - h, l)) / (2 * h), rtol=1e-7, atol=1e-9)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        assert np.allclose(d_s[:, k], (loss(x, l + e) - loss(x, l - e)) / (2 * h), rtol=1e-7, atol=1e-9), k
    # the published form: scales sqrt(s^2 + f^2), coefficient sqrt(det(S^2) / det(S^2 + f^2 I))
    s2 = np.exp(l) ** 2
    assert np.allclose(fwd["sp"], np.sqrt(s2 + f[:, None] ** 2), rtol=1e-14)
    assert np.allclose(fwd["oc"], 1 / (1 + np.exp(-x)) * np.sqrt(s2.prod(axis=1) / (s2 + f[:, None] ** 2).prod(axis=1)), rtol=1e-13)
    assert np.allclose(fwd["t"], 1 - fwd["r"], atol=1e-15)


def _look_at_z(offset):
    """Transposed view matrix (16 floats) of a camera at `offset` looking down +z."""
    m = np.eye(4, dtype=np.float32)
    m[3, :3] = -np.asarray(offset, np.float32)
    return m.reshape(16)


def test_reference_filter_an_unseen_gaussian_takes_the_largest_seen_distance():
    views = np.stack([_look_at_z((0, 0, 0)), _look_at_z((0, 0, -1))])
    intr = np.array([[100, 100, 64, 48], [140, 120, 64, 48]], np.float32)
    xyz = np.array([[0, 0, 2], [0, 0, 5], [0, 0, -3], [40, 0, 1], [0, 0, 0.1], [np.nan, 0, 2]], np.float32)
    filt, n = R.filter_3d(xyz, views, intr)
    assert n.tolist() == [2, 2, 0, 0, 1, 0]         # behind both; far outside the margin; inside camera 0's near plane; NaN
    # (fmax is the larger fx)
    want = [np.float32(d) / np.float32(140.0) * R.SQRT_FIFTH for d in (2.0, 5.0, 5.0, 5.0, np.float32(0.1) + np.float32(1.0), 5.0)]
    assert R.same_bits(filt, np.array(want, np.float32))
    # nothing seen, or no camera: zeros
    for v, k in ((views, intr), (views[:0], intr[:0])):
        filt, n = R.filter_3d(xyz[2:4], v, k)
        assert filt.tolist() == [0, 0] and n.tolist() == [0, 0] and filt.dtype == np.float32


# ---- C ABI ----

def test_smoothing_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    assert "hs_smoothing_filter_args" in header and "hs_smoothing_apply_args" in header
    assert set(NAMES) <= set(lib.EXPORTS)
    assert set(re.findall(r"\b(hs_[a-z_]+)\s*\(", header)) == set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309 == lib.HS_VERSION       # (detected by name: the version does not move)


def test_smoothing_structs_match_c(lib, tmp_path):
    lines = []
    want = []
    for S in (lib.hs_smoothing_filter_args, lib.hs_smoothing_apply_args):
        fields = [n for n, _ in S._fields_]
        lines += [f'printf("%zu\\n", sizeof({S.__name__}));'] + [f'printf("%zu\\n", offsetof({S.__name__}, {n}));' for n in fields]
        want += [C.sizeof(S)] + [getattr(S, n).offset for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want


def test_workspace_bytes_is_monotone_and_bounded(lib):
    L = lib.load()
    last = 0
    for P in (0, 1, 255, 256, 257, 1000, 4097, 65536, 524287, 524288, 524289, 10 ** 6, 10 ** 8, (1 << 30) - 1):
        b = L.hs_smoothing_filter_workspace_bytes(P)
        assert b >= last and b % 256 == 0 and b >= 8 * min((P + 255) // 256, 2048), (P, b)
        last = b
    assert last == 8 * 2048                                       # the grid is capped: the workspace stops growing
    for P in (-1, 1 << 30):
        assert L.hs_smoothing_filter_workspace_bytes(P) == lib.HS_EINVAL and f"P={P}".encode() in L.hs_last_error()


def test_smoothing_validates_before_touching_the_gpu(lib):
    """Every argument error of the three entry points is HS_EINVAL with a message that names the field, and the no-ops
    succeed -- on a machine without a GPU: no HIP call is made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy address: validation must fail before it is dereferenced

    def filt(**kw):
        a = lib.hs_smoothing_filter_args()
        a.P, a.C = 100, 3
        for k in ("xyz", "viewmatrices", "intrinsics", "filter", "n_views", "workspace"):
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.hs_smoothing_filter(C.byref(a), None), L.hs_last_error()

    def app(fn, **kw):
        a = lib.hs_smoothing_apply_args()
        a.P, a.g_begin, a.g_end = 100, 0, 100
        for k in ("opacity_raw", "scales_raw", "filter", "opacities", "scales", "dL_dopacities", "dL_dscales"):
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, fn)(C.byref(a), None), L.hs_last_error()

    for fn in NAMES[1:]:
        assert getattr(L, fn)(None, None) == lib.HS_EINVAL and L.hs_last_error() == f"{fn}: null args".encode()
    cases = [(dict(P=-1), b"P=-1"), (dict(P=1 << 30), b"P=1073741824"), (dict(C=-1), b"C=-1"), (dict(C=1 << 20), b"C=1048576"),
             (dict(xyz=None), b"null xyz"), (dict(viewmatrices=None), b"null viewmatrices"),
             (dict(intrinsics=None), b"null intrinsics"), (dict(filter=None), b"null filter"),
             (dict(workspace=None), b"null workspace"), (dict(xyz=one + 2), b"xyz must be 4-byte aligned"),
             (dict(viewmatrices=one + 1), b"viewmatrices must be 4-byte aligned"),
             (dict(intrinsics=one + 3), b"intrinsics must be 4-byte aligned"), (dict(filter=one + 2), b"filter must be 4-byte aligned"),
             (dict(n_views=one + 2), b"n_views must be 4-byte aligned"), (dict(workspace=one + 128), b"workspace must be 256-byte aligned"),
             (dict(workspace=one + 4), b"workspace must be 256-byte aligned")]
    for kw, text in cases:
        rc, msg = filt(**kw)
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_smoothing_filter:") and text in msg, (kw, rc, msg)
    # no-ops: an empty cloud looks at no pointer
    assert filt(P=0, xyz=None, filter=None, workspace=None, viewmatrices=None, intrinsics=None, n_views=None)[0] == lib.HS_OK
    assert filt(P=0, C=0)[0] == lib.HS_OK

    fwd = [(dict(P=-1), b"P=-1"), (dict(P=1 << 30), b"P=1073741824"), (dict(opacity_raw=None), b"null opacity_raw"),
           (dict(scales_raw=None), b"null scales_raw"), (dict(filter=None), b"null filter"), (dict(opacities=None), b"null opacities"),
           (dict(scales=None), b"null scales"), (dict(opacity_raw=one + 2), b"opacity_raw must be 4-byte aligned"),
           (dict(scales_raw=one + 1), b"scales_raw must be 4-byte aligned"), (dict(filter=one + 3), b"filter must be 4-byte aligned"),
           (dict(opacities=one + 2), b"opacities must be 4-byte aligned"), (dict(scales=one + 1), b"scales must be 4-byte aligned")]
    bwd = [(dict(P=-1), b"P=-1"), (dict(P=1 << 30), b"P=1073741824"), (dict(g_end=101), b"g_end=101"), (dict(g_begin=-1), b"g_begin=-1"),
           (dict(g_begin=60, g_end=50), b"g_begin=60, g_end=50"), (dict(P=0), b"g_end=100"),
           (dict(opacity_raw=None), b"null opacity_raw"), (dict(scales_raw=None), b"null scales_raw"), (dict(filter=None), b"null filter"),
           (dict(dL_dopacities=None), b"null dL_dopacities"), (dict(dL_dscales=None), b"null dL_dscales"),
           (dict(opacity_raw=one + 2), b"opacity_raw must be 4-byte aligned"), (dict(scales_raw=one + 2), b"scales_raw must be 4-byte aligned"),
           (dict(filter=one + 1), b"filter must be 4-byte aligned"), (dict(dL_dopacities=one + 1), b"dL_dopacities must be 4-byte aligned"),
           (dict(dL_dscales=one + 3), b"dL_dscales must be 4-byte aligned")]
    for fn, cs in ((NAMES[2], fwd), (NAMES[3], bwd)):
        for kw, text in cs:
            rc, msg = app(fn, **kw)
            assert rc == lib.HS_EINVAL and msg.startswith(fn.encode() + b":") and text in msg, (fn, kw, rc, msg)
    nothing = dict(opacity_raw=None, scales_raw=None, filter=None, opacities=None, scales=None, dL_dopacities=None, dL_dscales=None)
    assert app(NAMES[2], P=0, **nothing)[0] == lib.HS_OK
    assert app(NAMES[3], P=0, g_begin=0, g_end=0, **nothing)[0] == lib.HS_OK
    assert app(NAMES[3], g_begin=37, g_end=37, **nothing)[0] == lib.HS_OK
    # the backward reads no activated tensor, the forward no gradient: their absence is not an error of the other call
    assert b"null" in app(NAMES[3], opacities=None, scales=None, filter=None)[1] and b"filter" in L.hs_last_error()
    assert b"null filter" in app(NAMES[2], dL_dopacities=None, dL_dscales=None, filter=None)[1]


# ---- Python ----

def test_compute_filter_argument_errors():
    from casualhdrsplat_amd import compute_filter_3D
    from casualhdrsplat_amd import smoothing
    xyz, views = torch.zeros(10, 3), torch.eye(4).repeat(3, 1, 1)
    with pytest.raises(TypeError, match="must be torch.Tensors"):
        compute_filter_3D(xyz.numpy(), views, 100.0, 100.0, 64, 48)
    with pytest.raises(TypeError, match="xyz must be float32"):
        compute_filter_3D(xyz.double(), views, 100.0, 100.0, 64, 48)
    with pytest.raises(TypeError, match="viewmatrices must be float32"):
        compute_filter_3D(xyz, views.double(), 100.0, 100.0, 64, 48)
    with pytest.raises(ValueError, match=r"xyz must have shape \[P, 3\]"):
        compute_filter_3D(torch.zeros(10, 4), views, 100.0, 100.0, 64, 48)
    with pytest.raises(ValueError, match="viewmatrices must have shape"):
        compute_filter_3D(xyz, torch.zeros(3, 3, 4), 100.0, 100.0, 64, 48)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_filter_3D(xyz, views, 100.0, 100.0, 64, 48)
    # intrinsics: a scalar, or one value per camera
    assert smoothing._per_camera("focal_x", 3, 4, torch.device("cpu")).tolist() == [3.0] * 4
    assert smoothing._per_camera("focal_x", [1, 2, 3], 3, torch.device("cpu")).tolist() == [1.0, 2.0, 3.0]
    assert smoothing._per_camera("width", torch.tensor([[5, 6], [7, 8]]), 4, torch.device("cpu")).tolist() == [5.0, 6.0, 7.0, 8.0]
    with pytest.raises(ValueError, match="focal_y holds 2 values for 3 cameras"):
        smoothing._per_camera("focal_y", [1.0, 2.0], 3, torch.device("cpu"))


def _settings():
    from casualhdrsplat_amd import GaussianRasterizationSettings, synthetic as S
    sc = S.make_scene(50, 64, 48, 1, seed=2)
    cam = sc.camera
    rs = GaussianRasterizationSettings(image_height=cam.H, image_width=cam.W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=sc.bg,
                                       scale_modifier=1.0, viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix,
                                       sh_degree=sc.sh_degree, campos=cam.campos)
    return sc, rs


def test_rasterizer_filter_argument_errors():
    """The checks that run before any device call: CPU tensors get as far as the filter's own validation."""
    from casualhdrsplat_amd import GaussianRasterizer
    sc, rs = _settings()
    P = sc.means3D.shape[0]
    good = torch.full((P,), 0.01)
    assert GaussianRasterizer(rs, parameterization="raw").filter_3D is None
    assert GaussianRasterizer(rs, parameterization="raw", filter_3D=good).filter_3D is good
    with pytest.raises(ValueError, match="filter_3D needs parameterization='raw'"):
        GaussianRasterizer(rs, filter_3D=good)
    args = (sc.means3D, torch.zeros_like(sc.means3D), torch.logit(sc.opacities.clamp(1e-3, 1 - 1e-3)))
    kw = dict(shs=sc.shs, scales=sc.scales.log(), rotations=sc.rotations * 3.0)
    late = GaussianRasterizer(rs)               # the attribute set later on an "activated" rasterizer: the call raises
    late.filter_3D = good
    with pytest.raises(ValueError, match="filter_3D needs parameterization='raw'"):
        late(*args, **kw)
    rast = GaussianRasterizer(rs, parameterization="raw", filter_3D=good)
    with pytest.raises(ValueError, match="cannot be combined with cov3D_precomp"):
        rast(*args, shs=sc.shs, cov3D_precomp=torch.zeros(P, 6))
    bad = [(torch.full((P + 1,), 0.01), "must have shape"), (torch.full((P, 2), 0.01), "must have shape"),
           (torch.full((1, P), 0.01), "must have shape"), (good.double(), "must be float32"), (good.numpy(), "must be a torch.Tensor"),
           (torch.full((P, 2), 0.01)[:, 0], "must be contiguous"), (good.clone().requires_grad_(True), "must not require grad")]
    for f, text in bad:
        rast.filter_3D = f
        with pytest.raises(ValueError, match=text):
            rast(*args, **kw)
    # a good filter ([P] or [P, 1]) passes its checks; CPU tensors then stop where they always did
    for f in (good, good.reshape(P, 1)):
        rast.filter_3D = f
        with pytest.raises(RuntimeError, match="tensors must live on a cuda"):
            rast(*args, **kw)


def test_example_and_writer_argument_errors(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_synthetic_smoothing", os.path.join(ROOT, "examples", "train_synthetic.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    with pytest.raises(ValueError, match="needs mcmc=True"):
        ex.run(P=100, steps=1, filter_3d=True, device="cpu")
    assert ex.main.__module__ and "--filter-3d" in open(os.path.join(ROOT, "examples", "train_synthetic.py")).read()
    from casualhdrsplat_amd import scene_io
    cloud = scene_io.init_from_points(np.random.default_rng(0).standard_normal((20, 3)), np.full((20, 3), 0.5), sh_degree=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene_io.save_ply(str(tmp_path / "f.ply"), cloud, filter_3D=torch.zeros(20))
    scene_io.save_ply(str(tmp_path / "plain.ply"), cloud)          # without a filter: what it always wrote
    back = scene_io.load_ply(str(tmp_path / "plain.ply"))
    assert torch.equal(back.log_scales, cloud.log_scales) and torch.equal(back.opacity_logit, cloud.opacity_logit)


# ---- resources ----

def test_smoothing_kernels_spill_nothing_keep_denormals_and_use_no_atomics(tmp_path):
    """From the compiler's resource report and the code object, built with the flags of the Makefile's EXACT recipes: four
    kernels, no spills, no scratch, fp32 denormals kept, IEEE divides and roots, 16-byte accesses in the apply kernels, LDS in
    the filter's two kernels only, no atomics anywhere."""
    src = os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "smoothing.hip")
    asm = str(tmp_path / "smoothing.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-fvisibility=hidden", "-std=c++17",
                        "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", src, "-o", asm],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert len(out) == 4 and sum("smoothing_apply_kernel" in k for k in out) == 2, sorted(out)
    assert sum("smoothing_depth_kernel" in k for k in out) == 1 and sum("smoothing_radius_kernel" in k for k in out) == 1
    for k, v in out.items():
        print(k, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
        assert (v["LDS Size"] == 0) == ("apply" in k), (k, v)
        assert v["Occupancy"] >= 4, (k, v)
    text = open(asm).read()
    assert re.findall(r"\.amdhsa_float_denorm_mode_32 (\d+)", text) == ["3"] * 4
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0"] * 4
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text and "ds_read_b128" in text
    assert "v_div_fixup_f32" in text and "v_div_scale_f32" in text and "v_sqrt_f32" in text and "v_exp_f32" in text
    assert "atomic" not in text and "scratch_" not in text
    source = open(src, encoding="utf-8").read()
    assert not re.search(r"hipMem(set|cpy)\w*", source) and not re.search(r"\batomic\w*\(", source)
    assert not re.search(r"hip(Malloc|Free|StreamSynchronize|DeviceSynchronize)\w*", source)
