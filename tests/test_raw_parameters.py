"""CPU checks of the stored parameterisation of the rasterizer (activate.hip, hs_activate / hs_activate_backward,
GaussianRasterizer(..., parameterization="raw")): the numpy restatement the GPU tests compare with
(tests/activation_reference.py) against float64 and the bars that follow from it, the C ABI (exports, struct layout, argument
validation before any HIP call), the Python argument errors, and the kernels' resources."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import activation_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_activate", "hs_activate_backward")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- the restatement against float64 ----

def test_bars_are_twice_the_measured_constants():
    """The float32 restatement against the float64 evaluation of the same formulas on 10^6 seeded rows (logits N(0, 3) plus
    the rows +-17, +-30, +-88, +-100 and 0; log scales U(-9, 3); quaternions N(0, 1) e^U(-3, 3)): each bar the GPU tests use
    is twice the constant measured here, rounded up to a power of two.  The constants are recorded in the reference module;
    those that do not involve the host's expf are IEEE arithmetic and are held to two decimals."""
    x, l, q, g = R.inputs()
    assert x.shape == (R.ROWS + len(R.SPECIAL_LOGITS),) and l.shape == (R.ROWS, 3) and q.shape == (R.ROWS, 4)
    act = R.activate(x, l, q)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in act)
    gs = (g["opacities"], g["scales"], g["rotations"])
    grads = R.backward(gs[0], act[0], gs[1], act[1], gs[2], act[2], q)
    assert all(d.dtype == np.float32 and np.isfinite(d).all() for d in grads)
    c = dict(R.forward_constants(x, l, q, act), **R.backward_constants(gs, act, q, grads))
    assert set(c) == set(R.BARS) == set(R.MEASURED)
    for k, v in c.items():
        print(f"{k}: c = {v:.4f} (recorded {R.MEASURED[k]}, bar {R.BARS[k]})")
    for k, v in c.items():
        assert R.BARS[k] == R.bar_of(v), (k, v)
        tol = 0.1 * R.MEASURED[k] if k in R.USES_EXP else 0.01
        assert abs(v - R.MEASURED[k]) <= tol, (k, v)


def test_reference_special_rows_and_the_clamp_rule():
    o, _, _ = R.activate(x=np.array(R.SPECIAL_LOGITS, np.float32))
    assert o[-1] == 0.5 and o[6] == 1.0 and o[7] == 0.0 and 0 < o[5] < 2.0 ** -126      # x = 0, 100, -100, -88 (denormal)
    # a zero quaternion stays zero (0 / 1e-12) and its gradient is g / 1e-12: the gradient of q / eps
    q = np.array([[0, 0, 0, 0], [3e-13, 0, 0, 0], [0, 2, 0, 0]], np.float32)
    g = np.array([[1, -2, 3, 4], [1, 1, 1, 1], [1, 1, 1, 1]], np.float32)
    _, _, u = R.activate(q=q)
    assert np.array_equal(u[0], [0, 0, 0, 0]) and u[1, 0] == np.float32(3e-13) / np.float32(1e-12) and u[2, 1] == 1.0
    _, _, d = R.backward(g_q=g, qhat=u, q=q)
    assert R.same_bits(d[:2], g[:2] / np.float32(1e-12))
    assert np.array_equal(d[2], [0.5, 0.0, 0.5, 0.5])          # the component along q is projected out, the rest divided by |q|
    # float64 on the same inputs: the same rule
    _, _, d64 = R.backward(g_q=g, qhat=u, q=q, dtype=np.float64)
    assert d64.dtype == np.float64 and np.allclose(d64[:2], g[:2].astype(np.float64) / float(np.float32(1e-12)), rtol=1e-15)


def test_reference_backward_is_the_derivative_of_the_forward():
    """Central differences of the float64 forward, contracted with g, against the float64 backward (on float64 activated
    values): a wrong formula does not pass; a rounding order does."""
    rng = np.random.default_rng(5)
    x, l = rng.normal(0, 2, 64), rng.uniform(-4, 2, (64, 3))
    q = rng.standard_normal((64, 4)) * np.exp(rng.uniform(-2, 2, (64, 1)))
    g = (rng.standard_normal(64), rng.standard_normal((64, 3)), rng.standard_normal((64, 4)))
    act = R.activate(x, l, q, np.float64)
    d = R.backward(g[0], act[0], g[1], act[1], g[2], act[2], q, np.float64)
    h = 1e-6
    num_o = (R.activate(x=x + h, dtype=np.float64)[0] - R.activate(x=x - h, dtype=np.float64)[0]) / (2 * h) * g[0]
    num_s = (R.activate(l=l + h, dtype=np.float64)[1] - R.activate(l=l - h, dtype=np.float64)[1]) / (2 * h) * g[1]
    assert np.allclose(d[0], num_o, rtol=1e-7, atol=1e-9) and np.allclose(d[1], num_s, rtol=1e-7, atol=1e-9)
    num_q = np.zeros_like(q)
    for k in range(4):
        e = np.zeros(4)
        e[k] = h
        diff = (R.activate(q=q + e, dtype=np.float64)[2] - R.activate(q=q - e, dtype=np.float64)[2]) / (2 * h)
        num_q[:, k] = (diff * g[2]).sum(axis=1)
    assert np.allclose(d[2], num_q, rtol=1e-6, atol=1e-8)
    # ... and torch's own activations agree with the float64 forward
    t = torch.from_numpy
    assert np.allclose(torch.sigmoid(t(x)).numpy(), act[0], rtol=1e-14) and np.allclose(torch.exp(t(l)).numpy(), act[1], rtol=1e-14)
    assert np.allclose(torch.nn.functional.normalize(t(q)).numpy(), act[2], rtol=1e-14)


# ---- C ABI ----

def test_activate_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    assert "hs_activate_args" in header
    assert set(NAMES) <= set(lib.EXPORTS)
    # header functions == EXPORTS still holds with the two new names
    assert set(re.findall(r"\b(hs_[a-z_]+)\s*\(", header)) == set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309 == lib.HS_VERSION       # (detected by name: the version does not move)


def test_activate_struct_matches_c(lib, tmp_path):
    A = lib.hs_activate_args
    fields = [n for n, _ in A._fields_]
    assert fields == ["P", "g_begin", "g_end", "opacity_raw", "scales_raw", "rotations_raw", "opacities", "scales", "rotations",
                      "dL_dopacities", "dL_dscales", "dL_drotations"]
    lines = ['printf("%zu\\n", sizeof(hs_activate_args));'] + [f'printf("%zu\\n", offsetof(hs_activate_args, {n}));' for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(A)] + [getattr(A, n).offset for n in fields]


def test_activate_validates_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the field, and the no-ops succeed -- on a machine without
    a GPU: no HIP call is made before the arguments are known to be good and there is something to do."""
    L = lib.load()
    one = 4096     # non-null dummy address: validation must fail before it is dereferenced

    def call(fn, **kw):
        a = lib.hs_activate_args()
        a.P, a.g_begin, a.g_end = 100, 0, 100
        for k in ("opacity_raw", "scales_raw", "rotations_raw", "opacities", "scales", "rotations", "dL_dopacities", "dL_dscales",
                  "dL_drotations"):
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, fn)(C.byref(a), None), L.hs_last_error()

    for fn in NAMES:
        assert getattr(L, fn)(None, None) == lib.HS_EINVAL and L.hs_last_error() == f"{fn}: null args".encode()
    fwd = [(dict(P=-1), b"P=-1"), (dict(P=1 << 30), b"P=1073741824"),
           (dict(opacities=None), b"opacity_raw is given but opacities is NULL"),
           (dict(scales=None), b"scales_raw is given but scales is NULL"),
           (dict(rotations=None), b"rotations_raw is given but rotations is NULL"),
           (dict(opacity_raw=one + 2), b"opacity_raw must be 4-byte aligned"), (dict(scales=one + 1), b"scales must be 4-byte aligned")]
    bwd = [(dict(P=-1), b"P=-1"), (dict(g_end=101), b"g_end=101"), (dict(g_begin=-1), b"g_begin=-1"),
           (dict(g_begin=60, g_end=50), b"g_begin=60, g_end=50"), (dict(P=0), b"g_end=100"),
           (dict(opacities=None), b"dL_dopacities is given but opacities is NULL"),
           (dict(scales=None), b"dL_dscales is given but scales is NULL"),
           (dict(rotations=None), b"dL_drotations is given but rotations is NULL"),
           (dict(rotations_raw=None), b"dL_drotations is given but rotations_raw is NULL"),
           (dict(dL_drotations=one + 3), b"dL_drotations must be 4-byte aligned")]
    for fn, cases in ((NAMES[0], fwd), (NAMES[1], bwd)):
        for kw, text in cases:
            rc, msg = call(fn, **kw)
            assert rc == lib.HS_EINVAL, (fn, kw, rc, msg)
            assert msg.startswith(fn.encode() + b":") and text in msg, (fn, kw, msg)
    # successful no-ops: an empty cloud, an empty range, no tensor present (no pointer is looked at, nothing is launched)
    absent = dict(opacity_raw=None, scales_raw=None, rotations_raw=None, dL_dopacities=None, dL_dscales=None, dL_drotations=None)
    assert call(NAMES[0], P=0)[0] == lib.HS_OK
    assert call(NAMES[1], P=0, g_begin=0, g_end=0)[0] == lib.HS_OK
    assert call(NAMES[1], g_begin=37, g_end=37)[0] == lib.HS_OK
    assert call(NAMES[0], **absent)[0] == lib.HS_OK and call(NAMES[1], **absent)[0] == lib.HS_OK


# ---- Python ----

def test_python_argument_errors():
    from casualhdrsplat_amd import GaussianRasterizationSettings, GaussianRasterizer, synthetic as S
    sc = S.make_scene(50, 64, 48, 1, seed=2)
    cam = sc.camera
    rs = GaussianRasterizationSettings(image_height=cam.H, image_width=cam.W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=sc.bg,
                                       scale_modifier=1.0, viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix,
                                       sh_degree=sc.sh_degree, campos=cam.campos)
    # the settings keep their published fields: the parameterisation is the rasterizer's
    assert "parameterization" not in GaussianRasterizationSettings._fields
    assert GaussianRasterizer(rs).parameterization == "activated"
    assert GaussianRasterizer(rs, parameterization="raw").parameterization == "raw"
    for bad in ("logit", "", None, "RAW"):
        with pytest.raises(ValueError, match="parameterization must be one of"):
            GaussianRasterizer(rs, parameterization=bad)
    args = (sc.means3D, torch.zeros_like(sc.means3D), torch.logit(sc.opacities.clamp(1e-3, 1 - 1e-3)))
    kw = dict(shs=sc.shs, scales=sc.scales.log(), rotations=sc.rotations * 3.0)
    msgs = []
    for how in ("activated", "raw"):      # CPU tensors: "raw" raises as the existing path does
        with pytest.raises(RuntimeError, match="tensors must live on a cuda") as e:
            GaussianRasterizer(rs, parameterization=how)(*args, **kw)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        GaussianRasterizer(rs, parameterization="raw")(*args, shs=sc.shs, scales=kw["scales"])


def test_gaussian_cloud_stored_names_the_optimizer_groups():
    from casualhdrsplat_amd import cloud_param_groups, scene_io
    xyz = np.random.default_rng(0).standard_normal((40, 3))
    cloud = scene_io.init_from_points(xyz, np.full((40, 3), 0.5), sh_degree=1)
    st = cloud.stored()
    assert list(st) == ["means3D", "opacities", "shs", "scales", "rotations"]
    assert torch.equal(st["opacities"], cloud.opacity_logit) and torch.equal(st["scales"], cloud.log_scales)
    assert torch.equal(st["rotations"], cloud.rotations) and st["opacities"].data_ptr() != cloud.opacity_logit.data_ptr()
    assert all(t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad for t in st.values())
    groups = cloud_param_groups(**st)
    assert [g["name"] for g in groups] == ["xyz", "opacity", "f_dc", "f_rest", "scaling", "rotation"]
    # the activated tensors are the activations of the stored ones
    act = cloud.activated()
    o, s, r = R.activate(st["opacities"].numpy(), st["scales"].numpy(), st["rotations"].numpy(), np.float64)
    assert np.allclose(act["opacities"].numpy(), o, rtol=1e-6) and np.allclose(act["scales"].numpy(), s, rtol=1e-6)
    assert np.allclose(act["rotations"].numpy(), r, atol=1e-6)


# ---- resources ----

def _resource_report(tu, asm):
    """({kernel: {field: int}}, ISA text) of one translation unit, from hipcc -Rpass-analysis=kernel-resource-usage (as
    test_host_logic._kernel_resources reads it), built with the flags of the Makefile's EXACT recipes."""
    src = os.path.join(ROOT, "casualhdrsplat_amd", "csrc", tu)
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-fvisibility=hidden", "-std=c++17",
                        "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", src,
                        "-o", asm], capture_output=True, text=True, timeout=600)
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
    return out, open(asm).read()


def test_activate_kernels_spill_nothing_need_no_scratch_no_lds_and_keep_denormals(tmp_path):
    """From the compiler's resource report and the code object: the two kernels hold the occupancy adam.hip's update kernel
    has in the SAME compiler's report of adam.hip (read here, not a number written down), spill nothing, use no scratch and
    no LDS, keep fp32 denormals, move 16 bytes per access, divide and take roots as IEEE says."""
    out, text = _resource_report("activate.hip", str(tmp_path / "activate.s"))
    adam, _ = _resource_report("adam.hip", str(tmp_path / "adam.s"))
    adam_update = next(v for k, v in adam.items() if "adam_update_kernel" in k)
    print("adam_update_kernel", adam_update)
    kernels = sorted(re.search(r"activate_\w+?_kernel", k).group() for k in out)
    assert kernels == ["activate_bwd_kernel", "activate_fwd_kernel"], sorted(out)
    for k, v in out.items():
        print(k, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
        assert v["LDS Size"] == 0, (k, v)
        assert v["Occupancy"] >= adam_update["Occupancy"] and v["VGPRs"] <= adam_update["VGPRs"], (k, v, adam_update)
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0", "0"]
    assert re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", text) == ["0", "0"]
    assert re.findall(r"\.amdhsa_float_denorm_mode_32 (\d+)", text) == ["3", "3"]
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text
    assert "v_div_fixup_f32" in text and "v_div_scale_f32" in text and "v_sqrt_f32" in text and "v_exp_f32" in text
    assert "atomic" not in text and "ds_write" not in text and "ds_read" not in text and "scratch_" not in text


def test_activate_source_has_no_memset_or_copy():
    text = open(os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "activate.hip"), encoding="utf-8").read()
    assert not re.search(r"hipMem(set|cpy)\w*", text)
    assert "__shared__" not in text and not re.search(r"\batomic\w*\(", text)
