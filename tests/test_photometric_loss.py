"""CPU checks of the fused L1 + D-SSIM loss (loss.hip, hs_photometric_loss*, casualhdrsplat_amd.losses): the fp64 restatement
of the published loss the GPU tests hold the kernels to, the C ABI (exports, struct layout, workspace arithmetic, argument
validation before any HIP call), the Python argument errors, and the kernels' register budget."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest
import torch

import loss_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_loss_workspace_bytes", "hs_photometric_loss", "hs_photometric_loss_backward")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- the restatement ----

def test_ssim_of_an_image_with_itself_is_one_with_zero_gradient():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(3, 23, 31, generator=g, dtype=torch.float64)
    xx = x.clone().requires_grad_(True)
    s = R.ssim_map(xx, x).mean()
    s.backward()
    assert abs(float(s.detach()) - 1.0) < 1e-14
    assert float(xx.grad.abs().max()) < 1e-12


def test_constant_images_give_the_closed_form_in_the_interior():
    """(2ab + C1) / (a^2 + b^2 + C1) -- exactly so once the window's sum s (1 within the fp32 rounding of the published
    window: sigma = a^2 s (1 - s) is not quite 0) is accounted for."""
    a, b = 0.3, 0.7
    m = R.ssim_map(torch.full((2, 20, 24), a, dtype=torch.float64), torch.full((2, 20, 24), b, dtype=torch.float64))
    inner = m[..., 5:-5, 5:-5]
    want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
    assert float((inner - want).abs().max()) < 1e-4, (float(inner.min()), want)
    s = float(R.window_2d(1, torch.float64).sum())
    m1, m2 = a * s, b * s
    s1, s2, s12 = a * a * s - m1 * m1, b * b * s - m2 * m2, a * b * s - m1 * m2
    exact = (2 * m1 * m2 + R.C1) * (2 * s12 + R.C2) / ((m1 * m1 + m2 * m2 + R.C1) * (s1 + s2 + R.C2))
    assert float((inner - exact).abs().max()) < 1e-10
    assert float((m[..., 0, 0] - want).abs().max()) > 1e-3       # (the zero padding reaches the corners)


def test_separable_and_2d_windows_agree_in_fp64():
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 3, 37, 29, generator=g, dtype=torch.float64)
    y = (x + 0.1 * torch.randn(x.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    a, b = R.ssim_map(x, y, outer_in_dtype=True), R.ssim_map(x, y, separable=True)
    assert float((a - b).abs().max()) < 1e-12
    # ... and the published window (outer product rounded to fp32) is the same up to that rounding
    assert float((R.ssim_map(x, y) - b).abs().max()) < 1e-7


def test_1d_window_is_the_published_one():
    g = R.gaussian_1d()
    assert g.dtype == torch.float32 and g.shape == (11,)
    assert abs(float(g.double().sum()) - 1.0) < 1e-6 and torch.equal(g, g.flip(0)) and int(g.argmax()) == 5


# ---- C ABI ----

def test_loss_symbols_are_exported_by_both_libraries(lib):
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert set(NAMES) <= set(lib.EXPORTS)


def test_loss_args_layout_matches_c(lib, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\n'
                   'int main(){printf("%zu %zu %zu %zu\\n", sizeof(hs_loss_args), offsetof(hs_loss_args, lambda_dssim),'
                   'offsetof(hs_loss_args, image), offsetof(hs_loss_args, dL_dimage));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = lib.hs_loss_args
    assert got == [C.sizeof(A), A.lambda_dssim.offset, A.image.offset, A.dL_dimage.offset]


@pytest.mark.parametrize("planes,H,W", [(1, 1, 1), (3, 5, 7), (3, 1080, 1920), (6, 50, 70), (1, 16, 64), (1, 17, 65),
                                        (7, 333, 129)])
def test_workspace_bytes_are_the_stated_arithmetic(lib, planes, H, W):
    L = lib.load()
    tiles = planes * (-(-H // 16)) * (-(-W // 64))
    pairs = -(-16 * tiles // 256) * 256
    assert L.hs_loss_workspace_bytes(planes, H, W, 0) == pairs
    assert L.hs_loss_workspace_bytes(planes, H, W, 1) == pairs + 12 * planes * H * W


def test_loss_entries_validate_before_touching_the_gpu(lib):
    L = lib.load()
    one = 4096   # non-null dummy addresses: validation must fail before any of them is dereferenced

    def args(**kw):
        a = lib.hs_loss_args()
        a.planes, a.H, a.W, a.lambda_dssim = 3, 32, 48, 0.2
        a.image = a.target = a.partials = a.out = a.dL_dloss = a.dL_dimage = one
        a.workspace = 4096
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    fwd, bwd = L.hs_photometric_loss, L.hs_photometric_loss_backward
    assert fwd(None, None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    assert bwd(None, None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    bad = [dict(planes=0), dict(H=0), dict(W=0), dict(planes=-2), dict(planes=1 << 11, H=1 << 10, W=1 << 10),
           dict(lambda_dssim=-0.01), dict(lambda_dssim=1.5), dict(lambda_dssim=float("nan"))]
    for kw in bad:
        for f, who in ((fwd, b"hs_photometric_loss"), (bwd, b"hs_photometric_loss_backward")):
            L.hs_last_error()
            assert f(C.byref(args(**kw)), None) == lib.HS_EINVAL, (kw, who)
            msg = L.hs_last_error()
            assert msg.startswith(who) and (b"shape" in msg or b"lambda" in msg), (kw, msg)
    for field in ("image", "target", "workspace", "out"):
        assert fwd(C.byref(args(**{field: None})), None) == lib.HS_EINVAL, field
        assert b"null" in L.hs_last_error()
    assert fwd(C.byref(args(workspace=4096 + 16)), None) == lib.HS_EINVAL and b"aligned" in L.hs_last_error()
    for field in ("image", "target", "partials", "dL_dloss", "dL_dimage"):
        assert bwd(C.byref(args(**{field: None})), None) == lib.HS_EINVAL, field
        assert b"null" in L.hs_last_error()
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1 << 11, 1 << 10, 1 << 10)):
        assert L.hs_loss_workspace_bytes(*shape, 1) == lib.HS_EINVAL
        assert b"hs_loss_workspace_bytes" in L.hs_last_error()
    # the largest admitted problem: planes * H * W = 2^31 - 1
    assert L.hs_loss_workspace_bytes(1, 1, (1 << 31) - 1, 0) > 0


# ---- Python ----

def test_python_argument_errors():
    from casualhdrsplat_amd import losses, photometric_loss, ssim
    assert losses.photometric_loss is photometric_loss and losses.ssim is ssim
    x = torch.rand(3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        photometric_loss(x, x.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ssim(x, x.clone())
    with pytest.raises(TypeError, match="float32"):
        photometric_loss(x.half(), x.half())
    with pytest.raises(TypeError, match="float32"):
        photometric_loss(x, x.double())
    with pytest.raises(ValueError, match="shape"):
        photometric_loss(x, torch.rand(3, 8, 9))
    with pytest.raises(ValueError, match=r"\[C, H, W\]"):
        photometric_loss(torch.rand(8, 8), torch.rand(8, 8))
    with pytest.raises(ValueError, match="target requires grad"):
        photometric_loss(x, x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="lambda_dssim"):
        photometric_loss(x, x.clone(), lambda_dssim=1.2)


# ---- resources ----

def test_loss_kernels_have_no_spill_and_no_scratch():
    src = os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "loss.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-fvisibility=hidden", "-std=c++17",
                            "-ffp-contract=fast", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                            "-o", os.path.join(tmp, "x.o")], capture_output=True, text=True, timeout=600)
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
    names = sorted(out)
    assert sum("loss_fwd_kernel" in k for k in names) == 2 and any("loss_bwd_kernel" in k for k in names) and \
        any("loss_reduce_kernel" in k for k in names), names
    for k, v in out.items():
        assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 2, (k, v)
