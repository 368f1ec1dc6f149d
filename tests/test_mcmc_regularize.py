"""CPU checks of the MCMC regularisers (mcmc_reg.hip, hs_mcmc_reg_workspace_bytes / hs_mcmc_regularize,
casualhdrsplat_amd.mcmc.regularize): the C ABI (exports, struct layout, the workspace formula, argument validation before any
HIP call), the Python argument errors, the measurement that fixes the bar of the GPU comparison
(tests/regularize_reference.py), and the kernels' resources."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import regularize_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_mcmc_reg_workspace_bytes", "hs_mcmc_regularize")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- C ABI ----

def test_regularize_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    assert re.search(r"\}\s*hs_mcmc_reg_args\s*;", header)
    assert set(NAMES) <= set(lib.EXPORTS)
    assert set(re.findall(r"\bHS_API\s+[\w\s\*]+?\b(hs_\w+)\s*\(", header)) == set(lib.EXPORTS)      # header == EXPORTS still holds
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309        # (detected by name: the version does not move)


def test_regularize_struct_matches_c(lib, tmp_path):
    A = lib.hs_mcmc_reg_args
    fields = [n for n, _ in A._fields_]
    lines = ['printf("%zu\\n", sizeof(hs_mcmc_reg_args));']
    lines += [f'printf("%zu\\n", offsetof(hs_mcmc_reg_args, {n}));' for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(A)] + [getattr(A, n).offset for n in fields]
    assert fields == ["P", "flags", "reserved", "lambda_opacity", "lambda_scale", "opacities", "scales", "dL_dopacities",
                      "dL_dscales", "loss", "workspace"]


def test_workspace_bytes_is_the_documented_formula(lib):
    L = lib.load()
    for P in (0, 1, 255, 256, 257, 4096, 4097, 10007, 1_000_000, (1 << 30) - 1):
        assert L.hs_mcmc_reg_workspace_bytes(P) == (16 * ((P + 255) // 256) + 255) // 256 * 256, P
    for P in (-1, 1 << 30, 1 << 40):
        assert L.hs_mcmc_reg_workspace_bytes(P) == lib.HS_EINVAL
        assert b"hs_mcmc_reg_workspace_bytes" in L.hs_last_error() and f"P={P}".encode() in L.hs_last_error()


def test_entry_point_validates_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the field -- on a machine without a GPU: no HIP call is
    made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy addresses: validation must fail before any of them is dereferenced

    def call(**kw):
        a = lib.hs_mcmc_reg_args()
        a.P, a.flags, a.lambda_opacity, a.lambda_scale = 100, 3, 0.01, 0.01
        for f in ("opacities", "scales", "dL_dopacities", "dL_dscales", "loss", "workspace"):
            setattr(a, f, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.hs_mcmc_regularize(C.byref(a), None), L.hs_last_error()

    assert L.hs_mcmc_regularize(None, None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    cases = [(dict(P=-1), b"P=-1"), (dict(P=1 << 30), b"P=1073741824"), (dict(flags=4), b"flags=4"), (dict(flags=-1), b"flags=-1"),
             (dict(lambda_opacity=-0.01), b"lambda_opacity=-0.01"), (dict(lambda_opacity=math.nan), b"lambda_opacity="),
             (dict(lambda_opacity=math.inf), b"lambda_opacity=inf"), (dict(lambda_scale=-1.0), b"lambda_scale=-1"),
             (dict(lambda_scale=math.nan), b"lambda_scale="), (dict(lambda_scale=math.inf), b"lambda_scale=inf"),
             (dict(opacities=None), b"null opacities"), (dict(scales=None), b"null scales"),
             (dict(dL_dopacities=None), b"null dL_dopacities"), (dict(dL_dscales=None), b"null dL_dscales"),
             (dict(opacities=one + 2), b"opacities must be 4-byte aligned"), (dict(scales=one + 1), b"scales must be 4-byte aligned"),
             (dict(dL_dopacities=one + 2), b"dL_dopacities must be 4-byte aligned"), (dict(dL_dscales=one + 3), b"dL_dscales must be 4-byte aligned"),
             (dict(loss=one + 2), b"loss must be 4-byte aligned"), (dict(workspace=None), b"null workspace"),
             (dict(workspace=one + 8), b"workspace must be 16-byte aligned"),
             # a gradient array may be NULL only when its lambda is 0, and the values are still read when the loss is asked for
             (dict(lambda_opacity=0.0, dL_dopacities=None, opacities=None), b"null opacities"),
             (dict(lambda_scale=0.0, dL_dscales=None, scales=None), b"null scales")]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == lib.HS_EINVAL, (kw, rc, msg)
        assert msg.startswith(b"hs_mcmc_regularize") and text in msg, (kw, msg)
    # nothing to do: no pointer is looked at, nothing is launched (this machine has no GPU to launch on)
    assert call(P=0, opacities=None, scales=None, dL_dopacities=None, dL_dscales=None, loss=None, workspace=None)[0] == lib.HS_OK
    assert call(lambda_opacity=0.0, lambda_scale=0.0, loss=None, workspace=None, opacities=None, scales=None, dL_dopacities=None,
                dL_dscales=None)[0] == lib.HS_OK


# ---- Python ----

def _host_cloud(monkeypatch, P=12, M=4):
    from casualhdrsplat_amd import cloud_param_groups, optim
    monkeypatch.setattr(optim, "_require_gpu", lambda t, what: None)
    t = {k: torch.zeros(P, *s, requires_grad=True) for k, s in (("means3D", (3,)), ("opacities", (1,)), ("shs", (M, 3)),
                                                                  ("scales", (3,)), ("rotations", (4,)))}
    return t, optim.GaussianAdam(cloud_param_groups(**t), eps=1e-15)


def test_python_raises_on_cpu_tensors_and_bad_arguments(monkeypatch):
    import casualhdrsplat_amd as pkg
    from casualhdrsplat_amd import densify, mcmc
    assert pkg.regularize is mcmc.regularize and "regularize" in pkg.__all__
    t, opt = _host_cloud(monkeypatch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mcmc.regularize(opt)
    with pytest.raises(TypeError, match="GaussianAdam"):
        mcmc.regularize(torch.optim.Adam([t["means3D"]]))
    # with the device guard on the PARAMETERS lifted, what is looked at before the library
    monkeypatch.setattr(densify, "_require_gpu", lambda t, what: None)
    for bad in (-0.01, math.nan, math.inf):
        with pytest.raises(ValueError, match="regularize: opacity_reg"):
            mcmc.regularize(opt, opacity_reg=bad)
        with pytest.raises(ValueError, match="regularize: scale_reg"):
            mcmc.regularize(opt, scale_reg=bad)
    with pytest.raises(ValueError, match="opacities tensor has no .grad: call after backward"):
        mcmc.regularize(opt)
    t["opacities"].grad = torch.zeros(12, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the gradient is a CPU tensor
        mcmc.regularize(opt)
    monkeypatch.setattr(mcmc, "_require_gpu", lambda t, what: None)
    with pytest.raises(ValueError, match="scales tensor has no .grad: call after backward"):
        mcmc.regularize(opt)
    with pytest.raises(ValueError, match="scales tensor has no .grad"):
        mcmc.regularize(opt, opacity_reg=0.0)
    t["scales"].grad = torch.zeros(12, 4)[:, :3]
    with pytest.raises(ValueError, match="contiguous float32"):
        mcmc.regularize(opt)
    # both weights zero and no value asked for: nothing is looked at, the library is not reached
    monkeypatch.setattr(mcmc.L, "load", lambda: pytest.fail("regularize with nothing to do reached the library"))
    t["opacities"].grad = t["scales"].grad = None
    assert mcmc.regularize(opt, opacity_reg=0.0, scale_reg=0.0, value=False) is None


# ---- the bar ----

def test_reg_bar_is_twice_the_measured_constant():
    """The constant of the bound, measured: worst c of the float32 restatement against float64 over the cases the GPU test
    runs (both flag settings, with and without the special rows), gradients and loss terms.  REG_BAR is twice the recorded
    worst, rounded up to a power of two; the restatement stays under half of it."""
    worst = 0.0
    for P in R.SIZES:
        for flags in (R.RAW_OPACITY | R.RAW_SCALES, 0):
            for special in (True, False):
                case = R.make_case(P, special=special)
                f32, f64 = R.regularize(case, flags=flags), R.regularize(case, flags=flags, dtype=np.float64)
                assert f32["g_o"].dtype == f32["g_s"].dtype == f32["loss"].dtype == np.float32
                cs = [R.check(f32[k], f64[k], f64[m], R.REG_BAR / 2, f"P={P} flags={flags} special={special}: {k}")
                      for k, m in (("g_o", "mag_o"), ("g_s", "mag_s"), ("loss", "mag_loss"))]
                print(f"P={P} flags={flags} special={special}: c = {cs[0]:.3f} (opacities) {cs[1]:.3f} (scales) {cs[2]:.3f} (loss)")
                worst = max(worst, *cs)
                if special and P >= 257:       # the special rows are there, and they are not all NaN afterwards
                    assert np.isnan(f64["loss"]).all() and np.isinf(f64["g_s"]).sum() == (3 if flags else 0)
                    assert np.isnan(f64["g_o"]).sum() == 4 and np.isnan(f64["g_s"]).sum() == 11
                else:
                    assert np.isfinite(f64["loss"]).all() and (f64["loss"] > 0).all()
    print(f"worst c = {worst:.3f}; recorded {R.REG_C_MEASURED}; bar {R.REG_BAR}")
    assert worst <= R.REG_BAR / 2
    assert R.REG_BAR == 2.0 ** math.ceil(math.log2(2.0 * R.REG_C_MEASURED))


def test_restatement_is_torch_autograd():
    """The gradient the restatement adds is what torch's autograd adds for lambda_o sigmoid(x).mean() + lambda_s
    exp(s).mean() (and |x|.mean() stored linear), in float64 to 1e-15 relative; the loss terms are those sums."""
    case = R.make_case(10007, special=False)
    for flags in (3, 0):
        ref = R.regularize(case, flags=flags, dtype=np.float64)
        x = torch.tensor(case["opacities"], dtype=torch.float64, requires_grad=True)
        s = torch.tensor(case["scales"], dtype=torch.float64, requires_grad=True)
        terms = (R.LAMBDA_O * (torch.sigmoid(x) if flags else x.abs()).mean(), R.LAMBDA_S * (torch.exp(s) if flags else s.abs()).mean())
        (terms[0] + terms[1]).backward()
        keep = ~np.isnan(case["g_o"])
        want_o = case["g_o"].astype(np.float64) + x.grad.numpy()
        want_s = case["g_s"].astype(np.float64) + s.grad.numpy()
        assert np.allclose(ref["g_o"][keep], want_o[keep], rtol=1e-13, atol=0.0)
        keep = ~np.isnan(case["g_s"])
        assert np.allclose(ref["g_s"][keep], want_s[keep], rtol=1e-13, atol=0.0)
        assert np.allclose(ref["loss"], [float(terms[0].detach()), float(terms[1].detach())], rtol=1e-13, atol=0.0)


def test_special_values_of_the_restatement():
    """Hand-checked rows: sign(0) = 0, a NaN stays in its own element, the sigmoid's tails add nothing, an infinite scale an
    infinite gradient; a lambda of 0 returns the gradient as it came; an empty cloud's terms are zero."""
    case = dict(P=3, opacities=np.array([[0.0], [-104.0], [math.nan]], dtype=np.float32),
                scales=np.array([[0.0, -0.0, math.nan], [math.inf, -math.inf, 1.0], [-2.0, 2.0, 104.0]], dtype=np.float32),
                g_o=np.array([[-0.0], [1e-4], [1e-4]], dtype=np.float32), g_s=np.full((3, 3), 1e-4, dtype=np.float32))
    lin = R.regularize(case, flags=0)
    assert R.same_bits(lin["g_o"][:2], np.array([[0.0], [np.float32(1e-4) + np.float32(0.01 / 3) * np.float32(-1)]], dtype=np.float32))
    assert np.isnan(lin["g_o"][2, 0]) and np.isnan(lin["g_s"][0, 2]) and np.isnan(lin["g_s"]).sum() == 1
    assert lin["g_s"][0, 0] == lin["g_s"][0, 1] == np.float32(1e-4) and lin["g_s"][1, 0] > 1e-4 > lin["g_s"][1, 1]
    raw = R.regularize(case, flags=3)
    assert raw["g_o"][1, 0] == np.float32(1e-4) and raw["g_o"][0, 0] == np.float32(0.01 / 3) * np.float32(0.25)
    assert raw["g_s"][1, 0] == np.inf and raw["g_s"][1, 1] == np.float32(1e-4) and raw["g_s"][2, 2] == np.inf
    assert R.regularize(case, flags=3, dtype=np.float64)["g_s"][2, 2] == np.inf         # the float32 range of the activated scale
    off = R.regularize(case, 0.0, 0.0)
    assert off["g_o"] is not None and R.same_bits(off["g_o"], case["g_o"]) and R.same_bits(off["g_s"], case["g_s"])
    empty = R.regularize(R.make_case(0))
    assert empty["loss"].tolist() == [0.0, 0.0] and empty["g_o"].shape == (0, 1)


# ---- resources ----

def test_regularize_kernels_spill_nothing_and_use_no_atomics(tmp_path):
    src = os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "mcmc_reg.hip")
    asm = str(tmp_path / "mcmc_reg.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-fvisibility=hidden", "-std=c++17",
                        "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", src,
                        "-o", asm], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(asm).read()
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    kernels = sorted(re.search(r"mcmc_reg\w*?_kernel", k).group() for k in out)
    assert kernels == ["mcmc_reg_kernel", "mcmc_reg_sum_kernel"], sorted(out)
    for k, v in out.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 8 and v["LDS Size"] == 4096, (k, v)
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0"] * 2 and "scratch_" not in text
    assert re.findall(r"\.amdhsa_float_denorm_mode_32 (\d+)", text) == ["3"] * 2               # denormals kept
    assert "v_div_fixup_f32" in text                                                           # IEEE division
    assert not re.findall(r"\b(?:global|flat|buffer|ds)_atomic_\w+", text)                     # no atomics at all
    # built without contraction: the command make itself gives for the object (the Makefile's rules are patterns over a table)
    cmd = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "mcmc_reg.o"],
                         capture_output=True, text=True, check=True).stdout
    assert re.findall(r"-ffp-contract=(\w+)", cmd) == ["off"] and " -c mcmc_reg.hip " in cmd, cmd
    body = open(src, encoding="utf-8").read()
    assert not re.search(r"hipMem(set|cpy)\w*\(", body)
    assert not re.search(r"hip(Stream|Device)Synchronize|hipMalloc|hipFree|atomic", re.sub(r"//.*", "", body))
