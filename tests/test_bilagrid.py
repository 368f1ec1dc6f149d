"""CPU checks of the bilateral-grid correction (bilagrid.hip, hs_bilagrid_*, casualhdrsplat_amd.bilagrid): the float64
restatement of tests/bilagrid_reference.py against torch's grid_sample + einsum formulation under autograd, the total
variation against autograd, the C ABI (exports, struct layouts, the workspace formula, every limit, argument validation before
any HIP call), the Python argument errors, the identity initialisation, and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import bilagrid_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_bilagrid_workspace_bytes", "hs_bilagrid_slice", "hs_bilagrid_slice_backward", "hs_bilagrid_tv",
         "hs_bilagrid_tv_backward")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- the definition ----

def torch_slice(image, grids, ids):
    """grid_sample(grids, 2 (x, y, z) - 1, bilinear, border, align_corners=True) followed by the affine; float64, CPU."""
    F, _, H, W = image.shape
    outs = []
    x = ((torch.arange(W, dtype=torch.float64) + 0.5) / W)[None, :].expand(H, W)
    y = ((torch.arange(H, dtype=torch.float64) + 0.5) / H)[:, None].expand(H, W)
    for f, g in enumerate(ids):
        if not 0 <= g < grids.shape[0]:
            outs.append(image[f])
            continue
        r, gg, b = image[f]
        z = 0.299 * r + 0.587 * gg + 0.114 * b
        at = 2.0 * torch.stack([x, y, z], dim=-1) - 1.0
        A = TF.grid_sample(grids[g][None], at[None, None], mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]
        A = A.reshape(3, 4, H, W)
        v = torch.stack([r, gg, b, torch.ones_like(r)])
        outs.append(torch.einsum("ikhw,khw->ihw", A, v))
    return torch.stack(outs)


CASES = [((1, 37, 70, 1, 5, 3, 4), [0]), ((3, 20, 33, 4, 4, 3, 4), [2, 0, 2]), ((2, 17, 31, 2, 1, 1, 1), [1, 0]),
         ((2, 16, 24, 2, 3, 1, 5), [-1, 1]), ((1, 9, 64, 1, 2, 2, 2), [0])]


@pytest.mark.parametrize("shape,ids", CASES)
def test_float64_restatement_is_grid_sample_and_the_affine(shape, ids):
    """Forward, dL_dimage (luma term and clamp convention included) and dL_dgrids of the float64 restatement against torch
    autograd through grid_sample, to 1e-12: clamped luma on both sides, pixels pinned exactly onto the clamp, a size-1 axis,
    a duplicate id, an unused grid and an identity frame are all in the cases."""
    case = R.make_case(*shape, ids=ids)
    img = torch.tensor(case["image"], dtype=torch.float64, requires_grad=True)
    grd = torch.tensor(case["grids"], dtype=torch.float64, requires_grad=True)
    out = torch_slice(img, grd, ids)
    out.backward(torch.tensor(case["d_out"], dtype=torch.float64))
    z = R.luma(case["image"].astype(np.float64).transpose(1, 0, 2, 3), np.float64)
    if shape[4] > 1:
        assert (z < 0).any() and (z > 1).any() and (z == 0).any()
    got = R.slice_forward(case["image"], case["grids"], ids, dtype=np.float64)
    assert np.abs(got - out.detach().numpy()).max() <= 1e-12
    d_img = R.slice_backward_image(case["image"], case["grids"], ids, case["d_out"], dtype=np.float64)
    assert np.abs(d_img - img.grad.numpy()).max() <= 1e-12
    d_grd, mag = R.slice_backward_grids(case["image"], case["grids"], ids, case["d_out"])
    assert np.abs(d_grd - grd.grad.numpy()).max() <= 1e-12
    assert (mag >= np.abs(d_grd) - 1e-12).all()
    for g in range(shape[3]):
        if g not in ids:
            assert not d_grd[g].any() and not mag[g].any()
    for f, g in enumerate(ids):
        if not 0 <= g < shape[3]:
            assert got[f].tobytes() == case["image"][f].astype(np.float64).tobytes()
            assert d_img[f].tobytes() == case["d_out"][f].astype(np.float64).tobytes()


def test_float32_restatement_stays_float32_and_close_to_the_truth():
    case = R.make_case(3, 20, 33, 4, 4, 3, 4, ids=[2, 0, 2])
    f32 = R.slice_forward(case["image"], case["grids"], case["ids"])
    f64 = R.slice_forward(case["image"], case["grids"], case["ids"], dtype=np.float64)
    assert f32.dtype == np.float32 and np.abs(f32 - f64).max() < 1e-5
    b32 = R.slice_backward_image(case["image"], case["grids"], case["ids"], case["d_out"])
    assert b32.dtype == np.float32
    # the identity grid returns the image: weights that sum to one in eight roundings
    ident = R.slice_forward(case["image"], R.identity(4, 4, 3, 4), case["ids"])
    assert np.abs(ident - case["image"]).max() < 1e-6


@pytest.mark.parametrize("shape", [(1, 8, 16, 16), (5, 4, 3, 4), (2, 1, 3, 4), (3, 4, 1, 1), (2, 1, 1, 1)])
def test_tv_restatement_is_torch_autograd(shape):
    G, L, Y, X = shape
    g = (R.identity(G, L, Y, X) + 0.3 * np.random.default_rng(1).standard_normal((G, 12, L, Y, X))).astype(np.float32)
    t = torch.tensor(g, dtype=torch.float64, requires_grad=True)
    want = sum(((t.narrow(ax, 1, n - 1) - t.narrow(ax, 0, n - 1)) ** 2).mean() for ax, n in ((2, L), (3, Y), (4, X)) if n > 1)
    got, grad = R.tv(g)
    if isinstance(want, int):
        assert got == 0.0 and not grad.any()
        return
    want.backward()
    assert abs(got - float(want.detach())) <= 1e-13 * abs(float(want.detach()))
    assert np.abs(grad - t.grad.numpy()).max() <= 1e-13 * np.abs(t.grad.numpy()).max()
    assert R.tv(R.identity(G, L, Y, X))[0] == 0.0


# ---- C ABI ----

def test_bilagrid_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
        assert re.fullmatch(r"hs_[a-z_]+", n)
    assert re.search(r"\}\s*hs_bilagrid_args\s*;", header) and re.search(r"\}\s*hs_bilagrid_tv_args\s*;", header)
    assert set(NAMES) <= set(lib.EXPORTS) and set(NAMES) <= set(lib.SIGNATURES)
    assert set(re.findall(r"\bHS_API\s+[\w\s\*]+?\b(hs_\w+)\s*\(", header)) == set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309        # (detected by name: the version does not move)
    assert int(re.search(r"#define HS_BILAGRID_TV_WORKSPACE_BYTES (\d+)", header).group(1)) == lib.HS_BILAGRID_TV_WORKSPACE_BYTES


@pytest.mark.parametrize("name", ["hs_bilagrid_args", "hs_bilagrid_tv_args"])
def test_bilagrid_structs_match_c(lib, tmp_path, name):
    A = getattr(lib, name)
    fields = [n for n, _ in A._fields_]
    lines = [f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {n}));' for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(A)] + [getattr(A, n).offset for n in fields]
    want = {"hs_bilagrid_args": ["F", "H", "W", "G", "L", "Y", "X", "reserved", "image", "grids", "grid_ids", "out", "dL_dout",
                                 "dL_dimage", "dL_dgrids", "workspace"],
            "hs_bilagrid_tv_args": ["G", "L", "Y", "X", "grids", "tv", "dL_dtv", "dL_dgrids", "workspace"]}
    assert fields == want[name]


GOOD = dict(F=2, H=40, W=72, G=3, L=4, Y=3, X=4)
LIMITS = [(dict(F=0), b"F=0"), (dict(H=0), b"H=0"), (dict(W=-1), b"W=-1"), (dict(G=0), b"G=0"), (dict(L=0), b"L=0"),
          (dict(L=17), b"L=17"), (dict(Y=0), b"Y=0"), (dict(Y=65), b"Y=65"), (dict(X=0), b"X=0"), (dict(X=65), b"X=65"),
          (dict(F=1, H=32768, W=21846), b"3*F*H*W="), (dict(F=1 << 30, H=1 << 30, W=1 << 30), b"3*F*H*W="),
          (dict(G=2731, L=16, Y=64, X=64), b"12*G*L*Y*X=")]


def test_workspace_bytes_is_the_documented_formula(lib):
    L = lib.load()
    shapes = [(1, 1080, 1920, 1, 8, 16, 16), (1, 800, 800, 1, 8, 16, 16), (4, 208, 320, 4, 8, 16, 16), (1, 37, 70, 1, 5, 3, 4),
              (2, 33, 65, 2, 1, 1, 1), (1, 16, 64, 1, 2, 2, 2), (3, 1, 1, 2, 16, 64, 64), (1, 5000, 3, 1, 2, 1, 1),
              (1, 5000, 3, 1, 2, 2, 1), (1, 100000, 7, 1, 1, 64, 1), (1, 32768, 21845, 1, 1, 1, 1), (1, 4, 4, 2730, 16, 64, 64)]
    for s in shapes:
        assert L.hs_bilagrid_workspace_bytes(*s) == R.workspace_bytes(*s), s
    assert R.chunks(1080, 16) == 5 and R.chunks(208, 16) == 2 and R.chunks(37, 3) == 2 and R.chunks(16, 2) == 1
    for kw, text in LIMITS:
        assert L.hs_bilagrid_workspace_bytes(*{**GOOD, **kw}.values()) == lib.HS_EINVAL, kw
        assert b"hs_bilagrid_workspace_bytes" in L.hs_last_error() and text in L.hs_last_error(), (kw, L.hs_last_error())


def test_entry_points_validate_before_touching_the_gpu(lib):
    """Every limit and every pointer error is HS_EINVAL with a message that names the entry point and the field -- on a
    machine without a GPU: no HIP call is made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy addresses: validation must fail before any of them is dereferenced

    def call(fn, **kw):
        a = lib.hs_bilagrid_args()
        for k, v in GOOD.items():
            setattr(a, k, v)
        for f in ("image", "grids", "grid_ids", "out", "dL_dout", "dL_dimage", "dL_dgrids", "workspace"):
            setattr(a, f, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, fn)(C.byref(a), None), L.hs_last_error()

    both = [(kw, t) for kw, t in LIMITS] + [(dict(image=None), b"null image"), (dict(grids=None), b"null grids"),
                                            (dict(grid_ids=None), b"null grid_ids"), (dict(image=one + 2), b"image must be 4-byte aligned"),
                                            (dict(grids=one + 1), b"grids must be 4-byte aligned"),
                                            (dict(grid_ids=one + 2), b"grid_ids must be 4-byte aligned")]
    only = {"hs_bilagrid_slice": [(dict(out=None), b"null out"), (dict(out=one + 2), b"out must be 4-byte aligned")],
            "hs_bilagrid_slice_backward": [(dict(dL_dout=None), b"null dL_dout"), (dict(dL_dout=one + 3), b"dL_dout must be 4-byte aligned"),
                                           (dict(dL_dimage=one + 2), b"dL_dimage must be 4-byte aligned"),
                                           (dict(dL_dgrids=one + 2), b"dL_dgrids must be 4-byte aligned"),
                                           (dict(workspace=None), b"null workspace"),
                                           (dict(workspace=one + 128), b"workspace must be 256-byte aligned")]}
    for fn in ("hs_bilagrid_slice", "hs_bilagrid_slice_backward"):
        assert getattr(L, fn)(None, None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
        for kw, text in both + only[fn]:
            rc, msg = call(fn, **kw)
            assert rc == lib.HS_EINVAL, (fn, kw, rc, msg)
            assert msg.startswith(fn.encode() + b":") and text in msg, (fn, kw, msg)
    # neither gradient asked for: nothing to do, no pointer beyond the checked ones is looked at, nothing is launched
    assert call("hs_bilagrid_slice_backward", dL_dimage=None, dL_dgrids=None, workspace=None)[0] == lib.HS_OK

    def tv(fn, **kw):
        a = lib.hs_bilagrid_tv_args()
        a.G, a.L, a.Y, a.X = 3, 4, 3, 4
        for f in ("grids", "tv", "dL_dtv", "dL_dgrids", "workspace"):
            setattr(a, f, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, fn)(C.byref(a), None), L.hs_last_error()

    lattice = [(kw, t) for kw, t in LIMITS if set(kw) <= {"G", "L", "Y", "X"}]
    assert len(lattice) == 8
    tv_only = {"hs_bilagrid_tv": [(dict(grids=None), b"null grids"), (dict(tv=None), b"null tv"), (dict(workspace=None), b"null workspace"),
                                  (dict(workspace=one + 16), b"workspace must be 256-byte aligned"), (dict(tv=one + 2), b"tv must be 4-byte aligned")],
               "hs_bilagrid_tv_backward": [(dict(grids=None), b"null grids"), (dict(dL_dtv=None), b"null dL_dtv"),
                                           (dict(dL_dgrids=None), b"null dL_dgrids"), (dict(dL_dgrids=one + 1), b"dL_dgrids must be 4-byte aligned")]}
    for fn in ("hs_bilagrid_tv", "hs_bilagrid_tv_backward"):
        assert getattr(L, fn)(None, None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
        for kw, text in lattice + tv_only[fn]:
            rc, msg = tv(fn, **kw)
            assert rc == lib.HS_EINVAL, (fn, kw, rc, msg)
            assert msg.startswith(fn.encode() + b":") and text in msg, (fn, kw, msg)


# ---- Python ----

def test_python_raises_on_cpu_tensors_and_bad_arguments(monkeypatch):
    import casualhdrsplat_amd as pkg
    from casualhdrsplat_amd import bilagrid as B
    for n in ("BilateralGrid", "slice_image", "tv_loss"):
        assert getattr(pkg, n) is getattr(B, n) and n in pkg.__all__
    img, grd = torch.zeros(2, 3, 8, 9), torch.zeros(3, 12, 4, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.slice_image(img, grd, [0, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.tv_loss(grd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.BilateralGrid(2)(img, [0, 1])
    with pytest.raises(TypeError, match="image must be a torch.Tensor"):
        B.slice_image(img.numpy(), grd, [0, 1])
    with pytest.raises(TypeError, match="image must be float32"):
        B.slice_image(img.double(), grd, [0, 1])
    for bad in (torch.zeros(8, 9), torch.zeros(2, 4, 8, 9), torch.zeros(1, 2, 3, 8, 9), torch.zeros(0, 3, 8, 9)):
        with pytest.raises(ValueError, match=r"image must be \[3, H, W\] or \[F, 3, H, W\]"):
            B.slice_image(bad, grd, [0, 1])
    with pytest.raises(TypeError, match="grids must be a torch.Tensor"):
        B.tv_loss(grd.numpy())
    with pytest.raises(TypeError, match="grids must be float32"):
        B.tv_loss(grd.half())
    for bad in (torch.zeros(3, 11, 4, 3, 4), torch.zeros(12, 4, 3, 4), torch.zeros(3, 12, 17, 3, 4), torch.zeros(3, 12, 4, 65, 4),
                torch.zeros(3, 12, 4, 3, 65), torch.zeros(0, 12, 4, 3, 4), torch.zeros(3, 12, 0, 3, 4)):
        with pytest.raises(ValueError, match="tv_loss: grids"):
            B.tv_loss(bad)
    with pytest.raises(ValueError, match="BilateralGrid: num=0"):
        B.BilateralGrid(0)
    with pytest.raises(ValueError, match="grid_W=17"):
        B.BilateralGrid(1, grid_W=17)
    # with the device guards lifted (a stand-in for .device.type), what is looked at before the library is reached
    monkeypatch.setattr(B.L, "load", lambda: pytest.fail("an argument error reached the library"))

    class OnGpu(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)

    gi, gg = img.as_subclass(OnGpu), grd.as_subclass(OnGpu)
    with pytest.raises(ValueError, match=r"one id per frame \(2\), got 3"):
        B.slice_image(gi, gg, [0, 1, 2])
    with pytest.raises(ValueError, match="grid id 3 outside the 3 grids"):
        B.slice_image(gi, gg, [0, 3])
    with pytest.raises(ValueError, match=r"one id per frame \(1\), got 2"):
        B.slice_image(gi[0], gg, [0, 1])
    for bad in ([0, 1.0], "ab", [True, 0], 1.5, None):
        with pytest.raises(TypeError, match="an int, a sequence of ints or an int32 device tensor"):
            B.slice_image(gi, gg, bad)
    with pytest.raises(TypeError, match="must be int32"):
        B.slice_image(gi, gg, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="must live on the image's device"):
        B.slice_image(gi, gg, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"one id per frame \(2\)"):
        B.slice_image(gi, gg, torch.zeros(3, dtype=torch.int32).as_subclass(OnGpu))


def test_identity_initialisation():
    from casualhdrsplat_amd import bilagrid as B
    m = B.BilateralGrid(3, device="cpu")
    assert isinstance(m.grids, torch.nn.Parameter) and m.grids.requires_grad and m.grids.dtype == torch.float32
    assert tuple(m.grids.shape) == (3, 12, 8, 16, 16) and [n for n, _ in m.named_parameters()] == ["grids"]
    assert m.grids.detach().numpy().tobytes() == R.identity(3, 8, 16, 16).tobytes()
    m = B.BilateralGrid(2, grid_X=4, grid_Y=3, grid_W=5, device="cpu")
    assert tuple(m.grids.shape) == (2, 12, 5, 3, 4)
    assert m.grids.detach().numpy().tobytes() == R.identity(2, 5, 3, 4).tobytes()
    # the identity grid is the identity map of the restatement, and its total variation is exactly zero
    case = R.make_case(1, 9, 11, 1, 5, 3, 4)
    out = R.slice_forward(case["image"], m.grids.detach().numpy()[:1], [0], dtype=np.float64)
    assert np.abs(out - case["image"]).max() <= 1e-15
    assert R.tv(m.grids.detach().numpy())[0] == 0.0


# ---- resources ----

def test_bilagrid_kernels_spill_nothing_and_use_no_atomics(tmp_path):
    src = os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "bilagrid.hip")
    asm = str(tmp_path / "bilagrid.s")
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
    kernels = sorted({re.search(r"bilagrid\w*?_kernel", k).group() for k in out})
    assert kernels == ["bilagrid_grid_partial_kernel", "bilagrid_grid_sum_kernel", "bilagrid_pixel_kernel", "bilagrid_tv_bwd_kernel",
                       "bilagrid_tv_kernel", "bilagrid_tv_sum_kernel"], sorted(out)
    assert len(out) == 10                               # pixel: forward, backward; grid partials: L up to 2, 4, 8, 16
    for k, v in out.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
        assert v["LDS Size"] <= 32768, (k, v)
    assert "scratch_" not in text
    assert set(re.findall(r"\.amdhsa_float_denorm_mode_32 (\d+)", text)) == {"3"}              # denormals kept
    assert "v_div_fixup_f32" in text                                                           # IEEE division
    assert not re.findall(r"\b(?:global|flat|buffer|ds)_atomic_\w+", text)                     # no atomics at all
    cmd = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "bilagrid.o"],
                         capture_output=True, text=True, check=True).stdout
    assert re.findall(r"-ffp-contract=(\w+)", cmd) == ["off"] and " -c bilagrid.hip " in cmd, cmd
    mk = open(os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bbilagrid\.o\b", mk, flags=re.M) and re.search(r"^#\s+bilagrid\s", mk, flags=re.M)
    assert re.search(r"^ASAN_DRIVERS\s*=.*\bbilagrid_host\b", mk, flags=re.M)
    body = open(src, encoding="utf-8").read()
    assert not re.search(r"hipMem(set|cpy)\w*\(", body)
    assert not re.search(r"hip(Stream|Device)Synchronize|hipMalloc|hipFree|atomic", re.sub(r"//.*", "", body))
