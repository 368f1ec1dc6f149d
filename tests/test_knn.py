"""CPU checks of the 3-nearest-neighbour scale initialisation (knn.hip, hs_knn_*, casualhdrsplat_amd.knn): the numpy
restatement of the ALGORITHM (tests/knn_reference.pruned) against the restatement of the CONTRACT (brute) bit for bit, the
contract against scipy's k-d tree in float64 within the derived bound, the C ABI (exports, struct layout, the workspace size,
argument validation before any HIP call), the Python argument errors, and the unchanged host path of init_from_points."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import knn_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_knn_workspace_bytes", "hs_knn_mean_dist_sq")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- the restatements ----

CASES = {f"uniform{P}": (lambda P=P: R.uniform(P)) for P in (2, 3, 4, 5, 65, 1025)}
CASES.update({k: (lambda k=k: R.degenerate_families()[k]) for k in R.degenerate_families()})
_BRUTE = {}


def _brute_of(name):
    if name not in _BRUTE:
        x = CASES[name]()
        x.setflags(write=False)
        want = R.brute(x)
        want.setflags(write=False)
        _BRUTE[name] = (x, want)
    return _BRUTE[name]


@pytest.mark.parametrize("B,S", [(4, None), (64, None), (4, 4)])
@pytest.mark.parametrize("name", sorted(CASES))
def test_pruned_search_equals_the_contract_bit_for_bit(name, B, S):
    """Both skip rules (the second one non-strict), the cleared seed list and own-box-first change no bit of the result."""
    x, want = _brute_of(name)
    stats = {}
    got = R.pruned(x, B, S, stats)
    bad = np.nonzero(R.bits(got) != R.bits(want))[0]
    assert bad.size == 0, (name, B, S, bad[:5], got[bad[:5]], want[bad[:5]])
    if name == "uniform1025" and B == 4:
        assert stats["scanned"] < stats["boxes"] // 2, stats        # ... while most boxes are skipped
    if name == "identical" and B == 4:
        assert stats["scanned"] <= 2 * len(x), stats               # the non-strict rule: own box, then at most one more


def test_known_values():
    assert R.brute(R.uniform(1)).tolist() == [0.0]
    assert not R.brute(R.repeated()).any() and not R.brute(R.identical(300)).any()
    lat = R.brute(R.lattice())
    assert (lat[R.lattice_interior()] == np.float32(0.25)).all() and R.lattice_interior().sum() == 216
    two = R.brute(np.asarray([[0, 0, 0], [1, 2, 2]], np.float32))
    assert two.tolist() == [9.0, 9.0]                              # k = 1
    three = R.brute(np.asarray([[0, 0, 0], [1, 0, 0], [0, 3, 0]], np.float32))
    assert three.tolist() == [5.0, 5.5, 9.5]                       # k = 2
    den = R.brute(R.denormal())
    assert (den > 0).any() and (den < np.finfo(np.float32).tiny).all()       # denormals are kept


def test_contract_against_the_kd_tree_in_float64(capsys):
    """|brute - ref64| <= 8 * 2^-24 * ref64: a relative 2^-24 for each of the roundings on the way to a term -- the three
    subtractions, the three squares, the two adds, the neighbour sum and the divide, every term non-negative -- counted
    generously (a subtraction's error doubles in its square, the sum's two adds and the distance's two adds each touch a
    term at most twice: 2 + 1 + 2 + 2 + 1 = 8).  The worst constant seen is printed."""
    from scipy.spatial import cKDTree
    x = R.uniform(20_000, seed=3)
    x64 = x.astype(np.float64)
    d, _ = cKDTree(x64).query(x64, k=4)
    ref = np.mean(d[:, 1:] ** 2, axis=1)
    got = R.brute(x).astype(np.float64)
    c = np.abs(got - ref) / (2.0 ** -24 * ref)
    with capsys.disabled():
        print(f"\nknn brute vs float64 k-d tree, 20000 uniform points: worst constant {c.max():.3f} (bound 8)")
    assert (np.abs(got - ref) <= 8 * 2.0 ** -24 * ref).all(), c.max()


# ---- C ABI ----

def test_knn_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    assert re.search(r"\}\s*hs_knn_args\s*;", header)
    assert set(NAMES) <= set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309        # (detected by name: the version does not move)


def test_knn_struct_matches_c(lib, tmp_path):
    A = lib.hs_knn_args
    fields = [n for n, _ in A._fields_]
    assert fields == ["P", "xyz", "mean_d2", "workspace", "status"]
    lines = ['printf("%zu\\n", sizeof(hs_knn_args));'] + [f'printf("%zu\\n", offsetof(hs_knn_args, {n}));' for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(A)] + [getattr(A, n).offset for n in fields]


def test_workspace_bytes_is_aligned_and_non_decreasing(lib):
    L = lib.load()
    sizes = [L.hs_knn_workspace_bytes(P) for P in (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 10_007, 131_072, 1_000_000, (1 << 30) - 1)]
    assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
    assert sizes == sorted(sizes)
    prev = L.hs_knn_workspace_bytes(0)
    for P in range(1, 600):
        cur = L.hs_knn_workspace_bytes(P)
        assert cur >= prev, P
        prev = cur
    assert sizes[-2] < 100 * 1_000_000               # (under 100 bytes per point at a million)
    for P in (-1, 1 << 30, 1 << 40):
        assert L.hs_knn_workspace_bytes(P) == lib.HS_EINVAL
        assert b"hs_knn_workspace_bytes" in L.hs_last_error() and f"P={P}".encode() in L.hs_last_error()


def test_mean_dist2_validates_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the argument -- on a machine without a GPU: no HIP call
    is made before the checks.  The addresses are never dereferenced."""
    L = lib.load()
    good = dict(P=100, xyz=0x10000, mean_d2=0x20000, workspace=0x30000, status=0x40000)

    def call(**kw):
        a = lib.hs_knn_args()
        for k, v in dict(good, **kw).items():
            setattr(a, k, v)
        return L.hs_knn_mean_dist_sq(C.byref(a), None), L.hs_last_error().decode()

    assert L.hs_knn_mean_dist_sq(None, None) == lib.HS_EINVAL and "null args" in L.hs_last_error().decode()
    for P in (-1, 1 << 30, 1 << 40):
        rc, msg = call(P=P)
        assert rc == lib.HS_EINVAL and f"P={P}" in msg, msg
    for name in ("xyz", "mean_d2", "workspace", "status"):
        rc, msg = call(**{name: 0})
        assert rc == lib.HS_EINVAL and f"null {name}" in msg, msg
    for name in ("xyz", "mean_d2", "status"):
        rc, msg = call(**{name: good[name] + 2})
        assert rc == lib.HS_EINVAL and f"{name} must be 4-byte aligned" in msg, msg
        rc, msg = call(**{name: good[name] + 1})
        assert rc == lib.HS_EINVAL and name in msg, msg
    rc, msg = call(workspace=good["workspace"] + 16)
    assert rc == lib.HS_EINVAL and "workspace must be 256-byte aligned" in msg, msg
    rc, msg = call(P=0)
    assert rc == lib.HS_OK                                   # nothing is launched: no GPU is needed for this either


# ---- Python ----

def test_python_argument_errors():
    from casualhdrsplat_amd import knn_mean_dist2
    import casualhdrsplat_amd
    assert "knn_mean_dist2" in casualhdrsplat_amd.__all__
    with pytest.raises(TypeError):
        knn_mean_dist2(np.zeros((4, 3), np.float32))
    with pytest.raises(TypeError):
        knn_mean_dist2(torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(TypeError):
        knn_mean_dist2(torch.zeros(4, 3, dtype=torch.float16))
    for shape in ((4,), (4, 2), (3, 4), (2, 4, 3)):
        with pytest.raises(ValueError):
            knn_mean_dist2(torch.zeros(*shape))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn_mean_dist2(torch.zeros(4, 3))


def test_init_from_points_without_a_device_is_the_host_path():
    """device=None: scipy's k-d tree on the host, CPU tensors -- and a CPU device named explicitly is the same path."""
    code = ("import sys, numpy as np, torch\n"
            "from casualhdrsplat_amd import scene_io as IO\n"
            "assert 'scipy' not in sys.modules and 'scipy.spatial' not in sys.modules\n"
            "x = np.random.default_rng(0).random((50, 3))\n"
            "rgb = np.full((50, 3), 128, np.uint8)\n"
            "c = IO.init_from_points(x, rgb, sh_degree=1)\n"
            "assert 'scipy.spatial' in sys.modules\n"
            "assert all(t.device.type == 'cpu' for t in (c.means3D, c.shs, c.opacity_logit, c.log_scales, c.rotations))\n"
            "d = IO.init_from_points(x, rgb, sh_degree=1, device='cpu')\n"
            "assert torch.equal(c.log_scales, d.log_scales) and torch.equal(c.shs, d.shs)\n"
            "from scipy.spatial import cKDTree\n"
            "dist, _ = cKDTree(x).query(x, k=4)\n"
            "want = np.log(np.sqrt(np.maximum(np.mean(dist[:, 1:] ** 2, axis=1), 1e-7))).astype(np.float32)\n"
            "assert np.array_equal(c.log_scales.numpy(), np.repeat(want[:, None], 3, axis=1))\n"
            "print('ok')\n")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT)
    assert out.strip().endswith(b"ok")
