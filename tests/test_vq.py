"""k-means SH codebook compression (vq.hip / vq.py / scene_io.save_vq): what can be checked without a GPU -- the C ABI's names
and struct, the workspace size, argument validation ahead of any HIP call, the wrappers' argument checks, the file format,
and the numpy restatements themselves on a planted problem."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import vq_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_vq_workspace_bytes", "hs_vq_assign", "hs_vq_update")
FIELDS = ["N", "D", "K", "x", "weights", "codebook_in", "codes", "dist2", "codebook_out", "counts", "workspace"]


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- C ABI ----

def test_vq_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
        assert re.fullmatch(r"hs_[a-z_]+", n)
    assert re.search(r"\}\s*hs_vq_args\s*;", header)
    assert set(NAMES) <= set(lib.EXPORTS) and set(NAMES) <= set(lib.SIGNATURES)
    assert set(re.findall(r"\bHS_API\s+[\w\s\*]+?\b(hs_\w+)\s*\(", header)) == set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309        # (detected by name: the version does not move)


def test_vq_struct_matches_c(lib, tmp_path):
    A = lib.hs_vq_args
    fields = [n for n, _ in A._fields_]
    assert fields == FIELDS
    lines = ['printf("%zu\\n", sizeof(hs_vq_args));'] + [f'printf("%zu\\n", offsetof(hs_vq_args, {n}));' for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(A)] + [getattr(A, n).offset for n in fields]


def test_workspace_bytes(lib):
    L = lib.load()
    last = 0
    for N in (0, 1, 63, 64, 255, 256, 257, 3001, 70000, 262144, 262145, 262400, 1 << 20, (1 << 20) + 1, 1 << 24, 1 << 30):
        for D, K in ((45, 4096), (1, 1), (48, 65536), (9, 256)):
            b = L.hs_vq_workspace_bytes(N, D, K)
            assert b > 0 and b % 256 == 0, (N, D, K, b)
    for D, K in ((45, 4096), (1, 1), (48, 65536), (24, 65)):
        last = 0
        for N in sorted(set(list(range(0, 3000, 37)) + [262144 + i for i in range(-3, 400, 7)] + [(1 << 20) + i for i in (-1, 0, 1)]
                            + [1 << 24, 1 << 30])):
            b = L.hs_vq_workspace_bytes(N, D, K)
            assert b >= last, (N, D, K, b, last)
            last = b
    # holds the row permutation, at least
    assert L.hs_vq_workspace_bytes(1 << 20, 45, 4096) >= 4 << 20
    for bad in ((100, 0, 8), (100, 49, 8), (100, 8, 0), (100, 8, 65537), (-1, 8, 8), (100, -1, 8), (100, 8, -1)):
        assert L.hs_vq_workspace_bytes(*bad) == lib.HS_EINVAL, bad
        assert b"hs_vq_workspace_bytes" in L.hs_last_error()
    assert L.hs_vq_workspace_bytes(100, 48, 65536) > 0 and L.hs_vq_workspace_bytes(100, 1, 1) > 0


def test_entry_points_validate_before_touching_the_gpu(lib):
    """Every limit and every pointer error is HS_EINVAL with a message that names the entry point and the field -- on a
    machine without a GPU: no HIP call is made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy addresses: validation must fail before any of them is dereferenced

    def call(fn, **kw):
        a = lib.hs_vq_args()
        a.N, a.D, a.K = 1000, 45, 64
        for f in FIELDS[3:]:
            setattr(a, f, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, fn)(C.byref(a), None), L.hs_last_error()

    limits = [(dict(D=0), b"D=0"), (dict(D=49), b"D=49"), (dict(K=0), b"K=0"), (dict(K=65537), b"K=65537"), (dict(N=-1), b"N=-1"),
              (dict(N=(1 << 30) + 1), b"N=1073741825")]
    both = limits + [(dict(x=None), b"null x"), (dict(codebook_in=None), b"null codebook_in"), (dict(codes=None), b"null codes"),
                     (dict(x=one + 2), b"x must be 4-byte aligned"), (dict(codes=one + 1), b"codes must be 4-byte aligned"),
                     (dict(codebook_in=one + 2), b"codebook_in must be 4-byte aligned")]
    only = {"hs_vq_assign": [(dict(dist2=one + 2), b"dist2 must be 4-byte aligned")],
            "hs_vq_update": [(dict(codebook_out=None), b"null codebook_out"), (dict(counts=None), b"null counts"),
                             (dict(workspace=None), b"null workspace"), (dict(workspace=one + 128), b"workspace must be 256-byte aligned"),
                             (dict(weights=one + 2), b"weights must be 4-byte aligned"),
                             (dict(counts=one + 2), b"counts must be 4-byte aligned")]}
    for fn in ("hs_vq_assign", "hs_vq_update"):
        assert getattr(L, fn)(None, None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
        for kw, text in both + only[fn]:
            rc, msg = call(fn, **kw)
            assert rc == lib.HS_EINVAL, (fn, kw, rc, msg)
            assert msg.startswith(fn.encode() + b":") and text in msg, (fn, kw, msg)
    # no rows: the assignment has nothing to write and launches nothing, with or without row pointers
    assert call("hs_vq_assign", N=0)[0] == lib.HS_OK
    assert call("hs_vq_assign", N=0, x=None, codes=None, dist2=None)[0] == lib.HS_OK
    assert call("hs_vq_assign", N=0, codebook_in=None)[0] == lib.HS_EINVAL
    assert call("hs_vq_update", N=0, codebook_out=None)[0] == lib.HS_EINVAL


# ---- Python ----

def test_python_raises_on_cpu_tensors_and_bad_arguments():
    import casualhdrsplat_amd as pkg
    from casualhdrsplat_amd import vq as V
    for n in ("kmeans", "kmeans_assign", "kmeans_update", "quantize_sh", "dequantize_sh", "VQResult"):
        assert getattr(pkg, n) is getattr(V, n) and n in pkg.__all__
    x, book = torch.zeros(100, 9), torch.zeros(8, 9)
    codes, w = torch.zeros(100, dtype=torch.int32), torch.ones(100)
    meta = "meta"       # a device that is neither the CPU nor a GPU: still refused
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.kmeans_assign(x, book)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.kmeans_update(x, codes, book, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.kmeans(x, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.kmeans(x.to(meta), 8, init=book.to(meta))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.quantize_sh(torch.zeros(100, 4, 3), 8)
    # dtypes
    with pytest.raises(TypeError, match="x must be torch.float32"):
        V.kmeans_assign(x.double(), book)
    with pytest.raises(TypeError, match="codebook must be torch.float32"):
        V.kmeans_assign(x, book.half())
    with pytest.raises(TypeError, match="codes must be torch.int32"):
        V.kmeans_update(x, codes.long(), book)
    with pytest.raises(TypeError, match="weights must be torch.float32"):
        V.kmeans_update(x, codes, book, w.double())
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        V.kmeans_assign(x.numpy(), book)
    # shapes
    with pytest.raises(ValueError, match="differ in D"):
        V.kmeans_assign(x, torch.zeros(8, 10))
    with pytest.raises(ValueError, match="dimension"):
        V.kmeans_assign(x[0], book)
    with pytest.raises(ValueError, match="one entry per row"):
        V.kmeans_update(x, codes[:99], book)
    with pytest.raises(ValueError, match="one entry per row"):
        V.kmeans_update(x, codes, book, w[:50])
    with pytest.raises(ValueError, match="outside"):
        V.kmeans_assign(torch.zeros(10, 49), torch.zeros(3, 49))
    with pytest.raises(ValueError, match="cannot seed"):
        V.kmeans(x, 101)
    with pytest.raises(ValueError, match="row indices"):
        V.kmeans(x, 8, init=[0, 1, 2])
    with pytest.raises(ValueError, match="centroids"):
        V.kmeans(x, 9, init=book)
    with pytest.raises(ValueError, match="K="):
        V.kmeans(x, 0)
    with pytest.raises(ValueError, match="M = 1"):
        V.quantize_sh(torch.zeros(100, 1, 3), 8)
    with pytest.raises(ValueError, match=r"\[P, M, 3\]"):
        V.quantize_sh(torch.zeros(100, 4), 8)
    # the gather is plain torch and runs anywhere
    dc, cb = torch.randn(5, 1, 3), torch.randn(3, 8, 3)
    sc = torch.tensor([2, 0, 1, 2, 2], dtype=torch.int32)
    out = V.dequantize_sh(dc, cb, sc)
    assert out.shape == (5, 9, 3) and torch.equal(out[:, :1], dc) and torch.equal(out[:, 1:], cb[sc.long()])
    with pytest.raises(ValueError, match="one code per Gaussian"):
        V.dequantize_sh(dc, cb, sc[:4])


def test_save_vq_load_vq_round_trip(tmp_path):
    from casualhdrsplat_amd import scene_io as S
    g = torch.Generator().manual_seed(3)
    P, M, K = 257, 16, 300
    cloud = S.GaussianCloud(torch.randn(P, 3, generator=g), torch.randn(P, M, 3, generator=g), torch.randn(P, 1, generator=g),
                            torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g))
    cloud.means3D[0, 0] = float("nan")           # bits, not values
    cloud.shs[1, 0, 2] = -0.0
    book = torch.randn(K, M - 1, 3, generator=g)
    codes = torch.randint(0, K, (P,), generator=g, dtype=torch.int32)
    codes[0], codes[1] = K - 1, 0
    path = str(tmp_path / "cloud.npz")
    S.save_vq(path, cloud, book, codes)
    with np.load(path) as z:
        assert set(z.files) == {"version", "means3D", "sh_dc", "opacity_logit", "log_scales", "rotations", "sh_codebook", "sh_codes"}
        assert z["sh_codes"].dtype == np.uint16 and z["sh_codes"].shape == (P,)
        assert all(z[k].dtype == np.float32 for k in z.files if k not in ("version", "sh_codes"))
        assert int(z["version"]) == S.VQ_VERSION
    # 14 floats + 2 bytes per Gaussian and the codebook, next to 59 floats (the zip container adds a few hundred bytes)
    assert abs(os.path.getsize(path) - (P * 58 + K * (M - 1) * 12)) < 4096
    back = S.load_vq(path)

    def bits(t):
        return t.contiguous().view(torch.int32)
    assert torch.equal(back.shs[:, 1:], book[codes.long()])
    assert torch.equal(bits(back.shs[:, :1]), bits(cloud.shs[:, :1]))
    for name in ("means3D", "opacity_logit", "log_scales", "rotations"):
        a, b = getattr(back, name), getattr(cloud, name)
        assert a.dtype == torch.float32 and a.shape == b.shape and torch.equal(bits(a), bits(b)), name
    assert back.sh_degree == 3
    with pytest.raises(ValueError, match="outside"):
        S.save_vq(path, cloud, book[:10], codes)
    with pytest.raises(ValueError, match="coefficients per entry"):
        S.save_vq(path, cloud, book[:, :3], codes)
    # K = 65536 still fits the 16-bit codes
    big = torch.zeros(65536, M - 1, 3)
    big[65535] = 7.0
    codes[5] = 65535
    S.save_vq(path, cloud, big, codes)
    assert torch.equal(S.load_vq(path).shs[5, 1:], big[65535])


# ---- the restatements ----

def test_restatement_recovers_planted_clusters():
    x, labels, centres, first = R.planted()
    assert x.shape == (3200, 45) and x.dtype == np.float32
    # the first assignment, against one row per blob, already recovers every label
    codes, d2 = R.assign(x, x[first])
    assert codes.dtype == np.int32 and d2.dtype == np.float32
    assert np.array_equal(codes, labels)
    assert np.all(d2[first] == 0.0)
    book, codes, d2, trace = R.lloyd(x, first, 3)
    assert np.array_equal(codes, labels)
    means = np.stack([x[labels == k].astype(np.float64).mean(0) for k in range(8)])
    assert np.abs(book - means).max() < 1e-5 and np.abs(book - centres).max() < 0.1
    assert all(b <= a for a, b in zip(trace, trace[1:]))


def test_restatement_ties_nan_and_update_rules():
    x = np.array([[1.0, 2.0], [0.0, 0.0], [np.nan, 1.0], [5.0, 5.0]], np.float32)
    book = np.array([[5.0, 5.0], [1.0, 2.0], [1.0, 2.0], [0.0, 1.0]], np.float32)
    codes, d2 = R.assign(x, book)
    assert codes.tolist() == [1, 3, 0, 0]                       # the duplicate at 2 never wins; the NaN row keeps 0
    assert d2[0] == 0.0 and d2[1] == 1.0 and np.isposinf(d2[2]) and d2[3] == 0.0
    w = np.array([1.0, 0.0, 3.0, 1.0], np.float32)
    out, counts, bound, _ = R.update(np.nan_to_num(x), codes, book, w)
    assert counts.tolist() == [2, 1, 0, 1]
    assert np.array_equal(out[2], book[2]) and np.array_equal(out[3], book[3])       # empty; all weights zero
    assert np.array_equal(out[0], np.array([(3 * 0 + 5) / 4, (3 * 1 + 5) / 4], np.float32))
    assert bound[2].max() == 0 and bound[3].max() == 0


def test_restatement_objective_never_rises_with_weights():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3001, 24)).astype(np.float32)
    w = rng.random(3001).astype(np.float32)
    rows = rng.permutation(3001)[:65]
    trace = R.lloyd(x, rows, 12, w)[3]
    assert len(trace) == 13 and all(b <= a for a, b in zip(trace, trace[1:]))
