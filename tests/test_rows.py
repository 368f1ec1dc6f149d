"""CPU checks of the score-driven row plans (rows.hip: hs_rows_workspace_bytes, hs_rows_plan; rows.py): the C ABI (exports,
struct layout, workspace arithmetic, argument validation before any HIP call), the Python argument errors, the numpy
restatement the GPU tests compare with (tests/rows_reference.py) against a brute-force definition of the order, and the
host-only sanitizer driver tests/native/rows_host.cpp."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rows_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_rows_workspace_bytes", "hs_rows_plan")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- C ABI ----

def test_rows_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    assert "hs_rows_args" in header
    assert set(NAMES) <= set(lib.EXPORTS)
    assert set(re.findall(r"\b(hs_[a-z_]+)\s*\(", header)) == set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309 == lib.HS_VERSION       # (detected by name: the version does not move)
    assert (lib.HS_ROWS_MASK, lib.HS_ROWS_KEEP, lib.HS_ROWS_DENSIFY) == (0, 1, 2)
    for name, value in (("HS_ROWS_MASK", 0), ("HS_ROWS_KEEP", 1), ("HS_ROWS_DENSIFY", 2)):
        assert re.search(rf"#define {name} {value}\b", header)


def test_rows_struct_matches_c(lib, tmp_path):
    S_ = lib.hs_rows_args
    fields = [n for n, _ in S_._fields_]
    lines = [f'printf("%zu\\n", sizeof({S_.__name__}));'] + [f'printf("%zu\\n", offsetof({S_.__name__}, {n}));' for n in fields]
    want = [C.sizeof(S_)] + [getattr(S_, n).offset for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want


def test_workspace_bytes_is_a_positive_multiple_of_16_that_does_not_decrease(lib):
    L = lib.load()
    last = 0
    for P in (0, 1, 255, 256, 257, 4096, 10007, 65536, 65537, 262144, 1_000_000, (1 << 30) - 1):
        b = L.hs_rows_workspace_bytes(P)
        a256 = lambda x: (x + 255) // 256 * 256        # noqa: E731
        assert b == a256(P) + a256(16 * ((P + 255) // 256)) + 263424, (P, b)     # the header's formula
        assert b > 0 and b % 16 == 0 and b >= last, (P, b)
        last = b
    for bad in (-1, 1 << 30, 1 << 40):
        assert L.hs_rows_workspace_bytes(bad) == -1 and b"hs_rows_workspace_bytes: P=" in L.hs_last_error(), bad


def test_rows_plan_validates_before_touching_the_gpu(lib):
    """Every limit of the header is HS_EINVAL with a message that names the field -- on a machine without a GPU: no HIP call
    is made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy address: validation must fail before it is dereferenced
    ptrs = ("score", "mask", "scales", "workspace", "row_map", "counts", "counts_host")

    def call(**kw):
        a = lib.hs_rows_args()
        a.P, a.k, a.mode, a.flags, a.tau_split = 100, 10, lib.HS_ROWS_KEEP, 0, 0.0
        for p in ptrs:
            setattr(a, p, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.hs_rows_plan(C.byref(a), None), L.hs_last_error()

    assert L.hs_rows_plan(None, None) == lib.HS_EINVAL and L.hs_last_error() == b"hs_rows_plan: null args"
    M, K, D = lib.HS_ROWS_MASK, lib.HS_ROWS_KEEP, lib.HS_ROWS_DENSIFY
    cases = [(dict(P=-1), b"P=-1"), (dict(P=1 << 30), b"P=1073741824"), (dict(k=-1), b"k=-1"), (dict(k=101), b"k=101"),
             (dict(mode=3), b"mode=3"), (dict(mode=-1), b"mode=-1"),
             (dict(flags=lib.HS_DENSIFY_RAW_OPACITY), b"flags=1"), (dict(flags=4), b"flags=4"),
             (dict(mode=D, tau_split=math.nan), b"tau_split is NaN"),
             (dict(counts=None), b"null counts"), (dict(counts=one + 2), b"counts must be 4-byte aligned"),
             (dict(counts_host=one + 1), b"counts_host must be 4-byte aligned"),
             (dict(row_map=None), b"null row_map"), (dict(row_map=one + 2), b"row_map must be 4-byte aligned"),
             (dict(workspace=None), b"null workspace"), (dict(workspace=one + 8), b"workspace must be 16-byte aligned"),
             (dict(score=None), b"null score"), (dict(score=one + 2), b"score must be 4-byte aligned"),
             (dict(mode=D, score=None), b"null score"), (dict(mode=D, scales=None), b"null scales"),
             (dict(mode=D, scales=one + 1), b"scales must be 4-byte aligned"), (dict(mode=M, k=0, mask=None), b"null mask")]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_rows_plan:") and text in msg, (kw, rc, msg)
    # tau_split is DENSIFY's alone, and a mode does not look at the pointers it does not read -- seen from the NEXT error
    rc, msg = call(mode=K, tau_split=math.nan, mask=None, scales=None, counts=None)
    assert rc == lib.HS_EINVAL and b"null counts" in msg
    rc, msg = call(mode=M, k=0, score=None, scales=None, mask=one + 1, counts=None)      # (a mask is bytes: any address)
    assert rc == lib.HS_EINVAL and b"null counts" in msg
    # with P == 0 no data pointer is looked at -- only counts, which is written: its absence is the error that remains
    rc, msg = call(P=0, k=0, score=None, mask=None, scales=None, workspace=None, row_map=None, counts=None)
    assert rc == lib.HS_EINVAL and b"null counts" in msg
    rc, msg = call(P=0, k=1)
    assert rc == lib.HS_EINVAL and b"k=1" in msg


# ---- Python ----

def test_python_names_and_argument_errors():
    import casualhdrsplat_amd as pkg
    from casualhdrsplat_amd import rows
    for n in ("prune_rows", "keep_top_k", "densify_top_k", "RowsResult"):
        assert getattr(pkg, n) is getattr(rows, n) and n in pkg.__all__
    cpu = torch.device("cpu")
    # a cloud on the CPU never gets as far as an optimizer (GaussianAdam refuses it: there is no fallback), and anything
    # that is not a GaussianAdam is refused by name
    m = torch.zeros(8, 3, requires_grad=True)
    for call in (lambda o: pkg.prune_rows(o, torch.zeros(8, dtype=torch.bool)), lambda o: pkg.keep_top_k(o, torch.zeros(8), 4),
                 lambda o: pkg.densify_top_k(o, torch.zeros(8), 4, extent=1.0)):
        with pytest.raises(TypeError, match="GaussianAdam"):
            call(torch.optim.Adam([m]))
    # the argument checks behind the three calls, each message naming the argument
    with pytest.raises(RuntimeError, match="score must live on a cuda"):
        rows._check_score("keep_top_k", torch.zeros(8), 8, cpu)
    for bad in (torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.int32), torch.zeros(7), torch.zeros(8, 1), torch.zeros(16)[::2]):
        with pytest.raises(ValueError, match=r"keep_top_k: score must be a contiguous float32 tensor \[8\]"):
            rows._check_score("keep_top_k", bad, 8, cpu)
    with pytest.raises(TypeError, match="score must be a torch.Tensor"):
        rows._check_score("keep_top_k", [0.0] * 8, 8, cpu)
    for bad in (-1, 9):
        with pytest.raises(ValueError, match=rf"densify_top_k: k={bad} outside \[0, P = 8\]"):
            rows._check_k("densify_top_k", bad, 8)
    for bad in (2.0, True, None):
        with pytest.raises(TypeError, match="k=.* must be an int"):
            rows._check_k("keep_top_k", bad, 8)
    assert rows._check_k("keep_top_k", 0, 8) == 0 and rows._check_k("keep_top_k", 8, 8) == 8
    with pytest.raises(ValueError, match=r"extras\[0\] must be a contiguous tensor \[8, \.\.\.\]"):
        rows._check_extras("prune_rows", [torch.zeros(7, 2)], 8, cpu)
    for bad in (torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float16), torch.zeros(8, dtype=torch.bool)):
        with pytest.raises(ValueError, match=r"extras\[0\] has dtype .*4-byte"):
            rows._check_extras("prune_rows", [bad], 8, cpu)
    with pytest.raises(RuntimeError, match=r"extras\[0\] must live on a cuda"):
        rows._check_extras("prune_rows", [torch.zeros(8, dtype=torch.int32)], 8, cpu)
    with pytest.raises(TypeError, match="extras must be a sequence"):
        rows._check_extras("prune_rows", torch.zeros(8), 8, cpu)
    with pytest.raises(ValueError, match=r"prune_rows: mask must be a contiguous bool or uint8 tensor \[8\]"):
        rows._check_mask("prune_rows", torch.zeros(8), 8, cpu)
    with pytest.raises(RuntimeError, match="mask must live on a cuda"):
        rows._check_mask("prune_rows", torch.zeros(8, dtype=torch.bool), 8, cpu)


# ---- the restatement against a brute-force definition ----

def _cmp(a, b):
    """The header's order on (score, row) pairs, best first: NaN lowest and all NaNs equal, -0 == +0, else numeric; among
    equal scores the lower row first."""
    (x, i), (y, j) = a, b
    nx, ny = math.isnan(x), math.isnan(y)
    if nx != ny:
        return 1 if nx else -1                   # the number comes first
    if not nx and x != y:                        # (0.0 == -0.0 in Python, as the order wants)
        return -1 if x > y else 1
    return -1 if i < j else 1


def _brute(score):
    return [i for _, i in sorted(((float(s), i) for i, s in enumerate(score)), key=functools.cmp_to_key(_cmp))]


def _inputs():
    rng = np.random.default_rng(5)
    out = [("single", np.array([1.5], np.float32)), ("single_nan", np.array([np.nan], np.float32))]
    for P in (2, 7, 33, 64):
        out.append((f"normal{P}", rng.standard_normal(P).astype(np.float32)))
        out.append((f"few{P}", rng.integers(0, 3, P).astype(np.float32)))
        out.append((f"specials{P}", R.SPECIALS[rng.integers(0, R.SPECIALS.size, P)]))
        out.append((f"signed_zeros{P}", np.where(rng.random(P) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)))
        out.append((f"nans{P}", np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)[rng.integers(0, 4, P)]))
    out.append(("every_special", R.SPECIALS.copy()))
    out.append(("every_special_reversed", R.SPECIALS[::-1].copy()))
    for name in R.FAMILIES:
        out.append((name, R.family(name, 61, seed=3)))
    return out


@pytest.mark.parametrize("name,score", _inputs(), ids=[n for n, _ in _inputs()])
def test_reference_is_the_brute_force_definition(name, score):
    """P <= 64, every k: the order, the selection, T, and the three plans' row maps and counts from first principles."""
    P = score.shape[0]
    want = _brute(score)
    assert R.order(score).tolist() == want
    rng = np.random.default_rng(P)
    scales = rng.standard_normal((P, 3)).astype(np.float32)
    scales[rng.random(P) < 0.1] = np.nan
    tau = np.float32(0.3)
    smax = [max((float(v) for v in row if not math.isnan(v)), default=math.nan) if not math.isnan(float(row[0])) else
            # (the comparisons start from scales[0]: a NaN there stays, since nothing compares greater than NaN)
            math.nan for row in scales]
    for k in range(P + 1):
        best = set(want[:k])
        sel, T = R.select(score, k)
        assert set(np.nonzero(sel)[0].tolist()) == best
        if k:
            last = float(score[want[k - 1]])
            ties = [i for i in range(P) if (math.isnan(float(score[i])) and math.isnan(last)) or float(score[i]) == last]
            assert T == len(ties) and T >= 1
        else:
            assert T == 0
        rm, counts = R.plan_keep(score, k)
        assert rm.tolist() == sorted(best) and counts == [k, k, 0, 0, P - k, 0, P, T]
        rm, counts = R.plan_densify(score, k, scales, tau)
        split = sorted(i for i in best if smax[i] > float(tau))
        clone = sorted(i for i in best if not smax[i] > float(tau))
        surv = [i for i in range(P) if i not in split]
        assert rm.tolist() == surv + [(1 << 30) | i for i in clone] + [(2 << 30) | i for i in split] + [(3 << 30) | i for i in split]
        assert counts == [P + k, len(surv), len(clone), 2 * len(split), 0, len(split), P, T]
    mask = rng.random(P) < 0.3
    rm, counts = R.plan_mask(mask)
    assert rm.tolist() == [i for i in range(P) if not mask[i]] and counts == [len(rm), len(rm), 0, 0, P - len(rm), 0, P, 0]


def test_key_is_monotone_and_canonical():
    f = lambda *bits: np.array(bits, np.uint32).view(np.float32)      # noqa: E731
    k = R.key(f(0xFF800000, 0xFF7FFFFF, 0x80800000, 0x807FFFFF, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x007FFFFF,
                0x00800000, 0x7F7FFFFF, 0x7F800000)).astype(np.int64)
    assert (np.diff(k) >= 0).all() and (np.diff(k) == 0).sum() == 1 and k[5] == k[6] == 0x80000000      # -0 == +0, nothing else ties
    assert R.key(f(0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)).tolist() == [0, 0, 0, 0] and k[0] == 0x007FFFFF > 0
    assert R.ks_of(R.family("seven", 257)) == sorted(set(R.ks_of(R.family("seven", 257))))


# ---- the host-only sanitizer driver ----

def test_rows_host_driver_is_part_of_the_sanitizer_build():
    """tests/native/rows_host.cpp walks hs_rows_* under the host-only AddressSanitizer + UBSan build `make asan` runs (a
    stand-alone program, no GPU); here: it exists, it is one of the Makefile's drivers, and it rejects what the header lists."""
    mk = open(os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "Makefile")).read()
    drivers = re.search(r"^ASAN_DRIVERS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "rows_host" in drivers
    src = open(os.path.join(ROOT, "tests", "native", "rows_host.cpp")).read()
    assert "int main()" in src and "hs_rows_plan" in src and "hs_rows_workspace_bytes" in src
    assert re.search(r"^OBJS\s*=.*\brows\.o\b", mk, flags=re.M) and not re.search(r"^FAST_TUS\s*=.*\brows\b", mk, flags=re.M)
