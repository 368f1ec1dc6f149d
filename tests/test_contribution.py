"""CPU checks of the blending-weight statistics (contrib.hip: hs_contribution_workspace_bytes, hs_contribution;
importance.py): the C ABI (exports, struct layout, argument validation before any HIP call), the Python argument errors, and
the numpy restatement the GPU tests compare with (tests/contribution_reference.py) against what follows from its definition."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import contribution_reference as R
import helpers as Hh
from casualhdrsplat_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_contribution_workspace_bytes", "hs_contribution")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def frame(oracle):
    """The second guarded scene of the GPU tests (600 Gaussians, 104 x 72, SH degree 1: partial tiles in both directions)
    with its oracle forward and the float64 statistics."""
    sc, seed = Hh.guarded_scene(oracle, 600, 104, 72, 1)
    assert seed == 0            # (tests/test_contribution_gpu.py counts on it)
    f, _ = Hh.run_oracle(oracle, sc, backward=False)
    return sc, f, R.contributions(f, 104, 72)


# ---- C ABI ----

def test_contribution_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    assert "hs_contribution_args" in header
    assert set(NAMES) <= set(lib.EXPORTS)
    assert set(re.findall(r"\b(hs_[a-z_]+)\s*\(", header)) == set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309 == lib.HS_VERSION       # (detected by name: the version does not move)


def test_contribution_struct_matches_c(lib, tmp_path):
    S_ = lib.hs_contribution_args
    fields = [n for n, _ in S_._fields_]
    lines = [f'printf("%zu\\n", sizeof({S_.__name__}));'] + [f'printf("%zu\\n", offsetof({S_.__name__}, {n}));' for n in fields]
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
        d = _dims(lib, capacity=cap)
        b = L.hs_contribution_workspace_bytes(C.byref(d))
        assert b > 0 and b % 256 == 0 and b >= 16 * cap + 16 * 1000 and b >= last, (cap, b)
        last = b
    assert L.hs_contribution_workspace_bytes(C.byref(_dims(lib, capacity=10 ** 5))) > \
        L.hs_contribution_workspace_bytes(C.byref(_dims(lib, capacity=10 ** 4)))
    # ... and with the instances: one row per (pose, Gaussian)
    assert L.hs_contribution_workspace_bytes(C.byref(_dims(lib, n_poses=4))) > L.hs_contribution_workspace_bytes(C.byref(_dims(lib)))
    assert L.hs_contribution_workspace_bytes(C.byref(_dims(lib, P=0, capacity=0))) == 256
    assert L.hs_contribution_workspace_bytes(None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    for bad in (dict(P=-1), dict(W=0), dict(n_poses=0), dict(capacity=-1), dict(capacity=1 << 30), dict(n_poses=3, n_frames=2)):
        assert L.hs_contribution_workspace_bytes(C.byref(_dims(lib, **bad))) == lib.HS_EINVAL, bad
        assert L.hs_last_error().startswith(b"hs_plan:"), bad


def test_contribution_validates_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the field, and the no-op succeeds -- on a machine without
    a GPU: no HIP call is made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy address: validation must fail before it is dereferenced
    fields = ("geom", "binning", "image", "ws", "pixel_weight", "weight_sum", "weight_max", "pixel_count")

    def call(dims=None, **kw):
        a = lib.hs_contribution_args()
        a.dims = dims if dims is not None else _dims(lib)
        for k in fields:
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.hs_contribution(C.byref(a), None), L.hs_last_error()

    assert L.hs_contribution(None, None) == lib.HS_EINVAL and L.hs_last_error() == b"hs_contribution: null args"
    cases = [(dict(geom=None), b"null geom"), (dict(binning=None), b"null binning"), (dict(image=None), b"null image"),
             (dict(ws=None), b"null ws"), (dict(weight_sum=None), b"null weight_sum"), (dict(weight_max=None), b"null weight_max"),
             (dict(pixel_count=None), b"null pixel_count"), (dict(ws=one + 128), b"ws must be 256-byte aligned"),
             (dict(geom=one + 16), b"geom must be 256-byte aligned"), (dict(weight_sum=one + 2), b"weight_sum must be 4-byte aligned"),
             (dict(pixel_count=one + 1), b"pixel_count must be 4-byte aligned"),
             (dict(pixel_weight=one + 2), b"pixel_weight must be 4-byte aligned")]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_contribution:") and text in msg, (kw, rc, msg)
    # dims that hs_plan refuses
    for bad in (dict(P=-1), dict(H=0), dict(n_poses=0), dict(capacity=1 << 30), dict(n_poses=4, n_frames=3), dict(n_frames=-1)):
        rc, msg = call(dims=_dims(lib, **bad))
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_plan:"), (bad, rc, msg)
    # an empty cloud is a no-op: no pointer is looked at
    assert call(dims=_dims(lib, P=0), **{k: None for k in fields})[0] == lib.HS_OK


# ---- Python ----

def test_python_names_and_argument_errors():
    import casualhdrsplat_amd as pkg
    from casualhdrsplat_amd import importance
    assert pkg.ContributionStats is importance.ContributionStats and pkg.accumulate_contributions is importance.accumulate_contributions
    assert {"ContributionStats", "accumulate_contributions"} <= set(pkg.__all__)
    st = pkg.ContributionStats(5, "cpu")
    assert st.weight_sum.dtype == torch.float32 and st.weight_max.dtype == torch.float32 and st.pixel_count.dtype == torch.int32
    assert all(tuple(t.shape) == (5,) and not t.any() for t in (st.weight_sum, st.weight_max, st.pixel_count))
    st.weight_sum += 1; st.weight_max += 2; st.pixel_count += 3
    st.reset()
    assert not st.weight_sum.any() and not st.weight_max.any() and not st.pixel_count.any()
    st.resize(9)
    assert all(tuple(t.shape) == (9,) and not t.any() for t in (st.weight_sum, st.weight_max, st.pixel_count))
    with pytest.raises(RuntimeError, match="keep_state=True"):
        pkg.accumulate_contributions(torch.zeros(3, 4, 4), st)     # not the output of a forward


# ---- the restatement ----

def test_reference_sums_to_the_accumulated_opacity(frame):
    """sum_g sum[g] = sum_p (1 - final_T[p]): every step adds alpha T to the left and takes it from T on the right."""
    sc, f, r = frame
    lhs, rhs = r["sum"].sum(), (1.0 - r["final_T"]).sum()
    assert rhs > 100 and abs(lhs - rhs) <= 1e-6 * rhs, (lhs, rhs)
    # ... with a weight image: sum_p e (1 - final_T)
    e = np.random.default_rng(3).random((72, 104))
    rw = R.contributions(f, 104, 72, pixel_weight=e)
    assert abs(rw["sum"].sum() - (e * (1.0 - r["final_T"])).sum()) <= 1e-6 * rhs
    # the float64 evaluation takes the oracle's decisions on a guarded frame
    assert np.array_equal(r["n_contrib"], f["n_contrib"].astype(np.int64))
    assert np.abs(r["final_T"] - f["final_T"]).max() <= 2e-5


def test_reference_count_is_the_number_of_contributing_pairs(frame):
    sc, f, r = frame
    assert r["count"].sum() == r["pairs"] > 10000
    assert ((r["count"] > 0) == (r["max"] > 0)).all() and ((r["count"] > 0) == (r["sum"] > 0)).all()
    assert (r["max"] <= 0.99).all() and (r["max"][r["count"] > 0] >= 1e-4 / 255).all()
    assert (r["sum"] <= r["count"] * r["max"] * (1 + 1e-12)).all() and (r["S"] >= 4 * r["sum"] * (1 - 1e-12)).all()
    assert (r["S_max"] >= 4 * np.maximum(r["max"], 0) * (1 - 1e-12)).all()
    # a third of the pixels masked out: those pairs are gone, the others keep their values
    e = np.ones((72, 104))
    e.reshape(-1)[::3] = 0.0
    rm = R.contributions(f, 104, 72, pixel_weight=e)
    assert rm["count"].sum() == rm["pairs"] < r["pairs"] and (rm["count"] <= r["count"]).all() and (rm["max"] <= r["max"]).all()


def _two_stacked(alpha):
    """Two identical Gaussians on the centre of a 16 x 16 frame: one tile, both on its list."""
    return dict(xy=np.array([[8.0, 8.0], [8.0, 8.0]], np.float32),
                conic_opacity=np.array([[0.05, 0.0, 0.05, alpha]] * 2, np.float32),
                ranges=np.array([[0, 2]], np.uint32), point_list=np.array([0, 1], np.uint32))


def test_two_stacked_gaussians_give_alpha_times_one_minus_alpha():
    a = 0.5
    centre = np.zeros((16, 16))
    centre[8, 8] = 1.0
    r = R.contributions(_two_stacked(a), 16, 16, pixel_weight=centre)
    assert r["sum"].tolist() == [a, a * (1 - a)] and r["max"].tolist() == [a, a * (1 - a)] and r["count"].tolist() == [1, 1]
    assert r["S"].tolist() == [4 * a, 5 * a * (1 - a)] and r["S_max"].tolist() == r["S"].tolist() and r["pairs"] == 2
    # an opaque pair: alpha clamps to 0.99
    r = R.contributions(_two_stacked(1.0), 16, 16, pixel_weight=centre)
    assert r["sum"][0] == 0.99 and r["count"][0] == 1
    # a negative weight enters the sum, never the count; the maximum of the call is the (negative) product
    r = R.contributions(_two_stacked(a), 16, 16, pixel_weight=-centre)
    assert r["sum"].tolist() == [-a, -a * (1 - a)] and r["count"].tolist() == [0, 0] and r["max"].tolist() == [-a, -a * (1 - a)]
    ws, wm, pc = R.accumulate((np.zeros(2), np.zeros(2), np.zeros(2, np.int64)), r)
    assert wm.tolist() == [0, 0] and pc.tolist() == [0, 0] and ws.tolist() == r["sum"].tolist()


def test_an_all_zero_weight_image_leaves_the_arrays_untouched(frame):
    sc, f, r = frame
    rz = R.contributions(f, 104, 72, pixel_weight=np.zeros((72, 104)))
    assert rz["pairs"] == 0 and not rz["sum"].any() and not rz["count"].any() and (rz["max"] == -np.inf).all()
    before = (np.full(600, 1.5), np.full(600, -0.25), np.full(600, 7, np.int64))
    after = R.accumulate(before, rz)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_float32_evaluation_stays_inside_the_bound(frame):
    """The bound the GPU test holds the kernel to, |x - ref| <= 1e-4 |ref| + C_BOUND 2^-24 S, against an honest float32
    evaluation of the definition (numpy: sequential float32 products, its own expf): inside, with room -- the bound is not
    one that only a float64 computation could meet."""
    sc, f, r = frame
    e = np.random.default_rng(5).random((72, 104)).astype(np.float32)
    for pw, r64 in ((None, r), (e, R.contributions(f, 104, 72, pixel_weight=e))):
        r32 = R.contributions(f, 104, 72, pixel_weight=pw, dtype=np.float32)
        assert np.array_equal(r32["count"], r64["count"]) and np.array_equal(r32["n_contrib"], r64["n_contrib"])
        c_sum = R.needed_constant(r32["sum"], r64["sum"], r64["S"])
        hit = r64["count"] > 0
        c_max = R.needed_constant(r32["max"][hit], r64["max"][hit], r64["S_max"][hit])
        print(f"float32 restatement: C needed {c_sum:.3f} (sum), {c_max:.3f} (max); C_BOUND = {Hh.C_BOUND}")
        assert c_sum <= Hh.C_BOUND and c_max <= Hh.C_BOUND, (c_sum, c_max)
        # ... and not by being loose: the float32 values do differ from the float64 ones
        assert (r32["sum"] != r64["sum"]).any()
