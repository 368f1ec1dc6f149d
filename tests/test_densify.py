"""CPU checks of the densify / prune of the cloud (densify.hip, hs_densify_*, casualhdrsplat_amd.densify): the C ABI
(exports, struct layout, argument validation before any HIP call, the workspace formula), the numpy restatement the GPU
tests compare bits with (tests/densify_reference.py) pinned against a literal torch restatement of the published procedure,
the measured constant of the raw-scale bound, the Python argument errors and the optimizer's tensor swap, and the kernels'
resources."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import densify_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_densify_workspace_bytes", "hs_densify_plan", "hs_densify_apply")

RAW_MEAN_C_MEASURED, RAW_MEAN_BAR, SIZES, case_seed = R.RAW_MEAN_C_MEASURED, R.RAW_MEAN_BAR, R.SIZES, R.case_seed


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- C ABI ----

def test_densify_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    for n in ("hs_densify_args", "hs_densify_matrix"):
        assert re.search(rf"\}}\s*{n}\s*;", header), n
    assert set(NAMES) <= set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309        # (detected by name: the version does not move)


def test_densify_structs_match_c(lib, tmp_path):
    A, M = lib.hs_densify_args, lib.hs_densify_matrix
    a_fields = [n for n, _ in A._fields_]
    m_fields = [n for n, _ in M._fields_]
    consts = ["HS_DENSIFY_MAX_MATRICES", "HS_DENSIFY_RAW_OPACITY", "HS_DENSIFY_RAW_SCALES", "HS_DENSIFY_COPY", "HS_DENSIFY_ZERO_NEW",
              "HS_DENSIFY_MEANS", "HS_DENSIFY_SCALES", "HS_DENSIFY_KIND_SURVIVOR", "HS_DENSIFY_KIND_CLONE", "HS_DENSIFY_KIND_CHILD0",
              "HS_DENSIFY_KIND_CHILD1", "HS_DENSIFY_COUNTS"]
    lines = ['printf("%zu %zu\\n", sizeof(hs_densify_args), sizeof(hs_densify_matrix));']
    lines += [f'printf("%zu\\n", offsetof(hs_densify_args, {n}));' for n in a_fields]
    lines += [f'printf("%zu\\n", offsetof(hs_densify_matrix, {n}));' for n in m_fields]
    lines += [f'printf("%d\\n", {c});' for c in consts]
    lines += ['{ float f = HS_DENSIFY_LOG_1_6; unsigned u; memcpy(&u, &f, 4); printf("%u\\n", u); }']
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(A), C.sizeof(M)] + [getattr(A, n).offset for n in a_fields] + [getattr(M, n).offset for n in m_fields] + \
        [getattr(lib, c) for c in consts] + [int(R.LOG_1_6.view(np.uint32))]
    assert got == want


def test_workspace_bytes_is_the_documented_formula(lib):
    L = lib.load()
    for P in (0, 1, 255, 256, 257, 10007, 1_000_000, (1 << 30) - 1):
        assert L.hs_densify_workspace_bytes(P) == (P + 255) // 256 * 256 + 16 * ((P + 255) // 256), P
    for P in (-1, 1 << 30, 1 << 40):
        assert L.hs_densify_workspace_bytes(P) == lib.HS_EINVAL
        assert b"hs_densify_workspace_bytes" in L.hs_last_error() and f"P={P}".encode() in L.hs_last_error()


def test_plan_and_apply_validate_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the field -- on a machine without a GPU: no HIP call is
    made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy addresses: validation must fail before any of them is dereferenced

    def call(fn, n=2, matrix=None, **kw):
        mats = (lib.hs_densify_matrix * max(n, 1))()
        for i in range(max(n, 1)):
            mats[i].src, mats[i].dst, mats[i].row_stride, mats[i].role = one, 2 * one, 3, lib.HS_DENSIFY_MEANS
        for k, v in (matrix or {}).items():
            setattr(mats[n - 1], k, v)
        a = lib.hs_densify_args()
        a.P, a.P_out, a.flags, a.r_max = 100, 150, 3, 20
        a.tau_grad, a.tau_split, a.o_min, a.sigma_max = 2e-4, -3.0, -5.0, math.inf
        for f in ("grad_accum", "denom", "max_radii", "opacities", "scales", "rotations", "noise", "workspace", "row_map", "counts"):
            setattr(a, f, one)
        a.counts_host = None
        a.matrices, a.n_matrices = mats, n
        for k, v in kw.items():
            setattr(a, k, v)
        rc = getattr(L, fn)(C.byref(a), None)
        return rc, L.hs_last_error()

    for fn in ("hs_densify_plan", "hs_densify_apply"):
        assert getattr(L, fn)(None, None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    common = [(dict(P=-1), b"P=-1"), (dict(P=1 << 30), b"P=1073741824"), (dict(flags=4), b"flags=4"), (dict(flags=-1), b"flags=-1")]
    plan = common + [
        (dict(r_max=-2), b"r_max=-2"), (dict(tau_grad=math.nan), b"tau_grad is NaN"), (dict(tau_split=math.nan), b"tau_split is NaN"),
        (dict(o_min=math.nan), b"o_min is NaN"), (dict(sigma_max=math.nan), b"sigma_max is NaN"),
        (dict(counts=None), b"null counts"), (dict(counts=one + 2), b"counts must be 4-byte aligned"),
        (dict(counts_host=one + 1), b"counts_host must be 4-byte aligned"),
        (dict(grad_accum=None), b"null grad_accum"), (dict(denom=None), b"null denom"), (dict(max_radii=None), b"null max_radii"),
        (dict(opacities=None), b"null opacities"), (dict(scales=None), b"null scales"), (dict(row_map=None), b"null row_map"),
        (dict(denom=one + 2), b"denom must be 4-byte aligned"), (dict(scales=one + 1), b"scales must be 4-byte aligned"),
        (dict(workspace=None), b"null workspace"), (dict(workspace=one + 8), b"workspace must be 16-byte aligned"),
    ]
    apply = common + [
        (dict(P_out=-1), b"P_out=-1"), (dict(P_out=201), b"P_out=201 outside [0, 2 P = 200]"),
        (dict(n=0), b"n_matrices=0"), (dict(n=17), b"n_matrices=17"), (dict(n_matrices=-1), b"n_matrices=-1"),
        (dict(matrices=None), b"null matrices"),
        (dict(matrix=dict(role=4)), b"matrices[1].role=4"), (dict(matrix=dict(role=-1)), b"matrices[1].role=-1"),
        (dict(matrix=dict(row_stride=0, role=0)), b"matrices[1].row_stride=0"),
        (dict(matrix=dict(row_stride=4)), b"matrices[1].row_stride=4: the MEANS and SCALES roles take rows of 3"),
        (dict(matrix=dict(row_stride=48, role=lib.HS_DENSIFY_SCALES)), b"matrices[1].row_stride=48"),
        (dict(matrix=dict(row_stride=1 << 36, role=0)), b"reaches 2^40"),
        (dict(matrix=dict(src=None)), b"matrices[1]: null src/dst"), (dict(matrix=dict(dst=None)), b"matrices[1]: null src/dst"),
        (dict(matrix=dict(src=one + 2)), b"matrices[1]: src/dst must be 4-byte aligned"),
        (dict(matrix=dict(dst=one)), b"matrices[1]: dst must not be src"),
        (dict(row_map=None), b"null row_map"), (dict(row_map=one + 2), b"row_map must be 4-byte aligned"),
        (dict(scales=None), b"null scales"), (dict(rotations=None), b"null rotations"), (dict(noise=None), b"null noise"),
        (dict(noise=one + 3), b"noise must be 4-byte aligned"),
    ]
    for fn, cases in (("hs_densify_plan", plan), ("hs_densify_apply", apply)):
        for kw, text in cases:
            rc, msg = call(fn, **kw)
            assert rc == lib.HS_EINVAL, (fn, kw, rc, msg)
            assert msg.startswith(fn.encode()) and text in msg, (fn, kw, msg)


# ---- the restatement ----

def _build_rotation(r):
    """Upstream's build_rotation (utils/general_utils.py), restated."""
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    R_ = torch.zeros((q.size(0), 3, 3), dtype=r.dtype)
    r_, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R_[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R_[:, 0, 1] = 2 * (x * y - r_ * z)
    R_[:, 0, 2] = 2 * (x * z + r_ * y)
    R_[:, 1, 0] = 2 * (x * y + r_ * z)
    R_[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R_[:, 1, 2] = 2 * (y * z - r_ * x)
    R_[:, 2, 0] = 2 * (x * z - r_ * y)
    R_[:, 2, 1] = 2 * (y * z + r_ * x)
    R_[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R_


def torch_densify_and_prune(case):
    """The published densify_and_prune (scene/gaussian_model.py: densify_and_clone, densify_and_split with N = 2,
    prune_points; restated from the publication, no upstream source is at hand) through boolean masks, cat and repeat, on
    the ACTIVATED values with the linear thresholds.  Where it departs from upstream, by the header's rules: a row with
    denom == 0 counts as gradient 0 (upstream: NaN only), the children's normal samples are std x the given noise of the
    source row, and derived rows carry their source's radius to the screen-size test (upstream zeroes the radii).  The
    optimizer's part (cat_tensors_to_optimizer / _prune_optimizer) is the zeros appended to / the rows cut from the moments."""
    pol = case["policy"]
    N = 2
    t = {k: torch.tensor(v) for k, v in case["cloud"].items()}
    mom = {k: [torch.tensor(a), torch.tensor(b)] for k, (a, b) in case["moments"].items()}
    P = case["P"]
    scaling = (lambda: torch.exp(t["scales"])) if pol["raw_scales"] else (lambda: t["scales"])
    opacity = (lambda: torch.sigmoid(t["opacities"])) if pol["raw_opacity"] else (lambda: t["opacities"])
    inv_scaling = torch.log if pol["raw_scales"] else (lambda x: x)
    noise = torch.tensor(case["noise"])
    radii = torch.tensor(case["max_radii"])
    src, kind = torch.arange(P), torch.zeros(P, dtype=torch.long)
    grads = torch.tensor(case["grad_accum"]) / torch.tensor(case["denom"])
    grads[grads.isnan()] = 0.0
    grads[torch.tensor(case["denom"]) == 0] = 0.0
    extent, pd = pol["extent"], pol["percent_dense"]

    def postfix(new, new_radii, new_src, new_kind):
        nonlocal radii, src, kind
        for k in t:
            t[k] = torch.cat([t[k], new[k]], dim=0)
            mom[k] = [torch.cat([m, torch.zeros_like(new[k])], dim=0) for m in mom[k]]
        radii, src, kind = torch.cat([radii, new_radii]), torch.cat([src, new_src]), torch.cat([kind, new_kind])

    def prune_points(mask):
        nonlocal radii, src, kind
        valid = ~mask
        for k in t:
            t[k] = t[k][valid]
            mom[k] = [m[valid] for m in mom[k]]
        radii, src, kind = radii[valid], src[valid], kind[valid]

    # densify_and_clone
    sel = torch.where(grads >= pol["grad_threshold"], True, False)
    sel = torch.logical_and(sel, torch.max(scaling(), dim=1).values <= pd * extent)
    postfix({k: v[sel] for k, v in t.items()}, radii[sel], src[sel], torch.ones(int(sel.sum()), dtype=torch.long))
    # densify_and_split
    n_now = t["means3D"].shape[0]
    padded = torch.zeros(n_now)
    padded[:P] = grads
    sel = torch.where(padded >= pol["grad_threshold"], True, False)
    sel = torch.logical_and(sel, torch.max(scaling(), dim=1).values > pd * extent)
    stds = scaling()[sel].repeat(N, 1)
    xi = torch.cat([noise[src[sel], k] for k in range(N)], dim=0)
    samples = stds * xi                                         # (torch.normal(mean = 0, std = stds) with the given normals)
    rots = _build_rotation(t["rotations"][sel]).repeat(N, 1, 1)
    new = {k: v[sel].repeat(N, *([1] * (v.dim() - 1))) for k, v in t.items()}
    new["means3D"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["means3D"][sel].repeat(N, 1)
    new["scales"] = inv_scaling(scaling()[sel].repeat(N, 1) / (0.8 * N))
    n_sel = int(sel.sum())
    postfix(new, radii[sel].repeat(N), src[sel].repeat(N), torch.cat([torch.full((n_sel,), 2 + k, dtype=torch.long) for k in range(N)]))
    prune_points(torch.cat((sel, torch.zeros(N * n_sel, dtype=torch.bool))))
    # the prune of densify_and_prune
    prune_mask = (opacity() < pol["min_opacity"]).squeeze(-1)
    if pol["max_screen_size"]:
        big_points_vs = radii > pol["max_screen_size"]
        big_points_ws = scaling().max(dim=1).values > 0.1 * extent
        prune_mask = torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws)
    prune_points(prune_mask)
    return t, mom, (kind << 30 | src).numpy().astype(np.uint32)


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("M", [1, 4])
def test_the_restatement_is_the_published_procedure(raw, M):
    """Same row map, bit-identical copied columns and moments (zeros in every new row), child scales and means to float32
    rounding (upstream goes through exp / log and a batched matrix product; the restatement's order is the header's).
    With stored-linear values the child scales are the same single division: bit for bit."""
    case = R.make_case(20011, M, seed=5 + M, raw_scales=raw, raw_opacity=raw)
    th = R.thresholds(**case["policy"])
    new, mom, row_map, counts = R.densify(case, th)
    t, tmom, t_map = torch_densify_and_prune(case)
    assert np.array_equal(row_map, t_map)
    P = case["P"]
    assert counts[0] == row_map.size and counts[1] + counts[2] + counts[3] == counts[0] and counts[6] == P
    assert 0.08 * P < counts[2] < 0.12 * P and 0.04 * P < counts[5] < 0.06 * P and 0.03 * P < counts[4] < 0.08 * P   # clone / split / gone
    kind = row_map >> 30
    child = kind >= 2
    assert child.sum() == counts[3] and (kind == 1).sum() == counts[2]
    for k in ("opacities", "shs", "rotations"):
        assert R.same_bits(new[k], t[k].numpy()), k
    for k in R.NAMES:
        assert R.same_bits(new[k][~child], t[k].numpy()[~child]), k
        for a, b in zip(mom[k], tmom[k]):
            assert R.same_bits(a, b.numpy()), k
            assert not a[kind != 0].any() and a[kind == 0].all()
    if raw:
        assert np.allclose(new["scales"][child], t["scales"].numpy()[child], rtol=0, atol=4 * 2.0 ** -24 * 8)   # |log sigma| < 8
    else:
        assert R.same_bits(new["scales"], t["scales"].numpy())
    src = (row_map & R.SRC_MASK)[child]
    _, mag = R.child_means(case["cloud"]["means3D"], case["cloud"]["scales"], case["cloud"]["rotations"], case["noise"], src,
                           kind[child].astype(np.int64) - 2, raw)
    err = np.abs(new["means3D"][child].astype(np.float64) - t["means3D"].numpy()[child].astype(np.float64))
    assert (err <= 2 * RAW_MEAN_BAR * 2.0 ** -24 * mag).all(), float((err / (2.0 ** -24 * mag)).max())     # (two fp32 evaluations)


def test_thresholds_are_converted_in_float64_to_the_space_of_the_values(lib):
    from casualhdrsplat_amd.densify import stored_thresholds
    for raw_s in (False, True):
        for raw_o in (False, True):
            for screen in (None, 0, 20):
                kw = dict(extent=5.3, grad_threshold=2e-4, percent_dense=0.01, min_opacity=0.005, max_screen_size=screen)
                th = R.thresholds(raw_scales=raw_s, raw_opacity=raw_o, **kw)
                got = stored_thresholds(kw["extent"], kw["grad_threshold"], kw["percent_dense"], kw["min_opacity"], screen, raw_s, raw_o)
                a = lib.hs_densify_args()
                for k, v in got.items():
                    setattr(a, k, v)
                for k in ("tau_grad", "tau_split", "o_min", "sigma_max"):
                    assert np.float32(getattr(a, k)) == th[k], (k, raw_s, raw_o, screen)
                assert a.r_max == th["r_max"] and a.flags == (2 if raw_s else 0) + (1 if raw_o else 0)
                assert (a.sigma_max == math.inf) == (not screen)
    th = R.thresholds(5.3, raw_scales=True, raw_opacity=True, max_screen_size=20)
    assert th["tau_split"] == np.float32(math.log(0.053)) and th["o_min"] == np.float32(math.log(0.005 / 0.995))
    assert th["sigma_max"] == np.float32(math.log(0.53))
    assert stored_thresholds(1.0, 0.0, 0.01, 0.0, None, True, True)["o_min"] == -math.inf
    assert stored_thresholds(1.0, 0.0, 0.01, 1.0, None, True, True)["o_min"] == math.inf
    with pytest.raises(ValueError, match="extent"):
        stored_thresholds(0.0, 2e-4, 0.01, 0.005, None, True, True)


def test_reference_edge_rows():
    """denom == 0 and NaN statistics count as gradient 0; a clone is pruned with its source; children are tested with the
    child's scale and the source's radius."""
    f = lambda *x: np.array(x, dtype=np.float32)          # noqa: E731
    th = R.thresholds(10.0, grad_threshold=1.0, percent_dense=0.1, min_opacity=0.1, max_screen_size=50, raw_scales=False, raw_opacity=False)
    #            0 plain  1 x/0   2 NaN   3 clone  4 clone,o  5 split   6 split,r  7 split: child 1.5/1.6 <= 1  8 big, unselected  9 transparent
    ga = f(0.5, 9.0, np.nan, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0)
    dn = f(1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    rad = np.array([0, 0, 0, 50, 0, 0, 51, 0, 0, 0], dtype=np.int32)
    opa = f(0.5, 0.5, 0.5, 0.5, 0.05, 0.5, 0.5, 0.5, 0.5, 0.0999)
    sc = np.full((10, 3), 0.5, dtype=np.float32)
    sc[5, 1] = sc[6, 2] = 1.2
    sc[7, 0] = 1.5
    sc[8, 1] = 1.5
    codes, row_map, counts = R.plan(ga, dn, rad, opa, sc, th)
    assert codes.tolist() == [1, 1, 1, 2, 0, 3, 0, 3, 0, 0]
    assert row_map.tolist() == [0, 1, 2, 3, (1 << 30) | 3, (2 << 30) | 5, (2 << 30) | 7, (3 << 30) | 5, (3 << 30) | 7]
    assert counts == [9, 4, 1, 4, 4, 3, 10, 0]


def test_raw_mean_bar_is_twice_the_measured_constant():
    """The constant of the raw-scale bound, measured: worst c of the float32 restatement against float64 over the eight
    raw-scale cases the GPU test runs; the bar is twice that, rounded up to a power of two."""
    worst = 0.0
    for P, M in SIZES:
        case = R.make_case(P, M, seed=case_seed(P, M))
        th = R.thresholds(**case["policy"])
        _, row_map, _ = R.plan(case["grad_accum"], case["denom"], case["max_radii"], case["cloud"]["opacities"], case["cloud"]["scales"], th)
        c = R.raw_mean_c(case, th, row_map)
        print(f"P={P} M={M}: c = {c:.4f}")
        worst = max(worst, c)
    print(f"worst c = {worst:.4f}; bar {RAW_MEAN_BAR}")
    assert abs(worst - RAW_MEAN_C_MEASURED) < 0.01
    assert RAW_MEAN_BAR == 2.0 ** math.ceil(math.log2(2.0 * worst))


# ---- Python ----

def _host_cloud(monkeypatch, P=12, M=4):
    from casualhdrsplat_amd import cloud_param_groups, optim
    monkeypatch.setattr(optim, "_require_gpu", lambda t, what: None)
    t = {k: torch.zeros(P, *s, requires_grad=True) for k, s in (("means3D", (3,)), ("opacities", (1,)), ("shs", (M, 3)),
                                                                  ("scales", (3,)), ("rotations", (4,)))}
    return t, optim.GaussianAdam(cloud_param_groups(**t), eps=1e-15)


def test_python_raises_on_cpu_tensors_and_bad_arguments(monkeypatch):
    import casualhdrsplat_amd as pkg
    from casualhdrsplat_amd import DensifyStats, densify
    assert pkg.densify_and_prune is densify.densify_and_prune and pkg.DensifyResult is densify.DensifyResult
    t, opt = _host_cloud(monkeypatch)
    stats = DensifyStats(12, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        densify.densify_and_prune(opt, stats, extent=1.0)
    with pytest.raises(TypeError, match="GaussianAdam"):
        densify.densify_and_prune(torch.optim.Adam([t["means3D"]]), stats, extent=1.0)
    # with the device guard lifted, what is looked at before the library: names, shapes, statistics, thresholds
    monkeypatch.setattr(densify, "_require_gpu", lambda t, what: None)
    with pytest.raises(TypeError, match="DensifyStats"):
        densify.densify_and_prune(opt, None, extent=1.0)
    with pytest.raises(ValueError, match=r"stats.grad_accum must be .*\[12\]"):
        densify.densify_and_prune(opt, DensifyStats(11, device="cpu"), extent=1.0)
    with pytest.raises(ValueError, match="extent"):
        densify.densify_and_prune(opt, stats, extent=-1.0)
    with pytest.raises(ValueError, match="noise must be"):
        densify.densify_and_prune(opt, stats, extent=1.0, noise=torch.zeros(12, 3, 2))
    from casualhdrsplat_amd import optim
    with pytest.raises(ValueError, match="no group for .*rotations"):
        densify._cloud_of(optim.GaussianAdam([dict(params=[t[k]], name=n, per_gaussian=True) for k, n in
                                              (("means3D", "xyz"), ("opacities", "opacity"), ("shs", "f_dc"), ("scales", "scaling"))]))
    with pytest.raises(ValueError, match="per_gaussian group 'extra'"):
        densify._cloud_of(optim.GaussianAdam([dict(params=[t["means3D"]], name="extra", per_gaussian=True)]))
    with pytest.raises(ValueError, match="3 floats per Gaussian"):
        densify._cloud_of(optim.GaussianAdam([dict(params=[t["rotations"]], name="xyz", per_gaussian=True)]))
    found = densify._cloud_of(opt)
    assert all(found[k] is t[k] for k in t)


def test_replace_params_swaps_tensors_and_keeps_the_device_tables(monkeypatch):
    t, opt = _host_cloud(monkeypatch)
    extra = torch.zeros(5, requires_grad=True)
    opt.add_param_group(dict(params=[extra], lr=1e-3))
    opt.prepare()
    state_before, hyper_before, entries_before = opt._dev_state, opt._dev_hyper, list(opt._entries)
    new = {k: (torch.ones(20, *v.shape[1:], requires_grad=True), torch.full((20, *v.shape[1:]), 2.0), torch.full((20, *v.shape[1:]), 3.0))
           for k, v in t.items()}
    opt.replace_params({t[k]: new[k] for k in t})
    assert opt._dev_state is state_before and opt._dev_hyper is hyper_before             # step count and products: untouched
    assert [g["name"] for g in opt.param_groups[:6]] == ["xyz", "opacity", "f_dc", "f_rest", "scaling", "rotation"]
    assert opt.param_groups[2]["params"][0] is new["shs"][0] and opt.param_groups[3]["params"][0] is new["shs"][0]
    assert [gi for gi, _ in opt._entries] == [gi for gi, _ in entries_before]
    assert all(any(p is new[k][0] for _, p in opt._entries) for k in t) and not any(p is t[k] for _, p in opt._entries for k in t)
    assert any(p is extra for _, p in opt._entries)
    for k in t:
        assert t[k] not in opt.state
        st = opt.state[new[k][0]]
        assert st["exp_avg"] is new[k][1] and st["exp_avg_sq"] is new[k][2] and "step" in st
    assert len(opt.state_dict()["state"]) == 6
    with pytest.raises(ValueError, match="not one of the optimizer's parameters"):
        opt.replace_params({t["shs"]: new["shs"]})
    with pytest.raises(ValueError, match="shape"):
        opt.replace_params({new["shs"][0]: (torch.ones(7, 4, 3, requires_grad=True), torch.ones(7, 4, 3), torch.ones(6, 4, 3))})
    with pytest.raises(ValueError, match="float32"):
        opt.replace_params({new["shs"][0]: (torch.ones(7, 4, 3, dtype=torch.float64), torch.ones(7, 4, 3), torch.ones(7, 4, 3))})


def test_densify_stats_resize():
    from casualhdrsplat_amd import DensifyStats
    s = DensifyStats(5, device="cpu")
    s.grad_accum += 1.0
    s.max_radii += 3
    s.resize(9)
    for x, dt in ((s.grad_accum, torch.float32), (s.denom, torch.float32), (s.max_radii, torch.int32)):
        assert x.shape == (9,) and x.dtype == dt and not x.any()


# ---- resources ----

def test_densify_kernels_spill_nothing_and_need_no_scratch(tmp_path):
    src = os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "densify.hip")
    asm = str(tmp_path / "densify.s")
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
    kernels = sorted(re.search(r"densify_\w+?_kernel", k).group() for k in out)
    assert kernels == ["densify_apply_kernel", "densify_classify_kernel", "densify_map_kernel", "densify_scan_kernel"], sorted(out)
    for k, v in out.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 8, (k, v)
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0"] * 4
    assert re.findall(r"\.amdhsa_float_denorm_mode_32 (\d+)", text) == ["3"] * 4            # denormals kept
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text                    # 16-byte accesses where they fit
    assert "v_div_fixup_f32" in text and "v_sqrt_f32" in text                                  # IEEE division and square root
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic|\bds_\w+_rtn", text) and "scratch_" not in text   # no atomics anywhere
    body = open(src, encoding="utf-8").read()
    assert not re.search(r"hipMem(set|cpy)\w*\(", body)                                        # cleared and copied by kernels only
