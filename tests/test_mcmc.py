"""CPU checks of the MCMC refinement of the cloud (mcmc.hip, hs_mcmc_*, casualhdrsplat_amd.mcmc): the C ABI (exports, struct
layout, the workspace formula, argument validation before any HIP call), the numpy restatement the GPU tests compare with
(tests/mcmc_reference.py) pinned against a literal torch restatement of the published relocate / sample_add /
inject_noise_to_position, the sampler's frequencies, the measured constant of the noise bound, the Python argument errors,
and the kernels' resources."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mcmc_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_mcmc_workspace_bytes", "hs_mcmc_sample", "hs_mcmc_update", "hs_mcmc_noise")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- C ABI ----

def test_mcmc_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    for n in ("hs_mcmc_args", "hs_mcmc_noise_args"):
        assert re.search(rf"\}}\s*{n}\s*;", header), n
    assert set(NAMES) <= set(lib.EXPORTS)
    assert set(re.findall(r"\bHS_API\s+[\w\s\*]+?\b(hs_\w+)\s*\(", header)) == set(lib.EXPORTS)      # header == EXPORTS still holds
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309        # (detected by name: the version does not move)


def test_mcmc_structs_match_c(lib, tmp_path):
    A, N = lib.hs_mcmc_args, lib.hs_mcmc_noise_args
    a_fields = [n for n, _ in A._fields_]
    n_fields = [n for n, _ in N._fields_]
    consts = ["HS_MCMC_RELOCATE", "HS_MCMC_GROW", "HS_MCMC_COUNTS"]
    lines = ['printf("%zu %zu\\n", sizeof(hs_mcmc_args), sizeof(hs_mcmc_noise_args));']
    lines += [f'printf("%zu\\n", offsetof(hs_mcmc_args, {n}));' for n in a_fields]
    lines += [f'printf("%zu\\n", offsetof(hs_mcmc_noise_args, {n}));' for n in n_fields]
    lines += [f'printf("%d\\n", {c});' for c in consts]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(A), C.sizeof(N)] + [getattr(A, n).offset for n in a_fields] + [getattr(N, n).offset for n in n_fields] + \
        [getattr(lib, c) for c in consts]
    assert got == want


def test_workspace_bytes_is_the_documented_formula(lib):
    from casualhdrsplat_amd.mcmc import workspace_layout
    L = lib.load()
    a = lambda x: (x + 255) // 256 * 256        # noqa: E731
    for P in (0, 1, 255, 256, 257, 10007, 1_000_000, (1 << 30) - 1):
        for n in (0, 1, P // 20, P):
            want = a(8 * P) + a(16 * ((P + 255) // 256 + 1)) + a(4 * P) + a(4 * n)
            assert L.hs_mcmc_workspace_bytes(P, n) == want == workspace_layout(P, n)["bytes"], (P, n)
    for P in (-1, 1 << 30, 1 << 40):
        assert L.hs_mcmc_workspace_bytes(P, 0) == lib.HS_EINVAL
        assert b"hs_mcmc_workspace_bytes" in L.hs_last_error() and f"P={P}".encode() in L.hs_last_error()
    for n in (-1, 1 << 30):
        assert L.hs_mcmc_workspace_bytes(10, n) == lib.HS_EINVAL and f"n_draws={n}".encode() in L.hs_last_error()


def test_entry_points_validate_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the field -- on a machine without a GPU: no HIP call is
    made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy addresses: validation must fail before any of them is dereferenced

    def call(fn, matrix=None, **kw):
        mats = (lib.hs_densify_matrix * 17)()
        for m in mats:
            m.src, m.dst, m.row_stride, m.role = None, one, 3, lib.HS_DENSIFY_COPY
        for k, v in (matrix or {}).items():
            setattr(mats[1], k, v)
        a = lib.hs_mcmc_args()
        a.P, a.n_draws, a.mode, a.flags, a.o_min, a.min_opacity = 100, 100, lib.HS_MCMC_RELOCATE, 3, -5.3, 0.005
        for f in ("opacities", "scales", "u", "workspace", "row_map", "counts"):
            setattr(a, f, one)
        a.counts_host = None
        a.matrices, a.n_matrices = mats, 15
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, fn)(C.byref(a), None), L.hs_last_error()

    for fn in ("hs_mcmc_sample", "hs_mcmc_update", "hs_mcmc_noise"):
        assert getattr(L, fn)(None, None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    grow = dict(mode=lib.HS_MCMC_GROW)
    common = [(dict(P=-1), b"P=-1"), (dict(P=1 << 30), b"P=1073741824"), (dict(mode=2), b"mode=2"), (dict(mode=-1), b"mode=-1"),
              (dict(flags=4), b"flags=4"), (dict(flags=-1), b"flags=-1"), (dict(n_draws=99), b"n_draws=99"),
              (dict(grow, n_draws=101), b"n_draws=101 outside [0, P = 100]"), (dict(grow, n_draws=-1), b"n_draws=-1"),
              (dict(workspace=None), b"null workspace"), (dict(workspace=one + 8), b"workspace must be 16-byte aligned"),
              (dict(opacities=None), b"null opacities"), (dict(opacities=one + 2), b"opacities must be 4-byte aligned")]
    sample = common + [
        (dict(o_min=math.nan), b"o_min is NaN"), (dict(counts=None), b"null counts"), (dict(counts=one + 2), b"counts must be 4-byte aligned"),
        (dict(counts_host=one + 1), b"counts_host must be 4-byte aligned"), (dict(u=None), b"null u"),
        (dict(u=one + 4), b"u must be 8-byte aligned"), (dict(grow, n_draws=5, row_map=None), b"null row_map"),
        (dict(grow, n_draws=5, row_map=one + 2), b"row_map must be 4-byte aligned")]
    update = common + [
        (dict(min_opacity=-0.1), b"min_opacity=-0.1"), (dict(min_opacity=1.5), b"min_opacity=1.5"), (dict(min_opacity=math.nan), b"min_opacity="),
        (dict(scales=None), b"null scales"), (dict(scales=one + 1), b"scales must be 4-byte aligned"),
        (dict(n_matrices=-1), b"n_matrices=-1"), (dict(n_matrices=17), b"n_matrices=17"), (dict(matrices=None), b"null matrices"),
        (dict(matrix=dict(role=lib.HS_DENSIFY_MEANS)), b"matrices[1].role=2"), (dict(matrix=dict(role=-1)), b"matrices[1].role=-1"),
        (dict(matrix=dict(row_stride=0)), b"matrices[1].row_stride=0"), (dict(matrix=dict(row_stride=1 << 36)), b"reaches 2^40"),
        (dict(matrix=dict(dst=None)), b"matrices[1]: null dst"), (dict(matrix=dict(dst=one + 2)), b"matrices[1]: dst must be 4-byte aligned"),
        (dict(matrix=dict(src=2 * one)), b"matrices[1]: src must be NULL or dst")]
    for fn, cases in (("hs_mcmc_sample", sample), ("hs_mcmc_update", update)):
        for kw, text in cases:
            rc, msg = call(fn, **kw)
            assert rc == lib.HS_EINVAL, (fn, kw, rc, msg)
            assert msg.startswith(fn.encode()) and text in msg, (fn, kw, msg)

    def noise(**kw):
        a = lib.hs_mcmc_noise_args()
        a.P, a.flags, a.scaler = 100, 3, 80.0
        for f in ("means3D", "opacities", "scales", "rotations", "xi"):
            setattr(a, f, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.hs_mcmc_noise(C.byref(a), None), L.hs_last_error()

    for kw, text in [(dict(P=-1), b"P=-1"), (dict(P=1 << 30), b"P=1073741824"), (dict(flags=8), b"flags=8"),
                     (dict(scaler=math.inf), b"scaler=inf"), (dict(scaler=math.nan), b"scaler="), (dict(means3D=None), b"null means3D"),
                     (dict(opacities=None), b"null opacities"), (dict(scales=None), b"null scales"), (dict(rotations=None), b"null rotations"),
                     (dict(xi=None), b"null xi"), (dict(xi=one + 2), b"xi must be 4-byte aligned"),
                     (dict(rotations=one + 1), b"rotations must be 4-byte aligned")]:
        rc, msg = noise(**kw)
        assert rc == lib.HS_EINVAL and msg.startswith(b"hs_mcmc_noise") and text in msg, (kw, rc, msg)
    assert noise(P=0, means3D=None, xi=None)[0] == lib.HS_OK                       # nothing to do, no pointer looked at


# ---- the restatement against the published procedure ----

def _binoms(dtype):
    n_max = R.N_MAX
    b = torch.zeros((n_max, n_max), dtype=dtype)
    for n in range(n_max):
        for k in range(n + 1):
            b[n, k] = math.comb(n, k)
    return b


def torch_compute_relocation(opacities, scales, ratios, binoms):
    """The published compute_relocation (Eq. 9 of the paper; upstream runs it as a CUDA kernel, one thread per row),
    restated from the publication: ratios clamped to n_max = 51, the 51 x 51 binomial table, the double loop."""
    n_max = binoms.shape[0]
    ratios = ratios.clamp(min=1, max=n_max)
    new_opacities = 1.0 - torch.pow(1.0 - opacities, 1.0 / ratios.to(opacities.dtype))
    denom_sum = torch.zeros_like(opacities)
    for i in range(1, n_max + 1):
        on = ratios >= i
        if not on.any():
            break
        for k in range(i):
            term = binoms[i - 1, k] * ((-1.0) ** k / math.sqrt(k + 1)) * torch.pow(new_opacities, k + 1)
            denom_sum = denom_sum + torch.where(on, term, torch.zeros_like(term))
    coeff = opacities / denom_sum
    return new_opacities, coeff[:, None] * scales


def torch_relocate(case, sampled_idxs, dtype):
    """The published relocate (gsplat's MCMCStrategy; restated from the publication): index assignment on every parameter,
    bincount for the ratios, zeros into both moments of the sampled rows.  `sampled_idxs` (one source per dead row)
    replaces torch.multinomial."""
    p = {k: torch.tensor(v, dtype=dtype) for k, v in case["cloud"].items()}
    mom = {k: [torch.tensor(a), torch.tensor(b)] for k, (a, b) in case["moments"].items()}
    min_opacity = case["min_opacity"]
    opacities = torch.sigmoid(p["opacities"].flatten())
    with np.errstate(all="ignore"):
        dead_mask = torch.tensor(~(case["cloud"]["opacities"].reshape(-1) > R.stored_o_min(min_opacity, True)))
    dead_indices = dead_mask.nonzero(as_tuple=True)[0]
    sampled_idxs = torch.as_tensor(sampled_idxs, dtype=torch.long)
    assert sampled_idxs.shape == dead_indices.shape
    new_opacities, new_scales = torch_compute_relocation(opacities[sampled_idxs], torch.exp(p["scales"])[sampled_idxs],
                                                         torch.bincount(sampled_idxs)[sampled_idxs] + 1, _binoms(dtype))
    new_opacities = torch.clamp(new_opacities, max=1.0 - torch.finfo(torch.float32).eps, min=min_opacity)
    p["opacities"][sampled_idxs] = torch.logit(new_opacities)[:, None]
    p["scales"][sampled_idxs] = torch.log(new_scales)
    for k in p:
        p[k][dead_indices] = p[k][sampled_idxs]
    for k in mom:
        for v in mom[k]:
            v[sampled_idxs] = 0
    return p, mom, (new_opacities, sampled_idxs)


def torch_sample_add(case, sampled_idxs, dtype):
    """The published sample_add: the same correction, the sampled rows appended (cat), zeros appended to both moments."""
    p = {k: torch.tensor(v, dtype=dtype) for k, v in case["cloud"].items()}
    mom = {k: [torch.tensor(a), torch.tensor(b)] for k, (a, b) in case["moments"].items()}
    opacities = torch.sigmoid(p["opacities"].flatten())
    sampled_idxs = torch.as_tensor(sampled_idxs, dtype=torch.long)
    new_opacities, new_scales = torch_compute_relocation(opacities[sampled_idxs], torch.exp(p["scales"])[sampled_idxs],
                                                         torch.bincount(sampled_idxs)[sampled_idxs] + 1, _binoms(dtype))
    new_opacities = torch.clamp(new_opacities, max=1.0 - torch.finfo(torch.float32).eps, min=case["min_opacity"])
    p["opacities"][sampled_idxs] = torch.logit(new_opacities)[:, None]
    p["scales"][sampled_idxs] = torch.log(new_scales)
    for k in p:
        p[k] = torch.cat([p[k], p[k][sampled_idxs]])
        mom[k] = [torch.cat([v, torch.zeros((len(sampled_idxs), *v.shape[1:]))]) for v in mom[k]]
    return p, mom


def torch_inject_noise(case, xi, scaler):
    """The published inject_noise_to_position: covariances from normalised quaternions and exp(scales) (R S)(R S)^T, the
    opacity gate 1 / (1 + exp(-100 ((1 - o) - 0.995))), einsum("bij,bj->bi")."""
    c = {k: torch.tensor(v) for k, v in case["cloud"].items()}
    opacities = torch.sigmoid(c["opacities"].flatten())
    scales = torch.exp(c["scales"])
    q = torch.nn.functional.normalize(c["rotations"], dim=-1)
    w, x, y, z = q.unbind(dim=-1)
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                      2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    M = Rm * scales[:, None, :]
    covars = torch.bmm(M, M.transpose(1, 2))

    def op_sigmoid(v, k=100, x0=0.995):
        return 1 / (1 + torch.exp(-k * (v - x0)))

    noise = torch.tensor(xi) * op_sigmoid(1 - opacities).unsqueeze(-1) * scaler
    noise = torch.einsum("bij,bj->bi", covars, noise)
    return c["means3D"] + noise


def _relocation_case(one_live=False):
    if one_live:                                   # one live row and 100 dead ones: the ratio clamps at 51
        case = R.make_case(101, 4, seed=3, dead_frac=0.0)
        case["cloud"]["opacities"][:] = -7.0
        case["cloud"]["opacities"][37] = 2.5
        case["cloud"]["opacities"][:, 0], _ = R.nudge(case["cloud"]["opacities"][:, 0], True)
        return case
    return R.make_case(4001, 4, seed=11, dead_frac=0.3)       # many dead rows: ratios up to a handful


@pytest.mark.parametrize("one_live", [False, True])
def test_relocation_is_the_published_procedure(one_live):
    """The restatement and the literal torch procedure, fed the SAME sources.  In float64 the two agree to 1e-9 in the stored
    values (two summation orders of D differ by 1e-14 of a sum whose condition reaches 1e4).  In float32 -- what upstream
    runs -- the new activated opacity x = 1 - (1 - o)^(1/r) carries the rounding of o against 1 - o:
        |dx| <= 2 u (3 + 5 / (1 - o)),  u = 2^-24   (o: 4 u relative; 1 - o: 5 u absolute; the root shrinks it; the
        subtraction adds u; doubled for torch's pow and sigmoid)
    and the scale factor o / D is held to the restatement's own D at x -+ that bound plus 2 u (terms + 4) cond.  Copies and
    the zeroed moments are identical."""
    case = _relocation_case(one_live)
    P = case["P"]
    new, mom, smp, (o64, s64) = R.relocate(case, case["u"], case["min_opacity"])
    dead = smp["sources"] >= 0
    assert dead.sum() == smp["counts"][1] == smp["counts"][2] > 0 and np.array_equal(dead, smp["dead"])
    assert int(smp["cnt"].max()) + 1 >= (101 if one_live else 4)
    upd = smp["cnt"] > 0
    for dtype in (torch.float64, torch.float32):
        t, tmom, (t_x, sampled) = torch_relocate(case, smp["sources"][dead], dtype)
        # structure: copies, untouched rows, moments -- identical
        src_of_dead = smp["sources"][dead]
        for k in R.NAMES:
            got = t[k].numpy()
            assert np.array_equal(got[dead], got[src_of_dead], equal_nan=True), k                  # a dead row IS its source
            keep = ~dead & ~upd
            assert R.DR.same_bits(got[keep].astype(np.float32), case["cloud"][k][keep]), k
            assert R.DR.same_bits(new[k][keep], case["cloud"][k][keep]) and R.DR.same_bits(new[k][dead], new[k][src_of_dead]), k
            if k in ("means3D", "shs", "rotations"):
                assert R.DR.same_bits(got.astype(np.float32), new[k]), k
            for a, b, old in zip(mom[k], tmom[k], case["moments"][k]):
                assert R.DR.same_bits(a, b.numpy()), k
                assert not a[upd].any() and R.DR.same_bits(a[~upd], old[~upd]), k
        got_o, got_s = t["opacities"].numpy().reshape(-1).astype(np.float64), t["scales"].numpy().astype(np.float64)
        if dtype == torch.float64:
            assert np.abs(got_o[upd] - o64[upd]).max() < 1e-9 and np.abs(got_s[upd] - s64[upd]).max() < 1e-9
            continue
        o = R.sigmoid64(case["cloud"]["opacities"].reshape(-1))
        ratio = np.minimum(smp["cnt"].astype(np.int64) + 1, R.N_MAX)
        x = 1.0 - np.power(1.0 - o, 1.0 / ratio)
        dx = 2 * U * (3 + 5 / (1 - o))
        x_t = np.zeros(P)
        x_t[sampled.numpy()] = t_x.numpy()
        xc = np.clip(x, case["min_opacity"], R.ONE_MINUS_EPS)
        assert (np.abs(x_t - xc)[upd] <= dx[upd] + U).all(), float((np.abs(x_t - xc)[upd] / dx[upd]).max())
        f = np.exp(s64[:, 0] - case["cloud"]["scales"][:, 0].astype(np.float64))               # o / D of the restatement
        f_t = np.exp(got_s[:, 0] - case["cloud"]["scales"][:, 0].astype(np.float64))
        for i in np.nonzero(upd)[0]:
            r = int(ratio[i])
            lo, hi = (R.factor(o[i], max(x[i] - dx[i], 0.0), r), R.factor(o[i], min(x[i] + dx[i], 1.0), r))
            (_, cond) = R.factor(o[i], x[i], r, with_cond=True)
            slack = 2 * U * (r * (r + 1) // 2 + 4) * cond * f[i] + 8 * U * f[i]
            assert min(lo, hi, f[i]) - slack <= f_t[i] <= max(lo, hi, f[i]) + slack, (i, r, f[i], f_t[i], lo, hi, slack)


def test_growth_is_the_published_procedure():
    case = R.make_case(3001, 4, seed=12)
    n_new = int(1.05 * case["P"]) - case["P"]
    new, mom, smp, (o64, s64) = R.grow(case, case["u"][:n_new], n_new, case["min_opacity"])
    assert smp["counts"][2] == n_new and (smp["sources"] >= 0).all()
    assert not np.isnan(case["cloud"]["opacities"].reshape(-1)[smp["sources"]]).any()             # a NaN row has weight 0
    t, tmom = torch_sample_add(case, smp["sources"], torch.float64)
    P = case["P"]
    upd = np.concatenate([smp["cnt"] > 0, np.ones(n_new, dtype=bool)])
    assert np.array_equal(smp["row_map"][:P], np.arange(P)) and np.array_equal(smp["row_map"][P:], smp["sources"].astype(np.uint32) | R.CLONE)
    for k in R.NAMES:
        got = t[k].numpy()
        assert got.shape == new[k].shape
        assert R.DR.same_bits(got[~upd].astype(np.float32), new[k][~upd]), k
        assert np.array_equal(got[P:], got[smp["sources"]], equal_nan=True) and R.DR.same_bits(new[k][P:], new[k][smp["sources"]]), k
        for a, b, old in zip(mom[k], tmom[k], case["moments"][k]):
            assert R.DR.same_bits(a, b.numpy()) and not a[P:].any() and R.DR.same_bits(a[:P], old), k     # sources keep their moments
    assert np.abs(t["opacities"].numpy().reshape(-1)[:P][smp["cnt"] > 0] - o64[smp["cnt"] > 0]).max() < 1e-9
    assert np.abs(t["scales"].numpy()[:P][smp["cnt"] > 0] - s64[smp["cnt"] > 0]).max() < 1e-9
    assert R.DR.same_bits(new["opacities"].reshape(-1)[:P][smp["cnt"] > 0], o64[smp["cnt"] > 0].astype(np.float32))


def test_noise_is_the_published_procedure():
    """Two float32 evaluations in different orders (upstream forms the covariance first): within twice the bar."""
    case = R.make_case(10007, 1, seed=R.case_seed(10007, 1))
    c = case["cloud"]
    ok = ~np.isnan(c["opacities"].reshape(-1))
    out, gs, mag = R.noise(c["means3D"], c["opacities"], c["scales"], c["rotations"], case["xi"], R.NOISE_SCALER, True, True)
    t = torch_inject_noise(case, case["xi"], float(np.float32(R.NOISE_SCALER))).numpy()
    err = np.abs(out.astype(np.float64) - t.astype(np.float64))[ok] / (U * mag[ok])
    assert (gs[ok] == 0).sum() > 100 and (gs[ok] != 0).sum() > 1000
    assert err.max() <= 2 * R.NOISE_BAR, float(err.max())
    assert np.isnan(out[~ok]).all() and R.DR.same_bits(out[ok & (gs == 0)], c["means3D"][ok & (gs == 0)])
    moved = np.abs(out - c["means3D"])[ok & (gs != 0)]
    assert moved.max() > 1e-4                                                    # the noise is not lost in the rounding


def _chi2_sf(x, k):
    """Survival function of chi-square with k degrees of freedom (Wilson-Hilferty: accurate to a few % for k > 30)."""
    z = ((x / k) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * k))) / math.sqrt(2.0 / (9.0 * k))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def test_sampler_frequencies_follow_the_weights():
    """200 rows, 2 x 10^5 draws from numpy's generator: chi-square of the source counts against w / S at p > 1e-3 for one
    fixed seed; dead and NaN rows are never drawn."""
    case = R.make_case(200, 1, seed=5, dead_frac=0.1)
    n = 200_000
    rng = np.random.default_rng(77)
    u = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64, endpoint=True)
    o = case["cloud"]["opacities"].reshape(-1)
    o_min = R.stored_o_min(case["min_opacity"], True)
    reloc = R.sample(o, u[:200], o_min, True, R.RELOCATE)
    dead = reloc["dead"]
    assert 5 < dead.sum() < 40 and np.isnan(o).sum() >= 1 and dead[np.isnan(o)].all()
    # the same prefix serves n draws: growth's sampler with the relocation's weights (dead rows at zero)
    smp = R.sample(np.where(dead, np.float32(-np.inf), o), u, o_min, True, R.GROW, n)
    w = reloc["w"].astype(np.float64)
    assert np.array_equal(smp["w"], reloc["w"]) and smp["cnt"].sum() == n
    assert not smp["cnt"][dead].any() and (smp["cnt"][~dead] > 0).all()
    expect = n * w[~dead] / w.sum()
    chi2 = float((((smp["cnt"][~dead] - expect) ** 2) / expect).sum())
    p = _chi2_sf(chi2, int((~dead).sum()) - 1)
    print(f"chi2 = {chi2:.1f} over {int((~dead).sum()) - 1} degrees of freedom, p = {p:.3f}")
    assert p > 1e-3


def test_draws_are_exact_integers():
    """Hand-checked rows: the weights, the prefix and mulhi64 draws at the boundaries of the 64-bit range."""
    o = np.array([0.0, np.nan, -40.0, 40.0, -6.0], dtype=np.float32)       # sigmoid: 1/2, -, 4e-18, 1, 0.00247 (dead)
    smp = R.sample(o, np.zeros(5, dtype=np.int64), R.stored_o_min(0.005, True), True, R.RELOCATE)
    assert smp["w"].tolist() == [1 << 23, 0, 0, 1 << 24, 0] and smp["dead"].tolist() == [False, True, True, False, True]
    S = 3 << 23
    u = np.array([0, (1 << 64) // 3 - 1, (1 << 64) // 3 + 1, (1 << 64) - 1, 1 << 63], dtype=np.uint64).view(np.int64)
    g = R.sample(np.where(smp["dead"], np.float32(-np.inf), o), u, R.stored_o_min(0.005, True), True, R.GROW, 5)
    assert g["S"] == S and g["sources"].tolist() == [0, 0, 3, 3, 3] and g["cnt"].tolist() == [2, 0, 0, 3, 0]
    empty = R.sample(np.full(4, -50.0, dtype=np.float32), u[:4], R.stored_o_min(0.005, True), True, R.RELOCATE)
    assert empty["S"] == 0 and empty["counts"] == [4, 4, 0, 0, 1, 0, 0, 0] and (empty["sources"] == -1).all()


def test_weights_keep_their_margin():
    """About one row in 3 x 10^4 lies within 2^-16 of a rounding boundary of its weight and is moved to the next float;
    afterwards none does, so a last-bit difference between two exp implementations cannot change a weight."""
    rng = np.random.default_rng(1)
    o = (2.0 * rng.standard_normal(300_000)).astype(np.float32)
    w = R.real_weights(o, True)
    closest = float(np.abs((w - np.floor(w)) - 0.5).min())
    fixed, moved = R.nudge(o, True)
    w = R.real_weights(fixed, True)
    print(f"closest weight {closest:.2e} from a boundary; {moved} of {o.size} rows moved")
    assert closest < 2.0 ** -16 and 1 <= moved <= 40
    assert np.abs((w - np.floor(w)) - 0.5).min() >= 2.0 ** -16


def test_noise_bar_is_twice_the_measured_constant():
    """The constant of the noise bound, measured: worst c of the float32 restatement against float64 over the cases the GPU
    test runs (raw and stored-linear); the bar is twice that, rounded up to a power of two."""
    worst = 0.0
    for P, M in R.SIZES:
        for raw in (True, False):
            case = R.make_case(P, M, seed=R.case_seed(P, M), raw=raw)
            c = R.noise_c(case, case["xi"])
            print(f"P={P} M={M} raw={raw}: c = {c:.3f}")
            worst = max(worst, c)
    print(f"worst c = {worst:.3f}; bar {R.NOISE_BAR}")
    assert abs(worst - R.NOISE_C_MEASURED) < 0.01 * R.NOISE_C_MEASURED + 0.01
    assert R.NOISE_BAR == 2.0 ** math.ceil(math.log2(2.0 * worst))


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
    assert pkg.relocate is mcmc.relocate and pkg.grow is mcmc.grow and pkg.inject_noise is mcmc.inject_noise
    assert pkg.RelocateResult is mcmc.RelocateResult and pkg.GrowResult is mcmc.GrowResult
    t, opt = _host_cloud(monkeypatch)
    for call in (lambda: mcmc.relocate(opt), lambda: mcmc.grow(opt, cap_max=100), lambda: mcmc.inject_noise(opt)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError, match="GaussianAdam"):
        mcmc.relocate(torch.optim.Adam([t["means3D"]]))
    # with the device guard lifted, what is looked at before the library
    monkeypatch.setattr(densify, "_require_gpu", lambda t, what: None)
    monkeypatch.setattr(mcmc, "_require_gpu", lambda t, what: None)
    for bad in (-0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="min_opacity"):
            mcmc.relocate(opt, min_opacity=bad)
        with pytest.raises(ValueError, match="min_opacity"):
            mcmc.grow(opt, cap_max=100, min_opacity=bad)
    with pytest.raises(ValueError, match=r"relocate: u must be .*int64 tensor \[12\]"):
        mcmc.relocate(opt, u=torch.zeros(11, dtype=torch.int64))
    with pytest.raises(ValueError, match="relocate: u must be"):
        mcmc.relocate(opt, u=torch.zeros(12, dtype=torch.int32))
    with pytest.raises(TypeError, match="relocate: u must be a torch.Tensor"):
        mcmc.relocate(opt, u=[0] * 12)
    for bad in (-1, 12.5, None, True):
        with pytest.raises(ValueError, match="grow: cap_max"):
            mcmc.grow(opt, cap_max=bad)
    for bad in (0.9, 2.5, math.nan):
        with pytest.raises(ValueError, match="grow: factor"):
            mcmc.grow(opt, cap_max=100, factor=bad)
    with pytest.raises(ValueError, match=r"grow: u must be .*\[6\]"):
        mcmc.grow(opt, cap_max=100, factor=1.5, u=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"inject_noise: xi must be .*\[12, 3\]"):
        mcmc.inject_noise(opt, xi=torch.zeros(12, 4))
    with pytest.raises(ValueError, match="inject_noise: lr \\* noise_lr"):
        mcmc.inject_noise(opt, noise_lr=math.inf)
    assert mcmc.stored_min_opacity(0.005, True) == math.log(0.005 / 0.995) and mcmc.stored_min_opacity(0.005, False) == 0.005
    assert mcmc.stored_min_opacity(0.0, True) == -math.inf and mcmc.stored_min_opacity(1.0, True) == math.inf
    a = pkg._lib.hs_mcmc_args()
    a.o_min = mcmc.stored_min_opacity(0.005, True)
    assert np.float32(a.o_min) == R.stored_o_min(0.005, True)


@pytest.mark.parametrize("cap_max,factor", [(12, 1.05), (5, 1.05), (0, 2.0), (100, 1.05), (100, 1.0)])
def test_grow_with_nothing_to_add_returns_the_same_tensors(monkeypatch, cap_max, factor):
    """cap_max <= P, or int(factor P) == P: the optimizer's own tensors, no library call (this runs without a GPU)."""
    from casualhdrsplat_amd import densify, mcmc
    t, opt = _host_cloud(monkeypatch)
    monkeypatch.setattr(densify, "_require_gpu", lambda t, what: None)
    monkeypatch.setattr(mcmc.L, "load", lambda: pytest.fail("grow with n_new == 0 reached the library"))
    res = mcmc.grow(opt, cap_max=cap_max, factor=factor)
    assert res.n_new == 0 and res.row_map is None and res.counts is None and res.source is None
    assert all(res.params[k] is t[k] for k in t)
    assert all(any(q is t[k] for g in opt.param_groups for q in g["params"]) for k in t)


# ---- resources ----

def test_mcmc_kernels_spill_nothing_and_need_no_scratch(tmp_path):
    src = os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "mcmc.hip")
    asm = str(tmp_path / "mcmc.s")
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
    kernels = sorted(re.search(r"mcmc_\w+?_kernel", k).group() for k in out)
    assert kernels == ["mcmc_counts_kernel", "mcmc_draw_kernel", "mcmc_noise_kernel", "mcmc_rows_kernel", "mcmc_scan_kernel",
                       "mcmc_source_kernel", "mcmc_weight_kernel"], sorted(out)
    for k, v in out.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 8, (k, v)
        if "noise" in k or "rows" in k or "draw" in k or "source" in k:
            assert v["LDS Size"] == 0, (k, v)
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0"] * 7 and "scratch_" not in text
    assert re.findall(r"\.amdhsa_float_denorm_mode_32 (\d+)", text) == ["3"] * 7               # denormals kept
    assert "global_load_dwordx4" in text                                                       # the quaternion, where aligned
    assert "v_div_fixup_f32" in text and "v_sqrt_f32" in text                                  # IEEE division and square root
    # built without contraction: the command make itself gives for the object (the Makefile's rules are patterns over a table)
    cmd = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "mcmc.o"],
                         capture_output=True, text=True, check=True).stdout
    assert re.findall(r"-ffp-contract=(\w+)", cmd) == ["off"] and " -c mcmc.hip " in cmd, cmd
    atomics = set(re.findall(r"\b(?:global|flat|buffer|ds)_atomic_\w+", text))
    assert atomics == {"global_atomic_add"}, atomics                                           # cnt and the source count: u32 adds only
    body = open(src, encoding="utf-8").read()
    assert not re.search(r"hipMem(set|cpy)\w*\(", body)                                        # cleared and copied by kernels only
    assert not re.search(r"hip(Stream|Device)Synchronize|hipMalloc|hipFree", body)

