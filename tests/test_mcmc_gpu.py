"""The MCMC refinement of the cloud (casualhdrsplat_amd.mcmc, mcmc.hip) on the MI355X against the numpy restatement
(tests/mcmc_reference.py): dead flags, integer weights, the prefix's last element, every drawn source, the draw counts and
growth's row map BIT FOR BIT; every copied row, every zeroed and every untouched moment, every row that is neither source
nor dead bit for bit; the corrected opacities and scales of the sources within one float32 ulp of the float64 restatement;
the position noise inside its measured bound; the edge cases; nothing written outside the rows owned; two runs the same
bits; one optimizer continued through step, relocate, grow, noise, step; and no host wait."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_reference as AR
import helpers as Hh
import mcmc_reference as R
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
PATTERN = np.float32(-123.5)
PAD = 8            # floats of pattern in front of and behind every array
U = 2.0 ** -24
same_bits = R.DR.same_bits


def _assert_bits(got, want, what):
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert g.shape == want.shape, (what, g.shape, want.shape)
    if not same_bits(g, want):
        bad = ~((g.view(np.uint32) == want.view(np.uint32)) | (np.isnan(g) & np.isnan(want)))
        i = tuple(int(x[0]) for x in np.nonzero(bad))
        raise AssertionError(f"{what} differs in {int(bad.sum())} of {bad.size} elements; first at {i}: got {g[i]!r} "
                             f"({g.view(np.uint32)[i]:#x}), reference {want[i]!r} ({want.view(np.uint32)[i]:#x})")


def _assert_one_ulp(got, ref64, what):
    ok = R.within_one_ulp(got, ref64)
    if not ok.all():
        i = tuple(int(x[0]) for x in np.nonzero(~ok))
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} beyond one ulp; first at {i}: got {got[i]!r}, float64 {ref64[i]!r}")


class Padded:
    """A device array with PAD floats of pattern on both sides, its data `offset` floats past a 16-byte boundary."""

    def __init__(self, x, offset=0, dtype=torch.float32, fill=float(PATTERN)):
        self.n, self.shape, self.offset = x.size, x.shape, offset
        self.fill = fill
        self.flat = torch.full((x.size + 2 * PAD + offset,), fill, dtype=dtype, device=DEV)
        self.view = self.flat[PAD + offset:PAD + offset + x.size]
        self.view.copy_(torch.tensor(np.ascontiguousarray(x).reshape(-1), dtype=dtype))
        assert self.view.data_ptr() % 16 == (4 * offset) % 16 or dtype != torch.float32

    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        h = self.flat.cpu().numpy()
        a, b = PAD + self.offset, PAD + self.offset + self.n
        assert (h[:a] == self.fill).all() and (h[b:] == self.fill).all(), "written outside the array"
        return h[a:b].reshape(self.shape).copy()


def abi_run(case, mode, n_draws=None, offset=0, update=True, min_opacity=None):
    """hs_mcmc_sample (+ hs_mcmc_update) through ctypes on a case, every array padded with a pattern.  Returns a dict of what
    the calls left: counts (pinned copy and device), the workspace's sections, row_map, and every tensor."""
    from casualhdrsplat_amd import _lib as L
    from casualhdrsplat_amd.mcmc import stored_min_opacity, workspace_layout
    lib = L.load()
    P = case["P"]
    n_draws = P if mode == R.RELOCATE else n_draws
    min_opacity = case["min_opacity"] if min_opacity is None else min_opacity
    raw_o, raw_s = case["raw_opacity"], case["raw_scales"]
    arrs = {k: tuple(Padded(x, offset) for x in (case["cloud"][k],) + tuple(case["moments"][k])) for k in R.NAMES}
    nbytes = lib.hs_mcmc_workspace_bytes(P, n_draws)
    lay = workspace_layout(P, n_draws)
    assert nbytes == lay["bytes"]
    ws = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    counts = Padded(np.full(8, -1, dtype=np.int32), dtype=torch.int32, fill=-7)
    counts_host = torch.full((8,), -1, dtype=torch.int32).pin_memory()
    u = torch.tensor(case["u"][:n_draws], device=DEV) if n_draws else torch.zeros(1, dtype=torch.int64, device=DEV)
    row_map = Padded(np.full(P + n_draws, -1, dtype=np.int32), dtype=torch.int32, fill=-7) if mode == R.GROW else None
    a = L.hs_mcmc_args()
    a.P, a.n_draws, a.mode = P, n_draws, mode
    a.flags = (2 if raw_s else 0) | (1 if raw_o else 0)
    a.o_min, a.min_opacity = stored_min_opacity(min_opacity, raw_o), min_opacity
    a.opacities, a.scales = arrs["opacities"][0].ptr(), arrs["scales"][0].ptr()
    a.u, a.workspace, a.counts, a.counts_host = u.data_ptr(), ws.data_ptr(), counts.ptr(), counts_host.data_ptr()
    a.row_map = row_map.ptr() if row_map is not None else None
    mats = []
    for k in R.NAMES:
        width = case["cloud"][k].size // P if P else int(np.prod(case["cloud"][k].shape[1:]))
        mats += [(arrs[k][0], width, L.HS_DENSIFY_COPY), (arrs[k][1], width, L.HS_DENSIFY_ZERO_NEW), (arrs[k][2], width, L.HS_DENSIFY_ZERO_NEW)]
    arr = (L.hs_densify_matrix * len(mats))()
    for d, (t, width, role) in zip(arr, mats):
        d.src, d.dst, d.row_stride, d.role = None, t.ptr(), width, role
    a.matrices, a.n_matrices = arr, len(mats)
    stream = torch.cuda.current_stream().cuda_stream
    L.check(lib.hs_mcmc_sample(C.byref(a), stream), "hs_mcmc_sample")
    if update:
        L.check(lib.hs_mcmc_update(C.byref(a), stream), "hs_mcmc_update")
    torch.cuda.synchronize()
    h = ws.cpu().numpy()
    assert (h[nbytes:] == 0xA5).all(), "written behind the workspace"
    nblk = (P + 255) // 256
    sec = lambda name, n, dt: h[lay[name]:lay[name] + n * np.dtype(dt).itemsize].view(dt).copy()     # noqa: E731
    blocks = sec("blocks", 2 * (nblk + 1), np.uint64).reshape(nblk + 1, 2)
    return dict(counts_host=counts_host.tolist(), counts=counts.get().tolist(), prefix=sec("prefix", P, np.uint64),
                block_prefix=blocks[:nblk, 0], S=int(blocks[nblk, 0]), block_dead=(blocks[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64),
                cnt=sec("cnt", P, np.uint32), sources=sec("sources", n_draws, np.int32),
                row_map=None if row_map is None else row_map.get().view(np.uint32),
                cloud={k: arrs[k][0].get() for k in R.NAMES}, moments={k: (arrs[k][1].get(), arrs[k][2].get()) for k in R.NAMES})


def check_sample(got, smp, P, what):
    """Counts, dead rows, weights, prefix, S, sources and cnt: the same integers."""
    assert got["counts_host"] == smp["counts"] and got["counts"] == smp["counts"], (what, got["counts_host"], got["counts"], smp["counts"])
    inner = got["prefix"].copy()
    w = inner.copy()
    first = np.arange(P) % 256 == 0
    w[~first] = inner[~first] - inner[np.nonzero(~first)[0] - 1]
    assert np.array_equal(w, smp["w"]), (what, int((w != smp["w"]).sum()))
    block_sums = np.add.reduceat(smp["w"], np.arange(0, P, 256)) if P else np.zeros(0, dtype=np.uint64)
    assert np.array_equal(got["block_prefix"], np.concatenate([np.zeros(min(P, 1), dtype=np.uint64), np.cumsum(block_sums, dtype=np.uint64)[:-1]])), what
    assert got["S"] == smp["S"], (what, got["S"], smp["S"])
    dead_blocks = np.add.reduceat(smp["dead"].astype(np.int64), np.arange(0, P, 256)) if P else np.zeros(0, dtype=np.int64)
    assert np.array_equal(got["block_dead"][:-1], dead_blocks) and got["block_dead"][-1] == smp["dead"].sum(), what
    assert np.array_equal(got["sources"], smp["sources"]), (what, int((got["sources"] != smp["sources"]).sum()))
    assert np.array_equal(got["cnt"], smp["cnt"]), what


def check_relocation(case, got, what):
    P = case["P"]
    new, mom, smp, (o64, s64) = R.relocate(case, case["u"], case["min_opacity"])
    check_sample(got, smp, P, what)
    upd, dead = smp["cnt"] > 0, smp["sources"] >= 0
    src = smp["sources"][dead]
    c = got["cloud"]
    _assert_one_ulp(c["opacities"].reshape(-1)[upd], o64[upd], f"{what}: opacities of the sources")
    _assert_one_ulp(c["scales"][upd], s64[upd], f"{what}: scales of the sources")
    keep = ~upd & ~dead
    for k in R.NAMES:
        _assert_bits(c[k][keep], case["cloud"][k][keep], f"{what}: {k} of rows that are neither source nor dead")
        _assert_bits(c[k][dead], c[k][src], f"{what}: {k} of dead rows against their sources")
        if k not in ("opacities", "scales"):
            _assert_bits(c[k], new[k], f"{what}: {k}")
        for j, name in enumerate(("exp_avg", "exp_avg_sq")):
            _assert_bits(got["moments"][k][j], mom[k][j], f"{what}: {k}.{name}")
            assert not got["moments"][k][j][upd].any()
    return smp


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("P,M", R.SIZES)
def test_relocation_is_the_reference(P, M, raw):
    case = R.make_case(P, M, seed=R.case_seed(P, M), raw=raw)
    got = abi_run(case, R.RELOCATE)
    smp = check_relocation(case, got, f"P={P} M={M} raw={raw}")
    if P >= 10007:
        o = case["cloud"]["opacities"].reshape(-1)
        assert 0.05 * P < smp["counts"][1] < 0.07 * P and np.isnan(o).sum() > 0.005 * P and smp["dead"][np.isnan(o)].all()
        assert smp["counts"][2] == smp["counts"][1] and 0 < smp["counts"][3] <= smp["counts"][2]
        assert (R.sigmoid64(o[~np.isnan(o)]).max() if raw else np.nanmax(o)) >= 1 - 2.0 ** -20 - 1e-9


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("P,M", R.SIZES)
def test_growth_is_the_reference(P, M, raw):
    """Through the front end: sample, sources corrected in place (moments kept), one gather into the new tensors."""
    from casualhdrsplat_amd import grow
    case = R.make_case(P, M, seed=R.case_seed(P, M) + 1, raw=raw)
    factor = 2.0 if P < 100 else 1.05
    n_new = int(factor * P) - P
    assert n_new >= 1
    opt, t = _optimizer_of(case)
    state_before = opt._dev_state.clone()
    res = grow(opt, cap_max=10 * P, factor=factor, min_opacity=case["min_opacity"], raw_scales=raw, raw_opacity=raw,
               u=torch.tensor(case["u"][:n_new], device=DEV))
    new, mom, smp, (o64, s64) = R.grow(case, case["u"][:n_new], n_new, case["min_opacity"])
    assert res.n_new == n_new and torch.equal(opt._dev_state, state_before)
    assert np.array_equal(res.row_map.cpu().numpy().view(np.uint32), smp["row_map"])
    assert np.array_equal(res.source.cpu().numpy()[P:], smp["sources"]) and res.counts.cpu().tolist() == smp["counts"]
    upd = np.concatenate([smp["cnt"] > 0, np.ones(n_new, dtype=bool)])
    for k in R.NAMES:
        p = res.params[k]
        assert p.is_leaf and p.requires_grad and p.shape == new[k].shape and any(q is p for g in opt.param_groups for q in g["params"])
        g = p.detach().cpu().numpy()
        _assert_bits(g[P:], g[smp["sources"]], f"{k}: new rows against their sources")
        if k in ("opacities", "scales"):
            _assert_bits(g[~upd], new[k][~upd], f"{k}: rows that are not sources")
        else:
            _assert_bits(g, new[k], k)
        for j, name in enumerate(("exp_avg", "exp_avg_sq")):
            _assert_bits(opt.state[p][name], mom[k][j], f"{k}.{name}")          # sources keep theirs, new rows zeros
    src = smp["cnt"] > 0
    _assert_one_ulp(res.params["opacities"].detach().cpu().numpy().reshape(-1)[:P][src], o64[src], "opacities of the sources")
    _assert_one_ulp(res.params["scales"].detach().cpu().numpy()[:P][src], s64[src], "scales of the sources")


def test_growth_weights_every_row():
    """Growth's sampler at the ABI: dead rows keep their weight, a NaN row has none; row_map and nothing behind it."""
    P, n_new = 10007, 500
    case = R.make_case(P, 1, seed=4)
    got = abi_run(case, R.GROW, n_draws=n_new)
    smp = R.sample(case["cloud"]["opacities"], case["u"][:n_new], R.stored_o_min(case["min_opacity"], True), True, R.GROW, n_new)
    check_sample(got, smp, P, "grow")
    assert (smp["w"][smp["dead"] & ~np.isnan(case["cloud"]["opacities"].reshape(-1))] > 0).all()
    assert np.array_equal(got["row_map"], smp["row_map"])
    for k in R.NAMES:                                         # the update of a growth touches no moment
        for j in range(2):
            _assert_bits(got["moments"][k][j], case["moments"][k][j], k)


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("P,M", R.SIZES)
def test_noise_is_inside_the_measured_bound(P, M, raw):
    """|hip - float64| <= NOISE_BAR 2^-24 (|mu| + sum |Sigma_ij| |v_j|) with NOISE_BAR = 64: twice the worst c = 29.63 the
    float32 restatement itself shows against float64 on these inputs (tests/test_mcmc.py measures it), rounded up to a power
    of two.  Rows whose gate times the scaler is zero keep their bits; every other tensor is untouched."""
    from casualhdrsplat_amd import inject_noise
    case = R.make_case(P, M, seed=R.case_seed(P, M), raw=raw)
    opt, t = _optimizer_of(case)
    inject_noise(opt, noise_lr=5e5, lr=1.6e-4, raw_scales=raw, raw_opacity=raw, xi=torch.tensor(case["xi"], device=DEV))
    c = case["cloud"]
    args = (c["means3D"], c["opacities"], c["scales"], c["rotations"], case["xi"], R.NOISE_SCALER, raw, raw)
    assert np.float32(1.6e-4 * 5e5) == np.float32(R.NOISE_SCALER)
    ref64, _, mag = R.noise(*args, dtype=np.float64)
    _, gs32, _ = R.noise(*args)
    got = t["means3D"].detach().cpu().numpy()
    nan = np.isnan(ref64).any(axis=1)
    assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any()
    ratio = np.abs(got.astype(np.float64) - ref64)[~nan] / (U * mag[~nan])
    print(f"P={P} M={M} raw={raw}: worst c against float64 = {float(ratio.max()) if ratio.size else 0.0:.3f} (bar {R.NOISE_BAR})")
    assert (ratio <= R.NOISE_BAR).all(), float(ratio.max())
    still = ~nan & (gs32 == 0)
    _assert_bits(got[still], c["means3D"][still], "rows with a closed gate")
    if P >= 10007:
        assert still.sum() > 0.1 * P and (~still & ~nan).sum() > 0.3 * P
        assert np.abs(got - c["means3D"])[~still & ~nan].max() > 1e-4
    for k in ("opacities", "shs", "scales", "rotations"):
        _assert_bits(t[k], c[k], k)


def _optimizer_of(case):
    from casualhdrsplat_amd import GaussianAdam, cloud_param_groups
    t = {k: torch.tensor(v, device=DEV).requires_grad_(True) for k, v in case["cloud"].items()}
    opt = GaussianAdam(cloud_param_groups(*[t[k] for k in R.NAMES]), eps=1e-15)
    opt.prepare()
    for k in R.NAMES:
        opt.state[t[k]]["exp_avg"].copy_(torch.tensor(case["moments"][k][0]))
        opt.state[t[k]]["exp_avg_sq"].copy_(torch.tensor(case["moments"][k][1]))
    return opt, t


# ---- edge cases ----

def _unchanged(case, got, what):
    for k in R.NAMES:
        _assert_bits(got["cloud"][k], case["cloud"][k], f"{what}: {k}")
        for j in range(2):
            _assert_bits(got["moments"][k][j], case["moments"][k][j], f"{what}: {k} moment {j}")


def test_no_dead_row_writes_nothing():
    P = 10007
    case = R.make_case(P, 4, seed=8, dead_frac=0.0, nan=False)
    got = abi_run(case, R.RELOCATE)
    assert got["counts_host"] == got["counts"] == [P, 0, 0, 0, 0, 0, 0, 0] and (got["sources"] == -1).all() and not got["cnt"].any()
    _unchanged(case, got, "no dead row")


def test_all_rows_dead_writes_nothing():
    P = 10007
    case = R.make_case(P, 4, seed=8)
    case["cloud"]["opacities"][:] = -7.0
    case["cloud"]["opacities"][::5] = np.nan
    got = abi_run(case, R.RELOCATE)
    assert got["counts_host"] == got["counts"] == [P, P, 0, 0, 1, 0, 0, 0] and got["S"] == 0
    assert (got["sources"] == -1).all() and not got["cnt"].any()
    _unchanged(case, got, "all rows dead")
    # growth with every weight zero (opacities whose sigmoid rounds to weight 0): no draw, the new rows name rows of the cloud
    case["cloud"]["opacities"][:] = -40.0
    got = abi_run(case, R.GROW, n_draws=500)
    assert got["counts"] == [P, P, 0, 0, 1, 0, 0, 0] and (got["sources"] == -1).all()
    assert np.array_equal(got["row_map"], np.concatenate([np.arange(P), np.arange(500) | R.CLONE]).astype(np.uint32))
    _unchanged(case, got, "growth with S = 0")


def test_one_live_row_and_a_hundred_dead_clamps_the_ratio():
    case = R.make_case(101, 4, seed=3, dead_frac=0.0)
    case["cloud"]["opacities"][:] = -7.0
    case["cloud"]["opacities"][37] = 2.5
    case["cloud"]["opacities"][:, 0], _ = R.nudge(case["cloud"]["opacities"][:, 0], True)
    got = abi_run(case, R.RELOCATE)
    smp = check_relocation(case, got, "one live row")
    assert smp["counts"] == [101, 100, 100, 1, 0, 0, 0, 0] and smp["cnt"][37] == 100
    # the ratio is 51, not 101: the float64 restatement at r = 51 is what the one-ulp comparison above used
    o64, _, cond = R.correction(case["cloud"]["opacities"], case["cloud"]["scales"], smp["cnt"], case["min_opacity"], True, True)
    x = 1.0 - (1.0 - R.sigmoid64(case["cloud"]["opacities"][37, 0])) ** (1.0 / 51)
    assert abs(o64[37] - np.log(x / (1 - x))) < 1e-12 and cond[37] > 1.0
    for k in R.NAMES:
        assert (got["cloud"][k].view(np.uint32) == got["cloud"][k][37].view(np.uint32)).all()       # every row is the live one now


def test_empty_cloud():
    from casualhdrsplat_amd import _lib as L
    case = R.make_case(0, 4, seed=1)
    empty = [0, 0, 0, 0, 1, 0, 0, 0]                  # no row, no draw, and S == 0
    got = abi_run(case, R.RELOCATE)
    assert got["counts_host"] == got["counts"] == empty == R.sample(np.zeros(0, np.float32), np.zeros(0, np.int64), -5.3, True, R.RELOCATE)["counts"]
    got = abi_run(case, R.GROW, n_draws=0)
    assert got["counts_host"] == got["counts"] == empty and got["row_map"].size == 0
    a = L.hs_mcmc_noise_args()
    a.P, a.flags, a.scaler = 0, 3, 80.0
    L.check(L.load().hs_mcmc_noise(C.byref(a), torch.cuda.current_stream().cuda_stream), "hs_mcmc_noise")
    torch.cuda.synchronize()


def test_growth_with_nothing_to_add_launches_nothing():
    from casualhdrsplat_amd import grow
    case = R.make_case(257, 1, seed=2)
    opt, t = _optimizer_of(case)
    res = grow(opt, cap_max=257)
    assert res.n_new == 0 and all(res.params[k] is t[k] for k in R.NAMES)
    for k in R.NAMES:
        _assert_bits(t[k], case["cloud"][k], k)


def test_unaligned_views_give_the_same_bits():
    """Every tensor one float past a 16-byte boundary: the same bits as aligned, nothing written around them (abi_run checks
    the pattern on both sides of every array, behind the workspace, around counts and row_map)."""
    case = R.make_case(10007, 16, seed=9)
    a, b = abi_run(case, R.RELOCATE, offset=0), abi_run(case, R.RELOCATE, offset=1)
    check_relocation(case, b, "offset 1")
    for k in R.NAMES:
        _assert_bits(b["cloud"][k], a["cloud"][k], k)
    from casualhdrsplat_amd import _lib as L
    c = case["cloud"]
    arrs = {k: Padded(c[k], 1) for k in ("means3D", "opacities", "scales", "rotations")}
    xi = Padded(case["xi"], 3)
    n = L.hs_mcmc_noise_args()
    n.P, n.flags, n.scaler = case["P"], 3, R.NOISE_SCALER
    n.means3D, n.opacities, n.scales, n.rotations = (arrs[k].ptr() for k in ("means3D", "opacities", "scales", "rotations"))
    n.xi = xi.ptr()
    L.check(L.load().hs_mcmc_noise(C.byref(n), torch.cuda.current_stream().cuda_stream), "hs_mcmc_noise")
    torch.cuda.synchronize()
    from casualhdrsplat_amd import inject_noise
    opt, t = _optimizer_of(case)
    inject_noise(opt, lr=1.6e-4, noise_lr=5e5, xi=torch.tensor(case["xi"], device=DEV))
    _assert_bits(arrs["means3D"].get(), t["means3D"].detach().cpu().numpy(), "noise through unaligned pointers")
    for k in ("opacities", "scales", "rotations"):
        _assert_bits(arrs[k].get(), c[k], k)


def test_two_runs_give_identical_bits():
    case = R.make_case(262144, 1, seed=2)
    runs = [abi_run(case, R.RELOCATE) for _ in range(2)]
    for key in ("prefix", "block_prefix", "cnt", "sources"):
        assert np.array_equal(runs[0][key], runs[1][key]), key
    assert runs[0]["counts"] == runs[1]["counts"] and runs[0]["S"] == runs[1]["S"]
    for k in R.NAMES:
        _assert_bits(runs[0]["cloud"][k], runs[1]["cloud"][k], k)
        for j in range(2):
            _assert_bits(runs[0]["moments"][k][j], runs[1]["moments"][k][j], k)


# ---- one optimizer through it all ----

def test_step_relocate_grow_noise_step_continues_the_same_optimizer():
    """One step, relocate, grow (10 007 -> 10 507), inject_noise, one more step: bit for bit the numpy Adam restatement
    continued on the restated tensors with the SAME step count (2) and running products.  The values the float64 correction
    and the noise produce are held to their bounds here and then taken over from the device, so that the second step is
    compared on equal inputs; before each sampling the opacities are moved away from weight boundaries on the CPU (the
    fixture's rule) in both copies.  Then a parameterization="raw" forward + backward on the grown cloud."""
    from casualhdrsplat_amd import GaussianAdam, GaussianRasterizer, cloud_param_groups, grow, inject_noise, relocate
    P, W, H = 10007, 160, 120
    case = R.make_case(P, 16, seed=6, nan=False)
    sc = S.make_scene(P, W, H, 3, seed=4)
    case["cloud"].update(means3D=sc.means3D.numpy().copy(), shs=sc.shs.numpy().copy(), rotations=sc.rotations.numpy().copy(),
                         scales=np.log(sc.scales.numpy()).astype(np.float32))
    rng = np.random.default_rng(12)
    t = {k: torch.tensor(v, device=DEV).requires_grad_(True) for k, v in case["cloud"].items()}
    opt = GaussianAdam(cloud_param_groups(*[t[k] for k in R.NAMES]), eps=1e-15)
    cols = [("means3D", 0, 3), ("opacities", 0, 1), ("shs", 0, 3), ("shs", 3, 48), ("scales", 0, 3), ("rotations", 0, 4)]
    hyper = lambda: [(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])) for g in opt.param_groups]   # noqa: E731
    ref = AR.AdamReference(len(cols))
    p_np = {k: v.copy() for k, v in case["cloud"].items()}
    m_np = {k: np.zeros_like(v) for k, v in p_np.items()}
    v_np = {k: np.zeros_like(v) for k, v in p_np.items()}

    def step(vis_np=None):
        rows = p_np["means3D"].shape[0]
        grads = {k: (1e-3 * rng.standard_normal(p_np[k].shape)).astype(np.float32) for k in R.NAMES}
        for k in R.NAMES:
            t[k].grad = torch.tensor(grads[k], device=DEV)
        opt.step(visibility=None if vis_np is None else torch.tensor(np.where(vis_np, 7, 0).astype(np.int32), device=DEV))
        d = ref.tick(hyper())
        for i, (k, a, b) in enumerate(cols):
            view = lambda x: x.reshape(rows, -1)[:, a:b]           # noqa: E731
            AR.update(view(p_np[k]), view(grads[k]), view(m_np[k]), view(v_np[k]), d[i], vis_np)

    def settle_weights():
        p_np["opacities"], _ = R.nudge(p_np["opacities"], True)
        with torch.no_grad():
            t["opacities"].copy_(torch.tensor(p_np["opacities"]))

    def moved_case():
        return dict(case, P=p_np["means3D"].shape[0], cloud=p_np, moments={k: (m_np[k], v_np[k]) for k in R.NAMES})

    def take_over(res_params, new, mom, upd, o64, s64):
        for k in R.NAMES:
            g = res_params[k].detach().cpu().numpy()
            if k in ("opacities", "scales"):
                _assert_bits(g[~upd], new[k][~upd], k)
            else:
                _assert_bits(g, new[k], k)
            p_np[k], m_np[k], v_np[k] = g.copy(), mom[k][0], mom[k][1]
            _assert_bits(opt.state[res_params[k]]["exp_avg"], m_np[k], f"{k}.exp_avg")
            _assert_bits(opt.state[res_params[k]]["exp_avg_sq"], v_np[k], f"{k}.exp_avg_sq")

    step()
    for k in R.NAMES:
        _assert_bits(t[k], p_np[k], f"step 1: {k}")
    state_before = opt._dev_state.clone()

    settle_weights()
    u1 = rng.integers(-(1 << 63), (1 << 63) - 1, P, dtype=np.int64, endpoint=True)
    res = relocate(opt, min_opacity=case["min_opacity"], u=torch.tensor(u1, device=DEV))
    new, mom, smp, (o64, s64) = R.relocate(moved_case(), u1, case["min_opacity"])
    assert res.counts.cpu().tolist() == smp["counts"] and smp["counts"][1] > 400
    assert np.array_equal(res.source.cpu().numpy(), smp["sources"]) and np.array_equal(res.cnt.cpu().numpy().view(np.uint32), smp["cnt"])
    upd, dead = smp["cnt"] > 0, smp["sources"] >= 0
    _assert_one_ulp(t["opacities"].detach().cpu().numpy().reshape(-1)[upd], o64[upd], "relocate: opacities")
    _assert_one_ulp(t["scales"].detach().cpu().numpy()[upd], s64[upd], "relocate: scales")
    take_over(t, new, mom, upd | dead, o64, s64)

    settle_weights()
    n_new = 500
    u2 = rng.integers(-(1 << 63), (1 << 63) - 1, n_new, dtype=np.int64, endpoint=True)
    gres = grow(opt, cap_max=20000, min_opacity=case["min_opacity"], u=torch.tensor(u2, device=DEV))
    new, mom, smp, (o64, s64) = R.grow(moved_case(), u2, n_new, case["min_opacity"])
    assert gres.n_new == n_new and np.array_equal(gres.row_map.cpu().numpy().view(np.uint32), smp["row_map"])
    upd = np.concatenate([smp["cnt"] > 0, np.ones(n_new, dtype=bool)])
    g_o, g_s = gres.params["opacities"].detach().cpu().numpy(), gres.params["scales"].detach().cpu().numpy()
    _assert_one_ulp(g_o.reshape(-1)[:P][smp["cnt"] > 0], o64[smp["cnt"] > 0], "grow: opacities")
    _assert_one_ulp(g_s[:P][smp["cnt"] > 0], s64[smp["cnt"] > 0], "grow: scales")
    _assert_bits(g_o[P:], g_o[smp["sources"]], "grow: new opacities")
    _assert_bits(g_s[P:], g_s[smp["sources"]], "grow: new scales")
    t = dict(gres.params)
    take_over(t, new, mom, upd, o64, s64)
    P1 = P + n_new
    assert t["means3D"].shape[0] == P1 == 10507

    xi = rng.standard_normal((P1, 3)).astype(np.float32)
    inject_noise(opt, noise_lr=5e5, xi=torch.tensor(xi, device=DEV))
    lr = float(next(g["lr"] for g in opt.param_groups if g["name"] == "xyz"))
    ref64, _, mag = R.noise(p_np["means3D"], p_np["opacities"], p_np["scales"], p_np["rotations"], xi, lr * 5e5, True, True, dtype=np.float64)
    got = t["means3D"].detach().cpu().numpy()
    assert (np.abs(got.astype(np.float64) - ref64) <= R.NOISE_BAR * U * mag).all() and not same_bits(got, p_np["means3D"])
    p_np["means3D"] = got.copy()
    assert torch.equal(opt._dev_state, state_before) and opt._read_t() == 1

    vis_np = rng.random(P1) < 0.6
    step(vis_np)
    assert opt._read_t() == 2 and ref.t == 2
    for k in R.NAMES:
        st = opt.state[t[k]]
        _assert_bits(t[k], p_np[k], f"step 2: {k}")
        _assert_bits(st["exp_avg"], m_np[k], f"step 2: {k}.exp_avg")
        _assert_bits(st["exp_avg_sq"], v_np[k], f"step 2: {k}.exp_avg_sq")

    rs, _, _ = Hh.settings_from_scene(sc, DEV)
    for v in t.values():
        v.grad = None
    rast = GaussianRasterizer(rs, parameterization="raw")
    out = rast(t["means3D"], torch.zeros_like(t["means3D"], requires_grad=True), t["opacities"], shs=t["shs"], scales=t["scales"],
               rotations=t["rotations"])
    (out[0] * sc.dL_dimage.to(DEV)).sum().backward()
    for k in R.NAMES:
        assert t[k].grad is not None and t[k].grad.shape == t[k].shape and bool(torch.isfinite(t[k].grad).all()), k
    assert float(t["means3D"].grad.abs().sum()) > 0


def test_relocate_and_noise_do_not_wait_for_the_device():
    """torch's sync debug mode raises on every host read torch itself would make (the library's side -- no HIP copy, no
    synchronisation in mcmc.hip -- is checked by reading the file: tests/test_mcmc.py)."""
    from casualhdrsplat_amd import _lib as L, inject_noise, relocate
    case = R.make_case(10007, 4, seed=13)
    opt, t = _optimizer_of(case)
    gen = torch.Generator(device=DEV).manual_seed(5)
    L.load()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = relocate(opt, min_opacity=case["min_opacity"], generator=gen)
        inject_noise(opt, generator=gen)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    counts = res.counts.cpu().tolist()
    assert counts[0] == 10007 and counts[1] == counts[2] > 400 and 0 < counts[3] <= counts[2] and counts[4:] == [0, 0, 0, 0]
    assert int((res.source >= 0).sum()) == counts[2] and int(res.cnt.sum()) == counts[2]
