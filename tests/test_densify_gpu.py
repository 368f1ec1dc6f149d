"""The densify / prune of the cloud (casualhdrsplat_amd.densify.densify_and_prune, densify.hip) on the MI355X against the
numpy restatement (tests/densify_reference.py): counts and row map bit for bit, every copied column of the parameters and
of Adam's moments bit for bit, zeros in the moments of new rows, child scales and (stored-linear scales) child means bit
for bit, child means with log scales within the measured bound; the edge cases; nothing written beyond P_out; two runs the
same bits; the next Adam step bit for bit the reference continued with the same step count and running products; and a
short training run through one densification."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import adam_reference as AR
import densify_reference as R
import helpers as Hh
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

RAW_MEAN_BAR, SIZES, case_seed = R.RAW_MEAN_BAR, R.SIZES, R.case_seed

DEV = "cuda"


def _assert_bits(got, want, what):
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert g.shape == want.shape, (what, g.shape, want.shape)
    if not R.same_bits(g, want):
        bad = ~((g.view(np.uint32) == want.view(np.uint32)) | (np.isnan(g) & np.isnan(want)))
        i = tuple(int(x[0]) for x in np.nonzero(bad))
        raise AssertionError(f"{what} differs in {int(bad.sum())} of {bad.size} elements; first at {i}: got {g[i]!r} "
                             f"({g.view(np.uint32)[i]:#x}), reference {want[i]!r} ({want.view(np.uint32)[i]:#x})")


def frontend(case, **override):
    """densify_and_prune on a case of make_case: the cloud under a GaussianAdam whose moments are the case's."""
    from casualhdrsplat_amd import DensifyStats, GaussianAdam, cloud_param_groups, densify_and_prune
    t = {k: torch.tensor(v, device=DEV).requires_grad_(True) for k, v in case["cloud"].items()}
    opt = GaussianAdam(cloud_param_groups(*[t[k] for k in R.NAMES]), eps=1e-15)
    opt.prepare()
    for k in R.NAMES:
        opt.state[t[k]]["exp_avg"].copy_(torch.tensor(case["moments"][k][0]))
        opt.state[t[k]]["exp_avg_sq"].copy_(torch.tensor(case["moments"][k][1]))
    stats = DensifyStats(case["P"], DEV)
    stats.grad_accum.copy_(torch.tensor(case["grad_accum"]))
    stats.denom.copy_(torch.tensor(case["denom"]))
    stats.max_radii.copy_(torch.tensor(case["max_radii"]))
    res = densify_and_prune(opt, stats, noise=torch.tensor(case["noise"], device=DEV), **dict(case["policy"], **override))
    return res, opt, stats


def check_against_reference(case, res, opt, stats, policy, what):
    th = R.thresholds(**policy)
    new, mom, row_map, counts = R.densify(case, th)
    got_counts = [res.counts[k] for k in ("P_out", "survivors", "clones", "children", "pruned_sources", "split_sources", "P_in")]
    assert got_counts == counts[:7], (what, got_counts, counts)
    assert np.array_equal(res.row_map.cpu().numpy().view(np.uint32), row_map), what
    assert np.array_equal(res.source.cpu().numpy(), row_map & R.SRC_MASK) and np.array_equal(res.kind.cpu().numpy(), row_map >> 30)
    child = (row_map >> 30) >= 2
    for k in R.NAMES:
        p = res.params[k]
        assert p.is_leaf and p.requires_grad and p.shape == new[k].shape, (what, k)
        st = opt.state[p]
        _assert_bits(st["exp_avg"], mom[k][0], f"{what}: {k}.exp_avg")
        _assert_bits(st["exp_avg_sq"], mom[k][1], f"{what}: {k}.exp_avg_sq")
        assert not st["exp_avg"][torch.tensor(row_map >> 30 != 0, device=DEV)].any()      # zeros in every new row
        if k == "means3D" and th["raw_scales"]:
            g = p.detach().cpu().numpy()
            _assert_bits(g[~child], new[k][~child], f"{what}: means3D of copied rows")
            if child.any():
                src, kk = (row_map & R.SRC_MASK)[child].astype(np.int64), (row_map >> 30)[child].astype(np.int64) - 2
                c = case["cloud"]
                ref64, mag = R.child_means(c["means3D"], c["scales"], c["rotations"], case["noise"], src, kk, True, np.float64)
                ratio = np.abs(g[child].astype(np.float64) - ref64) / (2.0 ** -24 * mag)
                print(f"{what}: child means, worst c against float64 = {float(ratio.max()):.3f} (bar {RAW_MEAN_BAR})")
                assert (ratio <= RAW_MEAN_BAR).all(), float(ratio.max())
        else:
            _assert_bits(p, new[k], f"{what}: {k}")
    assert stats.grad_accum.shape == (counts[0],) and not stats.grad_accum.any() and not stats.denom.any() and not stats.max_radii.any()
    assert all(any(q is res.params[k] for g in opt.param_groups for q in g["params"]) for k in R.NAMES)
    return counts


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("P,M", SIZES)
def test_densify_is_the_reference(P, M, raw):
    """Structure and copies bit for bit; child means with log scales (the one place a library function, expf, enters)
    within RAW_MEAN_BAR = 32: twice the worst c = 8.03 the float32 restatement itself shows against float64 on these
    inputs (tests/test_densify.py measures it), rounded up to a power of two."""
    case = R.make_case(P, M, seed=case_seed(P, M), raw_scales=raw, raw_opacity=raw)
    assert P < 1000 or ((case["denom"] == 0).any() and np.isnan(case["grad_accum"]).any())
    res, opt, stats = frontend(case)
    counts = check_against_reference(case, res, opt, stats, case["policy"], f"P={P} M={M} raw={raw}")
    if P >= 10007:
        assert 0.08 * P < counts[2] < 0.12 * P and 0.04 * P < counts[5] < 0.06 * P and 0.03 * P < counts[4] < 0.08 * P


@pytest.mark.parametrize("edge", ["nothing", "all_pruned", "all_split"])
def test_edge_policies(edge):
    P = 10007
    case = R.make_case(P, 4, seed=3)
    over = dict(nothing=dict(grad_threshold=math.inf, min_opacity=0.0, max_screen_size=None),
                all_pruned=dict(min_opacity=1.0),
                all_split=dict(grad_threshold=0.0, percent_dense=1e-9, min_opacity=0.0, max_screen_size=None))[edge]
    res, opt, stats = frontend(case, **over)
    check_against_reference(case, res, opt, stats, dict(case["policy"], **over), edge)
    if edge == "nothing":            # the output is the input, bit for bit
        assert res.counts["P_out"] == P and np.array_equal(res.row_map.cpu().numpy(), np.arange(P))
        for k in R.NAMES:
            _assert_bits(res.params[k], case["cloud"][k], k)
            _assert_bits(opt.state[res.params[k]]["exp_avg_sq"], case["moments"][k][1], k)
    elif edge == "all_pruned":
        assert res.counts["P_out"] == 0 and res.counts["pruned_sources"] == P and res.params["shs"].shape == (0, 4, 3)
    else:
        assert res.counts["P_out"] == 2 * P and res.counts["children"] == 2 * P and res.counts["split_sources"] == P


def abi_run(case, th, offset=0, spare=0, pattern=-123.5):
    """hs_densify_plan + hs_densify_apply through ctypes.  offset = 1: every source and destination array starts one float
    past a 16-byte boundary.  spare: extra rows of `pattern` behind every destination.  Returns (counts from the pinned
    buffer, counts from the device, row_map [2 P] with 0xFFFFFFFF where unwritten, {name: (param, m, v)} full destinations)."""
    from casualhdrsplat_amd import _lib as L
    lib = L.load()
    P = case["P"]

    def dev(x, dtype=torch.float32):
        flat = torch.zeros(x.size + offset + 4, dtype=dtype, device=DEV)
        flat[offset:offset + x.size] = torch.tensor(x.reshape(-1), dtype=dtype)
        return flat[offset:offset + x.size]

    srcs = {k: (dev(case["cloud"][k]), dev(case["moments"][k][0]), dev(case["moments"][k][1])) for k in R.NAMES}
    ga, dn, rad = dev(case["grad_accum"]), dev(case["denom"]), dev(case["max_radii"], torch.int32)
    noise = dev(case["noise"])
    ws = torch.empty(max(lib.hs_densify_workspace_bytes(P), 16), dtype=torch.uint8, device=DEV)
    row_map = torch.full((2 * P + 4,), -1, dtype=torch.int32, device=DEV)
    counts_dev = torch.full((8,), -1, dtype=torch.int32, device=DEV)
    counts_host = torch.full((8,), -1, dtype=torch.int32).pin_memory()
    a = L.hs_densify_args()
    a.P, a.flags, a.r_max = P, (2 if th["raw_scales"] else 0) | (1 if th["raw_opacity"] else 0), th["r_max"]
    a.tau_grad, a.tau_split, a.o_min, a.sigma_max = (float(th[k]) for k in ("tau_grad", "tau_split", "o_min", "sigma_max"))
    a.grad_accum, a.denom, a.max_radii = ga.data_ptr(), dn.data_ptr(), rad.data_ptr()
    a.opacities, a.scales, a.rotations = srcs["opacities"][0].data_ptr(), srcs["scales"][0].data_ptr(), srcs["rotations"][0].data_ptr()
    a.noise, a.workspace, a.row_map = noise.data_ptr(), ws.data_ptr(), row_map.data_ptr()
    a.counts, a.counts_host = counts_dev.data_ptr(), counts_host.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    L.check(lib.hs_densify_plan(C.byref(a), stream), "hs_densify_plan")
    torch.cuda.synchronize()
    got = counts_host.tolist()
    P_out = got[0]
    assert 0 <= P_out <= 2 * P
    dsts, mats = {}, []
    for k in R.NAMES:
        width = case["cloud"][k].size // P if P else int(np.prod(case["cloud"][k].shape[1:]))
        ds = []
        for i, src in enumerate(srcs[k]):
            flat = torch.full(((P_out + spare) * width + offset + 4,), pattern, device=DEV)
            ds.append(flat)
            mats.append((src, flat[offset:], width, R.ROLES[k] if i == 0 else R.ZERO_NEW))
        dsts[k] = (ds, width)
    arr = (L.hs_densify_matrix * len(mats))()
    for d, (src, dst, width, role) in zip(arr, mats):
        d.src, d.dst, d.row_stride, d.role = src.data_ptr(), dst.data_ptr(), width, role
        assert offset == 0 or (d.src % 16 == 4 * offset and d.dst % 16 == 4 * offset)
    a.P_out, a.matrices, a.n_matrices = P_out, arr, len(mats)
    L.check(lib.hs_densify_apply(C.byref(a), stream), "hs_densify_apply")
    torch.cuda.synchronize()
    out = {k: tuple(f.cpu().numpy() for f in ds) for k, (ds, _) in dsts.items()}
    return got, counts_dev.cpu().tolist(), row_map.cpu().numpy().view(np.uint32), out, {k: w for k, (_, w) in dsts.items()}


@pytest.mark.parametrize("offset", [0, 1])
def test_abi_unaligned_pointers_and_nothing_written_beyond_p_out(offset):
    """Sources and destinations that are only 4-byte aligned (offset = 1) give the same bits as aligned ones; destinations
    allocated with 37 spare rows of a pattern keep the pattern in every element at or beyond row P_out (and in the floats
    before the first row); row_map keeps its fill beyond P_out; the device counts equal the pinned copy."""
    P, spare, pattern = 10007, 37, np.float32(-123.5)
    case = R.make_case(P, 16, seed=9, raw_scales=False, raw_opacity=True)
    th = R.thresholds(**case["policy"])
    new, mom, row_map, counts = R.densify(case, th)
    got, got_dev, got_map, out, widths = abi_run(case, th, offset=offset, spare=spare, pattern=float(pattern))
    assert got == counts and got_dev == counts
    P_out = counts[0]
    assert np.array_equal(got_map[:P_out], row_map) and (got_map[P_out:] == 0xFFFFFFFF).all()
    for k in R.NAMES:
        w = widths[k]
        for flat, want, name in zip(out[k], (new[k],) + mom[k], ("param", "exp_avg", "exp_avg_sq")):
            body = flat[offset:offset + P_out * w]
            _assert_bits(body, want.reshape(-1), f"offset {offset}: {k}.{name}")
            assert (flat[:offset] == pattern).all() and (flat[offset + P_out * w:] == pattern).all(), (k, name)


def test_abi_empty_cloud():
    """P_in = 0: the plan writes zero counts (device and pinned copy), the apply has nothing to do."""
    case = R.make_case(0, 4, seed=1)
    th = R.thresholds(**case["policy"])
    got, got_dev, got_map, out, _ = abi_run(case, th, spare=2)
    assert got == [0] * 8 and got_dev == [0] * 8 and (got_map == 0xFFFFFFFF).all()
    for k in R.NAMES:
        assert all((f == np.float32(-123.5)).all() for f in out[k])


def test_two_runs_give_identical_bits():
    case = R.make_case(100003, 16, seed=2)
    runs = []
    for _ in range(2):
        res, opt, _ = frontend(case)
        runs.append([res.row_map] + [x for k in R.NAMES for x in (res.params[k].detach(), opt.state[res.params[k]]["exp_avg"],
                                                                 opt.state[res.params[k]]["exp_avg_sq"])])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_the_next_adam_step_continues_the_same_optimizer():
    """Three steps, a densification, then opt.step(visibility=radii): bit for bit the numpy Adam reference continued on the
    gathered parameters and moments with the SAME step count (4) and running products -- not a rebuilt optimizer."""
    from casualhdrsplat_amd import DensifyStats, GaussianAdam, cloud_param_groups, densify_and_prune
    P = 10007
    case = R.make_case(P, 16, seed=6)
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

    for _ in range(3):
        step()
    stats = DensifyStats(P, DEV)
    stats.grad_accum.copy_(torch.tensor(case["grad_accum"]))
    stats.denom.copy_(torch.tensor(case["denom"]))
    stats.max_radii.copy_(torch.tensor(case["max_radii"]))
    state_before = opt._dev_state.clone()
    res = densify_and_prune(opt, stats, noise=torch.tensor(case["noise"], device=DEV), **case["policy"])
    assert torch.equal(opt._dev_state, state_before) and opt._read_t() == 3
    # the reference: the same gather on its parameters and moments (the scales and opacities moved in three steps: replan)
    th = R.thresholds(**case["policy"])
    moved = dict(case, cloud=p_np, moments={k: (m_np[k], v_np[k]) for k in R.NAMES})
    new, mom, row_map, counts = R.densify(moved, th)
    assert np.array_equal(res.row_map.cpu().numpy().view(np.uint32), row_map) and counts[2] > 500 and counts[3] > 500
    for k in R.NAMES:
        p_np[k], m_np[k], v_np[k] = new[k], mom[k][0], mom[k][1]
        t[k] = res.params[k]
        if k != "means3D":
            _assert_bits(t[k], p_np[k], f"after densify: {k}")
    p_np["means3D"] = res.params["means3D"].detach().cpu().numpy().copy()       # (child means: expf, held to its bound elsewhere)
    vis_np = rng.random(counts[0]) < 0.6
    step(vis_np)
    assert opt._read_t() == 4 and ref.t == 4
    for k in R.NAMES:
        st = opt.state[t[k]]
        _assert_bits(t[k], p_np[k], f"step 4: {k}")
        _assert_bits(st["exp_avg"], m_np[k], f"step 4: {k}.exp_avg")
        _assert_bits(st["exp_avg_sq"], v_np[k], f"step 4: {k}.exp_avg_sq")
    assert float(opt.state_dict()["state"][0]["step"]) == 4.0


def test_training_through_one_densification():
    """DensifyStats-fed training on a synthetic scene: the learner starts from every fourth Gaussian of the scene that
    rendered the target, trains 60 steps (GaussianAdam on logit opacities / log scales, visibility = radii), densifies once
    from the statistics the backward accumulated (thresholds at the medians of what it saw, so about half of the seen rows
    are cloned or split), re-creates the rasterizer at the new P and trains 90 more.  Every loss is finite, P grows, and
    the mean loss of the last ten steps is below that of the ten steps before the densification (plumbing, not a
    convergence rate)."""
    from casualhdrsplat_amd import (DensifyStats, GaussianAdam, GaussianRasterizer, cloud_param_groups, densify_and_prune,
                                    photometric_loss)
    W, H, deg = 160, 120, 1
    sc = S.make_scene(4000, W, H, deg, seed=4)
    rs, _, _ = Hh.settings_from_scene(sc, DEV)
    with torch.no_grad():
        full = {k: getattr(sc, k).to(DEV) for k in R.NAMES}
        out = GaussianRasterizer(rs)(full["means3D"], torch.zeros_like(full["means3D"]), full["opacities"], shs=full["shs"],
                                     scales=full["scales"], rotations=full["rotations"])
        target = out[0].clone()
    sub = slice(0, None, 4)
    leaf = dict(means3D=full["means3D"][sub].clone(), opacities=torch.logit(full["opacities"][sub].clamp(1e-3, 1 - 1e-3)),
                shs=full["shs"][sub].clone(), scales=torch.log(full["scales"][sub]), rotations=full["rotations"][sub].clone())
    leaf = {k: v.contiguous().requires_grad_(True) for k, v in leaf.items()}
    P0 = leaf["means3D"].shape[0]
    extent = float(full["means3D"].std(dim=0).norm())
    opt = GaussianAdam(cloud_param_groups(*[leaf[k] for k in R.NAMES], spatial_lr_scale=extent), eps=1e-15)
    stats = DensifyStats(P0, DEV)
    rast = GaussianRasterizer(rs, densify_stats=stats)
    losses, before, after = [], 60, 90

    def train_step():
        for v in leaf.values():
            v.grad = None
        m2 = torch.zeros_like(leaf["means3D"], requires_grad=True)
        o = rast(leaf["means3D"], m2, torch.sigmoid(leaf["opacities"]), shs=leaf["shs"], scales=torch.exp(leaf["scales"]),
                 rotations=leaf["rotations"])
        loss = photometric_loss(o[0], target, 0.2)
        loss.backward()
        opt.step(visibility=o[1])
        losses.append(float(loss.detach()))

    for _ in range(before):
        train_step()
    seen = stats.denom > 0
    assert int(seen.sum()) > P0 // 4
    g_med = float(stats.mean_grad()[seen].median())
    s_med = float(torch.exp(leaf["scales"].detach()).max(dim=1).values.median())
    res = densify_and_prune(opt, stats, extent=extent, grad_threshold=g_med, percent_dense=s_med / extent, min_opacity=0.005,
                            generator=torch.Generator(device=DEV).manual_seed(1))
    leaf = dict(res.params)
    P1 = res.counts["P_out"]
    print(f"P {P0} -> {P1}: {res.counts}")
    assert P1 > P0 and res.counts["clones"] > 0 and res.counts["children"] > 0 and leaf["means3D"].shape[0] == P1
    rast = GaussianRasterizer(rs, densify_stats=stats)          # re-created at the new P
    for _ in range(after):
        train_step()
    print("losses:", " ".join(f"{x:.5f}" for x in losses))
    assert all(math.isfinite(x) for x in losses)
    assert int((stats.denom > 0).sum()) > 0 and stats.denom.shape == (P1,)
    pre, last = float(np.mean(losses[before - 10:before])), float(np.mean(losses[-10:]))
    print(f"mean loss of the ten steps before the densification {pre:.5f}, of the last ten {last:.5f}")
    assert last < pre, (pre, last)
