"""The 3-nearest-neighbour scale initialisation (casualhdrsplat_amd.knn_mean_dist2, knn.hip) on the MI355X against the numpy
restatement of its contract (tests/knn_reference.brute) BIT FOR BIT: fewer than three neighbours, the seed window, ragged
and degenerate boxes, a reconstruction-like cloud of 131 072 points on sampled rows; the result under a permutation of the
points; two runs and a 4-byte-aligned view the same bits; nothing written beyond P rows or beyond the stated workspace; and
scene_io.init_from_points(device="cuda") against the host path, usable by the rasterizer as it comes."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as Hh
import knn_reference as R
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
_BRUTE = {}


def knn(x):
    from casualhdrsplat_amd import knn_mean_dist2
    out = knn_mean_dist2(torch.from_numpy(np.array(x, np.float32)).to(DEV))
    assert out.dtype == torch.float32 and out.shape == (len(x),) and out.device.type == "cuda"
    return out.cpu().numpy()


def brute_of(key, make):
    """(points, brute(points)) of a named cloud, computed once and shared read-only."""
    if key not in _BRUTE:
        x = make()
        x.setflags(write=False)
        want = R.brute(x)
        want.setflags(write=False)
        _BRUTE[key] = (x, want)
    return _BRUTE[key]


def assert_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(R.bits(got) != R.bits(want))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} rows differ; first at {i}: got {got[i]!r} "
                             f"({R.bits(got)[i]:#x}), reference {want[i]!r} ({R.bits(want)[i]:#x})")


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 10_007])
def test_uniform_points_bit_for_bit(P):
    x, want = brute_of(f"uniform{P}", lambda: R.uniform(P))
    assert_bits(knn(x), want, f"uniform P={P}")


@pytest.mark.parametrize("name", ["line", "plane", "clusters", "repeated", "lattice", "denormal"])
def test_degenerate_clouds_bit_for_bit(name):
    x, want = brute_of(name, lambda: R.degenerate_families()[name])
    got = knn(x)
    assert_bits(got, want, name)
    if name == "repeated":
        assert not R.bits(got).any()                                   # exact zeros
    if name == "lattice":
        assert (got[R.lattice_interior()] == np.float32(0.25)).all()
    if name == "denormal":
        assert (got > 0).any() and (got < np.finfo(np.float32).tiny).all()


def test_65536_identical_points_finish_with_exact_zeros():
    """Every bound and every distance is 0: only the non-strict skip rule (lb >= best[k - 1] once the list is full) keeps a
    wave from scanning all 1024 boxes for every point."""
    got = knn(R.identical(65_536))
    assert got.shape == (65_536,) and not R.bits(got).any()


def test_reconstruction_like_cloud_on_sampled_rows():
    P = 131_072
    x = R.sfm_like(P, seed=7)
    rows = np.random.default_rng(11).choice(P, 512, replace=False)
    want = R.brute(x, rows)
    got = knn(x)
    assert np.isfinite(got).all() and (got >= 0).all()
    assert_bits(got[rows], want, "sfm-like P=131072, sampled rows")


@pytest.mark.parametrize("name", ["uniform10007", "sfm4099"])
def test_the_result_follows_a_permutation_of_the_points(name):
    """knn(x[perm]) == knn(x)[perm]: the values do not depend on the Morton sort's input order or on ties in it."""
    x = R.uniform(10_007) if name == "uniform10007" else R.sfm_like(4099, seed=2)
    perm = np.random.default_rng(5).permutation(len(x))
    assert_bits(knn(x[perm]), knn(x)[perm], name)


def test_two_runs_and_an_offset_view_give_the_same_bits():
    from casualhdrsplat_amd import knn_mean_dist2
    x, want = brute_of("uniform10007", lambda: R.uniform(10_007))
    t = torch.from_numpy(x.copy()).to(DEV)
    a, b = knn_mean_dist2(t), knn_mean_dist2(t)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    flat = torch.empty(3 * len(x) + 1, dtype=torch.float32, device=DEV)
    view = flat[1:].view(len(x), 3)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4            # 4-byte aligned only
    c = knn_mean_dist2(view)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert_bits(a.cpu().numpy(), want, "uniform P=10007")
    nc = t.t().contiguous().t()                                          # not contiguous: made so by the front end
    assert not nc.is_contiguous()
    assert torch.equal(a.view(torch.int32), knn_mean_dist2(nc).view(torch.int32))


@pytest.mark.parametrize("P", [5, 1025])
def test_nothing_is_written_beyond_p_rows_or_the_stated_workspace(P):
    from casualhdrsplat_amd import _lib as L
    lib = L.load()
    x, want = brute_of(f"uniform{P}", lambda: R.uniform(P))
    xyz = torch.from_numpy(x.copy()).to(DEV)
    ws_bytes, pad = int(lib.hs_knn_workspace_bytes(P)), 4096
    out = torch.full((P + 64,), -7.0, dtype=torch.float32, device=DEV)
    ws = torch.full((ws_bytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    assert ws.data_ptr() % 256 == 0
    a = L.hs_knn_args()
    a.P, a.xyz, a.mean_d2, a.workspace, a.status = P, xyz.data_ptr(), out.data_ptr(), ws.data_ptr(), status.data_ptr()
    L.check(lib.hs_knn_mean_dist_sq(C.byref(a), torch.cuda.current_stream().cuda_stream), "hs_knn_mean_dist_sq")
    torch.cuda.synchronize()
    assert status.tolist() == [0, 77, 77, 77]
    assert_bits(out[:P].cpu().numpy(), want, f"raw call P={P}")
    assert (out[P:] == -7.0).all()
    assert (ws[ws_bytes:] == 0xA5).all()


def test_non_finite_coordinates_are_refused():
    from casualhdrsplat_amd import knn_mean_dist2
    x = torch.rand(100, 3, device=DEV)
    x[17, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        knn_mean_dist2(x)
    x[17, 1] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        knn_mean_dist2(x)
    assert knn_mean_dist2(torch.empty(0, 3, device=DEV)).shape == (0,)


def test_init_from_points_on_the_device_against_the_host_path():
    """log_scales within 2e-6 absolute of the host path's: half the distances' relative bound 8 * 2^-24 (tests/test_knn.py;
    log sqrt halves a relative error) = 2.4e-7, plus the float32 rounding of log_s itself, |log_s| * 2^-24 <= 6e-7 with
    |log_s| <= 10 -- both paths take the floor, the root and the log in float64.  Every other tensor is equal."""
    from casualhdrsplat_amd import GaussianRasterizer
    from casualhdrsplat_amd import scene_io as IO
    P = 10_007
    sc = S.make_scene(P, 160, 120, 3, seed=4, hdr=False)
    xyz = sc.means3D.numpy().astype(np.float32)                          # fp32-representable: both paths see the same points
    rgb = np.random.default_rng(9).integers(0, 256, (P, 3)).astype(np.uint8)
    host = IO.init_from_points(xyz.astype(np.float64), rgb, sh_degree=3)
    dev = IO.init_from_points(xyz.astype(np.float64), rgb, sh_degree=3, device=DEV)
    by_tensor = IO.init_from_points(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), sh_degree=3)
    for c in (dev, by_tensor):
        for t in (c.means3D, c.shs, c.opacity_logit, c.log_scales, c.rotations):
            assert t.device.type == "cuda" and t.dtype == torch.float32 and t.is_contiguous()
        assert float(host.log_scales.abs().max()) <= 10.0
        err = float((c.log_scales.cpu().double() - host.log_scales.double()).abs().max())
        print(f"init_from_points: max |log_scales(device) - log_scales(host)| = {err:.3e} (bound 2e-6)")
        assert err <= 2e-6, err
        assert torch.equal(c.means3D.cpu(), host.means3D) and torch.equal(c.shs.cpu(), host.shs)
        assert torch.equal(c.opacity_logit.cpu(), host.opacity_logit) and torch.equal(c.rotations.cpu(), host.rotations)
    assert torch.equal(dev.log_scales, by_tensor.log_scales)
    one = IO.init_from_points(xyz[:1], rgb[:1], sh_degree=0, device=DEV)   # a single point: d2 = 1, log_s = 0
    assert one.log_scales.tolist() == [[0.0, 0.0, 0.0]] and one.shs.shape == (1, 1, 3)

    st = dev.stored(DEV)
    rs, _, _ = Hh.settings_from_scene(sc, DEV)
    rast = GaussianRasterizer(rs, parameterization="raw")
    out = rast(st["means3D"], torch.zeros_like(st["means3D"]), st["opacities"], shs=st["shs"], scales=st["scales"],
               rotations=st["rotations"])
    img = out[0]
    assert img.shape == (3, 120, 160) and bool(torch.isfinite(img).all()) and float(img.abs().sum()) > 0
