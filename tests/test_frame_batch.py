"""Frames in one rasterizer call (hs_dims.n_frames, settings.n_frames): everything that can be checked without a GPU --
hs_plan's sizes, the argument limits of the C ABI, the export, the Python argument errors and the shapes
HDRBlurFormation.forward_frames hands to the rasterizer."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (P, M, sh_degree, W, H, n_poses, capacity, crf_K): the dims tests/test_abi.py plans with, single- and multi-pose, with and
# without a CRF table, and one odd-sized HDR frame
DIMS = [(1000, 16, 3, 128, 128, 1, 10000, 0), (10, 1, 0, 32, 32, 1, 100, 0), (100_000, 1, 0, 800, 800, 1, 900_000, 0),
        (700, 1, 0, 256, 256, 16, 10_000, 0), (200_000, 1, 0, 1920, 1080, 4, 1_000_000, 0), (1500, 4, 1, 72, 40, 4, 20_000, 64),
        (1500, 4, 1, 72, 40, 12, 60_000, 256)]


@pytest.fixture(scope="module")
def lib():
    from casualhdrsplat_amd import _lib
    _lib.load()
    return _lib


def _plan(lib, dims, n_frames):
    d = lib.hs_dims(*dims, n_frames)
    sz, lay = lib.hs_sizes(), lib.hs_layout()
    rc = lib.load().hs_plan(C.byref(d), C.byref(sz), C.byref(lay))
    return rc, sz, lay


def _fields(s):
    return [getattr(s, n) for n, _ in s._fields_]


def test_plan_without_frames_is_the_plan_it_was(lib):
    """n_frames 0 and 1 are the call without frames: every size and every hs_layout offset equals those of a struct whose
    last word is zero (what the field was: `reserved`, 0)."""
    for dims in DIMS:
        rc0, sz0, lay0 = _plan(lib, dims, 0)
        rc1, sz1, lay1 = _plan(lib, dims, 1)
        assert rc0 == rc1 == lib.HS_OK
        assert _fields(sz0) == _fields(sz1) and _fields(lay0) == _fields(lay1), dims
        # ... and through the Python helper, whose default is the zeroed field
        _, szp, layp = lib.plan(*dims)
        assert _fields(szp) == _fields(sz0) and _fields(layp) == _fields(lay0)
    # the image workspace of a call without frames, stated: final_T and n_contrib per pose, one radiance plane per pose plus
    # ONE mean plane when N > 1, a work count and an order entry per (pose, tile); each region rounded up to 256 bytes
    P, M, deg, W, H, N, cap, K = DIMS[5]
    a256 = lambda n: (n + 255) // 256 * 256
    tiles = ((W + 15) // 16) * ((H + 15) // 16) * N
    want = 2 * a256(W * H * N * 4) + a256(W * H * 3 * 4 * (N + 1)) + 2 * a256(tiles * 4)
    assert _plan(lib, DIMS[5], 0)[1].image_bytes == want


def test_plan_with_frames_grows_the_image_workspace_by_the_extra_mean_planes(lib):
    """F = 3 frames of N = 4 poses: the image workspace holds one mean-radiance plane PER FRAME behind the 12 per-pose planes
    instead of one in all.  With a256(n) = n rounded up to 256 and plane = 3 * H * W * 4 bytes,
        image_bytes(F) - image_bytes(no frames) = a256(plane * (F * N + F)) - a256(plane * (F * N + 1));
    nothing else changes size, and nothing carved before pose_hdr moves."""
    dims = DIMS[6]
    P, M, deg, W, H, NP, cap, K = dims
    F, N = 3, 4
    assert NP == F * N
    rc0, sz0, lay0 = _plan(lib, dims, 0)
    rc3, sz3, lay3 = _plan(lib, dims, F)
    assert rc0 == rc3 == lib.HS_OK
    a256 = lambda n: (n + 255) // 256 * 256
    plane = 3 * H * W * 4
    extra = a256(plane * (F * N + F)) - a256(plane * (F * N + 1))
    assert extra > 0 and sz3.image_bytes - sz0.image_bytes == extra
    assert (sz3.geom_bytes, sz3.binning_bytes, sz3.bwd_bytes) == (sz0.geom_bytes, sz0.binning_bytes, sz0.bwd_bytes)
    for name, _ in lay0._fields_:
        if name in ("tile_work", "tile_order"):        # carved behind pose_hdr: they move by exactly the extra planes
            assert getattr(lay3, name) - getattr(lay0, name) == extra, name
        else:
            assert getattr(lay3, name) == getattr(lay0, name), name
    # one pose per frame keeps no mean plane at all: a batch of 4 plain views holds the 4 per-pose planes only, where the
    # 4-pose average without frames holds a fifth
    dims1 = (P, M, deg, W, H, 4, cap, K)
    assert _plan(lib, dims1, 0)[1].image_bytes - _plan(lib, dims1, 4)[1].image_bytes == a256(plane * 5) - a256(plane * 4)
    # the CRF-gradient scratch is one row per (pixel block, plane): its planes are the call's poses whatever the frames
    assert lay3.inst_grads - lay3.crf_partials == lay0.inst_grads - lay0.crf_partials > 0


@pytest.mark.parametrize("n_poses,n_frames,why", [(12, -1, "negative"), (12, 5, "not a divisor of n_poses"),
                                                  (4, 8, "more frames than poses")])
def test_frame_limits_are_einval_before_any_hip_call(lib, n_poses, n_frames, why):
    """n_frames < 0, n_poses % n_frames != 0 and n_frames > n_poses: HS_EINVAL from hs_plan, and from hs_forward / hs_backward
    with null data pointers (they plan first: nothing has touched the GPU)."""
    L = lib.load()
    d = lib.hs_dims(10, 1, 0, 32, 32, n_poses, 100, 0, n_frames)
    sz = lib.hs_sizes()
    assert L.hs_plan(C.byref(d), C.byref(sz), None) == lib.HS_EINVAL, why
    assert b"n_frames" in L.hs_last_error()
    a = lib.hs_fwd_args()
    a.dims = d
    assert L.hs_forward(C.byref(a), None) == lib.HS_EINVAL and b"n_frames" in L.hs_last_error()
    b = lib.hs_bwd_args()
    b.dims = d
    assert L.hs_backward(C.byref(b), None) == lib.HS_EINVAL and b"n_frames" in L.hs_last_error()
    # the neighbouring valid value passes on to the next check (this struct's null pointers)
    a.dims = lib.hs_dims(10, 1, 0, 32, 32, 12, 100, 0, 3)
    assert L.hs_forward(C.byref(a), None) == lib.HS_EINVAL and b"null" in L.hs_last_error()


def test_per_image_gradients_are_einval_with_frames(lib):
    """dL_dout_alpha / dL_dout_invdepth are gradients of ONE image: together with n_frames > 1 hs_backward refuses them
    before it looks at anything else; without frames the same struct passes on to the null-pointer check."""
    L = lib.load()
    for field in ("dL_dout_alpha", "dL_dout_invdepth"):
        b = lib.hs_bwd_args()
        b.dims = lib.hs_dims(10, 1, 0, 32, 32, 12, 100, 0, 3)
        setattr(b, field, 4096)
        assert L.hs_backward(C.byref(b), None) == lib.HS_EINVAL
        assert b"n_frames" in L.hs_last_error() and b"per-image" in L.hs_last_error(), L.hs_last_error()
        b.dims.n_frames = 1
        assert L.hs_backward(C.byref(b), None) == lib.HS_EINVAL and b"n_frames" not in L.hs_last_error()


def test_probe_is_declared_listed_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bHS_API\s+int\s+hs_max_frames\s*\(\s*void\s*\)", header)
    assert re.search(r"\bint32_t\s+n_frames\s*;", header) and not re.search(r"\bint32_t\s+reserved\s*;\s*}\s*hs_dims", header)
    assert "hs_max_frames" in lib.EXPORTS
    assert set(re.findall(r"\b(hs_[a-z_]+)\s*\(", header)) == set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert re.search(r"\bT hs_max_frames\b", out), path
    assert lib.load().hs_version() == 309 == lib.HS_VERSION          # (detected by name: the version does not move)
    assert lib.max_frames() == lib.load().hs_max_frames() >= 21845   # every pose may be a frame of its own
    assert [n for n, _ in lib.hs_dims._fields_][-1] == "n_frames" and C.sizeof(lib.hs_dims) == 40


def test_a_library_without_the_probe_refuses_frames(lib, monkeypatch):
    """A stale library has no hs_max_frames and reads n_frames as a reserved word: asking it for frames is a RuntimeError
    that says so, not one image of all poses; calls without frames go through."""
    real = lib.load()

    class Stale:
        def __getattr__(self, name):
            if name == "hs_max_frames":
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(lib, "_lib", Stale())
    try:
        assert lib.max_frames() == 0
        with pytest.raises(RuntimeError, match="hs_max_frames"):
            lib.plan(10, 1, 0, 32, 32, 12, 100, 0, 3)
        lib.plan(10, 1, 0, 32, 32, 12, 100, 0, 1)
        lib.plan(10, 1, 0, 32, 32, 12, 100)
    finally:
        monkeypatch.setattr(lib, "_lib", real)


def _settings(n_frames, n_poses, exposure=None, hdr=True, shape4=False):
    from casualhdrsplat_amd import GaussianRasterizationSettings
    eye = torch.eye(4)
    V = eye.repeat(n_poses, 1, 1)
    Cp = torch.zeros(n_poses, 3)
    if shape4:
        V, Cp = V.reshape(n_frames, -1, 4, 4), Cp.reshape(n_frames, -1, 3)
    return GaussianRasterizationSettings(
        image_height=40, image_width=72, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=eye,
        projmatrix=eye, sh_degree=0, campos=torch.zeros(3), exposure=exposure,
        crf_table=torch.linspace(0, 1, 16).repeat(3, 1) if hdr else None, viewmatrices=V, projmatrices=V.clone(), camposes=Cp,
        n_frames=n_frames)


def _call(rs, **kw):
    from casualhdrsplat_amd import GaussianRasterizer
    P = 8
    m = torch.zeros(P, 3)
    return GaussianRasterizer(rs, **kw)(m, torch.zeros_like(m), torch.full((P, 1), 0.5), shs=torch.zeros(P, 1, 3),
                                        scales=torch.ones(P, 3), rotations=torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1))


def test_settings_field_is_appended_and_defaults_to_no_frames():
    from casualhdrsplat_amd import GaussianRasterizationSettings as RS
    assert RS._fields[-1] == "n_frames" and RS._field_defaults["n_frames"] == 1


def test_argument_errors_are_value_errors_before_anything_touches_a_gpu():
    """CPU tensors everywhere: a well-formed call ends in the "MI355X only" RuntimeError; each malformed one in a ValueError
    BEFORE it."""
    with pytest.raises(RuntimeError, match="MI355X"):
        _call(_settings(3, 12, exposure=torch.tensor([0.5, 1.0, 1.7])))
    with pytest.raises(RuntimeError, match="MI355X"):                      # [F,N,...] cameras are accepted
        _call(_settings(3, 12, exposure=torch.tensor([0.5, 1.0, 1.7]), shape4=True))
    with pytest.raises(ValueError, match="n_frames=5"):                    # 12 poses are not 5 frames
        _call(_settings(5, 12, exposure=torch.ones(5)))
    with pytest.raises(ValueError, match="n_frames=8"):                    # more frames than poses
        _call(_settings(8, 4, exposure=torch.ones(8)))
    with pytest.raises(ValueError, match="one value per frame"):           # an exposure of the wrong length
        _call(_settings(3, 12, exposure=torch.tensor(0.5)))
    with pytest.raises(ValueError, match="one value per frame"):
        _call(_settings(3, 12, exposure=torch.ones(12)))
    with pytest.raises(ValueError, match="n_frames"):
        _call(_settings(-2, 12))
    for kw in ({"return_alpha": True}, {"return_invdepth": True}):         # per-image outputs together with frames
        with pytest.raises(ValueError, match="per-image"):
            _call(_settings(3, 12, exposure=torch.ones(3)), **kw)
        with pytest.raises(RuntimeError, match="MI355X"):                  # ... and without frames they are what they were
            _call(_settings(1, 12, exposure=torch.tensor(0.5)), **kw)
    # frames need the pose stacks
    from casualhdrsplat_amd import GaussianRasterizationSettings
    rs = _settings(1, 1)._replace(viewmatrices=None, projmatrices=None, camposes=None, n_frames=2)
    assert isinstance(rs, GaussianRasterizationSettings)
    with pytest.raises(ValueError, match="viewmatrices"):
        _call(rs)


def test_forward_frames_hands_the_rasterizer_one_call_of_the_right_shapes():
    """HDRBlurFormation.forward_frames: ONE factory call whose settings hold the listed frames' cameras_all() slices,
    exp(log_exposure[frame_ids]) and n_frames = F; the images come back [F,3,H,W]."""
    from casualhdrsplat_amd.image_formation import HDRBlurFormation, ImplicitCRF, TrajectorySpline, knots_from_lookat
    W, H, n_all, N, P = 72, 40, 4, 3, 6
    seen = []

    def factory(settings):
        seen.append(settings)
        F = settings.n_frames

        def rast(means3D, means2D, opacities, shs=None, scales=None, rotations=None):
            shape = (F, 3, H, W) if F > 1 else (3, H, W)
            return torch.zeros(shape), torch.zeros(P, dtype=torch.int32), torch.ones(shape)
        return rast

    model = HDRBlurFormation(TrajectorySpline(knots_from_lookat(n_all + 3), kind="cubic"), n_all, W, H, 0.5, 0.4, n_virtual=N,
                             crf=ImplicitCRF(K=16), sh_degree=1, rasterizer_factory=factory)
    with torch.no_grad():
        model.log_exposure.copy_(torch.tensor([0.0, -0.7, 0.5, 0.2]))
    cloud = (torch.zeros(P, 3), torch.full((P, 1), 0.5), torch.zeros(P, 4, 3), torch.ones(P, 3), torch.ones(P, 4))
    V, PV, Cp = model.cameras_all()
    for ids in ([0, 1, 2, 3], [2, 0, 3], range(4), [1]):
        seen.clear()
        ldr, hdr, radii, means2D = model.forward_frames(ids, *cloud)
        ids = list(ids)
        F = len(ids)
        assert len(seen) == 1
        rs = seen[0]
        assert rs.n_frames == F and (rs.image_width, rs.image_height) == (W, H) and rs.blur_domain == "ldr"
        assert tuple(rs.viewmatrices.shape) == (F, N, 4, 4) and tuple(rs.projmatrices.shape) == (F, N, 4, 4)
        assert tuple(rs.camposes.shape) == (F, N, 3) and tuple(rs.exposure.shape) == (F,)
        assert tuple(rs.crf_table.shape) == (3, 16)
        assert torch.equal(rs.viewmatrices, V[ids]) and torch.equal(rs.projmatrices, PV[ids]) and torch.equal(rs.camposes, Cp[ids])
        assert torch.equal(rs.exposure, torch.exp(model.log_exposure)[ids])
        assert tuple(ldr.shape) == tuple(hdr.shape) == (F, 3, H, W) and tuple(radii.shape) == (P,)
        assert tuple(means2D.shape) == (P, 3)
    # a given cameras_all() result is used as it is: no second pass over the spline
    seen.clear()
    model.forward_frames([3, 1], *cloud, cameras=(V, PV, Cp))
    assert seen[0].viewmatrices.data_ptr() != V.data_ptr() and torch.equal(seen[0].viewmatrices, V[[3, 1]])
    with pytest.raises(ValueError, match="frame_ids"):
        model.forward_frames([0, 4], *cloud)
    with pytest.raises(ValueError, match="frame_ids"):
        model.forward_frames([], *cloud)


def test_example_refuses_batch_frames_under_graph():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_synthetic_fb", os.path.join(ROOT, "examples", "train_synthetic.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    with pytest.raises(ValueError, match="batch-frames"):
        ex.run(P=10, W=32, H=32, frames=2, virtual=2, steps=1, device="cpu", graph=True, batch_frames=True)
