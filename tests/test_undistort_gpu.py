"""Lens undistortion on the GPU (undistort.hip): the map bit for bit against the numpy float32 restatement (OPENCV_FISHEYE, whose
atanf is the device library's, against float64 in pixels), the remap bit for bit for uint8 HWC and fp32 CHW frames and
S = 1, 2, 3 on a hand-made map with every special the definition names and on the cameras' own maps, every element written
whatever the buffers held, no frames / one frame / more frames than one workgroup walks, and an end-to-end check against an
analytic image that does not go through the forward model.  97 x 61 source, seconds each.

HS_PARITY_REPORT=1 writes the fisheye figures to profiles/undistort_parity.json."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import poison
import undistort_reference as R
from casualhdrsplat_amd import undistort as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, F = R.W_SRC, R.H_SRC, 3
GRID_W, GRID_H = 120, 48          # the hand-made map: outputs 120, 60 and 40 wide (no multiple of 64), more than one block each way
_PARITY = {}


def gpu(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a copy: the cached inputs are read-only)


def same_bits(t, want):
    got = t.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    if os.environ.get("HS_PARITY_REPORT") and _PARITY:
        with open(os.path.join(ROOT, "profiles", "undistort_parity.json"), "w") as fh:
            json.dump(dict(bound="OPENCV_FISHEYE map: |device - float64| <= 4 x max |numpy float32 restatement - float64|, in source pixels",
                           cases=_PARITY), fh, indent=1, sort_keys=True)
            fh.write("\n")


# ---- inputs, made once ----

@functools.lru_cache(maxsize=None)
def frames_u8(n=F):
    a = np.random.default_rng(11).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    a[0, 0, 0], a[0, -1, -1], a[0, 0, -1], a[0, -1, 0] = (255, 0, 255), (0, 255, 0), (1, 2, 3), (254, 253, 252)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frames_f32(n=F):
    a = (np.random.default_rng(12).standard_normal((n, 3, H, W)) * 3.0).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def hand_map():
    """Random in-range positions; entries exactly on pixel centres (wx = wy = 0); on the last centre (px = W - 1, py = H - 1);
    outside the source on each side, far outside, at infinity; a NaN in x, one in y, one in both."""
    rng = np.random.default_rng(13)
    m = np.stack([rng.uniform(0.5, W - 0.5, (GRID_H, GRID_W)), rng.uniform(0.5, H - 0.5, (GRID_H, GRID_W))], axis=-1).astype(np.float32)
    centres = rng.random((GRID_H, GRID_W)) < 0.15
    m[centres] = np.floor(m[centres]) + np.float32(0.5)
    m[3, 5] = (W - 0.5, H - 0.5); m[3, 6] = (W - 0.5, 10.25); m[3, 7] = (20.75, H - 0.5); m[3, 8] = (0.5, 0.5)
    m[4, 64] = (W - 1.5, H - 1.5); m[4, 65] = (W - 1.0, H - 1.0)
    m[7, 1] = (-3.0, 12.0); m[7, 2] = (W + 5.0, 12.0); m[7, 3] = (30.0, -2.0); m[7, 4] = (30.0, H + 7.0)
    m[7, 70] = (0.25, 0.25); m[7, 71] = (W - 0.25, H - 0.25); m[7, 72] = (-1e30, 1e30); m[7, 73] = (np.inf, -np.inf)
    m[9, 9] = (np.nan, 12.0); m[9, 100] = (12.0, np.nan); m[47, 119] = (np.nan, np.nan)
    m[0, 0] = (W - 0.5, 0.5); m[47, 118] = (0.5, H - 0.5)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def hand_want(kind, S):
    want = R.remap_f32(frames_u8() if kind == "u8" else frames_f32(), hand_map(), S)
    want.setflags(write=False)
    return want


def frames_of(kind, n=F):
    return frames_u8(n) if kind == "u8" else frames_f32(n)


# ---- the map ----

@pytest.mark.parametrize("factor", [1, 2])
@pytest.mark.parametrize("name", R.EXACT)
def test_map_is_the_restatement_bit_for_bit(name, factor):
    cam, out, Wf, Hf, m32, valid, _ = R.camera_case(name, factor)
    umap = U.undistort_map(cam, factor, device=DEV)
    assert umap.map.shape == (Hf, Wf, 2) and umap.map.dtype == torch.float32 and umap.valid.shape == (Hf, Wf) and umap.valid.dtype == torch.uint8
    assert umap.factor == factor and umap.source_size == (W, H)
    assert (umap.camera.width, umap.camera.height, umap.camera.model) == (out.width, out.height, "PINHOLE")
    assert umap.camera.params.tolist() == out.params.tolist()
    got = umap.map.cpu().numpy()
    bad = np.argwhere(got.view(np.int32) != m32.view(np.int32))
    assert bad.size == 0, (name, factor, bad[:4], [(got[tuple(b)], m32[tuple(b)]) for b in bad[:4]])
    assert same_bits(umap.valid, valid) and bool(umap.valid.all())


def test_map_marks_samples_outside_the_source():
    """A grid larger than the rule allows (the raw entry point on a 2 x wider and taller grid): the restatement's bits, and
    both values of `valid`."""
    import ctypes as C
    from casualhdrsplat_amd import _lib as L
    cam = R.camera("opencv")
    Wf, Hf = 190, 114
    m32, valid = R.map_f32(cam, Wf, Hf)
    assert valid.any() and not valid.all()
    model, f4, k8 = U.kernel_parameters(cam)
    grid = poison.fill_(torch.empty((Hf, Wf, 2), dtype=torch.float32, device=DEV), "nan")
    v = poison.fill_(torch.empty((Hf, Wf), dtype=torch.uint8, device=DEV), "a5")
    a = L.hs_undistort_args()
    a.model, a.W, a.H, a.Wf, a.Hf = model, W, H, Wf, Hf
    a.fx, a.fy, a.cx, a.cy = (float(x) for x in f4)
    a.k = (C.c_float * 8)(*[float(x) for x in k8])
    a.map, a.valid = grid.data_ptr(), v.data_ptr()
    L.check(L.load().hs_undistort_map(C.byref(a), U._stream(grid.device)), "hs_undistort_map")
    assert same_bits(grid, m32) and same_bits(v, valid)


@pytest.mark.parametrize("factor", [1, 2])
def test_fisheye_map_against_float64_in_pixels(factor):
    """The device atanf need not be numpy's: the map is held to the float64 map in source pixels.  The yardstick is the numpy
    float32 restatement's own distance to float64 on the same case (1.3e-5 px on the CPU); the device gets 4 x that -- a few
    ulp each in atanf and in the quotient, at coordinates of about 100 px."""
    cam, out, Wf, Hf, m32, valid, m64 = R.camera_case("opencv_fisheye", factor)
    yard = float(np.abs(m32.astype(np.float64) - m64).max())
    bound = 4.0 * yard
    umap = U.undistort_map(cam, factor, device=DEV)
    got = umap.map.cpu().numpy()
    assert got.shape == m32.shape and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - m64).max())
    differing = int((got.view(np.int32) != m32.view(np.int32)).sum())
    _PARITY[f"opencv_fisheye_factor{factor}"] = dict(grid=[Wf, Hf], restatement_to_float64_px=float(f"{yard:.3e}"), bound_px=float(f"{bound:.3e}"),
                                                     device_to_float64_px=float(f"{err:.3e}"), entries_differing_from_restatement=differing,
                                                     entries=int(got.size))
    print(f"fisheye map factor {factor}: restatement {yard:.3e} px, device {err:.3e} px (bound {bound:.3e}), {differing} of {got.size} "
          "entries differ from the restatement", flush=True)
    assert 1e-6 < yard < 1e-4
    assert err <= bound, (err, bound)
    clear = R.hull_margin(m64, W, H) > bound
    assert clear.all()                                                    # (the condition of test_undistort.py: everything is inside)
    assert np.array_equal(umap.valid.cpu().numpy()[clear], valid[clear])


# ---- the remap ----

@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_remap_hand_made_map_bit_for_bit(kind, S):
    want = hand_want(kind, S)
    got = U.remap_frames(gpu(frames_of(kind)), gpu(hand_map()), S)
    assert got.shape == (F, 3, GRID_H // S, GRID_W // S) and got.dtype == torch.float32
    g = got.cpu().numpy()
    bad = np.argwhere(g.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, (kind, S, len(bad), bad[:6], [(g[tuple(b)], want[tuple(b)]) for b in bad[:6]])
    if S == 1:
        src = frames_u8().transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255) if kind == "u8" else frames_f32()
        assert np.array_equal(g[:, :, 3, 5], src[:, :, H - 1, W - 1]) and np.array_equal(g[:, :, 3, 8], src[:, :, 0, 0])   # the last / first centre
        assert np.array_equal(g[:, :, 7, 73], src[:, :, 0, W - 1])                                                        # (+inf, -inf) clamps
        assert not g[:, :, 9, 9].any() and not g[:, :, 9, 100].any() and not g[:, :, 47, 119].any()                     # NaN samples as 0
        if kind == "u8":
            assert g.min() >= 0.0 and g.max() <= 1.0 and g.max() == 1.0


@pytest.mark.parametrize("factor", [1, 2, 3])
@pytest.mark.parametrize("name", list(R.CAMERAS))
def test_remap_camera_maps_bit_for_bit(name, factor):
    umap = U.undistort_map(R.camera(name), factor, device=DEV)
    grid = umap.map.cpu().numpy()
    for kind in ("u8", "f32"):
        got = U.undistort_frames(gpu(frames_of(kind)), umap)
        assert got.shape == (F, 3, umap.camera.height, umap.camera.width)
        assert same_bits(got, R.remap_f32(frames_of(kind), grid, factor)), (name, factor, kind)


@pytest.mark.parametrize("pattern", ["ff", "nan", "a5", "random"])
def test_every_element_is_written_and_runs_repeat(monkeypatch, pattern):
    cam = R.camera("full_opencv")
    base = U.undistort_map(cam, 2, device=DEV)
    outs = {kind: U.remap_frames(gpu(frames_of(kind)), gpu(hand_map()), 3) for kind in ("u8", "f32")}
    assert same_bits(outs["u8"], hand_want("u8", 3)) and same_bits(outs["f32"], hand_want("f32", 3))
    with poison.poisoned(monkeypatch, pattern) as session:
        again = U.undistort_map(cam, 2, device=DEV)
        outs2 = {kind: U.remap_frames(gpu(frames_of(kind)), gpu(hand_map()), 3) for kind in ("u8", "f32")}
        cam_out = U.undistort_frames(gpu(frames_u8()), again)
    fills = session.require("casualhdrsplat_amd.undistort", at_least=5)   # map, valid, three outputs
    assert {f.dtype for f in fills} == {torch.float32, torch.uint8}
    assert poison.bytes_of(again.map) == poison.bytes_of(base.map) and poison.bytes_of(again.valid) == poison.bytes_of(base.valid)
    for kind in outs:
        assert poison.bytes_of(outs2[kind]) == poison.bytes_of(outs[kind]), kind
    assert poison.bytes_of(cam_out) == poison.bytes_of(U.undistort_frames(gpu(frames_u8()), base))


def test_no_frames_and_a_single_frame():
    umap = U.undistort_map(R.camera("radial"), 2, device=DEV)
    Ho, Wo = umap.camera.height, umap.camera.width
    for empty in (torch.empty(0, H, W, 3, dtype=torch.uint8, device=DEV), torch.empty(0, 3, H, W, device=DEV)):
        out = U.undistort_frames(empty, umap)
        assert out.shape == (0, 3, Ho, Wo) and out.dtype == torch.float32
    for kind in ("u8", "f32"):
        batch = gpu(frames_of(kind))
        full = U.undistort_frames(batch, umap)
        one = U.undistort_frames(batch[1], umap)
        assert one.shape == (3, Ho, Wo) and poison.bytes_of(one) == poison.bytes_of(full[1])
        assert poison.bytes_of(U.undistort_frames(batch[1:2], umap)) == poison.bytes_of(full[1:2])


@pytest.mark.parametrize("kind,n,S", [("u8", 8, 2), ("u8", 9, 2), ("f32", 19, 1)])
def test_more_frames_than_one_workgroup_walks(kind, n, S):
    """A workgroup walks up to 8 frames: 8 is one run, 9 two runs of 5 and 4, 19 three runs of 7, 7 and 5."""
    frames = frames_of(kind, n)
    got = U.remap_frames(gpu(frames), gpu(hand_map()), S)
    assert same_bits(got, R.remap_f32(frames, hand_map(), S))


def test_more_runs_of_frames_than_the_grid_has_slices():
    """65535 slices of frames at most: 8 x 65535 + 3 frames of 2 x 2 pixels make runs of 9."""
    n = 8 * 65535 + 3
    rng = np.random.default_rng(17)
    frames = rng.integers(0, 256, (n, 2, 2, 3), dtype=np.uint8)
    grid = np.array([[(0.5, 0.5), (1.5, 0.5), (1.0, 1.0), (0.75, 1.25)], [(1.5, 1.5), (0.5, 1.5), (np.nan, 1.0), (9.0, -9.0)]], np.float32)
    got = U.remap_frames(gpu(frames), gpu(grid), 1)
    assert same_bits(got, R.remap_f32(frames, grid, 1))
    got = U.remap_frames(gpu(frames), gpu(grid), 2)
    assert got.shape == (n, 3, 1, 2) and same_bits(got, R.remap_f32(frames, grid, 2))


# ---- end to end ----

def test_end_to_end_against_an_analytic_image():
    """Independent of the forward model's code path.  The scene is a smooth image of PINHOLE coordinates,
        I_c(u, v) = 0.5 + 0.2 sin(2 u + 0.3 + 0.7 c) + 0.15 cos(3 v - 0.2 + 0.7 c) + 0.1 sin(1.5 u + 2.5 v + 0.7 c),
    the captured frame is I at the Newton-undistorted centre of every source pixel (float64 on the host, a SIMPLE_RADIAL camera
    with k = -0.12, f = 80), and after undistort_frames every output pixel must equal I at its own centre within the bilinear
    bound M / 4 = 2 M / 8 plus 2^-20 for fp32, M = a bound on the pure second derivatives of the captured image per source pixel:
        |grad I| <= sqrt(0.55^2 + 0.7^2) < 0.8903 (|I_u| <= 0.2 2 + 0.1 1.5, |I_v| <= 0.15 3 + 0.1 2.5),
        |Hess I| <= 2.35 (the larger absolute row sum: I_uu <= 1.025, I_vv <= 1.975, I_uv <= 0.375).
    The captured image is g(x, y) = I(U(q)), q = ((x - cx) / f, (y - cy) / f), U the inverse of D(p) = p (1 + k |p|^2).
    DD(p) = (1 + k r^2) Id + 2 k p p^T is symmetric with eigenvalues 1 + k r^2 and 1 + 3 k r^2, so with k < 0
    |DU| <= Lam = 1 / (1 - 3 |k| r^2); D^2 D[a, b] = 2 k ((a.b) p + (p.a) b + (p.b) a) has norm <= 6 |k| r |a| |b|, and
    D^2 U[e, e] = -DU D^2 D[DU e, DU e] has norm <= 6 |k| r Lam^3.  Hence, r_max being the largest pinhole radius inside the frame
    (at a corner: U is radial and monotone),
        M = (2.35 Lam^2 + 0.8903 x 6 |k| r_max Lam^3) / f^2                      (about 7.9e-4; M / 4 about 2.0e-4).
    The fp32 term: the frame's rounding (2^-25), three roundings per lerp of values below 1, and the fp32 map's error of
    about 2e-5 px times a slope below 0.8903 Lam / f = 0.014 per pixel: 5e-7 together, under 2^-20.  A resampling that is
    off by a twentieth of a pixel somewhere misses the bound."""
    k, f = -0.12, 80.0
    cam = R.camera("simple_radial_barrel")
    assert cam.params.tolist() == [f, R.CX, R.CY, k]
    image = lambda u, v, c: (0.5 + 0.2 * np.sin(2 * u + 0.3 + 0.7 * c) + 0.15 * np.cos(3 * v - 0.2 + 0.7 * c)
                             + 0.1 * np.sin(1.5 * u + 2.5 * v + 0.7 * c))
    x, y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    u, v = U.undistort_points("SIMPLE_RADIAL", np.array([k]), (x - R.CX) / f, (y - R.CY) / f)
    r_max = float(np.hypot(u, v).max())
    assert r_max == max(float(np.hypot(u[j, i], v[j, i])) for j in (0, -1) for i in (0, -1)) and 0.7 < r_max < 0.8
    lam = 1.0 / (1.0 - 3.0 * abs(k) * r_max ** 2)
    M = (2.35 * lam ** 2 + 0.8903 * 6.0 * abs(k) * r_max * lam ** 3) / f ** 2
    assert 6e-4 < M < 8e-4
    frame = np.stack([image(u, v, c) for c in range(3)]).astype(np.float32)
    umap = U.undistort_map(cam, 1, device=DEV)
    got = U.undistort_frames(gpu(frame), umap).cpu().numpy().astype(np.float64)
    Wo, Ho = umap.camera.width, umap.camera.height
    fx, fy, cx, cy = umap.camera.params
    assert (fx, fy, cx, cy) == (f, f, Wo / 2, Ho / 2)
    xo, yo = np.meshgrid(np.arange(Wo) + 0.5, np.arange(Ho) + 0.5)
    want = np.stack([image((xo - cx) / fx, (yo - cy) / fy, c) for c in range(3)])
    err = float(np.abs(got - want).max())
    print(f"end to end: largest error {err:.3e}, bound {M / 4 + 2.0 ** -20:.3e} (M = {M:.3e})", flush=True)
    assert err <= M / 4 + 2.0 ** -20, (err, M)
