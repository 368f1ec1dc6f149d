"""numpy restatements of the lens undistortion (csrc/undistort.hip, casualhdrsplat_amd/undistort.py) and the test cameras.

map_f32 / remap_f32 restate the two kernels operation by operation in float32, in the order stated at the top of undistort.hip:
the GPU must give their bits (the OPENCV_FISHEYE map, whose atanf is the device library's, is held to map_f64 in pixels
instead).  map_f64 is the same map in float64 from the unrounded camera.  rule_size restates the size rule of
undistorted_camera with a solver of its own (a fixed-point iteration, not the package's Newton).  Not a test module: tests
import it."""
import functools

import numpy as np

from casualhdrsplat_amd import undistort as U
from casualhdrsplat_amd.scene_io import ColmapCamera

W_SRC, H_SRC = 97, 61
CX, CY = 50.3, 29.1
# name -> (model, parameters): the cameras of the tests, all on a 97 x 61 source
CAMERAS = {
    "simple_pinhole": ("SIMPLE_PINHOLE", [80.0, CX, CY]),
    "pinhole": ("PINHOLE", [80.0, 78.0, CX, CY]),
    "simple_radial_barrel": ("SIMPLE_RADIAL", [80.0, CX, CY, -0.12]),
    "simple_radial_pincushion": ("SIMPLE_RADIAL", [80.0, CX, CY, 0.15]),
    "radial": ("RADIAL", [80.0, CX, CY, -0.10, 0.03]),
    "opencv": ("OPENCV", [80.0, 78.0, CX, CY, -0.10, 0.03, 0.004, -0.003]),
    "full_opencv": ("FULL_OPENCV", [80.0, 78.0, CX, CY, -0.10, 0.03, 0.004, -0.003, 0.01, 0.02, -0.01, 0.005]),
    "opencv_fisheye": ("OPENCV_FISHEYE", [60.0, 59.0, CX, CY, -0.03, 0.01, -0.004, 0.001]),
}
EXACT = tuple(n for n in CAMERAS if n != "opencv_fisheye")      # no transcendental: bit for bit


def camera(name: str) -> ColmapCamera:
    model, params = CAMERAS[name]
    return ColmapCamera(1, model, W_SRC, H_SRC, np.asarray(params, np.float64))


def f32(x):
    return np.float32(x)


def distort_f32(model_id: int, k, u, v):
    """undistort.hip's distort<MODEL>: u, v float32 arrays, k float32[8]."""
    one = f32(1)
    if model_id in (0, 1):
        return u, v
    uu, vv = u * u, v * v
    r2 = uu + vv
    if model_id == 2:
        rad = k[0] * r2
        return u + u * rad, v + v * rad
    if model_id == 3:
        r4 = r2 * r2
        rad = k[0] * r2 + k[1] * r4
        return u + u * rad, v + v * rad
    if model_id in (4, 6):
        r4, uv = r2 * r2, u * v
        tu = (k[2] + k[2]) * uv + k[3] * (r2 + (uu + uu))
        tv = (k[3] + k[3]) * uv + k[2] * (r2 + (vv + vv))
        if model_id == 4:
            rad = k[0] * r2 + k[1] * r4
            return u + (u * rad + tu), v + (v * rad + tv)
        r6 = r4 * r2
        num = ((one + k[0] * r2) + k[1] * r4) + k[4] * r6
        den = ((one + k[5] * r2) + k[6] * r4) + k[7] * r6
        s = num / den
        return u * s + tu, v * s + tv
    assert model_id == 5
    r = np.sqrt(r2)
    big = r > f32(1e-8)
    t = np.arctan(r)
    t2 = t * t
    t4 = t2 * t2
    t6, t8 = t4 * t2, t4 * t4
    td = t * ((((one + k[0] * t2) + k[1] * t4) + k[2] * t6) + k[3] * t8)
    s = np.where(big, td / np.where(big, r, one), one).astype(np.float32)
    return u * s, v * s


def map_f32(cam: ColmapCamera, Wf: int, Hf: int):
    """(map [Hf, Wf, 2] float32, valid [Hf, Wf] uint8): undistort_map_kernel restated."""
    model_id, (fx, fy, cx, cy), k = U.kernel_parameters(cam)
    half = f32(0.5)
    x = ((np.arange(Wf, dtype=np.float32) + half) - half * f32(Wf)) / fx
    y = ((np.arange(Hf, dtype=np.float32) + half) - half * f32(Hf)) / fy
    u, v = np.meshgrid(x, y)
    with np.errstate(all="ignore"):
        ud, vd = distort_f32(model_id, k, u, v)
        sx, sy = ud * fx + cx, vd * fy + cy
        valid = (sx >= half) & (sx <= f32(cam.width) - half) & (sy >= half) & (sy <= f32(cam.height) - half)
    out = np.stack([sx, sy], axis=-1)
    assert out.dtype == np.float32
    return out, valid.astype(np.uint8)


def map_f64(cam: ColmapCamera, Wf: int, Hf: int):
    """The map in float64 from the unrounded camera: [Hf, Wf, 2]."""
    fx, fy, cx, cy, k = U.intrinsics(cam)
    u, v = np.meshgrid((np.arange(Wf) + 0.5 - Wf / 2.0) / fx, (np.arange(Hf) + 0.5 - Hf / 2.0) / fy)
    ud, vd = U.distort(cam.model, k, u, v)
    return np.stack([ud * fx + cx, vd * fy + cy], axis=-1)


def remap_f32(frames: np.ndarray, grid: np.ndarray, S: int) -> np.ndarray:
    """undistort_remap_kernel restated: frames uint8 [F, H, W, 3] or float32 [F, 3, H, W], grid float32 [Hf, Wf, 2] ->
    float32 [F, 3, Hf / S, Wf / S]."""
    u8 = frames.dtype == np.uint8
    planes = frames.transpose(0, 3, 1, 2).astype(np.float32) if u8 else frames
    assert planes.dtype == np.float32 and grid.dtype == np.float32
    F, _, H, W = planes.shape
    Hf, Wf, _ = grid.shape
    acc = np.zeros((F, 3, Hf // S, Wf // S), np.float32)
    half, zero, one = f32(0.5), f32(0), f32(1)
    with np.errstate(invalid="ignore"):
        for j in range(S):
            for i in range(S):
                sx, sy = grid[j::S, i::S, 0], grid[j::S, i::S, 1]
                ok = ~(np.isnan(sx) | np.isnan(sy))
                px = np.minimum(np.maximum(np.where(np.isnan(sx), zero, sx - half), zero), f32(W - 1))
                py = np.minimum(np.maximum(np.where(np.isnan(sy), zero, sy - half), zero), f32(H - 1))
                x0 = np.minimum(np.floor(px).astype(np.int32), W - 2)
                y0 = np.minimum(np.floor(py).astype(np.int32), H - 2)
                wx, wy = px - x0.astype(np.float32), py - y0.astype(np.float32)
                t00, t01 = planes[:, :, y0, x0], planes[:, :, y0, x0 + 1]
                t10, t11 = planes[:, :, y0 + 1, x0], planes[:, :, y0 + 1, x0 + 1]
                ox, oy = one - wx, one - wy
                top = ox * t00 + wx * t01
                bot = ox * t10 + wx * t11
                s = oy * top + wy * bot
                acc = acc + np.where(ok, s, zero)
    out = acc / f32(S * S)
    if u8:
        out = out / f32(255)
    assert out.dtype == np.float32
    return out


def invert_fixed_point(model: str, k, ud, vd, iters: int = 200):
    """(u, v) with distort(u, v) = (ud, vd), by the iteration x <- x - (distort(x) - target): a contraction for the mild
    distortions of CAMERAS.  Independent of the package's Newton."""
    u, v = np.array(ud, np.float64), np.array(vd, np.float64)
    for _ in range(iters):
        fu, fv = U.distort(model, k, u, v)
        u, v = u - (fu - ud), v - (fv - vd)
    return u, v


def rule_size(cam: ColmapCamera, factor: int):
    """(W', H') by the rule of undistorted_camera's docstring, with invert_fixed_point."""
    fx, fy, cx, cy, k = U.intrinsics(cam)
    W, H = cam.width, cam.height
    ys, xs = np.arange(H) + 0.5, np.arange(W) + 0.5
    inv = lambda x, y: invert_fixed_point(cam.model, k, (x - cx) / fx, (y - cy) / fy)
    u_left, u_right = inv(np.full(H, 0.5), ys)[0], inv(np.full(H, W - 0.5), ys)[0]
    v_top, v_bottom = inv(xs, np.full(W, 0.5))[1], inv(xs, np.full(W, H - 0.5))[1]
    a, b = min(-u_left.max(), u_right.min()), min(-v_top.max(), v_bottom.min())
    return 2 * factor * int(np.floor(fx * a / factor)), 2 * factor * int(np.floor(fy * b / factor))


@functools.lru_cache(maxsize=None)
def camera_case(name: str, factor: int):
    """(camera, output camera, Wf, Hf, map float32, valid, map float64) of a test camera: computed once, not to be modified."""
    cam = camera(name)
    out = U.undistorted_camera(cam, factor)
    Wf, Hf = out.width * factor, out.height * factor
    m32, valid = map_f32(cam, Wf, Hf)
    m64 = map_f64(cam, Wf, Hf)
    for a in (m32, valid, m64):
        a.setflags(write=False)
    return cam, out, Wf, Hf, m32, valid, m64


def hull_margin(m64: np.ndarray, W: int, H: int) -> np.ndarray:
    """Distance in pixels of every float64 sample to the edge of the hull of the source's pixel centres (negative: outside)."""
    sx, sy = m64[..., 0], m64[..., 1]
    return np.minimum(np.minimum(sx - 0.5, W - 0.5 - sx), np.minimum(sy - 0.5, H - 0.5 - sy))
