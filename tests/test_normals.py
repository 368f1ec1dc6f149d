"""CPU checks of the depth-normal consistency term and of the per-Gaussian normal (normals.hip: hs_normal_consistency*,
hs_gaussian_normals*; normals.normal_consistency_loss, normals.gaussian_normals): the TRUTH the GPU tests compare with
(tests/normals_reference.py) against what follows from the definition -- central finite differences in float64, the closed
form of a tilted plane, the identity between the kernel's closed form and the plain cross product -- its float32 restatement
against the bound the GPU tests hold the kernels to, on the same cases (`case`, `gn_case`, shared with
tests/test_normals_gpu.py), the C ABI (exports, struct layout, validation before any HIP call) and the Python refusals."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest
import torch

import normals_reference as NR
from casualhdrsplat_amd import normals as NM      # (the module under test: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_normal_consistency_workspace_bytes", "hs_normal_consistency", "hs_normal_consistency_backward",
         "hs_gaussian_normals", "hs_gaussian_normals_backward")

# ---- the cases of the GPU tests: name -> (B, H, W), what is given, holes as (kind, b, y, x) ----
# The kernels' tile is 64 x 16: (2, 33, 129) is one more than a multiple of it in both directions, (1, 16, 64) exactly one
# tile, (1, 5, 70) and (2, 37, 70) cut the tile unevenly, (1, 208, 320) is the example's frame (13 x 5 tiles).
ALL = ("alpha", "weight", "rot")
SHAPES = {
    "one_interior": ((1, 3, 3), ALL, ()),
    "row": ((1, 1, 7), ALL, ()),
    "two_columns": ((1, 7, 2), ALL, ()),
    "strip": ((1, 5, 70), ("alpha",), (("d0", 0, 2, 64),)),
    "holes": ((2, 37, 70), ALL, (("d0", 0, 0, 0), ("nan", 0, 0, 20), ("a0", 0, 10, 30), ("a0", 0, 10, 31), ("d0", 1, 16, 64),
                                 ("nan", 1, 15, 63), ("a0", 1, 36, 69), ("d0", 1, 20, 0))),
    "one_tile": ((1, 16, 64), (), ()),
    "tile_plus_one": ((2, 33, 129), ("weight", "rot"), (("d0", 0, 16, 64), ("nan", 1, 32, 128), ("d0", 1, 15, 64))),
    "example": ((1, 208, 320), ALL, (("d0", 0, 100, 127), ("d0", 0, 100, 128), ("nan", 0, 207, 5))),
}
EXTRA = {"fd": ((1, 7, 9), ALL, (("d0", 0, 3, 4),))}      # the finite-difference case of this file
_CASES = {}


def case(name):
    """dict(invdepth, alpha, normals, weight, rot, g, fx, fy) as float32 numpy (None for what the case leaves out)"""
    if name in _CASES:
        return _CASES[name]
    (B, H, W), given, holes = SHAPES[name] if name in SHAPES else EXTRA[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    yy, xx = np.mgrid[0:H, 0:W]
    z = np.stack([4.0 + 1.6 * np.sin(3.0 * xx / W + b) * np.cos(2.0 * yy / H + 0.5 * b) for b in range(B)])
    z = np.clip(z * (1.0 + 0.01 * rng.standard_normal(z.shape)), 2.0, 6.0)        # a smooth surface with 1 % noise
    alpha = (0.3 + 0.7 * rng.random((B, H, W))).astype(np.float32)
    a = alpha if "alpha" in given else np.ones_like(alpha)
    invdepth = (a / z).astype(np.float32)
    for kind, b, y, x in holes:
        if kind == "d0":
            invdepth[b, y, x] = 0.0
        elif kind == "nan":
            invdepth[b, y, x] = np.nan
        else:
            assert "alpha" in given
            alpha[b, y, x] = 0.0
    n = rng.standard_normal((B, 3, H, W))
    normals = (n / np.linalg.norm(n, axis=1, keepdims=True) * a[:, None]).astype(np.float32)
    rot = np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(B)])
    rot *= np.sign(np.linalg.det(rot))[:, None, None]
    _CASES[name] = dict(
        invdepth=invdepth, alpha=alpha if "alpha" in given else None, normals=normals,
        weight=rng.random((B, H, W)).astype(np.float32) if "weight" in given else None,
        rot=rot.astype(np.float32) if "rot" in given else None, g=rng.standard_normal((B, H, W)).astype(np.float32),
        fx=1.1 * max(W, 3), fy=0.9 * max(W, 3), holes=holes, shape=(B, H, W))
    return _CASES[name]


def ref_args(c):
    return (c["invdepth"], c["normals"], c["fx"], c["fy"], c["alpha"], c["weight"], c["rot"], c["g"])


_REFS = {}


def reference(name):
    """(truth, magnitudes) of a case, computed once"""
    if name not in _REFS:
        c = case(name)
        _REFS[name] = (NR.truth(*ref_args(c)), NR.magnitudes(*ref_args(c)))
    return _REFS[name]


GN_SIZES = (1, 63, 64, 65, 1000)
_GN = {}


def gn_case(P):
    """dict(rotations, scales, means3D, campos, g): ties in the scales, both signs, a zero quaternion (P > 1)"""
    if P in _GN:
        return _GN[P]
    rng = np.random.default_rng(200 + P)
    q = (rng.standard_normal((P, 4)) * rng.uniform(0.3, 3.0, (P, 1))).astype(np.float32)
    s = rng.uniform(0.01, 1.0, (P, 3)).astype(np.float32)
    if P > 10:
        q[5] = 0.0
        s[7] = (0.2, 0.2, 0.5)       # tie of 0 and 1: k = 0
        s[8] = (0.5, 0.2, 0.2)       # tie of 1 and 2: k = 1
        s[9] = (0.3, 0.3, 0.3)       # all equal: k = 0
    if P > 100:                      # rows without a direction beside |q| = 0 (hdrsplat.h): zeros both ways
        q[11, 2] = np.inf
        q[12, 0] = np.nan
        q[13] = (1e20, 0.0, 1e20, 0.0)          # the fp32 sum of squares overflows
        q[14] = (0.0, 1e-30, 0.0, 0.0)          # ... underflows to 0
    means = rng.standard_normal((P, 3)).astype(np.float32)
    campos = np.array([0.3, -0.2, 4.0], np.float32)
    g = rng.standard_normal((P, 3)).astype(np.float32)
    _GN[P] = dict(rotations=q, scales=s, means3D=means, campos=campos, g=g)
    # no row sits on the sign's threshold: the margin is far above its own rounding
    m = NR.gaussian_normals(q, s, means, campos, g, mode="mag")
    assert (m["margin"][m["live"]] > 64 * 2.0 ** -24 * m["margin_mag"][m["live"]]).all(), P
    return _GN[P]


def gn_args(c):
    return (c["rotations"], c["scales"], c["means3D"], c["campos"], c["g"])


# ---- the truth against what follows from the definition ----

def _loss64(d, a, N, c):
    t = NR.truth(d, N, c["fx"], c["fy"], a, c["weight"], c["rot"], c["g"], cast=np.float64)
    return float((t["out"] * c["g"].astype(np.float64)).sum())


def test_float64_gradients_against_central_differences():
    c = case("fd")
    d, a, N = (c[k].astype(np.float64) for k in ("invdepth", "alpha", "normals"))
    t = NR.truth(d, N, c["fx"], c["fy"], a, c["weight"], c["rot"], c["g"], cast=np.float64)
    assert t["interior"].sum() == 5 * 7 - 5 and t["out"][0, 3, 4] == 0 and t["out"][0, 3, 5] == 0
    eps = 1e-6
    for key, x in (("d_invdepth", d), ("d_alpha", a), ("d_normals", N)):
        fd = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            if key != "d_normals" and not t["valid"][idx]:
                continue
            val = []
            for sign in (1.0, -1.0):
                y = x.copy()
                y[idx] += sign * eps
                val.append(_loss64(y if key == "d_invdepth" else d, y if key == "d_alpha" else a, y if key == "d_normals" else N, c))
            fd[idx] = (val[0] - val[1]) / (2 * eps)
        scale = np.abs(t[key]).max()
        assert scale > 1e-2 and np.abs(fd - t[key]).max() <= 1e-7 * scale, (key, scale, np.abs(fd - t[key]).max())
    # the hole and the samples that feed no interior pixel (the corners) have exactly no gradient
    for key in ("d_invdepth", "d_alpha"):
        assert t[key][0, 3, 4] == 0 and t[key][0, 0, 0] == 0 and t[key][0, 6, 8] == 0 and t[key][0, 0, 4] != 0


def test_a_tilted_plane_yields_its_own_normal():
    """The plane n . X = c seen in perspective: z = c / (n . ray), every difference of back-projected points lies in the plane,
    so the depth normal is the plane's, turned to the camera (n . P < 0)."""
    H, W, fx, fy = 12, 17, 20.0, 14.0
    n = np.array([0.3, -0.5, -0.81])
    n /= np.linalg.norm(n)
    xh, yh = NR._centres(H, W)
    ray = np.stack(np.broadcast_arrays(xh[None, :] / fx, yh[:, None] / fy, np.ones((H, W))), -1)
    c0 = -5.0                                  # n . P = c0 < 0: the plane faces the camera with this n
    z = c0 / (ray @ n)
    assert (z > 0).all()
    t = NR.truth((1.0 / z)[None], np.zeros((1, 3, H, W)), fx, fy, cast=np.float64)
    got = np.moveaxis(t["depth_normals"][0], 0, -1)[1:-1, 1:-1]
    assert np.abs(got - n).max() <= 1e-12 and t["interior"].sum() == (H - 2) * (W - 2)
    # through a rotation, and against normals that agree: a zero map
    R = np.linalg.qr(np.random.default_rng(1).standard_normal((3, 3)))[0]
    N = np.broadcast_to((R @ n)[:, None, None], (3, H, W))[None]
    t = NR.truth((1.0 / z)[None], N, fx, fy, cam_to_world=R[None], cast=np.float64)
    assert np.abs(t["out"]).max() <= 1e-12


@pytest.mark.parametrize("name", tuple(SHAPES))
def test_the_closed_form_is_the_plain_definition(name):
    c = case(name)
    t, f = reference(name)[0], NR.closed_form(*ref_args(c))
    for k in NR.KEYS:
        scale = max(1.0, np.abs(t[k]).max())
        assert np.abs(t[k] - f[k]).max() <= 1e-11 * scale, (name, k)
        assert ((t[k] == 0) == (f[k] == 0)).all(), (name, k)


def _brute_interior(c):
    B, H, W = c["shape"]
    d, a = c["invdepth"], c["alpha"]
    ok = lambda b, y, x: bool(np.isfinite(d[b, y, x]) and d[b, y, x] > 0 and (a is None or (np.isfinite(a[b, y, x]) and a[b, y, x] > 0)))
    return {(b, y, x) for b in range(B) for y in range(1, H - 1) for x in range(1, W - 1)
            if all(ok(b, y + dy, x + dx) for dy, dx in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)))}


@pytest.mark.parametrize("name", tuple(SHAPES))
def test_holes_kill_exactly_the_pixels_the_definition_says(name):
    c = case(name)
    B, H, W = c["shape"]
    t = reference(name)[0]
    want = _brute_interior(c)
    assert {tuple(i) for i in np.argwhere(t["interior"])} == want
    killed = {(b, y + dy, x + dx) for _, b, y, x in c["holes"] for dy, dx in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0))
              if 1 <= y + dy <= H - 2 and 1 <= x + dx <= W - 2}
    assert len(want) == B * max(H - 2, 0) * max(W - 2, 0) - len(killed)
    for k in NR.KEYS:
        off = ~t["interior"] if t[k].ndim == 3 else np.broadcast_to(~t["interior"][:, None], t[k].shape)
        if k in ("out", "depth_normals", "d_normals"):
            assert not t[k][off].any(), (name, k)
    assert not t["d_invdepth"][~t["valid"]].any() and not t["d_alpha"][~t["valid"]].any()
    if name == "holes":        # a corner hole kills nothing, an edge hole one pixel, an adjacent pair eight
        i = t["interior"]
        assert i[0, 1, 1] and not i[0, 1, 20] and i[0, 1, 19] and i[0, 1, 21] and i[0, 2, 20]
        assert (~i[0, 9:12, 29:33]).sum() == 8 and i[0, 9, 29] and i[0, 11, 32]


@pytest.mark.parametrize("name", tuple(SHAPES))
def test_the_float32_restatement_lies_inside_the_bound_with_constant_one(name):
    """The bound of the GPU tests is worth something only if the float32 restatement alone sits well inside it: constant <= 1
    on every case and output (the GPU tests allow C_BOUND = 8)."""
    c = case(name)
    t, m = reference(name)
    f = NR.closed_form(*ref_args(c), dtype=np.float32)
    need = {k: NR.needed(f[k], t[k], m[k]) for k in NR.KEYS}
    print(f"normals float32 restatement {name}: C needed {need}")
    assert all(f[k].dtype == np.float32 for k in NR.KEYS)
    assert all(v <= 1.0 for v in need.values()), (name, need)
    for k in NR.KEYS:
        assert ((f[k] == 0) == (t[k] == 0)).all(), (name, k)
        assert (m[k] >= np.abs(t[k]) * (1 - 1e-12)).all(), (name, k)      # the magnitude dominates the number it stands beside
    if min(c["shape"][1:]) >= 3:
        assert np.abs(t["d_invdepth"]).max() > 1e-2 and np.abs(t["out"]).max() > 1e-2


# ---- the per-Gaussian normal ----

def _rotation_matrix(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("P", GN_SIZES)
def test_gaussian_normals_restatement(P):
    c = gn_case(P)
    t = NR.gaussian_normals(*gn_args(c))
    f = NR.gaussian_normals(*gn_args(c), mode=np.float32)
    m = NR.gaussian_normals(*gn_args(c), mode="mag")
    live = t["live"]
    assert np.abs(np.linalg.norm(t["normals"][live], axis=1) - 1).max() <= 1e-12
    toward = (t["normals"] * (c["campos"].astype(np.float64) - c["means3D"])).sum(1)
    assert (toward[live] >= 0).all() and (f["sign"] == t["sign"]).all()
    for i in range(P):       # the shortest axis of the covariance R S^2 R^T the rasterizer builds
        if live[i]:
            col = _rotation_matrix(c["rotations"][i].astype(np.float64))[:, t["k"][i]]
            assert np.abs(t["normals"][i] - t["sign"][i] * col).max() <= 1e-12, i
    if P > 10:
        assert not live[5] and not t["normals"][5].any() and not t["d_rotations"][5].any() and not f["d_rotations"][5].any()
        if P > 100:
            dead = [5, 11, 12, 13, 14]
            assert not live[dead].any() and live.sum() == P - 5
            assert all(not x[k][dead].any() for x in (t, f) for k in ("normals", "d_rotations"))
        assert tuple(t["k"][7:10]) == (0, 1, 0) and (t["sign"] > 0).any() and (t["sign"] < 0).any()
        s = c["scales"]
        assert (t["k"] == NR.shortest_axis(np.log(s))).all()          # a monotone map of the scales: the same axis
        cov = _rotation_matrix(c["rotations"][0].astype(np.float64)) @ np.diag(s[0].astype(np.float64) ** 2)
        cov = cov @ _rotation_matrix(c["rotations"][0].astype(np.float64)).T
        vals, vecs = np.linalg.eigh(cov)
        assert abs(abs(vecs[:, 0] @ t["normals"][0]) - 1) <= 1e-9
    need = {k: NR.needed(f[k], t[k], m[k]) for k in ("normals", "d_rotations")}
    assert all(v <= 1.0 for v in need.values()), (P, need)
    # the gradient is orthogonal to q (the normal does not depend on |q|)
    assert np.abs((t["d_rotations"][live] * c["rotations"][live]).sum(1)).max() <= 1e-9 * max(1.0, np.abs(t["d_rotations"]).max())


def test_gaussian_normals_gradient_against_finite_differences():
    c = gn_case(63)
    q = c["rotations"].astype(np.float64)
    g = c["g"].astype(np.float64)
    t = NR.gaussian_normals(*gn_args(c))

    def value(qq):       # float64 rotations: the plain definition, with k and the sign of the base point
        out = 0.0
        for i in range(qq.shape[0]):
            if t["live"][i]:
                out += t["sign"][i] * _rotation_matrix(qq[i])[:, t["k"][i]] @ g[i]
        return out

    eps = 1e-6
    fd = np.zeros_like(q)
    for idx in np.ndindex(*q.shape):
        if not t["live"][idx[0]]:
            continue
        hi, lo = q.copy(), q.copy()
        hi[idx] += eps
        lo[idx] -= eps
        fd[idx] = (value(hi) - value(lo)) / (2 * eps)
    scale = np.abs(t["d_rotations"]).max()
    assert scale > 0.1 and np.abs(fd - t["d_rotations"]).max() <= 1e-7 * scale


# ---- C ABI ----

@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


def test_the_header_declares_exactly_the_exports(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hdrsplat.h")).read(), flags=re.S)
    declared = re.findall(r"\bHS_API\s+(?:const\s+)?\w+\s*\*?\s*(hs_\w+)\s*\(", header)
    assert sorted(declared) == sorted(lib.EXPORTS) and len(set(declared)) == len(declared)
    assert set(NAMES) <= set(declared)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == lib.HS_VERSION == 309       # (detected by name: the version does not move)
    import casualhdrsplat_amd as pkg
    assert {"normal_consistency_loss", "gaussian_normals"} <= set(pkg.__all__)


@pytest.mark.parametrize("name", ("hs_normal_consistency_args", "hs_gaussian_normals_args"))
def test_structs_match_c(lib, tmp_path, name):
    S_ = getattr(lib, name)
    fields = [n for n, _ in S_._fields_]
    lines = [f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {n}));' for n in fields]
    want = [C.sizeof(S_)] + [getattr(S_, n).offset for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want


def test_the_calls_validate_before_touching_the_gpu(lib):
    L = lib.load()
    one = 4096
    ws = L.hs_normal_consistency_workspace_bytes
    assert ws(1, 1080, 1920) == 0 and ws(2, 1, 1) == 0
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1 << 10, 1 << 10, 1 << 10)):
        assert ws(*bad) == lib.HS_EINVAL and L.hs_last_error().startswith(b"hs_normal_consistency_workspace_bytes:"), bad

    def nc(which, **kw):
        a = lib.hs_normal_consistency_args()
        a.B, a.H, a.W, a.fx, a.fy = 2, 16, 24, 20.0, 21.0
        for k in ("invdepth", "alpha", "normals", "weight", "cam_to_world", "out", "depth_normals", "dL_dout", "dL_dnormals",
                  "dL_dinvdepth", "dL_dalpha"):
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, which)(C.byref(a), None), L.hs_last_error()

    for which, pointers, required in (
            ("hs_normal_consistency", ("invdepth", "alpha", "normals", "weight", "cam_to_world", "out", "depth_normals"),
             ("invdepth", "normals")),
            ("hs_normal_consistency_backward", ("invdepth", "alpha", "normals", "weight", "cam_to_world", "dL_dout", "dL_dnormals",
                                                "dL_dinvdepth", "dL_dalpha"), ("invdepth", "normals", "dL_dout"))):
        assert getattr(L, which)(None, None) == lib.HS_EINVAL and L.hs_last_error() == which.encode() + b": null args"
        for k in pointers:
            rc, msg = nc(which, **{k: one + 2})
            assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and k.encode() + b" must be 4-byte aligned" in msg, (k, msg)
        for k in required:
            rc, msg = nc(which, **{k: None})
            assert rc == lib.HS_EINVAL and b"null " + k.encode() in msg, (k, msg)
        for bad in (dict(B=0), dict(H=0), dict(W=-3), dict(B=1 << 12, H=1 << 10, W=1 << 10), dict(fx=0.0), dict(fy=float("nan")),
                    dict(fx=float("inf"))):
            rc, msg = nc(which, **bad)
            assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":"), (bad, msg)
    rc, msg = nc("hs_normal_consistency", out=None, depth_normals=None)
    assert rc == lib.HS_EINVAL and b"nothing to write" in msg
    rc, msg = nc("hs_normal_consistency_backward", alpha=None)
    assert rc == lib.HS_EINVAL and b"dL_dalpha without alpha" in msg
    # nothing asked for: a successful no-op
    assert nc("hs_normal_consistency_backward", dL_dnormals=None, dL_dinvdepth=None, dL_dalpha=None)[0] == lib.HS_OK

    def gn(which, **kw):
        a = lib.hs_gaussian_normals_args()
        a.P = 100
        for k in ("rotations", "scales", "means3D", "campos", "normals", "dL_dnormals", "dL_drotations"):
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, which)(C.byref(a), None), L.hs_last_error()

    for which, pointers in (("hs_gaussian_normals", ("rotations", "scales", "means3D", "campos", "normals")),
                            ("hs_gaussian_normals_backward", ("rotations", "scales", "means3D", "campos", "dL_dnormals", "dL_drotations"))):
        assert getattr(L, which)(None, None) == lib.HS_EINVAL and L.hs_last_error() == which.encode() + b": null args"
        for k in pointers:
            rc, msg = gn(which, **{k: None})
            assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and b"null " + k.encode() in msg, (k, msg)
            wide = k in ("rotations", "dL_drotations")
            rc, msg = gn(which, **{k: one + (4 if wide else 2)})
            assert rc == lib.HS_EINVAL and k.encode() + (b" must be 16-byte aligned" if wide else b" must be 4-byte aligned") in msg, (k, msg)
        for bad in (-1, 1 << 30):
            rc, msg = gn(which, P=bad)
            assert rc == lib.HS_EINVAL and b"P=" in msg
        assert gn(which, P=0, **{k: None for k in pointers})[0] == lib.HS_OK      # no rows: a no-op that looks at no pointer


# ---- Python ----

def test_python_refusals():
    import inspect
    import casualhdrsplat_amd as pkg
    ncl, gnm = pkg.normal_consistency_loss, pkg.gaussian_normals
    assert ncl is NM.normal_consistency_loss and gnm is NM.gaussian_normals
    assert list(inspect.signature(ncl).parameters) == ["invdepth", "normals", "fx", "fy", "alpha", "weight", "cam_to_world",
                                                       "return_depth_normals"]
    assert list(inspect.signature(gnm).parameters) == ["rotations", "scales", "means3D", "campos"]
    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")     # a device that is not the CPU
    d, N = torch.zeros(4, 5), torch.zeros(3, 4, 5)
    with pytest.raises(RuntimeError, match=r"normal_consistency_loss on an MI355X only: invdepth .*\(no CPU fallback\)"):
        ncl(d, N, 5.0, 5.0)
    with pytest.raises(TypeError, match="invdepth must be a torch.Tensor"):
        ncl(np.zeros((4, 5), np.float32), N, 5.0, 5.0)
    with pytest.raises(TypeError, match="invdepth must be float32"):
        ncl(d.double(), N, 5.0, 5.0)
    with pytest.raises(ValueError, match=r"invdepth must be \[H, W\] or \[B, H, W\]"):
        ncl(torch.zeros(5), N, 5.0, 5.0)
    with pytest.raises(ValueError, match=r"invdepth must be \[H, W\] or \[B, H, W\]"):
        ncl(torch.zeros(1, 1, 4, 5), N, 5.0, 5.0)
    md, mN = meta(2, 4, 5), meta(2, 3, 4, 5)
    with pytest.raises(TypeError, match="normals must be float32"):
        ncl(md, meta(2, 3, 4, 5, dtype=torch.float16), 5.0, 5.0)
    with pytest.raises(ValueError, match=r"normals must be \[2, 3, 4, 5\]"):
        ncl(md, meta(3, 4, 5), 5.0, 5.0)
    with pytest.raises(ValueError, match=r"alpha must be \[2, 4, 5\]"):
        ncl(md, mN, 5.0, 5.0, alpha=meta(2, 4, 6))
    with pytest.raises(ValueError, match=r"weight must be \[2, 4, 5\]"):
        ncl(md, mN, 5.0, 5.0, weight=meta(4, 5))
    with pytest.raises(ValueError, match="invdepth and normals live on different devices"):
        ncl(md, torch.zeros(2, 3, 4, 5), 5.0, 5.0)
    with pytest.raises(ValueError, match="invdepth and alpha live on different devices"):
        ncl(md, mN, 5.0, 5.0, alpha=torch.zeros(2, 4, 5))
    with pytest.raises(TypeError, match="fx must be a Python float"):
        ncl(md, mN, torch.tensor(5.0), 5.0)
    with pytest.raises(ValueError, match="fy=0.0 must be finite and positive"):
        ncl(md, mN, 5.0, 0.0)
    with pytest.raises(ValueError, match=r"cam_to_world must be \[3, 3\] or \[2, 3, 3\]"):
        ncl(md, mN, 5.0, 5.0, cam_to_world=meta(4, 4))
    with pytest.raises(TypeError, match="cam_to_world must be float32"):
        ncl(md, mN, 5.0, 5.0, cam_to_world=meta(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="invdepth and cam_to_world live on different devices"):
        ncl(md, mN, 5.0, 5.0, cam_to_world=torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match=r"\(no CPU fallback\)"):      # everything consistent, and not on the GPU
        ncl(md, mN, 5.0, 5.0, alpha=md, weight=md, cam_to_world=meta(3, 3))
    q, s, m, cp = torch.zeros(6, 4), torch.zeros(6, 3), torch.zeros(6, 3), torch.zeros(3)
    with pytest.raises(RuntimeError, match=r"gaussian_normals on an MI355X only: rotations .*\(no CPU fallback\)"):
        gnm(q, s, m, cp)
    with pytest.raises(TypeError, match="scales must be a torch.Tensor"):
        gnm(q, None, m, cp)
    with pytest.raises(TypeError, match="means3D must be float32"):
        gnm(q, s, m.double(), cp)
    with pytest.raises(ValueError, match=r"rotations must be \[P, 4\]"):
        gnm(torch.zeros(6, 3), s, m, cp)
    with pytest.raises(ValueError, match=r"scales must be \[6, 3\]"):
        gnm(q, torch.zeros(5, 3), m, cp)
    with pytest.raises(ValueError, match="campos must hold 3 floats"):
        gnm(q, s, m, torch.zeros(4))
    with pytest.raises(ValueError, match="rotations and means3D live on different devices"):
        gnm(meta(6, 4), meta(6, 3), torch.zeros(6, 3), meta(3))
