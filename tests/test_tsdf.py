"""CPU checks of the TSDF fusion and the mesh extraction (tsdf.hip: hs_tsdf_integrate, hs_tsdf_mesh_plan, hs_tsdf_mesh_emit;
tsdf.TSDFVolume, scene_io.save_mesh_ply): the restatement the GPU tests compare with (tests/tsdf_reference.py) against closed
forms -- a fronto-parallel plane, an analytic sphere, a partly observed volume --, the cases of the GPU tests and proof that
they exercise every branch of the walk, the C ABI (exports, struct layout, validation before any HIP call), the Python
refusals and the PLY round trip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tsdf_reference as TR
from casualhdrsplat_amd import scene_io
from casualhdrsplat_amd import synthetic as S
from casualhdrsplat_amd import tsdf as T      # (the module under test: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_tsdf_integrate", "hs_tsdf_mesh_workspace_bytes", "hs_tsdf_mesh_plan", "hs_tsdf_mesh_emit")
f32 = np.float32
U = 2.0 ** -24           # unit roundoff of fp32

# ---- the cases of the GPU tests (shared with tests/test_tsdf_gpu.py; every reference is computed once) ----
# The integration's brick is 32 x 8 x 4 samples: 37 x 21 x 19 is a multiple in no direction and spans 2 x 3 x 5 workgroups.
DIMS, H_VOX, ORIGIN = (37, 21, 19), 0.11, (-2.0, -1.15, -1.0)
FRAMES, HW, SEEDS = 3, (31, 45), (3, 5, 12)
MIN_ALPHA, MAX_DEPTH = 0.5, 3.0
_CACHE = {}


def frames_case():
    """dict(invdepth, alpha, color [F, ...], views [F, 4, 4], fx, fy): three free 6-DoF cameras around a volume they partly see,
    smooth depth maps that cut through it, and every kind of pixel the walk refuses."""
    if "frames" in _CACHE:
        return _CACHE["frames"]
    Hh, Ww = HW
    rng = np.random.default_rng(20)
    cams = [S.random_camera(Ww, Hh, seed) for seed in SEEDS]
    views = np.stack([c.viewmatrix.numpy() for c in cams]).astype(f32)
    fx, fy = Ww / (2 * cams[0].tanfovx), Hh / (2 * cams[0].tanfovy)
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    depth = np.stack([2.2 + 1.2 * np.sin(4.0 * xx / Ww + f) * np.cos(3.0 * yy / Hh - f) for f in range(FRAMES)])   # 1.0 .. 3.4
    alpha = (0.55 + 0.45 * rng.random(depth.shape)).astype(f32)
    alpha[0, 3:6, 10:20] = 0.3                                   # below min_alpha
    alpha[1, 20, 7] = 0.0
    alpha[2, 8, 8] = np.nan
    invdepth = (alpha / depth).astype(f32)
    invdepth[0, 12, 30:36] = 0.0
    invdepth[1, 5:9, 5:9] = -0.4
    invdepth[1, 15, 20:24] = np.nan
    invdepth[2, 25:28, 11:14] = np.inf
    invdepth[2, 2, 40] = -np.inf
    color = rng.random((FRAMES, 3, Hh, Ww)).astype(f32)
    _CACHE["frames"] = dict(invdepth=invdepth, alpha=alpha, color=color, views=views, fx=float(fx), fy=float(fy))
    return _CACHE["frames"]


def integrated(color, f_begin=0, f_end=FRAMES, start=None, stats=None):
    """the restatement's volume after frames f_begin .. f_end of frames_case(), from `start` (None: an empty volume)"""
    key = ("integrated", color, f_begin, f_end, id(start) if start is not None else None)
    if key in _CACHE and stats is None:
        return _CACHE[key]
    c = frames_case()
    vol = TR.empty_volume(DIMS, color) if start is None else start
    sl = slice(f_begin, f_end)
    out = TR.integrate(vol, ORIGIN, H_VOX, 4 * f32(H_VOX), c["invdepth"][sl], c["views"][sl], c["fx"], c["fy"], alpha=c["alpha"][sl],
                       color=c["color"][sl] if color else None, min_alpha=MIN_ALPHA, max_depth=MAX_DEPTH, stats=stats)
    if start is None:
        _CACHE[key] = out
    return out


def sphere_volume(n, color=False, h=0.125, r_cells=7.3):
    """(vol, origin, h, centre, r): clamp((|p - c| - r) / trunc, -1, 1) on an n^3 lattice, weight 1, the sphere strictly inside"""
    key = ("sphere", n, color, h, r_cells)
    if key not in _CACHE:
        origin = (0.3, -1.7, 2.1)
        ax = [TR.lattice(o, h, n).astype(np.float64) for o in origin]
        c = np.array([a[0] + (0.5 * (n - 1) + d) * h for a, d in zip(ax, (0.13, -0.21, 0.37))])
        r = r_cells * h
        dist = np.sqrt((ax[0][None, None, :] - c[0]) ** 2 + (ax[1][None, :, None] - c[1]) ** 2 + (ax[2][:, None, None] - c[2]) ** 2)
        vol = dict(tsdf=np.clip((dist - r) / (4 * h), -1, 1).astype(f32), weight=np.ones((n, n, n), f32), color=None)
        if color:
            rng = np.random.default_rng(n)
            vol["color"] = rng.random((3, n, n, n)).astype(f32)
        _CACHE[key] = (vol, origin, h, c, r)
    return _CACHE[key]


def plane_volume(dims):
    """a plane z = const through otherwise free space, every sample observed: one sheet of vertices and faces"""
    nx, ny, nz = dims
    vol = TR.empty_volume(dims)
    vol["weight"][:] = 1
    k = np.arange(nz, dtype=np.float64)
    vol["tsdf"][:] = np.clip((0.3 * nz + 0.37 - k) / 4.0, -1, 1).astype(f32)[:, None, None]
    return vol


def mesh_of(key, vol, origin, h, min_weight=1.0):
    if ("mesh", key) not in _CACHE:
        _CACHE[("mesh", key)] = TR.extract_mesh(vol, origin, h, min_weight)
    return _CACHE[("mesh", key)]


# ---- the restatement against closed forms ----

def _topology(vertices, faces):
    """(E, edges in exactly two faces and once in each direction, referenced vertices)"""
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    und = np.sort(d, 1)
    _, counts = np.unique(und, axis=0, return_counts=True)
    directed = np.unique(d, axis=0)
    return counts.size, bool((counts == 2).all() and directed.shape[0] == d.shape[0]), np.unique(faces)


def test_a_plane_seen_by_translated_cameras():
    """F cameras with one orientation, translated, look at the plane z = 4 (their depth maps are constant).  With a lattice,
    a truncation and depths that are dyadic, every operation of the walk is exact: an observed sample holds
    min(1, (z_plane - z) / trunc) EXACTLY after any number of frames, and weight counts the frames that saw it.
    Mesh vertices.  pa and pb are within 2 U |p| of the lattice each (product and sum), pb - pa within 4 U |p| + U h of the
    edge, s = a / (a - b) within 3 U of the exact ratio of the stored values, the product within U h and the last sum within
    U |p|: |z - z_plane| <= 7 U |p| + 5 U h <= 8 U max|coordinate| (h < |p| / 5 here)."""
    dims, h, origin, zp = (12, 10, 16), 0.125, (-0.7, -0.6, 3.03125), 4.0
    Hh, Ww, fx = 24, 32, 20.0
    shifts = [(0.0, 0.0, 0.0), (0.3, -0.2, 2.0), (-0.25, 0.1, -4.0), (3.0, 0.0, 0.0), (0.1, 0.1, 0.0)]
    pz = TR.lattice(origin[2], h, dims[2])
    for F in (1, 2, 5):
        views = np.stack([np.eye(4, dtype=f32) for _ in range(F)])
        invd = np.empty((F, Hh, Ww), f32)
        for f, (tx, ty, tz) in enumerate(shifts[:F]):
            views[f][3, :3] = (-tx, -ty, -tz)                     # transposed convention: the translation is the last ROW
            invd[f] = 1.0 / (zp - tz)                             # 1/4, 1/2, 1/8: exact, and 1 / them too
        vol = TR.integrate(TR.empty_volume(dims), origin, h, 4 * h, invd, views, fx, fx)
        seen = vol["weight"] > 0
        want = np.minimum(f32(1), (f32(zp) - pz) / f32(4 * h))[:, None, None]
        assert (vol["tsdf"][seen] == np.broadcast_to(want, seen.shape)[seen]).all(), F
        assert (vol["tsdf"][~seen] == 1).all() and min(F, 3) <= vol["weight"].max() <= F
        assert not seen[pz > zp + 4 * h].any() and seen[pz <= zp + 4 * h].any(axis=(1, 2)).all()
        if F == 5:
            assert len(np.unique(vol["weight"])) > 3              # camera 3 sees a part only
        v, faces, _, info = TR.extract_mesh(vol, origin, h)
        assert info["T"] > 0 and info["V"] == v.shape[0]
        bound = 8 * U * max(abs(o) + h * n for o, n in zip(origin, dims))
        assert np.abs(v[:, 2].astype(np.float64) - zp).max() <= bound
        tri = v[faces.astype(np.int64)].astype(np.float64)
        normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert (normal[:, 2] < 0).all()                           # free space is towards the cameras: -z


def test_two_calls_are_one_call_in_the_restatement():
    whole = integrated(True)
    parts = integrated(True, 1, 3, start=integrated(True, 0, 1))
    for k in ("tsdf", "weight", "color"):
        assert whole[k].tobytes() == parts[k].tobytes(), k


def test_the_gpu_case_exercises_every_branch():
    stats = {}
    vol = integrated(True, stats=stats)
    print("tsdf frames case:", stats)
    assert all(stats[k] > 50 for k in ("behind", "outside", "invalid", "far", "occluded", "clamped", "fused")), stats
    c = frames_case()
    d = c["invdepth"]
    assert (d == 0).any() and (d < 0).any() and np.isnan(d).any() and np.isposinf(d).any() and (c["alpha"] < MIN_ALPHA).any()
    w = vol["weight"]
    assert (w == 0).any() and (w == 1).any() and (w >= 2).any() and (vol["tsdf"] < 0).any() and (vol["tsdf"][w > 0] == 1).any()
    assert np.isfinite(vol["tsdf"]).all() and np.isfinite(vol["color"]).all()
    # without the refused pixels the result differs: they matter to this volume
    v, f, col, info = mesh_of("frames", vol, ORIGIN, H_VOX)
    assert info["T"] > 500 and col.shape == v.shape and f.max() < v.shape[0]


@pytest.mark.parametrize("n", (17, 33))
def test_an_analytic_sphere_gives_a_closed_oriented_mesh(n):
    """clamp((|p - c| - r) / trunc, -1, 1) with r >= 6 h (trunc = 4 h clips no crossing edge: its ends are within sqrt(3) h of
    the surface).  The mesh is a closed 2-manifold of genus 0, oriented outwards, every vertex is referenced, and every vertex
    radius is within the sag of a chord of length <= sqrt(3) h, 3 h^2 / (8 r), of r -- plus the rounding of the stored values
    (U trunc each, through a / (a - b) with |a - b| >= the edge's projection) and of the interpolation (8 U |p|): 1e-5 h covers
    both by orders of magnitude."""
    vol, origin, h, c, r = sphere_volume(n, r_cells=7.3 if n == 33 else 6.2)
    v, faces, _, info = mesh_of(("sphere", n), vol, origin, h)
    V, Tn = v.shape[0], faces.shape[0]
    assert (info["V"], info["T"]) == (V, Tn) and Tn > 1000
    E, manifold, used = _topology(v, faces)
    assert manifold and V - E + Tn == 2 and used.size == V
    tri = v[faces.astype(np.int64)].astype(np.float64)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((normal * (tri.mean(1) - c)).sum(1) > 0).all()
    radius = np.linalg.norm(v.astype(np.float64) - c, axis=1)
    assert np.abs(radius - r).max() <= 3 * h * h / (8 * r) + 1e-5 * h, (np.abs(radius - r).max(), 3 * h * h / (8 * r))


def test_unobserved_samples_cut_the_mesh_at_whole_tetrahedra():
    vol, origin, h, c, r = sphere_volume(17, color=True, r_cells=6.2)
    vol = dict(vol, weight=vol["weight"].copy())
    vol["weight"][:, :, :7] = 0.5                                  # below min_weight = 1
    vol["weight"][9:, 5, 8:] = 0.0
    vol["weight"][3, 3, 12] = np.nan
    v, faces, col, info = TR.extract_mesh(vol, origin, h, 1.0)
    full = mesh_of(("sphere", 17), sphere_volume(17, r_cells=6.2)[0], origin, h)
    assert 0 < faces.shape[0] < full[1].shape[0] and faces.min() >= 0 and faces.max() < v.shape[0] and col.shape == v.shape
    obs = (vol["weight"] >= 1).reshape(-1)
    nx = 17
    offset = np.array([(k & 1) + ((k >> 1) & 1) * nx + (k >> 2) * nx * nx for k in range(8)])
    cell, tet = info["cell_q"][info["face_cell_tet"] // 6], info["face_cell_tet"] % 6
    assert obs[cell[:, None] + offset[TR.TET_CORNER[tet]]].all()
    # ... and every fully observed tetrahedron the surface crosses is there: the count of the restatement equals a direct one
    ins = (vol["tsdf"] < 0).reshape(-1)
    direct = 0
    for q in info["cell_q"]:
        for t in range(6):
            corners = q + offset[TR.TET_CORNER[t]]
            if obs[corners].all():
                direct += (0, 1, 2, 1, 0)[int(ins[corners].sum())]
    assert direct == faces.shape[0]
    # the rim: vertices whose faces went with the unobserved samples stay, unreferenced
    assert np.unique(faces).size < v.shape[0] == info["V"]
    # lowering the threshold brings the first slab back
    v2, f2, _, _ = TR.extract_mesh(vol, origin, h, 0.5)
    assert f2.shape[0] > faces.shape[0]


def test_an_empty_or_all_outside_volume_has_no_mesh():
    vol = TR.empty_volume((5, 4, 3), color=True)
    for w in (0.0, 1.0):
        vol["weight"][:] = w
        v, f, col, info = TR.extract_mesh(vol, (0, 0, 0), 0.1)
        assert v.shape == (0, 3) and f.shape == (0, 3) and col.shape == (0, 3) and info["T"] == 0 and f.dtype == np.int32
    # a value of exactly 0 counts as outside; next to a negative one it puts the vertex ON the sample: zero-area faces stay
    vol["tsdf"][:] = 1
    vol["tsdf"][1, 1, 1] = -0.5
    vol["tsdf"][1, 2, 2] = -0.5                                   # two inside neighbours of the zero in one tetrahedron:
    vol["tsdf"][1, 1, 2] = 0.0                                    # both of its vertices fall on the zero sample
    v, f, _, info = TR.extract_mesh(vol, (0, 0, 0), 0.1)
    tri = v[f.astype(np.int64)].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert info["T"] > 0 and (area == 0).any() and _topology(v, f)[1]


# ---- mesh files ----

def test_mesh_ply_round_trip(tmp_path):
    vol, origin, h, c, r = sphere_volume(17, r_cells=6.2)
    v, f, _, _ = mesh_of(("sphere", 17), vol, origin, h)
    col = np.random.default_rng(0).uniform(-0.2, 1.2, v.shape).astype(f32)
    col[0] = (np.nan, 0.5, 1.0)
    path = str(tmp_path / "m.ply")
    scene_io.save_mesh_ply(path, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(col))
    head = open(path, "rb").read(400)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % v.shape[0])
    assert b"property uchar red\n" in head and b"element face %d\nproperty list uchar int vertex_indices\nend_header\n" % f.shape[0] in head
    v2, f2, c2 = scene_io.load_mesh_ply(path)
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes() and c2.dtype == np.uint8
    want = np.floor(np.clip(np.nan_to_num(col.astype(np.float64)), 0, 1) * 255 + 0.5).astype(np.uint8)
    assert (c2 == want).all() and c2.min() == 0 and c2.max() == 255 and tuple(c2[0]) == (0, 128, 255)
    scene_io.save_mesh_ply(path, v, f)
    v3, f3, c3 = scene_io.load_mesh_ply(path)
    assert c3 is None and v3.tobytes() == v.tobytes() and f3.tobytes() == f.tobytes()
    scene_io.save_mesh_ply(path, np.zeros((0, 3), f32), np.zeros((0, 3), np.int32))
    assert [x.shape for x in scene_io.load_mesh_ply(path)[:2]] == [(0, 3), (0, 3)]
    with pytest.raises(ValueError, match="a face index outside the 3 vertices"):
        scene_io.save_mesh_ply(path, np.zeros((3, 3), f32), np.array([[0, 1, 3]]))
    with pytest.raises(ValueError, match=r"colors must be \[3, 3\]"):
        scene_io.save_mesh_ply(path, np.zeros((3, 3), f32), np.array([[0, 1, 2]]), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="not a mesh PLY"):
        scene_io.save_ply(path, scene_io.GaussianCloud(torch.zeros(1, 3), torch.zeros(1, 1, 3), torch.zeros(1), torch.zeros(1, 3),
                                                       torch.zeros(1, 4)))
        scene_io.load_mesh_ply(path)


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
    assert pkg.TSDFVolume is T.TSDFVolume and "TSDFVolume" in pkg.__all__


def test_the_build_knows_the_unit():
    mk = open(os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\btsdf\.o\b", mk, flags=re.M) and not re.search(r"^FAST_TUS\s*=.*\btsdf\b", mk, flags=re.M)
    assert "tsdf_host" in re.search(r"^ASAN_DRIVERS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    src = open(os.path.join(ROOT, "tests", "native", "tsdf_host.cpp")).read()
    assert "int main()" in src and all(n in src for n in NAMES)


def test_struct_matches_c(lib, tmp_path):
    name, S_ = "hs_tsdf_args", lib.hs_tsdf_args
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
    ws = L.hs_tsdf_mesh_workspace_bytes
    assert ws(37, 21, 19) == (4 * 14763 + 15) // 16 * 16 + 16 * 58 + (14763 + 15) // 16 * 16
    assert ws(1024, 1024, 1024) > 5 << 30
    for bad in ((1, 8, 8), (8, 0, 8), (8, 8, -1), (1025, 1024, 1024), (1 << 16, 1 << 16, 2)):
        assert ws(*bad) == lib.HS_EINVAL and L.hs_last_error().startswith(b"hs_tsdf_mesh_workspace_bytes:"), bad

    pointers = ("tsdf", "weight", "color", "invdepth", "alpha", "frame_color", "viewmatrices", "workspace", "totals", "vertices",
                "faces", "colors")

    def call(which, **kw):
        a = lib.hs_tsdf_args()
        a.nx, a.ny, a.nz, a.F, a.H, a.W = 37, 21, 19, 3, 31, 45
        a.origin = (C.c_float * 3)(-2.0, -1.0, 0.5)
        a.voxel_size, a.trunc, a.fx, a.fy, a.min_alpha, a.max_depth, a.min_weight = 0.1, 0.4, 20.0, 21.0, 0.5, float("inf"), 1.0
        a.n_vertices, a.n_faces = 10, 20
        for k in pointers:
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, (C.c_float * 3)(*v) if k == "origin" else v)
        return getattr(L, which)(C.byref(a), None), L.hs_last_error()

    used = {"hs_tsdf_integrate": (("tsdf", "weight", "invdepth", "viewmatrices"), ("color", "alpha", "frame_color")),
            "hs_tsdf_mesh_plan": (("tsdf", "weight", "workspace", "totals"), ()),
            "hs_tsdf_mesh_emit": (("tsdf", "weight", "workspace", "vertices", "faces"), ("color", "colors"))}
    for which, (required, optional) in used.items():
        assert getattr(L, which)(None, None) == lib.HS_EINVAL and L.hs_last_error() == which.encode() + b": null args"
        for k in required:
            rc, msg = call(which, **{k: None})
            assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and b"null " + k.encode() in msg, (which, k, msg)
        for k in required + optional:
            align = {"workspace": 16, "totals": 8}.get(k, 4)
            rc, msg = call(which, **{k: one + align // 2})
            assert rc == lib.HS_EINVAL and k.encode() + b" must be %d-byte aligned" % align in msg, (which, k, msg)
        for bad in (dict(nx=1), dict(ny=0), dict(nz=-4), dict(nx=1 << 11, ny=1 << 10, nz=1 << 10), dict(nx=1 << 20, ny=1 << 20),
                    dict(voxel_size=0.0), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")), dict(voxel_size=-1.0),
                    dict(origin=(0.0, float("nan"), 0.0)), dict(origin=(float("inf"), 0.0, 0.0))):
            rc, msg = call(which, **bad)
            assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":"), (which, bad, msg)
        assert call(which, nx=1 << 10, ny=1 << 10, nz=1 << 10, **{required[-1]: None})[1].find(b"null " + required[-1].encode()) > 0

    which = "hs_tsdf_integrate"
    for bad, text in ((dict(F=0), b"F=0"), (dict(H=0), b"H=0"), (dict(W=-1), b"W=-1"), (dict(F=1 << 10, H=1 << 10, W=1 << 10), b"2^31"),
                      (dict(F=1, H=1, W=65537), b"W=65537"), (dict(F=1, H=65537, W=1), b"H=65537"),
                      (dict(fx=0.0), b"fx=0"), (dict(fy=float("nan")), b"fy=nan"), (dict(fx=float("inf")), b"fx=inf"),
                      (dict(trunc=0.0), b"trunc=0"), (dict(trunc=float("inf")), b"trunc=inf"), (dict(trunc=-0.1), b"trunc=-0.1"),
                      (dict(min_alpha=float("nan")), b"min_alpha"), (dict(max_depth=0.0), b"max_depth=0"),
                      (dict(max_depth=float("nan")), b"max_depth=nan"), (dict(max_depth=-2.0), b"max_depth=-2"),
                      (dict(color=None), b"frame_color given for a volume without colour"),
                      (dict(frame_color=None), b"the volume has colour")):
        rc, msg = call(which, **bad)
        assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and text in msg, (bad, msg)
    for which in ("hs_tsdf_mesh_plan", "hs_tsdf_mesh_emit"):
        rc, msg = call(which, min_weight=float("nan"))
        assert rc == lib.HS_EINVAL and b"min_weight" in msg
    which = "hs_tsdf_mesh_emit"
    for bad, text in ((dict(n_vertices=-1), b"n_vertices=-1"), (dict(n_faces=1 << 31), b"n_faces=2147483648"),
                      (dict(n_vertices=1 << 31), b"n_vertices=2147483648"),
                      (dict(color=None), b"colors given for a volume without colour"), (dict(colors=None), b"the volume has colour")):
        rc, msg = call(which, **bad)
        assert rc == lib.HS_EINVAL and text in msg, (bad, msg)
    # an empty mesh: a successful no-op that needs no output
    assert call(which, n_vertices=0, n_faces=0, vertices=None, faces=None)[0] == lib.HS_OK
    assert call(which, n_vertices=0, n_faces=0, vertices=None, faces=None, color=None, colors=None)[0] == lib.HS_OK


# ---- Python ----

def test_python_refusals():
    import inspect
    V = T.TSDFVolume
    assert list(inspect.signature(V.__init__).parameters)[1:] == ["origin", "voxel_size", "dims", "trunc", "color", "device"]
    assert list(inspect.signature(V.integrate).parameters)[1:] == ["invdepth", "viewmatrices", "fx", "fy", "alpha", "color",
                                                                    "min_alpha", "max_depth"]
    assert inspect.signature(V.integrate).parameters["min_alpha"].default == 0.5
    assert inspect.signature(V.integrate).parameters["max_depth"].default == float("inf")
    assert inspect.signature(V.extract_mesh).parameters["min_weight"].default == 1.0
    o = (0.0, 0.0, 0.0)
    with pytest.raises(RuntimeError, match=r"a TSDFVolume on an MI355X only: .*\(no CPU fallback\)"):
        V(o, 0.1, (4, 4, 4), device="cpu")
    with pytest.raises(ValueError, match="dims=.* must be at least 2 each"):
        V(o, 0.1, (4, 1, 4))
    with pytest.raises(ValueError, match="more than 2\\^30 samples"):
        V(o, 0.1, (1025, 1024, 1024))
    with pytest.raises(TypeError, match="dims must be three integers"):
        V(o, 0.1, (4, 4))
    with pytest.raises(TypeError, match="dims must be three integers"):
        V(o, 0.1, (4, 4.5, 4))
    with pytest.raises(ValueError, match="voxel_size=0.0 must be finite and positive"):
        V(o, 0.0, (4, 4, 4))
    with pytest.raises(TypeError, match="voxel_size must be a Python float"):
        V(o, torch.tensor(0.1), (4, 4, 4))
    with pytest.raises(ValueError, match="trunc=-1.0 must be finite and positive"):
        V(o, 0.1, (4, 4, 4), trunc=-1.0)
    with pytest.raises(ValueError, match="origin must be three finite numbers"):
        V((0.0, float("nan"), 0.0), 0.1, (4, 4, 4))
    with pytest.raises(ValueError, match="hi=.* must be above lo="):
        V.from_bounds((0, 0, 0), (1, 0, 1), 0.1)
    with pytest.raises(RuntimeError, match=r"\(no CPU fallback\)"):
        V.from_bounds((0, 0, 0), (1, 1, 1), 0.1, device="cpu")

    def blank(color=False, dims=(6, 5, 4)):              # the host side of a volume, with tensors on a device that is not the CPU
        v = V.__new__(V)._configure((0.5, 0.25, -1.0), 0.1, dims, None, color)
        nx, ny, nz = dims
        v.tsdf, v.weight = torch.ones(nz, ny, nx, device="meta"), torch.zeros(nz, ny, nx, device="meta")
        v.color = torch.zeros(3, nz, ny, nx, device="meta") if color else None
        return v

    v = blank()
    assert v.trunc == 4 * v.voxel_size == 4 * float(f32(0.1)) and v.dims == (6, 5, 4) and v.origin == (0.5, 0.25, -1.0)
    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")
    d, vm = meta(2, 8, 9), meta(2, 4, 4)
    with pytest.raises(RuntimeError, match=r"TSDFVolume.integrate \(invdepth\) on an MI355X only: .*\(no CPU fallback\)"):
        v.integrate(torch.zeros(2, 8, 9), torch.zeros(2, 4, 4), 5.0, 5.0)
    with pytest.raises(TypeError, match="invdepth must be a torch.Tensor"):
        v.integrate(np.zeros((2, 8, 9), f32), vm, 5.0, 5.0)
    with pytest.raises(TypeError, match="invdepth must be float32"):
        v.integrate(meta(2, 8, 9, dtype=torch.float64), vm, 5.0, 5.0)
    with pytest.raises(ValueError, match=r"invdepth must be \[F, H, W\]"):
        v.integrate(meta(8, 9), vm, 5.0, 5.0)
    with pytest.raises(ValueError, match=r"invdepth must be \[F, H, W\]"):
        v.integrate(meta(0, 8, 9), meta(0, 4, 4), 5.0, 5.0)
    with pytest.raises(ValueError, match="2\\^31 / 3 pixels or more"):
        v.integrate(meta(1 << 10, 1 << 10, 1 << 10), vm, 5.0, 5.0)
    with pytest.raises(ValueError, match="frames of 65537 x 1 are outside H, W <= 65536"):
        v.integrate(meta(1, 1, 65537), meta(1, 4, 4), 5.0, 5.0)
    with pytest.raises(ValueError, match=r"viewmatrices must be \[2, 4, 4\]"):
        v.integrate(d, meta(4, 4), 5.0, 5.0)
    with pytest.raises(TypeError, match="viewmatrices must be float32"):
        v.integrate(d, meta(2, 4, 4, dtype=torch.float64), 5.0, 5.0)
    with pytest.raises(ValueError, match="invdepth and viewmatrices live on different devices"):
        v.integrate(d, torch.zeros(2, 4, 4), 5.0, 5.0)
    with pytest.raises(ValueError, match=r"alpha must be \[2, 8, 9\]"):
        v.integrate(d, vm, 5.0, 5.0, alpha=meta(2, 8, 8))
    with pytest.raises(ValueError, match="color given for a volume without colour"):
        v.integrate(d, vm, 5.0, 5.0, color=meta(2, 3, 8, 9))
    with pytest.raises(ValueError, match="the volume has colour: pass color"):
        blank(True).integrate(d, vm, 5.0, 5.0)
    with pytest.raises(ValueError, match=r"color must be \[2, 3, 8, 9\]"):
        blank(True).integrate(d, vm, 5.0, 5.0, color=meta(2, 8, 9, 3))
    with pytest.raises(TypeError, match="fx must be a Python float"):
        v.integrate(d, vm, torch.tensor(5.0), 5.0)
    with pytest.raises(ValueError, match="fy=0.0 must be finite and positive"):
        v.integrate(d, vm, 5.0, 0.0)
    with pytest.raises(ValueError, match="min_alpha=nan must be a number"):
        v.integrate(d, vm, 5.0, 5.0, min_alpha=float("nan"))
    with pytest.raises(ValueError, match="max_depth=0.0 must be > 0"):
        v.integrate(d, vm, 5.0, 5.0, max_depth=0.0)
    with pytest.raises(RuntimeError, match=r"\(no CPU fallback\)"):       # everything consistent, and not on the GPU
        blank(True).integrate(d, vm, 5.0, 5.0, alpha=d, color=meta(2, 3, 8, 9))
    with pytest.raises(ValueError, match="min_weight=nan must be a number"):
        v.extract_mesh(float("nan"))
    with pytest.raises(RuntimeError, match=r"TSDFVolume.extract_mesh \(the volume's tsdf\) on an MI355X only"):
        v.extract_mesh()
    v.weight = torch.zeros(4, 5, 7, device="meta")
    with pytest.raises(ValueError, match=r"the volume's weight must be a contiguous float32 tensor of shape \[4, 5, 6\]"):
        v.extract_mesh()
