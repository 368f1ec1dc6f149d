"""GPU checks of the TSDF fusion and the mesh extraction (tsdf.hip through tsdf.TSDFVolume and through the C ABI): every output
bit for bit against the numpy float32 restatement (tests/tsdf_reference.py, held to closed forms by tests/test_tsdf.py, whose
cases these are).  The restatement has no brick cull and no scan: equality shows that neither changes a bit or an order."""
import ctypes as C

import numpy as np
import pytest
import torch

import poison
import test_tsdf as TC
import tsdf_reference as TR
from casualhdrsplat_amd import _lib as L
from casualhdrsplat_amd.tsdf import TSDFVolume

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


def _gpu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _volume(dims, origin, h, ref=None, color=False):
    """a TSDFVolume on the GPU, filled from a restatement's volume dict when one is given"""
    vol = TSDFVolume(origin, h, dims, color=color, device=DEV)
    if ref is not None:
        vol.tsdf.copy_(_gpu(ref["tsdf"]))
        vol.weight.copy_(_gpu(ref["weight"]))
        if color:
            vol.color.copy_(_gpu(ref["color"]))
    return vol


def _same_volume(vol, ref, what):
    for k in ("tsdf", "weight", "color"):
        got = getattr(vol, k)
        if ref[k] is None:
            assert got is None
            continue
        a, b = got.cpu().numpy(), ref[k]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def _integrate(vol, c, sl, color):
    vol.integrate(_gpu(c["invdepth"][sl]), _gpu(c["views"][sl]), c["fx"], c["fy"], alpha=_gpu(c["alpha"][sl]),
                  color=_gpu(c["color"][sl]) if color else None, min_alpha=TC.MIN_ALPHA, max_depth=TC.MAX_DEPTH)


def _same_mesh(got, want, what):
    names = ("vertices", "faces", "colors")
    for n, g, w in zip(names, got, want[:3]):
        if w is None:
            continue
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, n, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, n, int((g != w).any(axis=1).sum()), int(np.argmax((g != w).any(axis=1))))


@pytest.mark.parametrize("color", (True, False))
def test_integrate_bit_for_bit(color):
    c = TC.frames_case()
    vol = _volume(TC.DIMS, TC.ORIGIN, TC.H_VOX, color=color)
    assert vol.trunc == float(4 * f32(TC.H_VOX)) and (vol.tsdf == 1).all() and (vol.weight == 0).all()
    _integrate(vol, c, slice(0, TC.FRAMES), color)
    _same_volume(vol, TC.integrated(color), "integrate")
    vol.reset()
    assert (vol.tsdf == 1).all() and (vol.weight == 0).all() and (not color or (vol.color == 0).all())


def test_two_calls_are_one_call():
    c = TC.frames_case()
    vol = _volume(TC.DIMS, TC.ORIGIN, TC.H_VOX, color=True)
    _integrate(vol, c, slice(0, 1), True)
    _same_volume(vol, TC.integrated(True, 0, 1), "frames 0 .. 1")
    _integrate(vol, c, slice(1, 3), True)
    _same_volume(vol, TC.integrated(True), "frames 0 .. 1 then 1 .. 3")


def test_the_brick_cull_changes_no_bit():
    """A volume of 3 x 5 x 6 bricks around two cameras that see a part of it each: whole bricks are behind a camera, whole bricks
    project outside its frame, others are cut by the frame's border or by the camera plane -- and 70 frames (more than a
    wave has lanes: two rounds of the cull's ballot), most of them copies, give the restatement's bits."""
    dims, h, origin = (70, 37, 22), 0.1, (-3.5, -1.8, -1.1)
    c = TC.frames_case()
    Hh, Ww = TC.HW
    order = [0, 1] * 3 + [2] + [1] * 63
    full = dead = cut = 0
    for f in (0, 1):
        m = TR.projects_inside(dims, origin, h, c["views"][f], c["fx"], c["fy"], Hh, Ww)
        for z0 in range(0, dims[2], 4):
            for y0 in range(0, dims[1], 8):
                for x0 in range(0, dims[0], 32):
                    b = m[z0:z0 + 4, y0:y0 + 8, x0:x0 + 32]
                    full, dead, cut = full + b.all(), dead + (not b.any()), cut + (b.any() and not b.all())
    assert dead >= 20 and cut >= 20, (full, dead, cut)
    pick = lambda k: np.ascontiguousarray(c[k][order])
    ref = TR.integrate(TR.empty_volume(dims, True), origin, h, 4 * f32(h), pick("invdepth"), pick("views"), c["fx"], c["fy"],
                       alpha=pick("alpha"), color=pick("color"), min_alpha=TC.MIN_ALPHA, max_depth=TC.MAX_DEPTH)
    assert ref["weight"].max() > 60 and (ref["weight"] == 0).any()
    vol = _volume(dims, origin, h, color=True)
    vol.integrate(_gpu(pick("invdepth")), _gpu(pick("views")), c["fx"], c["fy"], alpha=_gpu(pick("alpha")), color=_gpu(pick("color")),
                  min_alpha=TC.MIN_ALPHA, max_depth=TC.MAX_DEPTH)
    _same_volume(vol, ref, "cull")


def _mesh_cases():
    sphere, origin, h, _, _ = TC.sphere_volume(33, color=True)
    return {"integrated": (TC.DIMS, TC.ORIGIN, TC.H_VOX, TC.integrated(True), True),
            "sphere": ((33, 33, 33), origin, h, sphere, True),
            "sphere_plain": ((33, 33, 33), origin, h, dict(sphere, color=None), False)}


@pytest.mark.parametrize("name", ("integrated", "sphere", "sphere_plain"))
def test_extract_mesh_bit_for_bit(name, monkeypatch):
    dims, origin, h, ref, color = _mesh_cases()[name]
    want = TC.mesh_of(("gpu", name), ref, origin, h)
    assert want[3]["T"] > 500
    vol = _volume(dims, origin, h, ref, color)
    got = vol.extract_mesh()
    assert len(got) == (3 if color else 2) and got[1].dtype == torch.int32
    _same_mesh(got, want, name)
    again = vol.extract_mesh()                                      # the same bits on every run
    for a, b in zip(got, again):
        assert poison.bytes_of(a) == poison.bytes_of(b)
    # whatever the plan's workspace, the totals and the outputs held before
    for pattern in ("ff", "random"):
        with poison.poisoned(monkeypatch, pattern) as session:
            dirty = vol.extract_mesh()
        fills = session.require("casualhdrsplat_amd.tsdf", at_least=4 + color)
        assert max(f.nbytes for f in fills) == L.load().hs_tsdf_mesh_workspace_bytes(*dims)
        for a, b in zip(got, dirty):
            assert poison.bytes_of(a) == poison.bytes_of(b), (name, pattern)
    if name == "integrated":                                        # another threshold: the restatement's again
        loose = TR.extract_mesh(ref, origin, h, 0.0)
        assert loose[3]["T"] > want[3]["T"]
        _same_mesh(vol.extract_mesh(min_weight=0.0), loose, "min_weight=0")


def test_a_volume_without_a_surface_gives_empty_tensors():
    vol = _volume((9, 7, 5), (0.0, 0.0, 0.0), 0.1, color=True)
    for w in (0.0, 1.0):                                            # nothing observed; everything observed and outside
        vol.weight.fill_(w)
        v, f, c = vol.extract_mesh()
        assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3) and f.dtype == torch.int32 and v.device.type == "cuda"
    # vertices but no face (one observed edge with a crossing, no observed tetrahedron): empty too
    vol.weight.zero_()
    vol.weight[2, 3, 4:6] = 1
    vol.tsdf[2, 3, 4] = -0.5
    ref = dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), color=vol.color.cpu().numpy())
    assert TR.extract_mesh(ref, (0.0, 0.0, 0.0), 0.1)[3]["V"] == 1
    v, f, c = vol.extract_mesh()
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)


# The scan has two levels: 256 samples per workgroup of the count, and one workgroup of 1024 threads over the workgroups' sums,
# each thread taking ceil(n / 1024) of them in a row.  One volume either side of each boundary.
@pytest.mark.parametrize("dims", ((8, 8, 4), (8, 8, 5), (64, 64, 64), (64, 64, 65)))
def test_the_scan_at_its_level_boundaries(dims):
    n = dims[0] * dims[1] * dims[2]
    assert (n <= 256, n <= 256 * 1024) == {256: (True, True), 320: (False, True), 262144: (False, True), 266240: (False, False)}[n]
    origin, h = (-1.0, 0.5, 2.0), 0.05
    ref = TC.plane_volume(dims)
    v, f, _, info = TR.extract_mesh(ref, origin, h)
    assert info["T"] == 8 * (dims[0] - 1) * (dims[1] - 1) and info["V"] == v.shape[0] > 0
    gv, gf = _volume(dims, origin, h, ref).extract_mesh()
    assert gv.shape == v.shape and gf.shape == f.shape
    gv, gf = gv.cpu().numpy(), gf.cpu().numpy()
    for got, want in ((gv, v), (gf, f)):
        assert got[:1000].tobytes() == want[:1000].tobytes() and got[-1000:].tobytes() == want[-1000:].tobytes()
    assert gf.min() == 0 and gf.max() == v.shape[0] - 1


def test_the_c_abi_on_preallocated_buffers_equals_python():
    dims, origin, h = TC.DIMS, TC.ORIGIN, TC.H_VOX
    c = TC.frames_case()
    lib = L.load()
    nx, ny, nz = dims
    tsdf = torch.ones((nz, ny, nx), device=DEV)
    weight = torch.zeros((nz, ny, nx), device=DEV)
    color = torch.zeros((3, nz, ny, nx), device=DEV)
    keep = [_gpu(c[k]) for k in ("invdepth", "alpha", "color", "views")]
    a = L.hs_tsdf_args()
    a.nx, a.ny, a.nz = dims
    a.F, (a.H, a.W) = TC.FRAMES, TC.HW
    a.origin = (C.c_float * 3)(*origin)
    a.voxel_size, a.trunc, a.fx, a.fy = h, float(4 * f32(h)), c["fx"], c["fy"]
    a.min_alpha, a.max_depth, a.min_weight = TC.MIN_ALPHA, TC.MAX_DEPTH, 1.0
    a.tsdf, a.weight, a.color = tsdf.data_ptr(), weight.data_ptr(), color.data_ptr()
    a.invdepth, a.alpha, a.frame_color, a.viewmatrices = (t.data_ptr() for t in keep)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    L.check(lib.hs_tsdf_integrate(C.byref(a), stream), "hs_tsdf_integrate")
    vol = _volume(dims, origin, h, color=True)
    _integrate(vol, c, slice(0, TC.FRAMES), True)
    for got, want in ((tsdf, vol.tsdf), (weight, vol.weight), (color, vol.color)):
        assert poison.bytes_of(got) == poison.bytes_of(want)
    want = vol.extract_mesh()
    V, T = want[0].shape[0], want[1].shape[0]
    workspace = poison.fill_(torch.empty(lib.hs_tsdf_mesh_workspace_bytes(*dims), dtype=torch.uint8, device=DEV), "a5")
    totals = poison.fill_(torch.empty(2, dtype=torch.int64, device=DEV), "ff")
    a.workspace, a.totals = workspace.data_ptr(), totals.data_ptr()
    L.check(lib.hs_tsdf_mesh_plan(C.byref(a), stream), "hs_tsdf_mesh_plan")
    assert totals.tolist() == [V, T]
    vertices = poison.fill_(torch.empty((V, 3), device=DEV), "nan")
    faces = poison.fill_(torch.empty((T, 3), dtype=torch.int32, device=DEV), "ff")
    colors = poison.fill_(torch.empty((V, 3), device=DEV), "nan")
    a.n_vertices, a.n_faces = V, T
    a.vertices, a.faces, a.colors = vertices.data_ptr(), faces.data_ptr(), colors.data_ptr()
    L.check(lib.hs_tsdf_mesh_emit(C.byref(a), stream), "hs_tsdf_mesh_emit")
    for got, w in zip((vertices, faces, colors), want):
        assert poison.bytes_of(got) == poison.bytes_of(w)


def test_the_example_writes_a_mesh(tmp_path):
    """examples/train_synthetic.py --mesh PATH: the command line itself (one process), small and short; the surface of the true
    geometry is not claimed, only that a mesh of the trained cloud's depth comes out, consistent with what the line prints."""
    import os
    import re
    import subprocess
    import sys
    from casualhdrsplat_amd import scene_io
    script = os.path.join(TC.ROOT, "examples", "train_synthetic.py")
    path = str(tmp_path / "out.ply")
    out = subprocess.run([sys.executable, script, "--steps", "5", "--P", "4000", "--W", "160", "--H", "112", "--frames", "2",
                          "--normal", "0.05", "--mesh", path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = next(l for l in out.stdout.splitlines() if l.startswith("mesh "))
    V, T, nx, ny, nz = (int(x) for x in re.search(r"V (\d+), T (\d+); volume (\d+) x (\d+) x (\d+) samples", line).groups())
    v, f, c = scene_io.load_mesh_ply(path)
    assert v.shape == (V, 3) and f.shape == (T, 3) and c.shape == (V, 3) and T > 100 and max(nx, ny, nz) in (160, 161)
    assert f.min() >= 0 and f.max() < V and np.isfinite(v).all()
    import importlib.util                                           # the refusal, in this process: it comes before any work
    spec = importlib.util.spec_from_file_location("train_synthetic_for_tsdf", script)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    with pytest.raises(ValueError, match=r"\(--mesh\) is not supported together with graph=True \(--graph\)"):
        example.run(steps=1, graph=True, mesh=path, quiet=True)
