"""GPU checks of the mesh clean-up by connected components (mesh.hip through mesh.clean_mesh / mesh.mesh_components and through
the C ABI): labels, sizes, totals, both index arrays, faces and the bits of vertices and colours, all with == against the
sequential numpy restatement (tests/mesh_reference.py, held to scipy and to closed forms by tests/test_mesh.py, whose cases these
are).  No tolerance appears anywhere: everything is an integer or a copy."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_reference as MR
import poison
import test_mesh as TM
from casualhdrsplat_amd import _lib as L
from casualhdrsplat_amd.mesh import clean_mesh, mesh_components
from casualhdrsplat_amd.tsdf import TSDFVolume

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


def _gpu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _same(got, want, what, color):
    """clean_mesh(..., return_index=True)'s tuple against MR.clean's dict"""
    names = ("vertices", "faces") + (("colors",) if color else ()) + ("vertex_index", "face_index")
    assert len(got) == len(names), (what, len(got))
    for n, g in zip(names, got):
        w = want[n]
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, n, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, n, int((g.reshape(g.shape[0], -1) != w.reshape(w.shape[0], -1)).any(axis=1).sum()))
    assert (got[0].shape[0], got[1].shape[0]) == want["totals"][:2]


def _components_match(name):
    v, f, _ = TM.CASES[name]()
    label, size = mesh_components(_gpu(f), v.shape[0])
    want_label, want_size = TM.reference_components(name)
    assert label.dtype == torch.int32 and size.dtype == torch.int32
    assert (label.cpu().numpy() == want_label).all() and (size.cpu().numpy() == want_size).all(), name


def _check(name, **kw):
    v, f, c = TM.CASES[name]()
    got = clean_mesh(_gpu(v), _gpu(f), _gpu(c), return_index=True, **kw)
    _same(got, TM.reference(name, **kw), (name, kw), c is not None)
    return got


# ---- the extractor's output ----

@pytest.fixture(scope="module")
def extracted():
    """the three-sphere meshes straight from TSDFVolume.extract_mesh on the GPU: the restatement's bits (test_tsdf_gpu.py)"""
    out = {}
    for zeros, color in ((False, False), (True, False), (False, True)):
        ref = TM.sphere_volume(zeros, color)
        vol = TSDFVolume(TM.SPHERE_ORIGIN, TM.SPHERE_H, TM.SPHERE_DIMS, color=color, device=DEV)
        vol.tsdf.copy_(_gpu(ref["tsdf"]))
        vol.weight.copy_(_gpu(ref["weight"]))
        if color:
            vol.color.copy_(_gpu(ref["color"]))
        mesh = vol.extract_mesh()
        for g, w in zip(mesh, TM.sphere_mesh(zeros, color)):
            assert poison.bytes_of(g) == poison.bytes_of(w)
        out[(zeros, color)] = mesh
    return out


SELECTIONS = (dict(min_faces=300), dict(keep_largest=1), dict(keep_largest=2, min_faces=600), dict())


@pytest.mark.parametrize("kw", SELECTIONS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "all")
def test_three_spheres_from_the_extractor(extracted, kw):
    v, f = extracted[(False, False)]
    want = TM.reference("spheres", **kw)
    got = clean_mesh(v, f, return_index=True, **kw)
    _same(got, want, kw, False)
    sizes = TM.SPHERE_SIZES[False]
    assert got[1].shape[0] == {"min_faces": sizes[0] + sizes[1], "keep_largest": sizes[0]}.get(next(iter(kw), None), sum(sizes))
    if not kw:                                                     # no selection: the mesh comes back identical
        assert poison.bytes_of(got[0]) == poison.bytes_of(v) and poison.bytes_of(got[1]) == poison.bytes_of(f)
        assert (got[2].cpu().numpy() == np.arange(v.shape[0])).all() and (got[3].cpu().numpy() == np.arange(f.shape[0])).all()
    plain = clean_mesh(v, f, **kw)                                 # without the index arrays: the same mesh
    assert len(plain) == 2 and all(poison.bytes_of(a) == poison.bytes_of(b) for a, b in zip(plain, got))


@pytest.mark.parametrize("remove", (True, False))
def test_samples_of_exactly_zero(extracted, remove):
    v, f = extracted[(True, False)]
    for kw in (dict(), dict(keep_largest=1), dict(min_faces=300)):
        want = TM.reference("spheres_zeros", remove_degenerate=remove, **kw)
        _same(clean_mesh(v, f, return_index=True, remove_degenerate=remove, **kw), want, (remove, kw), False)
        assert want["totals"][2] == 3                              # the slivers still count: three components, not more
    whole = clean_mesh(v, f, remove_degenerate=remove)
    assert whole[1].shape[0] == f.shape[0] - (32 if remove else 0)
    _components_match("spheres_zeros")


def test_colours_are_gathered_with_the_vertices(extracted):
    v, f, c = extracted[(False, True)]
    for kw in (dict(min_faces=300), dict(keep_largest=1), dict()):
        got = clean_mesh(v, f, c, return_index=True, **kw)
        _same(got, TM.reference("spheres_color", **kw), kw, True)
        assert poison.bytes_of(got[2]) == poison.bytes_of(c[got[3].long()])
    assert len(clean_mesh(v, f, c)) == 3


# ---- deep trees, ties, boundaries ----

@pytest.mark.parametrize("name", ("ribbon", "ribbon_permuted"))
def test_a_ribbon_is_one_component(name):
    v, f, _ = TM.CASES[name]()
    label, size = mesh_components(_gpu(f), v.shape[0])
    assert (label == 0).all() and (size == TM.RIBBON_FACES).all()
    _components_match(name)
    got = _check(name, keep_largest=1)
    assert got[1].shape[0] == TM.RIBBON_FACES and poison.bytes_of(got[0]) == poison.bytes_of(v)
    assert _check(name, min_faces=TM.RIBBON_FACES + 1)[1].shape[0] == 0


def test_a_comb_of_fans_ties_go_to_the_lower_label():
    _components_match("comb")
    for kw in (dict(keep_largest=600), dict(keep_largest=1), dict(keep_largest=600, min_faces=8), dict(min_faces=4),
               dict(keep_largest=TM.COMB_FANS), dict(keep_largest=TM.COMB_FANS + 5, remove_degenerate=False), dict(keep_largest=2999)):
        _check("comb", **kw)
    v, f, c = TM.comb()
    whole = clean_mesh(_gpu(v), _gpu(f), _gpu(c), remove_degenerate=False)
    assert whole[1].shape[0] == f.shape[0] and whole[0].shape[0] == np.unique(f).size < v.shape[0]    # the spare vertices go


def test_one_large_mesh_past_the_scans_boundaries():
    """T and V above 262144 = 256 flags per workgroup x 1024 threads of the one scanning workgroup: every thread of the scan
    takes more than one workgroup's sum, in both tables."""
    v, f, _ = TM.large()
    assert f.shape[0] > TM.SCAN_BOUNDARY and v.shape[0] > TM.SCAN_BOUNDARY
    _components_match("large")
    for kw in (dict(keep_largest=1), dict(min_faces=30), dict(keep_largest=7, min_faces=40), dict()):
        got = _check("large", **kw)
    assert got[0].shape[0] == v.shape[0] - TM.LARGE_SPARE


# ---- invalid faces, empty cases ----

def test_invalid_faces():
    v, f, _ = TM.sphere_mesh()
    V = v.shape[0]
    bad = f.copy()
    bad[7, 1] = -1
    bad[4000, 2] = V
    bad[4001] = (V + 5, 0, 1)
    with pytest.raises(ValueError, match=rf"clean_mesh: 3 of the {f.shape[0]} faces have an index outside \[0, {V}\)"):
        clean_mesh(_gpu(v), _gpu(bad))
    label, size = mesh_components(_gpu(bad), V)
    want_label, want_size = MR.components(bad, V)
    assert (label.cpu().numpy() == want_label).all() and (size.cpu().numpy() == want_size).all()
    assert label[[7, 4000, 4001]].tolist() == [-1, -1, -1] and size[[7, 4000, 4001]].tolist() == [0, 0, 0]


def test_empty_cases():
    v, f, c = TM.sphere_mesh(color=True)
    gv, gf, gc = _gpu(v), _gpu(f), _gpu(c)
    none = torch.zeros((0, 3), dtype=torch.int32, device=DEV)
    for out in (clean_mesh(gv, none, gc, return_index=True), clean_mesh(gv, gf, gc, min_faces=10 ** 6, return_index=True),
                clean_mesh(gv, gf, gc, min_faces=1 << 40, keep_largest=1 << 70, return_index=True),
                clean_mesh(torch.zeros((0, 3), device=DEV), none, torch.zeros((0, 3), device=DEV), return_index=True)):
        assert [tuple(t.shape) for t in out] == [(0, 3), (0, 3), (0, 3), (0,), (0,)]
        assert [t.dtype for t in out] == [torch.float32, torch.int32, torch.float32, torch.int32, torch.int32]
        assert all(t.device.type == "cuda" for t in out)
    label, size = mesh_components(none, 5)
    assert label.shape == size.shape == (0,) and label.dtype == torch.int32
    # faces that are all degenerate: components exist, nothing is kept
    same = torch.tensor([[0, 0, 1], [1, 2, 2]], dtype=torch.int32, device=DEV)
    assert clean_mesh(gv, same)[1].shape == (0, 3) and clean_mesh(gv, same, remove_degenerate=False)[0].shape == (3, 3)


# ---- reproducibility; the workspace ----

def test_two_runs_give_the_same_bits():
    for name, kw in (("ribbon_permuted", dict(keep_largest=1)), ("comb", dict(keep_largest=600)), ("large", dict(min_faces=30))):
        v, f, c = TM.CASES[name]()
        gv, gf, gc = _gpu(v), _gpu(f), _gpu(c)
        runs = [clean_mesh(gv, gf, gc, return_index=True, **kw) + mesh_components(gf, v.shape[0]) for _ in range(2)]
        for a, b in zip(*runs):
            assert poison.bytes_of(a) == poison.bytes_of(b), name


def _abi_clean(v, f, c, fill, **kw):
    """plan + emit through ctypes on preallocated buffers: the workspace and every output pre-filled with `fill`, each with a
    guard of 64 bytes behind it.  Returns the outputs, the totals and the guards."""
    lib = L.load()
    V, T = v.shape[0], f.shape[0]
    nbytes = lib.hs_mesh_workspace_bytes(V, T)
    assert nbytes == TM.workspace_formula(V, T)
    guard = 64

    def buffer(n):
        t = poison.fill_(torch.empty(n + guard, dtype=torch.uint8, device=DEV), fill)
        t[n:] = 0x3C
        return t

    ws, totals = buffer(nbytes), buffer(32)
    a = L.hs_mesh_args()
    a.n_vertices, a.n_faces = V, T
    a.min_faces, a.keep_largest, a.remove_degenerate = kw.get("min_faces", 0), kw.get("keep_largest", 0), 1
    a.vertices, a.faces, a.colors = v.data_ptr(), f.data_ptr(), c.data_ptr()
    a.workspace, a.totals = ws.data_ptr(), totals.data_ptr()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    L.check(lib.hs_mesh_clean_plan(C.byref(a), stream), "hs_mesh_clean_plan")
    tot = totals[:32].view(torch.int64).tolist()
    Vo, To = tot[:2]
    outs = dict(vertices=buffer(12 * Vo), faces=buffer(12 * To), colors=buffer(12 * Vo), vertex_index=buffer(4 * Vo), face_index=buffer(4 * To))
    a.n_vertices_out, a.n_faces_out = Vo, To
    a.vertices_out, a.faces_out, a.colors_out = outs["vertices"].data_ptr(), outs["faces"].data_ptr(), outs["colors"].data_ptr()
    a.vertex_index, a.face_index = outs["vertex_index"].data_ptr(), outs["face_index"].data_ptr()
    L.check(lib.hs_mesh_clean_emit(C.byref(a), stream), "hs_mesh_clean_emit")
    torch.cuda.synchronize()
    for name, t in list(outs.items()) + [("workspace", ws), ("totals", totals)]:
        assert (t[-guard:] == 0x3C).all(), (name, "written behind its end")
    return {k: t[:-guard].cpu().numpy().tobytes() for k, t in outs.items()}, tot


@pytest.mark.parametrize("name,kw", (("comb", dict(keep_largest=600, min_faces=3)), ("spheres_color", dict(min_faces=300))))
def test_the_workspace_may_hold_anything(name, kw):
    """Through the C ABI, plan + emit with the workspace, the totals and the outputs pre-filled with 0x00 and with 0xFF: the same
    outputs, the restatement's; the inputs keep their bits and nothing is written behind the end of any buffer -- only the
    outputs are written (tests/test_workspace_contents_gpu.py states the same contract for the rasterizer's workspaces)."""
    v, f, c = TM.CASES[name]()
    gv, gf, gc = _gpu(v), _gpu(f), _gpu(c)
    want = TM.reference(name, **kw)
    runs = [_abi_clean(gv, gf, gc, fill, **kw) for fill in ("zero", "ff")]
    assert runs[0] == runs[1]
    outs, tot = runs[0]
    assert tuple(tot) == want["totals"]
    for k, b in outs.items():
        assert b == want[k].tobytes(), k
    assert poison.bytes_of(gv) == v.tobytes() and poison.bytes_of(gf) == f.tobytes() and poison.bytes_of(gc) == c.tobytes()


def test_python_hands_over_uninitialised_buffers(monkeypatch):
    """clean_mesh under poisoned allocations (workspace, totals and every output): the same bits"""
    v, f, c = TM.comb()
    gv, gf, gc = _gpu(v), _gpu(f), _gpu(c)
    clean = clean_mesh(gv, gf, gc, keep_largest=600, return_index=True)
    for pattern in ("ff", "random"):
        with poison.poisoned(monkeypatch, pattern) as session:
            dirty = clean_mesh(gv, gf, gc, keep_largest=600, return_index=True) + mesh_components(gf, v.shape[0])
        fills = session.require("casualhdrsplat_amd.mesh", at_least=7 + 3)
        assert max(x.nbytes for x in fills) == L.load().hs_mesh_workspace_bytes(v.shape[0], f.shape[0])
        for a, b in zip(clean + mesh_components(gf, v.shape[0]), dirty):
            assert poison.bytes_of(a) == poison.bytes_of(b), pattern
