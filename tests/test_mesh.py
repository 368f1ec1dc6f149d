"""CPU checks of the mesh clean-up by connected components (mesh.hip: hs_mesh_components, hs_mesh_clean_plan, hs_mesh_clean_emit;
mesh.clean_mesh, mesh.mesh_components): the restatement the GPU tests compare with (tests/mesh_reference.py) against an
independent witness (scipy's connected_components) on every case of the GPU tests and against closed forms, the C ABI (exports,
struct layout, workspace formula, validation before any HIP call), the Python refusals, the build and the example's flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mesh_reference as MR
import tsdf_reference as TR
from casualhdrsplat_amd import mesh as M      # (the module under test: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_mesh_workspace_bytes", "hs_mesh_components", "hs_mesh_clean_plan", "hs_mesh_clean_emit")
f32 = np.float32
_CACHE = {}

# ---- the cases of the GPU tests (shared with tests/test_mesh_gpu.py; every mesh and every reference is computed once) ----
SPHERE_DIMS, SPHERE_ORIGIN, SPHERE_H = (24, 24, 24), (0.3, -1.7, 2.1), 0.125
SPHERES = ((8.3, 8.6, 9.1, 6.05), (18.4, 17.6, 5.3, 2.2), (5.2, 19.1, 18.7, 1.4))      # centre (i, j, k) and radius, in cells
SPHERE_ZEROS = ((9, 8, 14), (5, 17, 20))                                               # (k, j, i): inside samples just under the surface
SPHERE_SIZES = {False: (4096, 512, 232), True: (4108, 516, 232)}                       # faces per sphere; with the two zeros
RIBBON_FACES = 30000
COMB_FANS, COMB_SIZES = 3000, (1, 2, 3, 5, 8, 3, 2)
# mesh.hip's scan (tsdf.hip's, restated) has two levels: 256 flags per workgroup, then ONE workgroup of 1024 threads, each taking
# ceil(n / (256 * 1024)) sums in a row: n > 262144 passes both boundaries, for the faces and for the vertices.  The select's
# histogram kernel and every other kernel is one element per thread with no further boundary.
LARGE_GRID, LARGE_SPARE, SCAN_BOUNDARY = 400, 110000, 256 * 1024


def sphere_volume(zeros=False, color=False):
    """a 24^3 volume with three disjoint spheres, every sample observed; zeros: two inside samples forced to exactly 0"""
    n = SPHERE_DIMS[0]
    ax = np.arange(n, dtype=np.float64)
    d = np.full((n, n, n), np.inf)
    for cx, cy, cz, r in SPHERES:
        d = np.minimum(d, np.sqrt((ax[None, None, :] - cx) ** 2 + (ax[None, :, None] - cy) ** 2 + (ax[:, None, None] - cz) ** 2) - r)
    tsdf = np.clip(d / 4, -1, 1).astype(f32)
    if zeros:
        for z in SPHERE_ZEROS:
            assert tsdf[z] < 0
            tsdf[z] = 0
    col = np.random.default_rng(7).random((3, n, n, n)).astype(f32) if color else None
    return dict(tsdf=tsdf, weight=np.ones((n, n, n), f32), color=col)


def sphere_mesh(zeros=False, color=False):
    key = ("spheres", zeros, color)
    if key not in _CACHE:
        _CACHE[key] = TR.extract_mesh(sphere_volume(zeros, color), SPHERE_ORIGIN, SPHERE_H)[:3]
    return _CACHE[key]


def ribbon(permuted):
    """one triangle strip of RIBBON_FACES faces; permuted: the vertex numbering AND the face order are seeded permutations"""
    key = ("ribbon", permuted)
    if key not in _CACHE:
        n = RIBBON_FACES
        rng = np.random.default_rng(11)
        i = np.arange(n, dtype=np.int64)
        faces = np.stack([i, i + 1, i + 2], 1)
        faces[1::2] = faces[1::2][:, [1, 0, 2]]
        vertices = np.stack([0.01 * np.arange(n + 2), (np.arange(n + 2) % 2).astype(np.float64), np.zeros(n + 2)], 1).astype(f32)
        if permuted:
            number = rng.permutation(n + 2)                     # vertex v becomes number[v]
            moved = np.empty_like(vertices)
            moved[number] = vertices
            vertices, faces = moved, number[faces][rng.permutation(n)]
        _CACHE[key] = (vertices, faces.astype(np.int32), None)
    return _CACHE[key]


def comb():
    """COMB_FANS disjoint fans whose sizes repeat (COMB_SIZES in turn), a vertex nothing references after every third fan, and
    in every tenth fan one more face that repeats an index (valid: it counts; degenerate: it is not kept).  Fan 4 has two rim
    vertices at one position, written -0 and +0 (degenerate by position); fan 11 has two rim vertices of NaNs (equal to nothing)."""
    if "comb" not in _CACHE:
        rng = np.random.default_rng(5)
        faces, at = [], 0
        special = {}
        for k in range(COMB_FANS):
            s = COMB_SIZES[k % len(COMB_SIZES)]
            c, rim = at, [at + 1 + i for i in range(s + 1)]
            faces += [(c, rim[i], rim[i + 1]) for i in range(s)]
            if k % 10 == 0:
                faces.append((rim[0], c, rim[0]))
            if k in (4, 11):
                special[k] = rim
            at += s + 2 + (1 if k % 3 == 2 else 0)
        vertices = rng.normal(size=(at, 3)).astype(f32)
        vertices[special[4][0]] = (0.0, 1.5, -0.0)
        vertices[special[4][1]] = (-0.0, 1.5, 0.0)
        vertices[special[11][0]] = vertices[special[11][1]] = (np.nan, np.nan, np.nan)
        colors = rng.random((at, 3)).astype(f32)
        _CACHE["comb"] = (vertices, np.array(faces, np.int32), colors)
    return _CACHE["comb"]


def large():
    """a LARGE_GRID^2 sheet (one component), 40 floaters of 4 .. 43 faces behind it and LARGE_SPARE vertices nothing references
    in front: T and V both above the scan's boundary"""
    if "large" not in _CACHE:
        g = LARGE_GRID
        rng = np.random.default_rng(3)
        idx = LARGE_SPARE + np.arange(g * g, dtype=np.int64).reshape(g, g)
        a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
        faces = [np.stack([a, b, c], 1), np.stack([b, d, c], 1)]
        at = LARGE_SPARE + g * g
        for k in range(40):
            s = 4 + k
            i = np.arange(s, dtype=np.int64)
            faces.append(np.stack([np.full(s, at), at + 1 + i, at + 2 + i], 1))
            at += s + 2
        faces = np.concatenate(faces)
        faces = faces[rng.permutation(faces.shape[0])[: faces.shape[0] // 64].tolist() + list(range(faces.shape[0]))]   # some faces twice
        vertices = rng.normal(size=(at, 3)).astype(f32)
        assert faces.shape[0] > SCAN_BOUNDARY and at > SCAN_BOUNDARY
        _CACHE["large"] = (vertices, faces.astype(np.int32), None)
    return _CACHE["large"]


CASES = {"spheres": lambda: sphere_mesh(), "spheres_zeros": lambda: sphere_mesh(zeros=True), "spheres_color": lambda: sphere_mesh(color=True),
         "ribbon": lambda: ribbon(False), "ribbon_permuted": lambda: ribbon(True), "comb": comb, "large": large}


def reference(name, **kw):
    """MR.clean of a case, computed once per selection"""
    key = ("clean", name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        v, f, c = CASES[name]()
        _CACHE[key] = MR.clean(v, f, c, label_size=reference_components(name), **kw)
    return _CACHE[key]


def reference_components(name):
    if ("components", name) not in _CACHE:
        v, f, _ = CASES[name]()
        _CACHE[("components", name)] = MR.components(f, v.shape[0])
    return _CACHE[("components", name)]


# ---- the restatement against an independent witness and closed forms ----

@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_against_scipy(name):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    v, f, _ = CASES[name]()
    V = v.shape[0]
    label, size = reference_components(name)
    f64 = f.astype(np.int64)
    rows, cols = np.concatenate([f64[:, 0], f64[:, 1]]), np.concatenate([f64[:, 1], f64[:, 2]])
    n, comp = connected_components(coo_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(V, V)), directed=False)
    low = np.full(n, V, np.int64)
    np.minimum.at(low, comp, np.arange(V))                      # scipy's labels -> the component's smallest vertex index
    want = low[comp[f64[:, 0]]]
    assert (label == want).all()
    count = np.bincount(want, minlength=V)
    assert (size == count[want]).all() and size.min() >= 1


def test_disjoint_tetrahedra_and_the_selection():
    k = 7
    tet = np.array([(0, 1, 2), (0, 3, 1), (1, 3, 2), (0, 2, 3)])
    faces = np.concatenate([tet + 4 * i for i in range(k)]).astype(np.int32)
    vertices = np.random.default_rng(0).normal(size=(4 * k, 3)).astype(f32)
    label, size = MR.components(faces, 4 * k)
    assert (size == 4).all() and (label == np.repeat(4 * np.arange(k), 4)).all()
    out = MR.clean(vertices, faces, keep_largest=3)              # ties go to the lower label
    assert out["kept_labels"] == [0, 4, 8] and out["totals"] == (12, 12, k, 0)
    assert out["faces"].tobytes() == faces[:12].tobytes() and out["vertices"].tobytes() == vertices[:12].tobytes()
    assert MR.clean(vertices, faces, keep_largest=100)["totals"] == (4 * k, 4 * k, k, 0)
    assert MR.clean(vertices, faces, min_faces=5)["totals"] == (0, 0, k, 0)
    assert MR.clean(vertices, faces, min_faces=4, keep_largest=2)["totals"] == (8, 8, k, 0)
    # an index outside [0, V) makes a face invalid: it belongs to nothing and the others do not notice
    bad = faces.copy()
    bad[5] = (4, -1, 6)
    bad[9] = (8, 9, 4 * k)
    label, size = MR.components(bad, 4 * k)
    assert label[5] == label[9] == -1 and size[5] == size[9] == 0 and size[4] == 3 and size[0] == 4 and label[4] == 4
    assert MR.clean(vertices, bad)["totals"] == (4 * k, 4 * k - 2, k, 2)
    # degenerate: equal indices, equal positions (-0 = +0), never a NaN
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0.0, 1, -0.0), (np.nan, 0, 0), (np.nan, 0, 0)], f32)
    f = np.array([(0, 1, 2), (0, 1, 1), (0, 2, 3), (0, 4, 5)], np.int32)
    assert MR.degenerate_faces(v, f).tolist() == [False, True, True, False]
    out = MR.clean(v, f)
    assert out["face_index"].tolist() == [0, 3] and out["vertex_index"].tolist() == [0, 1, 2, 4, 5] and out["totals"] == (5, 2, 1, 0)
    assert MR.clean(v, f, remove_degenerate=False)["totals"] == (6, 4, 1, 0)


@pytest.mark.parametrize("zeros", (False, True))
def test_three_spheres_are_three_closed_components(zeros):
    """every component of the marching-tetrahedra mesh is a closed surface of genus 0: every edge is used exactly twice and
    V - E + F = 2 -- also with two samples of exactly 0, whose degenerate slivers are what keeps the surface stitched"""
    v, f, _ = sphere_mesh(zeros)
    label, size = MR.components(f, v.shape[0])
    labels, counts = np.unique(label, return_counts=True)
    assert tuple(sorted(counts, reverse=True)) == SPHERE_SIZES[zeros] and labels[0] == 0
    deg = MR.degenerate_faces(v, f)
    assert deg.sum() == (32 if zeros else 0)
    for l in labels:
        part = f[label == l].astype(np.int64)
        edges = np.sort(np.concatenate([part[:, [0, 1]], part[:, [1, 2]], part[:, [2, 0]]]), 1)
        uniq, uses = np.unique(edges, axis=0, return_counts=True)
        assert (uses == 2).all() and np.unique(part).size - uniq.shape[0] + part.shape[0] == 2, l
    full = MR.clean(v, f, remove_degenerate=False)
    assert full["faces"].tobytes() == f.tobytes() and full["vertices"].tobytes() == v.tobytes() and full["totals"][2] == 3
    small = SPHERE_SIZES[zeros][2]
    assert MR.clean(v, f, min_faces=300, remove_degenerate=False)["totals"][1] == f.shape[0] - small
    assert MR.clean(v, f, keep_largest=1, remove_degenerate=False)["totals"][1] == SPHERE_SIZES[zeros][0]
    assert MR.clean(v, f, keep_largest=2, min_faces=600, remove_degenerate=False)["totals"][1] == SPHERE_SIZES[zeros][0]
    if zeros:
        assert MR.clean(v, f)["totals"][1] == f.shape[0] - 32


def test_the_cases_are_what_they_claim():
    for permuted in (False, True):
        label, size = reference_components("ribbon_permuted" if permuted else "ribbon")
        assert (label == 0).all() and (size == RIBBON_FACES).all()
    v, f, _ = comb()
    label, size = reference_components("comb")
    assert np.unique(label).size == COMB_FANS and np.unique(f).size < v.shape[0] and (f[:, 0] == f[:, 2]).sum() == COMB_FANS // 10
    out = reference("comb", keep_largest=600)
    sizes = {}
    for l in out["kept_labels"]:
        sizes.setdefault(int(size[label == l][0]), []).append(l)
    assert sum(len(x) for x in sizes.values()) == 600 and len(sizes) > 1
    cut = min(sizes)                                               # the cut falls inside a class of equal sizes ...
    all_of_cut = np.unique(label[size == cut])
    assert len(sizes[cut]) < all_of_cut.size and sorted(sizes[cut]) == all_of_cut[:len(sizes[cut])].tolist()   # ... lower labels win
    deg = MR.degenerate_faces(v, f)
    assert deg.sum() == COMB_FANS // 10 + 1                        # the repeated indices and fan 4's -0 / +0; not fan 11's NaNs
    v, f, _ = large()
    label, size = reference_components("large")
    assert np.unique(label).size == 41 and label.min() == LARGE_SPARE and size.max() > SCAN_BOUNDARY


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
    assert set(NAMES) <= set(declared) and all(re.fullmatch(r"[a-z_]+", n) for n in NAMES)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == lib.HS_VERSION == 309       # (detected by name: the version does not move)
    import casualhdrsplat_amd as pkg
    assert pkg.clean_mesh is M.clean_mesh and pkg.mesh_components is M.mesh_components
    assert "clean_mesh" in pkg.__all__ and "mesh_components" in pkg.__all__


def test_the_build_knows_the_unit():
    mk = open(os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bmesh\.o\b", mk, flags=re.M) and not re.search(r"^FAST_TUS\s*=.*\bmesh\b", mk, flags=re.M)
    assert re.search(r"^#\s+mesh\s+\S", mk, flags=re.M)           # its line in the per-unit comment
    assert "mesh_host" in re.search(r"^ASAN_DRIVERS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    src = open(os.path.join(ROOT, "tests", "native", "mesh_host.cpp")).read()
    assert "int main()" in src and all(n in src for n in NAMES)


def test_struct_matches_c(lib, tmp_path):
    name, S_ = "hs_mesh_args", lib.hs_mesh_args
    fields = [n for n, _ in S_._fields_]
    lines = [f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {n}));' for n in fields]
    want = [C.sizeof(S_)] + [getattr(S_, n).offset for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\nint main(){' + "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want


def workspace_formula(V, T):
    r = lambda x: (x + 15) // 16 * 16
    return 3 * r(4 * V) + r(4 * T) + r(8 * ((V + 255) // 256)) + r(8 * ((T + 255) // 256)) + 8256


def test_the_calls_validate_before_touching_the_gpu(lib):
    L = lib.load()
    one = 4096
    ws = L.hs_mesh_workspace_bytes
    for V, T in ((0, 0), (1, 1), (3, 7), (257, 513), (2426, 4840), (1 << 20, 2654208), ((1 << 31) - 1, (1 << 31) - 1)):
        assert ws(V, T) == workspace_formula(V, T), (V, T)
    assert ws(0, 0) == 8256 and ws(3, 7) == 3 * 16 + 32 + 16 + 16 + 8256
    for bad in ((-1, 5), (5, -1), (1 << 31, 5), (5, 1 << 31), (1 << 62, 1 << 62)):
        assert ws(*bad) == lib.HS_EINVAL and L.hs_last_error().startswith(b"hs_mesh_workspace_bytes:"), bad

    pointers = ("vertices", "faces", "colors", "workspace", "label", "size", "totals", "vertices_out", "faces_out", "colors_out",
                "vertex_index", "face_index")

    def call(which, **kw):
        a = lib.hs_mesh_args()
        a.n_vertices, a.n_faces, a.min_faces, a.keep_largest, a.remove_degenerate = 100, 200, 3, 2, 1
        a.n_vertices_out, a.n_faces_out = 10, 20
        for k in pointers:
            setattr(a, k, one)
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(L, which)(C.byref(a), None), L.hs_last_error()

    used = {"hs_mesh_components": (("faces", "workspace", "label", "size"), ()),
            "hs_mesh_clean_plan": (("faces", "workspace", "vertices", "totals"), ()),
            "hs_mesh_clean_emit": (("faces", "workspace", "vertices", "vertices_out", "faces_out"),
                                   ("colors", "colors_out", "vertex_index", "face_index"))}
    for which, (required, optional) in used.items():
        assert getattr(L, which)(None, None) == lib.HS_EINVAL and L.hs_last_error() == which.encode() + b": null args"
        for k in required:                                        # null pointers, one by one
            rc, msg = call(which, **{k: None})
            assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and b"null " + k.encode() in msg, (which, k, msg)
        for k in required + optional:                             # misalignment, one by one
            align = {"workspace": 16, "totals": 8}.get(k, 4)
            rc, msg = call(which, **{k: one + align // 2})
            assert rc == lib.HS_EINVAL and k.encode() + b" must be %d-byte aligned" % align in msg, (which, k, msg)
        for bad, text in ((dict(n_vertices=-1), b"n_vertices=-1"), (dict(n_faces=-3), b"n_faces=-3"),
                          (dict(n_vertices=1 << 31), b"n_vertices=2147483648"), (dict(n_faces=1 << 31), b"n_faces=2147483648")):
            rc, msg = call(which, **bad)
            assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and text in msg, (which, bad, msg)
        # the largest counts pass the count check: the next refusal is reached
        assert b"null workspace" in call(which, n_vertices=(1 << 31) - 1, n_faces=(1 << 31) - 1, n_vertices_out=0, n_faces_out=0,
                                         workspace=None)[1]

    which = "hs_mesh_clean_plan"
    for bad, text in ((dict(min_faces=-1), b"min_faces=-1"), (dict(keep_largest=-2), b"keep_largest=-2"),
                      (dict(remove_degenerate=2), b"remove_degenerate=2"), (dict(remove_degenerate=-1), b"remove_degenerate=-1")):
        rc, msg = call(which, **bad)
        assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and text in msg, (bad, msg)
    which = "hs_mesh_clean_emit"
    for bad, text in ((dict(n_vertices_out=-1), b"n_vertices_out=-1"), (dict(n_vertices_out=101), b"n_vertices_out=101"),
                      (dict(n_faces_out=-1), b"n_faces_out=-1"), (dict(n_faces_out=201), b"n_faces_out=201"),
                      (dict(colors=None), b"colors_out given for a mesh without colours"),
                      (dict(colors_out=None), b"the mesh has colours")):
        rc, msg = call(which, **bad)
        assert rc == lib.HS_EINVAL and msg.startswith(which.encode() + b":") and text in msg, (bad, msg)
    # nothing to do is a successful no-op that needs no output: an empty result, and components of no faces
    assert call(which, n_vertices_out=0, n_faces_out=0, vertices_out=None, faces_out=None, vertices=None)[0] == lib.HS_OK
    assert call("hs_mesh_components", n_faces=0, faces=None, label=None, size=None)[0] == lib.HS_OK


# ---- Python ----

def test_python_refusals():
    import inspect
    sig = inspect.signature(M.clean_mesh)
    assert list(sig.parameters) == ["vertices", "faces", "colors", "min_faces", "keep_largest", "remove_degenerate", "return_index"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[3:])
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, 0, None, True, False]
    assert list(inspect.signature(M.mesh_components).parameters) == ["faces", "n_vertices"]
    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")
    v, f = meta(10, 3), meta(20, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"clean_mesh \(faces\) on an MI355X only: .*\(no CPU fallback\)"):
        M.clean_mesh(torch.zeros(10, 3), torch.zeros(20, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"\(no CPU fallback\)"):           # everything consistent, and not on the GPU
        M.clean_mesh(v, f, meta(10, 3), min_faces=3, keep_largest=2, remove_degenerate=False, return_index=True)
    with pytest.raises(TypeError, match="vertices must be a torch.Tensor"):
        M.clean_mesh(np.zeros((10, 3), f32), f)
    with pytest.raises(TypeError, match="faces must be a torch.Tensor"):
        M.clean_mesh(v, np.zeros((20, 3), np.int32))
    with pytest.raises(TypeError, match="vertices must be float32"):
        M.clean_mesh(meta(10, 3, dtype=torch.float64), f)
    with pytest.raises(TypeError, match="faces must be int32"):
        M.clean_mesh(v, meta(20, 3, dtype=torch.int64))
    with pytest.raises(TypeError, match="colors must be float32"):
        M.clean_mesh(v, f, meta(10, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"vertices must be \[N, 3\]"):
        M.clean_mesh(meta(10, 4), f)
    with pytest.raises(ValueError, match=r"faces must be \[N, 3\]"):
        M.clean_mesh(v, meta(60, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"colors must be \[10, 3\]"):
        M.clean_mesh(v, f, meta(9, 3))
    with pytest.raises(ValueError, match="faces holds 2147483648 rows, 2\\^31 or more"):
        M.clean_mesh(v, meta(1 << 31, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="vertices holds 2147483648 rows"):
        M.clean_mesh(meta(1 << 31, 3), f)
    with pytest.raises(ValueError, match="faces and vertices live on different devices"):
        M.clean_mesh(torch.zeros(10, 3), f)
    with pytest.raises(ValueError, match="faces and colors live on different devices"):
        M.clean_mesh(v, f, torch.zeros(10, 3))
    with pytest.raises(ValueError, match="min_faces=-1 must be >= 0"):
        M.clean_mesh(v, f, min_faces=-1)
    with pytest.raises(TypeError, match="min_faces must be a Python int"):
        M.clean_mesh(v, f, min_faces=2.0)
    with pytest.raises(ValueError, match="keep_largest=0 must be >= 1"):
        M.clean_mesh(v, f, keep_largest=0)
    with pytest.raises(TypeError, match="keep_largest must be a Python int"):
        M.clean_mesh(v, f, keep_largest=True)
    with pytest.raises(TypeError, match="remove_degenerate and return_index must be bool"):
        M.clean_mesh(v, f, remove_degenerate=1)
    with pytest.raises(TypeError):
        M.clean_mesh(v, f, None, 3)                              # the options are keyword-only
    with pytest.raises(RuntimeError, match=r"mesh_components \(faces\) on an MI355X only"):
        M.mesh_components(f, 10)
    with pytest.raises(TypeError, match="faces must be int32"):
        M.mesh_components(meta(20, 3, dtype=torch.int64), 10)
    with pytest.raises(TypeError, match="n_vertices must be a Python int"):
        M.mesh_components(f, 10.0)
    with pytest.raises(ValueError, match="n_vertices=-1 outside"):
        M.mesh_components(f, -1)
    with pytest.raises(ValueError, match="n_vertices=2147483648 outside"):
        M.mesh_components(f, 1 << 31)


def test_the_example_refuses_the_flags_without_a_mesh(capsys):
    import importlib.util
    script = os.path.join(ROOT, "examples", "train_synthetic.py")
    spec = importlib.util.spec_from_file_location("train_synthetic_for_mesh", script)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    for flags in (["--mesh-min-faces", "100"], ["--mesh-keep-largest", "1"], ["--mesh-min-faces", "5", "--mesh-keep-largest", "2"]):
        with pytest.raises(SystemExit) as e:
            example.main(["--steps", "1"] + flags)
        assert e.value.code == 2 and "give that too" in capsys.readouterr().err
    with pytest.raises(ValueError, match=r"clean the mesh of mesh=PATH \(--mesh\)"):
        example.run(steps=1, mesh_keep_largest=1, quiet=True)
    with pytest.raises(ValueError, match=r"clean the mesh of mesh=PATH \(--mesh\)"):
        example.run(steps=1, mesh_min_faces=10, quiet=True)
    with pytest.raises(ValueError, match="must be >= 1"):
        example.run(steps=1, mesh="x.ply", mesh_keep_largest=0, quiet=True)
    with pytest.raises(ValueError, match="must be >= 0"):
        example.run(steps=1, mesh="x.ply", mesh_min_faces=-1, quiet=True)
