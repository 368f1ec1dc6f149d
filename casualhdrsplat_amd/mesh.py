"""Mesh clean-up by connected components (mesh.hip, through hs_mesh_* of include/hdrsplat.h): the last step from a trained
cloud to a surface.  TSDFVolume.extract_mesh returns a raw mesh -- every floater and every patch of haze that survived the
regularisers is a closed blob of its own next to the surface; clean_mesh clusters the triangles, keeps the large clusters,
drops degenerate faces and the vertices nothing references.

    vertices, faces, colors = vol.extract_mesh()
    vertices, faces, colors = clean_mesh(vertices, faces, colors, keep_largest=1)       # or min_faces=500, or both
    scene_io.save_mesh_ply("mesh.ply", vertices, faces, colors)

Definitions (hdrsplat.h states them, tests/mesh_reference.py restates them): a face is valid when its indices are in [0, V);
two valid faces are connected when they share a vertex INDEX (nothing is welded); a component's label is the smallest vertex
index its faces reference and its size the number of its valid faces, degenerate ones included; a face is degenerate when two of
its indices are equal or two of its corners are equal in all three coordinates (fp32 ==).  Components are ordered by (size
descending, label ascending).  Everything is integer or a copy: the result is exact, in input order, and the same bits on every
run.  clean_mesh reads four numbers on the host, once (as extract_mesh reads two); mesh_components reads none.  It allocates, so
it cannot be captured into a HIP graph.  GPU tensors only, fp32 / int32 only (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .rasterizer import _on_device, _stream
from .tsdf import _device

MAX_COUNT = 1 << 31


def _mesh_tensor(what: str, name: str, t, dtype, like=None, rows=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{what}: {name} must be {str(dtype).replace('torch.', '')}, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3 or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{what}: {name} must be [{'N' if rows is None else rows}, 3], got {tuple(t.shape)}")
    if t.shape[0] >= MAX_COUNT:
        raise ValueError(f"{what}: {name} holds {t.shape[0]} rows, 2^31 or more")
    if like is not None and t.device != like.device:
        raise ValueError(f"{what}: faces and {name} live on different devices")
    return t


def _count(what: str, name: str, v, least: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{what}: {name} must be a Python int, got {type(v).__name__}")
    if v < least:
        raise ValueError(f"{what}: {name}={v} must be >= {least}")
    return min(v, 1 << 62)


def mesh_components(faces, n_vertices):
    """(label [T] int32, size [T] int32): for every face the label of its component -- the smallest vertex index the
    component's faces reference -- and the component's number of faces.  A face with an index outside [0, n_vertices) gets
    label -1 and size 0.  Reads nothing on the host: a policy of your own can stay on the device."""
    what = "mesh_components"
    _mesh_tensor(what, "faces", faces, torch.int32)
    if isinstance(n_vertices, bool) or not isinstance(n_vertices, int):
        raise TypeError(f"{what}: n_vertices must be a Python int, got {type(n_vertices).__name__}")
    if not 0 <= n_vertices < MAX_COUNT:
        raise ValueError(f"{what}: n_vertices={n_vertices} outside [0, 2^31)")
    dev = _device(f"{what} (faces)", faces.device)
    T = faces.shape[0]
    label = torch.empty(T, dtype=torch.int32, device=dev)
    size = torch.empty(T, dtype=torch.int32, device=dev)
    if T == 0:
        return label, size
    lib = L.load()
    f = faces.detach().contiguous()
    workspace = torch.empty(int(lib.hs_mesh_workspace_bytes(n_vertices, T)), dtype=torch.uint8, device=dev)
    a = L.hs_mesh_args()
    a.n_vertices, a.n_faces = n_vertices, T
    a.faces, a.workspace, a.label, a.size = f.data_ptr(), workspace.data_ptr(), label.data_ptr(), size.data_ptr()
    with _on_device(dev):
        L.check(lib.hs_mesh_components(C.byref(a), _stream(dev)), "hs_mesh_components")
    return label, size


def clean_mesh(vertices, faces, colors=None, *, min_faces=0, keep_largest=None, remove_degenerate=True, return_index=False):
    """(vertices' [V', 3], faces' [T', 3][, colors' [V', 3]][, vertex_index [V'] int32, face_index [T'] int32]): the faces of the
    kept components, minus degenerate ones when remove_degenerate is set, in input order; the vertices they reference, in input
    order; indices remapped, colours gathered, floats copied bit for bit.

    min_faces:    keep components of at least this many faces (0: all).
    keep_largest: keep the first n components by (size descending, label ascending) (None: all).  Both given: a component
                  must pass both.
    return_index: also the input index of every output vertex and face.
    Empty tensors when T = 0 or nothing is kept.  ValueError when a face has an index outside [0, V), naming how many."""
    what = "clean_mesh"
    _mesh_tensor(what, "faces", faces, torch.int32)
    _mesh_tensor(what, "vertices", vertices, torch.float32, like=faces)
    if colors is not None:
        _mesh_tensor(what, "colors", colors, torch.float32, like=faces, rows=vertices.shape[0])
    min_faces = _count(what, "min_faces", min_faces, 0)
    keep_largest = 0 if keep_largest is None else _count(what, "keep_largest", keep_largest, 1)
    if not isinstance(remove_degenerate, bool) or not isinstance(return_index, bool):
        raise TypeError(f"{what}: remove_degenerate and return_index must be bool")
    dev = _device(f"{what} (faces)", faces.device)
    V, T = vertices.shape[0], faces.shape[0]
    lib = L.load()
    keep = [t.detach().contiguous() if t is not None else None for t in (vertices, faces, colors)]
    workspace = torch.empty(int(lib.hs_mesh_workspace_bytes(V, T)), dtype=torch.uint8, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    a = L.hs_mesh_args()
    a.n_vertices, a.n_faces, a.min_faces, a.keep_largest, a.remove_degenerate = V, T, min_faces, keep_largest, int(remove_degenerate)
    a.vertices, a.faces = keep[0].data_ptr() if V else None, keep[1].data_ptr() if T else None
    a.colors = keep[2].data_ptr() if colors is not None and V else None
    a.workspace, a.totals = workspace.data_ptr(), totals.data_ptr()
    with _on_device(dev):
        L.check(lib.hs_mesh_clean_plan(C.byref(a), _stream(dev)), "hs_mesh_clean_plan")
        Vo, To, _, invalid = (int(n) for n in totals.tolist())         # the one host read
        if invalid:
            raise ValueError(f"{what}: {invalid} of the {T} faces have an index outside [0, {V})")
        if To == 0:
            Vo = 0
        out_v = torch.empty((Vo, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((To, 3), dtype=torch.int32, device=dev)
        out_c = torch.empty((Vo, 3), dtype=torch.float32, device=dev) if colors is not None else None
        v_index = torch.empty(Vo, dtype=torch.int32, device=dev) if return_index else None
        f_index = torch.empty(To, dtype=torch.int32, device=dev) if return_index else None
        if To > 0:
            a.n_vertices_out, a.n_faces_out = Vo, To
            a.vertices_out, a.faces_out = out_v.data_ptr(), out_f.data_ptr()
            a.colors_out = out_c.data_ptr() if a.colors else None
            a.vertex_index = v_index.data_ptr() if return_index else None
            a.face_index = f_index.data_ptr() if return_index else None
            L.check(lib.hs_mesh_clean_emit(C.byref(a), _stream(dev)), "hs_mesh_clean_emit")
    out = (out_v, out_f) + ((out_c,) if colors is not None else ())
    return out + ((v_index, f_index) if return_index else ())
