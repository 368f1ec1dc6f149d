"""Numpy restatement of the mesh clean-up by connected components (mesh.hip; the definitions of include/hdrsplat.h), sequential:
a plain union-find over the vertices, face by face, then the selection and the compaction as the header words them.  Everything
is integer or a copy, so the GPU tests compare with ==.  tests/test_mesh.py holds this file to an independent witness (scipy's
connected_components) and to closed forms."""
import numpy as np

f32 = np.float32


def valid_faces(faces, n_vertices):
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    return ((f >= 0) & (f < n_vertices)).all(1)


def components(faces, n_vertices):
    """(label [T] int32, size [T] int32): the smallest vertex index of every face's component and the component's number of
    valid faces; -1 and 0 for a face with an index outside [0, n_vertices)."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    ok = valid_faces(f, n_vertices)
    parent = list(range(n_vertices))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in f[ok].tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)      # the root is the tree's minimum
    root = np.array([find(v) for v in range(n_vertices)], np.int64).reshape(-1)
    label = np.full(f.shape[0], -1, np.int64)
    label[ok] = root[f[ok, 0]]
    count = np.bincount(label[ok], minlength=max(n_vertices, 1))
    size = np.zeros(f.shape[0], np.int64)
    size[ok] = count[label[ok]]
    return label.astype(np.int32), size.astype(np.int32)


def degenerate_faces(vertices, faces):
    """per VALID face (the caller masks): two equal indices, or two corners equal in all three coordinates with fp32 =="""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    v = np.asarray(vertices, f32)
    out = np.zeros(f.shape[0], bool)
    for i, j in ((0, 1), (1, 2), (0, 2)):
        out |= f[:, i] == f[:, j]
        out |= (v[f[:, i]] == v[f[:, j]]).all(1)
    return out


def clean(vertices, faces, colors=None, min_faces=0, keep_largest=None, remove_degenerate=True, label_size=None):
    """(label_size: components(faces, V) when the caller has it already)  dict(vertices, faces, colors, vertex_index, face_index, totals = (V', T', components, invalid faces), kept_labels)."""
    v = np.asarray(vertices, f32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    V = v.shape[0]
    ok = valid_faces(f, V)
    label, size = components(f, V) if label_size is None else label_size
    labels, first = np.unique(label[ok], return_index=True)
    sizes = size[ok][first]
    order = sorted(range(labels.size), key=lambda i: (-int(sizes[i]), int(labels[i])))
    if keep_largest is not None:
        order = order[:min(keep_largest, len(order))]
    kept_labels = [int(labels[i]) for i in order if sizes[i] >= min_faces]
    keep = ok & np.isin(label, np.array(kept_labels, np.int64))
    if remove_degenerate:
        deg = np.zeros(f.shape[0], bool)
        deg[ok] = degenerate_faces(v, f[ok])
        keep &= ~deg
    face_index = np.nonzero(keep)[0].astype(np.int32)
    used = np.zeros(V, bool)
    used[f[keep].reshape(-1)] = True
    vertex_index = np.nonzero(used)[0].astype(np.int32)
    new = np.full(V, -1, np.int32)
    new[vertex_index] = np.arange(vertex_index.size, dtype=np.int32)
    return dict(vertices=v[vertex_index], faces=new[f[keep].astype(np.int64)].reshape(-1, 3).astype(np.int32),
                colors=None if colors is None else np.asarray(colors, f32)[vertex_index],
                vertex_index=vertex_index, face_index=face_index,
                totals=(int(vertex_index.size), int(face_index.size), int(labels.size), int((~ok).sum())), kept_labels=kept_labels)
