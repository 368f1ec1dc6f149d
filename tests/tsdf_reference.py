"""The TSDF kernels (csrc/tsdf.hip: hs_tsdf_integrate, hs_tsdf_mesh_plan, hs_tsdf_mesh_emit) restated in numpy float32: the
operation order stated at the top of tsdf.hip, one rounded operation per numpy operation, so that the GPU tests can compare
bit for bit.  The integration here has NO brick cull: every sample visits every frame.  tests/test_tsdf.py holds this file to
closed forms (a plane, a sphere); tests/test_tsdf_gpu.py holds the kernels to this file."""
import numpy as np

f32 = np.float32

# lattice direction (dx, dy, dz) of edge number e, owned by the lower end
EDGE_DIR = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
DIR_EDGE = np.array([0, 0, 1, 3, 2, 4, 5, 6])          # direction bits (x = 1, y = 2, z = 4) -> edge number
# cell corners (bits) of the corners 0 .. 3 of tetrahedron t: 000 -> e_a -> e_a + e_b -> 111, permutations in lexicographic order
TET_CORNER = np.array([[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]])
TET_ODD = (False, True, True, False, False, True)
TET_EDGE = np.array([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]])
# case (bit m: corner m inside) -> triangles, tetrahedron edges of each: positively oriented tetrahedron, normal to the outside
TET_TRI = np.array([
    [0, 0, 0, 0, 0, 0, 0], [1, 0, 1, 2, 0, 0, 0], [1, 0, 4, 3, 0, 0, 0], [2, 1, 2, 4, 1, 4, 3],
    [1, 1, 3, 5, 0, 0, 0], [2, 0, 5, 2, 0, 3, 5], [2, 0, 4, 5, 0, 5, 1], [1, 2, 4, 5, 0, 0, 0],
    [1, 2, 5, 4, 0, 0, 0], [2, 0, 1, 5, 0, 5, 4], [2, 0, 5, 3, 0, 2, 5], [1, 1, 5, 3, 0, 0, 0],
    [2, 1, 3, 4, 1, 4, 2], [1, 0, 3, 4, 0, 0, 0], [1, 0, 2, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0]])


def lattice(o, h, n):
    """o + h * i for i = 0 .. n-1 in float32 (one product, one sum)"""
    return (f32(o) + f32(h) * np.arange(n, dtype=f32)).astype(f32)


def empty_volume(dims, color=False):
    nx, ny, nz = dims
    return dict(tsdf=np.ones((nz, ny, nx), f32), weight=np.zeros((nz, ny, nx), f32),
                color=np.zeros((3, nz, ny, nx), f32) if color else None)


def projects_inside(dims, origin, voxel_size, view, fx, fy, H, W):
    """[nz, ny, nx] bool: the samples that pass zc > 0 and the bounds test in one frame (the two tests a brick can fail as a whole)"""
    nx, ny, nz = dims
    h, fx, fy, V = f32(voxel_size), f32(fx), f32(fy), view.astype(f32)
    px = lattice(origin[0], h, nx)[None, None, :]
    py = lattice(origin[1], h, ny)[None, :, None]
    pz = lattice(origin[2], h, nz)[:, None, None]
    with np.errstate(all="ignore"):
        xc = ((px * V[0, 0] + py * V[1, 0]) + pz * V[2, 0]) + V[3, 0]
        yc = ((px * V[0, 1] + py * V[1, 1]) + pz * V[2, 1]) + V[3, 1]
        zc = ((px * V[0, 2] + py * V[1, 2]) + pz * V[2, 2]) + V[3, 2]
        u = fx * (xc / zc) + f32(0.5) * f32(W)
        v = fy * (yc / zc) + f32(0.5) * f32(H)
    return (zc > 0) & (u >= 0) & (u < f32(W)) & (v >= 0) & (v < f32(H))


def integrate(vol, origin, voxel_size, trunc, invdepth, viewmatrices, fx, fy, alpha=None, color=None, min_alpha=0.5,
              max_depth=np.inf, stats=None):
    """A new volume dict: `vol` after the frames, visited in order.  `stats` (a dict): how many (sample, frame) pairs left the
    walk at each test -- what a test uses to show its input exercises every branch."""
    tsdf, weight = vol["tsdf"].copy(), vol["weight"].copy()
    col = None if vol["color"] is None else vol["color"].copy()
    nz, ny, nx = tsdf.shape
    F, H, W = invdepth.shape
    h, trunc, fx, fy = f32(voxel_size), f32(trunc), f32(fx), f32(fy)
    px = lattice(origin[0], h, nx)[None, None, :]
    py = lattice(origin[1], h, ny)[None, :, None]
    pz = lattice(origin[2], h, nz)[:, None, None]
    halfW, halfH, Wf, Hf = f32(0.5) * f32(W), f32(0.5) * f32(H), f32(W), f32(H)
    count = lambda key, m: stats.__setitem__(key, stats.get(key, 0) + int(m.sum())) if stats is not None else None
    with np.errstate(all="ignore"):
        for f in range(F):
            V = viewmatrices[f].astype(f32)
            xc = ((px * V[0, 0] + py * V[1, 0]) + pz * V[2, 0]) + V[3, 0]
            yc = ((px * V[0, 1] + py * V[1, 1]) + pz * V[2, 1]) + V[3, 1]
            zc = ((px * V[0, 2] + py * V[1, 2]) + pz * V[2, 2]) + V[3, 2]
            live = zc > 0
            count("behind", ~live)
            u = fx * (xc / zc) + halfW
            v = fy * (yc / zc) + halfH
            inb = (u >= 0) & (u < Wf) & (v >= 0) & (v < Hf)
            count("outside", live & ~inb)
            live = live & inb
            ix = np.where(live, u, 0).astype(np.int32)
            iy = np.where(live, v, 0).astype(np.int32)
            d = invdepth[f][iy, ix]
            a = alpha[f][iy, ix] if alpha is not None else np.ones_like(d)
            valid = np.isfinite(d) & (d > 0) & np.isfinite(a) & (a > 0) & (a >= f32(min_alpha))
            count("invalid", live & ~valid)
            live = live & valid
            depth = a / d
            near = depth <= f32(max_depth)
            count("far", live & ~near)
            live = live & near
            sdf = depth - zc
            count("occluded", live & (sdf < -trunc))
            live = live & ~(sdf < -trunc)
            t = sdf / trunc
            count("clamped", live & (t > 1))
            t = np.where(t > 1, f32(1), t)
            count("fused", live)
            w1 = weight + f32(1)
            tsdf = np.where(live, (tsdf * weight + t) / w1, tsdf)
            if col is not None:
                for c in range(3):
                    col[c] = np.where(live, (col[c] * weight + color[f, c][iy, ix]) / w1, col[c])
            weight = np.where(live, w1, weight)
    return dict(tsdf=tsdf.astype(f32), weight=weight.astype(f32), color=col)


def extract_mesh(vol, origin, voxel_size, min_weight=1.0):
    """(vertices [V, 3] float32, faces [T, 3] int32, colors [V, 3] float32 or None) in the kernels' order; empty when T = 0.
    Also returned: a dict with V and T as counted (before the T = 0 rule) and the flat (cell, tetrahedron) of every face."""
    tsdf, weight, col = vol["tsdf"], vol["weight"], vol["color"]
    nz, ny, nx = tsdf.shape
    h = f32(voxel_size)
    obs = weight >= f32(min_weight)
    ins = tsdf < 0
    has = np.zeros((nz, ny, nx, 7), bool)
    for e, (dx, dy, dz) in enumerate(EDGE_DIR):
        A = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        B = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        has[A + (e,)] = obs[A] & obs[B] & (ins[A] != ins[B])
    flat = has.reshape(-1)                                      # index 7 q + e
    vid = np.cumsum(flat, dtype=np.int64) - 1
    sel = np.nonzero(flat)[0]
    q, e = sel // 7, sel % 7
    i, j, k = q % nx, (q // nx) % ny, q // (nx * ny)
    dirs = np.array(EDGE_DIR)
    other = q + dirs[e, 0] + dirs[e, 1] * nx + dirs[e, 2] * nx * ny
    tf = tsdf.reshape(-1)
    with np.errstate(all="ignore"):
        a, b = tf[q], tf[other]
        s = a / (a - b)
        vertices = np.empty((sel.size, 3), f32)
        for c, idx in enumerate((i, j, k)):
            pa = f32(origin[c]) + h * idx.astype(f32)
            pb = f32(origin[c]) + h * (idx + dirs[e, c]).astype(f32)
            vertices[:, c] = pa + s * (pb - pa)
        colors = None
        if col is not None:
            cf = col.reshape(3, -1)
            colors = np.stack([cf[c][q] + s * (cf[c][other] - cf[c][q]) for c in range(3)], 1).astype(f32)

    K, J, I = nz - 1, ny - 1, nx - 1
    corner = lambda arr, c: arr[(c >> 2):(c >> 2) + K, ((c >> 1) & 1):((c >> 1) & 1) + J, (c & 1):(c & 1) + I]
    kk, jj, ii = np.meshgrid(np.arange(K), np.arange(J), np.arange(I), indexing="ij")
    qcell = (kk * ny + jj) * nx + ii
    offset = np.array([(c & 1) + ((c >> 1) & 1) * nx + (c >> 2) * nx * ny for c in range(8)])
    idx_all = np.zeros((K, J, I, 6, 2, 3), np.int64)
    emit = np.zeros((K, J, I, 6, 2), bool)
    for t in range(6):
        cs = TET_CORNER[t]
        allobs = corner(obs, cs[0]) & corner(obs, cs[1]) & corner(obs, cs[2]) & corner(obs, cs[3])
        code = sum(corner(ins, cs[m]).astype(np.int64) << m for m in range(4)) * allobs
        for r in range(2):
            emit[..., t, r] = TET_TRI[code, 0] > r
            for c in range(3):
                te = TET_TRI[code, 1 + 3 * r + c]
                ca, cb = cs[TET_EDGE[te, 0]], cs[TET_EDGE[te, 1]]
                got = vid[(qcell + offset[ca]) * 7 + DIR_EDGE[cb ^ ca]]
                idx_all[..., t, r, (c if c == 0 or not TET_ODD[t] else 3 - c)] = got
    keep = emit.reshape(-1)
    faces = idx_all.reshape(-1, 3)[keep].astype(np.int32)
    where = np.nonzero(keep)[0] // 2                            # 6 cell + t
    info = dict(V=int(sel.size), T=int(faces.shape[0]), face_cell_tet=where, cell_q=qcell.reshape(-1))
    if faces.shape[0] == 0:
        return np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), (None if col is None else np.zeros((0, 3), f32)), info
    return vertices, faces, colors, info
