#!/usr/bin/env python3
"""The mesh clean-up by connected components (casualhdrsplat_amd.mesh.clean_mesh: hs_mesh_clean_plan, one host read,
hs_mesh_clean_emit) against what a pipeline does without it, alternated in one process on the same mesh:

  host    the copy of vertices and faces to the host, scipy.sparse.csgraph.connected_components, numpy compaction, the copy back
  torch   label propagation on the GPU in torch: labels = vertex indices, scatter_reduce(amin) over the faces' corners and one
          pointer jump (label = label[label]) per round to a fixed point (one host read per round), then masks and cumsum

    python scripts/time_mesh.py --out profiles/mesh_timing.json

Meshes: TSDFVolume.extract_mesh of a sphere of radius 1.2 in a cube of side 4 (the README's) at 256^3 and 512^3, with --floaters
small spheres (radius 2.2 voxels, 528 faces each) scattered outside it.  Selection: min_faces = 1000 -- the sphere stays,
every floater goes.  All three forms must return the same mesh (checked once, with ==).
Figures: plan and emit by device events around each call, clean_mesh and the two other forms by wall time around the call
ending in a synchronise; the median and the extremes over --iters calls after a warm-up, the forms alternated in --rounds
blocks.  hs_mesh_components (init, hook, flatten, sizes, write) is timed too: plan minus it is the flags, sums, scan and bases.
Byte model of plan + emit (hdrsplat.h): per face 4 reads of its 12 B (hook, sizes, keep, emit), 36 B of gathered corners
(the degenerate test), 12 B of flags and new indices, 12 B gathered new indices and 12 B written per kept face; per vertex
some 40 B of workspace traffic, 12 B read and 12 B written per kept vertex: model_bytes = 96 T + 40 V + 12 T' + 24 V';
model_GBps = that over plan + emit, frac_of_copy = that over the rate of a 1 GiB device copy (2 GiB moved) timed in the same
run.  The union-find's walks and atomics are NOT in the model: what the fraction falls short of is mostly them."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from casualhdrsplat_amd import TSDFVolume, clean_mesh
from casualhdrsplat_amd import _lib as L

SIDE, RADIUS, FLOATER_CELLS, MIN_FACES = 4.0, 1.2, 2.2, 1000
COPY_BYTES = 1 << 30


def timed(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def walled(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), calls=len(ms))


def copy_rate(dev, iters=20):
    src = torch.empty(COPY_BYTES, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    ms = statistics.median(timed(lambda: dst.copy_(src), iters, warmup=3))
    return 2 * COPY_BYTES / (ms * 1e-3) / 1e9, ms


def sphere_with_floaters(n, floaters, dev):
    """(vertices, faces) of extract_mesh: the sphere and `floaters` small spheres at seeded places outside it, none touching"""
    h = SIDE / (n - 1)
    vol = TSDFVolume((-SIDE / 2,) * 3, h, (n, n, n), device=dev)
    axis = -SIDE / 2 + h * torch.arange(n, device=dev, dtype=torch.float32)
    dist = (axis[None, None, :] ** 2 + axis[None, :, None] ** 2 + axis[:, None, None] ** 2).sqrt() - RADIUS
    rng = np.random.default_rng(1)
    axis_h = axis.cpu().numpy().astype(np.float64)
    cell = 12                                                       # one floater per 12^3 cells at most: they cannot touch
    slots = rng.permutation((n // cell) ** 3)
    placed = 0
    r = FLOATER_CELLS * h
    for s in slots:
        if placed == floaters:
            break
        i, j, k = (int(x) * cell + cell // 2 for x in np.unravel_index(s, (n // cell,) * 3))
        c = [axis_h[i] + 0.3 * h, axis_h[j] - 0.2 * h, axis_h[k] + 0.1 * h]
        if float(np.linalg.norm(c)) - RADIUS < 8 * h:               # inside the sphere or too near it
            continue
        sl = [slice(x - 5, x + 6) for x in (i, j, k)]
        d = ((axis[sl[0]][None, None, :] - c[0]) ** 2 + (axis[sl[1]][None, :, None] - c[1]) ** 2 +
             (axis[sl[2]][:, None, None] - c[2]) ** 2).sqrt() - r
        part = dist[sl[2], sl[1], sl[0]]
        part.copy_(torch.minimum(part, d))
        placed += 1
    vol.tsdf.copy_((dist / vol.trunc).clamp(-1, 1))
    vol.weight.fill_(1.0)
    del dist
    v, f = vol.extract_mesh()
    return v, f, placed


def host_clean(v, f, min_faces):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    vh, fh = v.cpu().numpy(), f.cpu().numpy().astype(np.int64)
    V = vh.shape[0]
    rows, cols = np.concatenate([fh[:, 0], fh[:, 1]]), np.concatenate([fh[:, 1], fh[:, 2]])
    _, comp = connected_components(coo_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(V, V)), directed=False)
    of_face = comp[fh[:, 0]]
    keep = np.bincount(of_face)[of_face] >= min_faces
    keep &= ~((vh[fh[:, 0]] == vh[fh[:, 1]]).all(1) | (vh[fh[:, 1]] == vh[fh[:, 2]]).all(1) | (vh[fh[:, 0]] == vh[fh[:, 2]]).all(1))
    used = np.zeros(V, bool)
    used[fh[keep].reshape(-1)] = True
    new = np.cumsum(used) - 1
    return (torch.from_numpy(vh[used]).to(v.device), torch.from_numpy(new[fh[keep]].astype(np.int32)).to(v.device))


def torch_clean(v, f, min_faces, rounds_out=None):
    V = v.shape[0]
    fl = f.long()
    label = torch.arange(V, device=v.device)
    corners = fl.reshape(-1)
    rounds = 0
    while True:
        m = label[fl].amin(1)
        new = label.scatter_reduce(0, corners, m.repeat_interleave(3), "amin")
        new = new[new]
        rounds += 1
        if torch.equal(new, label):                                 # (the host read of the round)
            break
        label = new
    of_face = label[fl[:, 0]]
    keep = torch.bincount(of_face, minlength=V)[of_face] >= min_faces
    a, b, c = v[fl[:, 0]], v[fl[:, 1]], v[fl[:, 2]]
    keep &= ~((a == b).all(1) | (b == c).all(1) | (a == c).all(1))
    used = torch.zeros(V, dtype=torch.bool, device=v.device)
    used[fl[keep].reshape(-1)] = True
    new_index = torch.cumsum(used, 0) - 1
    if rounds_out is not None:
        rounds_out.append(rounds)
    return v[used], new_index[fl[keep]].to(torch.int32)


class Abi:
    """plan, emit and components on preallocated buffers, so that each can be timed alone"""

    def __init__(self, v, f, min_faces):
        self.lib = L.load()
        dev = v.device
        V, T = v.shape[0], f.shape[0]
        self.keep = (v, f)
        self.ws = torch.empty(self.lib.hs_mesh_workspace_bytes(V, T), dtype=torch.uint8, device=dev)
        self.totals = torch.empty(4, dtype=torch.int64, device=dev)
        self.label = torch.empty(T, dtype=torch.int32, device=dev)
        self.size = torch.empty(T, dtype=torch.int32, device=dev)
        a = self.a = L.hs_mesh_args()
        a.n_vertices, a.n_faces, a.min_faces, a.keep_largest, a.remove_degenerate = V, T, min_faces, 0, 1
        a.vertices, a.faces, a.workspace, a.totals = v.data_ptr(), f.data_ptr(), self.ws.data_ptr(), self.totals.data_ptr()
        a.label, a.size = self.label.data_ptr(), self.size.data_ptr()
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.plan()
        self.Vo, self.To = self.totals.tolist()[:2]
        self.out_v = torch.empty((self.Vo, 3), device=dev)
        self.out_f = torch.empty((self.To, 3), dtype=torch.int32, device=dev)
        a.n_vertices_out, a.n_faces_out, a.vertices_out, a.faces_out = self.Vo, self.To, self.out_v.data_ptr(), self.out_f.data_ptr()

    def plan(self):
        L.check(self.lib.hs_mesh_clean_plan(C.byref(self.a), self.stream), "hs_mesh_clean_plan")

    def emit(self):
        L.check(self.lib.hs_mesh_clean_emit(C.byref(self.a), self.stream), "hs_mesh_clean_emit")

    def components(self):
        L.check(self.lib.hs_mesh_components(C.byref(self.a), self.stream), "hs_mesh_components")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--slow-iters", type=int, default=4, help="calls of the host and the torch form")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sizes", nargs="*", type=int, default=[256, 512])
    ap.add_argument("--floaters", type=int, default=3000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh.py measures on an MI355X: no GPU here, nothing is measured")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), min_faces=MIN_FACES, sizes={})
    gbps, copy_ms = copy_rate(dev)
    result["copy_1GiB"] = dict(median_ms=copy_ms, GBps=gbps)
    print(f"copy 1 GiB: {copy_ms:.3f} ms, {gbps:.0f} GB/s", flush=True)

    for n in a.sizes:
        v, f, placed = sphere_with_floaters(n, a.floaters, dev)
        V, T = v.shape[0], f.shape[0]
        abi = Abi(v, f, MIN_FACES)
        fused = lambda: clean_mesh(v, f, min_faces=MIN_FACES)
        host = lambda: host_clean(v, f, MIN_FACES)
        rounds = []
        plain = lambda: torch_clean(v, f, MIN_FACES, rounds)
        want = fused()
        same = all(torch.equal(x, y) for other in (host(), plain()) for x, y in zip(want, other))
        abi.plan()
        abi.emit()
        same = same and torch.equal(abi.out_v, want[0]) and torch.equal(abi.out_f, want[1])
        ms = {k: [] for k in ("plan", "emit", "components", "clean_mesh", "host", "torch")}
        per = max(a.iters // a.rounds, 1)
        slow = max(a.slow_iters // a.rounds, 1)
        for _ in range(a.rounds):
            ms["plan"] += timed(abi.plan, per)
            ms["emit"] += timed(abi.emit, per)
            ms["components"] += timed(abi.components, per)
            ms["clean_mesh"] += walled(fused, per)
            ms["host"] += walled(host, slow)
            ms["torch"] += walled(plain, slow)
        totals = abi.totals.tolist()
        model = 96 * T + 40 * V + 12 * abi.To + 24 * abi.Vo
        row = dict(samples=n ** 3, floaters=placed, V=V, T=T, V_clean=abi.Vo, T_clean=abi.To, n_components=totals[2],
                   same_mesh_from_all_forms=bool(same), torch_rounds=rounds[-1], model_bytes=model,
                   **{k: stats(x) for k, x in ms.items()})
        kernels = row["plan"]["median_ms"] + row["emit"]["median_ms"]
        row["model_GBps"] = model / (kernels * 1e-3) / 1e9
        row["frac_of_copy"] = row["model_GBps"] / gbps
        row["speedup_over_host"] = row["host"]["median_ms"] / row["clean_mesh"]["median_ms"]
        row["speedup_over_torch"] = row["torch"]["median_ms"] / row["clean_mesh"]["median_ms"]
        result["sizes"][f"{n}^3"] = row
        print(f"{n}^3", json.dumps(row), flush=True)
        del abi, v, f, want
        torch.cuda.empty_cache()

    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
