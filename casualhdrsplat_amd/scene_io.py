"""Scene I/O either side of the rasterizer: Gaussian clouds as PLY in the layout every 3DGS
trainer and viewer exchanges, and COLMAP sparse reconstructions (the "SfM" arrow of
/root/reference/assets/pipeline.png) as initialisation.  Host-side numpy code, no GPU work -- except init_from_points(..., device="cuda"), whose
neighbour search is the library's (knn.py) --: the rasterizer takes the tensors these functions return.

PLY layout (binary little endian or ascii, one `vertex` element), properties in this order:
    x y z  nx ny nz  f_dc_0..2  f_rest_0..3*(M-1)-1  opacity  scale_0..2  rot_0..3
with f_rest stored CHANNEL-major (f_rest_{c*(M-1)+k} = coefficient k+1 of channel c), opacity as a logit, scales as
logs, rot as an un-normalised (w, x, y, z) quaternion -- i.e. the pre-activation parameters of the optimiser.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

SH_C0 = 0.28209479177387814

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


@dataclass
class GaussianCloud:
    """Pre-activation parameters as stored on disk."""
    means3D: torch.Tensor        # [P,3]
    shs: torch.Tensor            # [P,M,3]
    opacity_logit: torch.Tensor  # [P,1]
    log_scales: torch.Tensor     # [P,3]
    rotations: torch.Tensor      # [P,4] (w,x,y,z), not normalised

    @property
    def sh_degree(self) -> int:
        return int(round(math.sqrt(self.shs.shape[1]))) - 1

    def activated(self, device=None) -> Dict[str, torch.Tensor]:
        """The tensors GaussianRasterizer.forward takes: opacities = sigmoid, scales = exp, unit quaternions."""
        d = dict(means3D=self.means3D, shs=self.shs, opacities=torch.sigmoid(self.opacity_logit),
                 scales=torch.exp(self.log_scales),
                 rotations=self.rotations / self.rotations.norm(dim=1, keepdim=True).clamp_min(1e-12))
        return {k: (v.to(device) if device is not None else v).contiguous() for k, v in d.items()}

    def stored(self, device=None) -> Dict[str, torch.Tensor]:
        """The five tensors in the STORED parameterisation -- logit opacities, log scales, unnormalised quaternions -- under
        the argument names of optim.cloud_param_groups: what a trainer updates (optim.GaussianAdam), compacts
        (densify_and_prune, whose thresholds are compared in this space) and hands to
        GaussianRasterizer(..., parameterization="raw") as they are.  Detached copies on `device`; the caller sets
        requires_grad."""
        d = dict(means3D=self.means3D, opacities=self.opacity_logit, shs=self.shs, scales=self.log_scales,
                 rotations=self.rotations)
        return {k: v.detach().to(device=device, dtype=torch.float32).contiguous().clone() for k, v in d.items()}


def _property_names(M: int):
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)]
    names += [f"f_rest_{i}" for i in range(3 * (M - 1))]
    names += ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    return names


def _fused(cloud: GaussianCloud, filter_3D: torch.Tensor):
    """(opacity logits [P, 1], log scales [P, 3]) of the cloud with the 3D smoothing filter folded in (the published
    save_fused_ply): hs_smoothing_apply on the filter's device, then the inverse activations."""
    from .smoothing import apply_filter_3D
    dev = filter_3D.device
    P = cloud.means3D.shape[0]
    x = cloud.opacity_logit.detach().to(device=dev, dtype=torch.float32).reshape(P, 1).contiguous()
    l = cloud.log_scales.detach().to(device=dev, dtype=torch.float32).reshape(P, 3).contiguous()
    o, s = apply_filter_3D(x, l, filter_3D)
    return torch.log(o) - torch.log1p(-o), torch.log(s)


def save_ply(path: str, cloud: GaussianCloud, filter_3D: Optional[torch.Tensor] = None) -> None:
    """`filter_3D` (smoothing.compute_filter_3D's result, on the GPU): write the FUSED cloud -- scales sqrt(s^2 + f^2) and
    opacities o sqrt(prod s^2 / (s^2 + f^2)), as logs and logits -- so that an ordinary viewer draws what was trained."""
    opacity_logit, log_scales = (cloud.opacity_logit, cloud.log_scales) if filter_3D is None else _fused(cloud, filter_3D)
    m = cloud.means3D.detach().cpu().numpy().astype(np.float32)
    sh = cloud.shs.detach().cpu().numpy().astype(np.float32)
    P, M = sh.shape[0], sh.shape[1]
    cols = [m, np.zeros((P, 3), np.float32), sh[:, 0, :],
            np.transpose(sh[:, 1:, :], (0, 2, 1)).reshape(P, 3 * (M - 1)),  # channel-major rest
            opacity_logit.detach().cpu().numpy().astype(np.float32).reshape(P, 1),
            log_scales.detach().cpu().numpy().astype(np.float32),
            cloud.rotations.detach().cpu().numpy().astype(np.float32)]
    table = np.ascontiguousarray(np.concatenate(cols, axis=1), dtype="<f4")
    names = _property_names(M)
    assert table.shape[1] == len(names)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % P
    header += "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(table.tobytes())


def _read_ply_vertices(path: str) -> Dict[str, np.ndarray]:
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, count, props, in_vertex = None, None, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                if in_vertex:
                    in_vertex = False          # elements after `vertex` are ignored (they follow it in the body)
                elif tok[1] == "vertex":
                    in_vertex, count = True, int(tok[2])
                elif count is None:
                    raise ValueError(f"{path}: an element precedes `vertex`; not a Gaussian-cloud PLY")
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError(f"{path}: list property in the vertex element")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if count is None or fmt is None:
            raise ValueError(f"{path}: no vertex element / format line")
        if fmt == "ascii":
            rows = np.loadtxt(f, dtype=np.float64, max_rows=count, ndmin=2)
            if rows.shape != (count, len(props)):
                raise ValueError(f"{path}: expected {count}x{len(props)} ascii values, got {rows.shape}")
            return {n: rows[:, i] for i, (n, _) in enumerate(props)}
        if fmt not in ("binary_little_endian", "binary_big_endian"):
            raise ValueError(f"{path}: unsupported PLY format {fmt}")
        end = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(n, end + t) for n, t in props])
        raw = f.read(dt.itemsize * count)
        if len(raw) != dt.itemsize * count:
            raise ValueError(f"{path}: truncated vertex data")
        rec = np.frombuffer(raw, dtype=dt, count=count)
        return {n: rec[n] for n, _ in props}


def load_ply(path: str) -> GaussianCloud:
    v = _read_ply_vertices(path)
    for need in ("x", "y", "z", "f_dc_0", "opacity", "scale_0", "rot_0"):
        if need not in v:
            raise ValueError(f"{path}: property `{need}` missing; not a Gaussian-cloud PLY")
    P = v["x"].shape[0]
    nrest = sum(1 for k in v if k.startswith("f_rest_"))
    if nrest % 3:
        raise ValueError(f"{path}: {nrest} f_rest properties is not a multiple of 3")
    M = nrest // 3 + 1
    if int(round(math.sqrt(M))) ** 2 != M:
        raise ValueError(f"{path}: {M} SH coefficients per channel is not a square")

    def col(*names):
        return np.stack([np.asarray(v[n], np.float32) for n in names], axis=1)

    sh = np.zeros((P, M, 3), np.float32)
    sh[:, 0, :] = col("f_dc_0", "f_dc_1", "f_dc_2")
    if M > 1:
        rest = col(*[f"f_rest_{i}" for i in range(nrest)]).reshape(P, 3, M - 1)
        sh[:, 1:, :] = np.transpose(rest, (0, 2, 1))
    t = torch.from_numpy
    return GaussianCloud(t(col("x", "y", "z")), t(sh), t(col("opacity")), t(col("scale_0", "scale_1", "scale_2")),
                         t(col("rot_0", "rot_1", "rot_2", "rot_3")))


VQ_VERSION = 1


def save_vq(path: str, cloud: GaussianCloud, sh_codebook: torch.Tensor, sh_codes: torch.Tensor) -> None:
    """The cloud with its view-dependent SH coefficients replaced by codes into a shared codebook (vq.quantize_sh), as an
    uncompressed .npz written to exactly `path`: `version`; means3D [P,3], sh_dc [P,1,3], opacity_logit [P,1], log_scales [P,3],
    rotations [P,4] as little-endian fp32 with the bits they have; sh_codebook [K,M-1,3] fp32; sh_codes [P] as uint16.
    cloud.shs[:, 1:] is not written (only its DC term is): load_vq rebuilds it as sh_codebook[sh_codes]."""
    def f32(t):
        return np.ascontiguousarray(t.detach().cpu().numpy(), dtype="<f4")
    P = cloud.means3D.shape[0]
    book = f32(sh_codebook)
    codes = sh_codes.detach().cpu().numpy()
    if book.ndim != 3 or book.shape[2] != 3 or not (1 <= book.shape[0] <= 65536):
        raise ValueError(f"save_vq: sh_codebook must be [K <= 65536, M-1, 3], got {book.shape}")
    if book.shape[1] != cloud.shs.shape[1] - 1:
        raise ValueError(f"save_vq: sh_codebook holds {book.shape[1]} coefficients per entry, the cloud has {cloud.shs.shape[1]} - 1")
    if codes.shape != (P,) or codes.dtype.kind not in "iu":
        raise ValueError(f"save_vq: sh_codes must hold one integer code per Gaussian ({P}), got {codes.dtype} {codes.shape}")
    if P and (codes.min() < 0 or codes.max() >= book.shape[0]):
        raise ValueError(f"save_vq: sh_codes outside [0, {book.shape[0]})")
    with open(path, "wb") as f:
        np.savez(f, version=np.int32(VQ_VERSION), means3D=f32(cloud.means3D), sh_dc=f32(cloud.shs[:, :1, :]),
                 opacity_logit=f32(cloud.opacity_logit), log_scales=f32(cloud.log_scales), rotations=f32(cloud.rotations),
                 sh_codebook=book, sh_codes=codes.astype("<u2"))


def load_vq(path: str) -> GaussianCloud:
    """The cloud save_vq wrote, with shs = [sh_dc, sh_codebook[sh_codes]]."""
    with np.load(path) as z:
        if int(z["version"]) != VQ_VERSION:
            raise ValueError(f"{path}: version {int(z['version'])}, this reader knows {VQ_VERSION}")
        book, codes = z["sh_codebook"], z["sh_codes"].astype(np.int64)
        if codes.size and codes.max() >= book.shape[0]:
            raise ValueError(f"{path}: a code outside the {book.shape[0]} codebook entries")
        shs = np.concatenate([z["sh_dc"], book[codes]], axis=1).astype(np.float32)
        t = lambda name: torch.from_numpy(z[name].astype(np.float32))
        return GaussianCloud(t("means3D"), torch.from_numpy(shs), t("opacity_logit"), t("log_scales"), t("rotations"))


# ------------------------------------------------------------------------------------------- triangle meshes
def _host(x, dtype) -> np.ndarray:
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x), dtype=dtype)


def save_mesh_ply(path: str, vertices, faces, colors=None) -> None:
    """A triangle mesh (tsdf.TSDFVolume.extract_mesh) as binary little-endian PLY, the layout mesh viewers read: element
    vertex (float x y z[, uchar red green blue]) and element face (list uchar int vertex_indices).  vertices [V, 3] float,
    faces [T, 3] integer, colors [V, 3] float or None: clamped to [0, 1] (a NaN: 0) and stored as round(255 c)."""
    v, f = _host(vertices, "<f4"), _host(faces, "<i4")
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"save_mesh_ply: vertices must be [V, 3] and faces [T, 3], got {v.shape} and {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"save_mesh_ply: a face index outside the {v.shape[0]} vertices")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        c = _host(colors, np.float64)
        if c.shape != v.shape:
            raise ValueError(f"save_mesh_ply: colors must be {list(v.shape)}, got {c.shape}")
        rgb = np.floor(np.clip(np.nan_to_num(c, nan=0.0), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vt = np.empty(v.shape[0], dtype=np.dtype(fields))
    for i, n in enumerate("xyz"):
        vt[n] = v[:, i]
    if colors is not None:
        for i, n in enumerate(("red", "green", "blue")):
            vt[n] = rgb[:, i]
    ft = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    ft["n"] = 3
    ft["i"] = f
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % v.shape[0]
    header += "".join(f"property {'float' if t == '<f4' else 'uchar'} {n}\n" for n, t in fields)
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % f.shape[0]
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(vt.tobytes())
        out.write(ft.tobytes())


def load_mesh_ply(path: str):
    """(vertices [V, 3] float32, faces [T, 3] int32, colors [V, 3] uint8 or None) of a file save_mesh_ply wrote."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        lines = []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated PLY header")
            lines.append(line.decode("ascii", "replace").split())
            if lines[-1] == ["end_header"]:
                break
        body = f.read()
    lines = [t for t in lines if t and t[0] != "comment"]
    counts = {t[1]: int(t[2]) for t in lines if t[0] == "element"}
    plain = [t[2] for t in lines if t[0] == "property" and t[1] != "list"]
    if (["format", "binary_little_endian", "1.0"] not in lines or list(counts) != ["vertex", "face"] or
            plain not in (["x", "y", "z"], ["x", "y", "z", "red", "green", "blue"]) or
            ["property", "list", "uchar", "int", "vertex_indices"] not in lines):
        raise ValueError(f"{path}: not a mesh PLY in the layout of save_mesh_ply")
    fields = [(n, "<f4") for n in "xyz"] + [(n, "u1") for n in plain[3:]]
    vdt, fdt = np.dtype(fields), np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    V, T = counts["vertex"], counts["face"]
    if len(body) != V * vdt.itemsize + T * fdt.itemsize:
        raise ValueError(f"{path}: {len(body)} bytes of data, the header announces {V * vdt.itemsize + T * fdt.itemsize}")
    vt = np.frombuffer(body, dtype=vdt, count=V)
    ft = np.frombuffer(body, dtype=fdt, count=T, offset=V * vdt.itemsize)
    if T and not (ft["n"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    vertices = np.stack([vt["x"], vt["y"], vt["z"]], 1).astype(np.float32) if V else np.zeros((0, 3), np.float32)
    colors = (np.stack([vt[n] for n in plain[3:]], 1) if V else np.zeros((0, 3), np.uint8)) if len(plain) == 6 else None
    return vertices, ft["i"].astype(np.int32).reshape(T, 3), colors


# ------------------------------------------------------------------------------------------- COLMAP sparse models
_CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5),
                  4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5),
                  8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
_MODEL_PARAMS = {name: n for name, n in _CAMERA_MODELS.values()}


@dataclass
class ColmapCamera:
    id: int
    model: str
    width: int
    height: int
    params: np.ndarray

    def focal(self) -> Tuple[float, float]:
        if self.model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE"):
            return float(self.params[0]), float(self.params[0])
        return float(self.params[0]), float(self.params[1])


@dataclass
class ColmapImage:
    id: int
    qvec: np.ndarray   # (w, x, y, z), world-to-camera rotation
    tvec: np.ndarray   # world-to-camera translation
    camera_id: int
    name: str


def _unpack(f, fmt):
    n = struct.calcsize(fmt)
    b = f.read(n)
    if len(b) != n:
        raise ValueError("truncated COLMAP binary file")
    return struct.unpack(fmt, b)


def read_points3D(path: str):
    """points3D.txt / points3D.bin -> (xyz float64 [N,3], rgb uint8 [N,3], reprojection error float64 [N])."""
    xyz, rgb, err = [], [], []
    if path.endswith(".txt"):
        with open(path) as f:
            for line in f:
                line = line.strip()
                if not line or line[0] == "#":
                    continue
                t = line.split()
                xyz.append([float(t[1]), float(t[2]), float(t[3])])
                rgb.append([int(t[4]), int(t[5]), int(t[6])])
                err.append(float(t[7]))
    else:
        with open(path, "rb") as f:
            (n,) = _unpack(f, "<Q")
            for _ in range(n):
                _id, x, y, z, r, g, b, e, track = _unpack(f, "<QdddBBBdQ")
                f.seek(8 * track, 1)
                xyz.append([x, y, z]); rgb.append([r, g, b]); err.append(e)
    return (np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(rgb, np.uint8).reshape(-1, 3),
            np.asarray(err, np.float64))


def read_cameras(path: str) -> Dict[int, ColmapCamera]:
    cams = {}
    if path.endswith(".txt"):
        with open(path) as f:
            for line in f:
                line = line.strip()
                if not line or line[0] == "#":
                    continue
                t = line.split()
                cams[int(t[0])] = ColmapCamera(int(t[0]), t[1], int(t[2]), int(t[3]), np.asarray(t[4:], np.float64))
    else:
        with open(path, "rb") as f:
            (n,) = _unpack(f, "<Q")
            for _ in range(n):
                cid, model_id, w, h = _unpack(f, "<iiQQ")
                name, npar = _CAMERA_MODELS[model_id]
                cams[cid] = ColmapCamera(cid, name, int(w), int(h), np.asarray(_unpack(f, "<" + "d" * npar), np.float64))
    for c in cams.values():
        if c.model not in _MODEL_PARAMS or len(c.params) != _MODEL_PARAMS[c.model]:
            raise ValueError(f"camera {c.id}: model {c.model} with {len(c.params)} parameters")
    return cams


def read_images(path: str) -> Dict[int, ColmapImage]:
    ims = {}
    if path.endswith(".txt"):
        with open(path) as f:
            lines = [ln.rstrip("\n") for ln in f if not ln.startswith("#")]
        # two lines per image; the second (2-D points) may be empty
        i = 0
        while i < len(lines):
            if not lines[i].strip():
                i += 1
                continue
            t = lines[i].split()
            ims[int(t[0])] = ColmapImage(int(t[0]), np.asarray(t[1:5], np.float64), np.asarray(t[5:8], np.float64),
                                         int(t[8]), " ".join(t[9:]))
            i += 2
    else:
        with open(path, "rb") as f:
            (n,) = _unpack(f, "<Q")
            for _ in range(n):
                iid, qw, qx, qy, qz, tx, ty, tz, cid = _unpack(f, "<idddddddi")
                name = b""
                while True:
                    ch = f.read(1)
                    if ch in (b"\x00", b""):
                        break
                    name += ch
                (npts,) = _unpack(f, "<Q")
                f.seek(24 * npts, 1)
                ims[iid] = ColmapImage(iid, np.array([qw, qx, qy, qz]), np.array([tx, ty, tz]), cid, name.decode("utf-8"))
    return ims


def qvec_to_rotmat(q: np.ndarray) -> np.ndarray:
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def colmap_view(image: ColmapImage, camera: ColmapCamera, znear: float = 0.01, zfar: float = 100.0):
    """(viewmatrix, projmatrix, campos, tanfovx, tanfovy) in the rasterizer's transposed convention."""
    from .synthetic import projection_matrix
    R, t = qvec_to_rotmat(image.qvec), image.tvec
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, t
    fx, fy = camera.focal()
    tanfovx, tanfovy = camera.width / (2.0 * fx), camera.height / (2.0 * fy)
    V = torch.from_numpy(w2c.T.copy())                               # transposed: row-vector convention
    full = V @ projection_matrix(znear, zfar, tanfovx, tanfovy).t()  # (proj @ w2c)^T
    campos = torch.from_numpy(-R.T @ t).float()
    return V.float().contiguous(), full.float().contiguous(), campos, tanfovx, tanfovy


def _init_from_points_gpu(xyz, rgb, sh_degree: int, initial_opacity: float, device) -> GaussianCloud:
    """init_from_points on a CUDA device: the neighbour distances from knn.knn_mean_dist2 (fp32, HIP), everything else as
    on the host path -- the floor, log sqrt and the colour in float64, rounded to float32 once."""
    from .knn import knn_mean_dist2
    device = torch.device(device)
    pts = (xyz.detach() if isinstance(xyz, torch.Tensor) else torch.from_numpy(np.asarray(xyz)))
    pts = pts.to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
    P = pts.shape[0]
    M = (sh_degree + 1) ** 2
    d2 = knn_mean_dist2(pts).double() if P > 1 else torch.ones(P, dtype=torch.float64, device=device)
    log_s = torch.log(torch.sqrt(torch.clamp_min(d2, 1e-7)))
    col = (rgb.detach().to(device) if isinstance(rgb, torch.Tensor) else torch.from_numpy(np.asarray(rgb)).to(device))
    sh = torch.zeros(P, M, 3, dtype=torch.float32, device=device)
    sh[:, 0, :] = ((col.double().reshape(-1, 3) / 255.0 - 0.5) / SH_C0).float()
    rot = torch.zeros(P, 4, dtype=torch.float32, device=device)
    rot[:, 0] = 1.0
    logit = math.log(initial_opacity / (1.0 - initial_opacity))
    return GaussianCloud(pts, sh, torch.full((P, 1), logit, dtype=torch.float32, device=device),
                         log_s[:, None].repeat(1, 3).float().contiguous(), rot)


def init_from_points(xyz, rgb, sh_degree: int = 3, initial_opacity: float = 0.1, device=None) -> GaussianCloud:
    """The published SfM initialisation: SH DC from the point colour, isotropic scale = distance scale of the three
    nearest neighbours (sqrt of the mean squared distance, floored at 1e-7), identity rotation, opacity 0.1.
    `device`: None (and host inputs) = on the host with scipy's k-d tree, CPU tensors; a CUDA device, or CUDA tensor
    inputs, = the neighbour search in HIP (knn.knn_mean_dist2) and the cloud on that device, without scipy."""
    if device is None:
        device = next((t.device for t in (xyz, rgb) if isinstance(t, torch.Tensor) and t.device.type == "cuda"), None)
    if device is not None and torch.device(device).type == "cuda":
        return _init_from_points_gpu(xyz, rgb, sh_degree, initial_opacity, device)
    from scipy.spatial import cKDTree
    xyz = np.asarray(xyz, np.float64)
    P = xyz.shape[0]
    M = (sh_degree + 1) ** 2
    k = min(4, P)
    if k > 1:
        d, _ = cKDTree(xyz).query(xyz, k=k)
        d2 = np.mean(d[:, 1:] ** 2, axis=1)
    else:
        d2 = np.ones(P)
    log_s = np.log(np.sqrt(np.maximum(d2, 1e-7)))
    sh = np.zeros((P, M, 3), np.float32)
    sh[:, 0, :] = (np.asarray(rgb, np.float64) / 255.0 - 0.5) / SH_C0
    rot = np.zeros((P, 4), np.float32)
    rot[:, 0] = 1.0
    logit = math.log(initial_opacity / (1.0 - initial_opacity))
    t = torch.from_numpy
    return GaussianCloud(t(xyz.astype(np.float32)), t(sh), torch.full((P, 1), logit, dtype=torch.float32),
                         t(np.repeat(log_s[:, None], 3, axis=1).astype(np.float32)), t(rot))
