"""Results must not depend on what the workspaces held.

The library's contract is "kernels only, no memset" (include/hdrsplat.h): the caller hands hs_forward / hs_backward and the
other entry points workspaces and output tensors with ARBITRARY bytes in them, and the library writes every word before it
reads it, clears it in a kernel of its own, or treats it as empty through a per-call tag.  DESIGN.md section 4.21 is the
audit behind this module: for every region of hs_layout and every scratch buffer of hs_photometric_loss, hs_knn_*,
hs_mcmc_* and hs_densify_*, which kernel reads it first, which one clears / tags / fully writes it before, and for how many
words.  Here every such buffer is filled with a pattern (tests/poison.py) before the call, and every result is compared BIT
FOR BIT with the run whose buffers held zeros: no tolerance anywhere.

  * forward at the C ABI (test_forward_*): a finished forward's hs_fwd_args is copied, every workspace and output is owned
    and filled here, hs_forward is called with the sorts forced per call -- forms x patterns x frames that cross the extent
    boundaries of the scratch formulas (255 / 256 / 257 ... 2^18 instances, 4096 tiles, 16 poses, no Gaussian, no visible one,
    too small a capacity followed by the same frame at a sufficient one in the SAME bytes);
  * backward and the whole Python path under poison.poisoned (test_python_path_*): every buffer the Python layer allocates
    with torch.empty* is filled; outputs and every gradient; the records prove which buffers were filled;
  * the other entry points through their wrappers (test_entry_point_*);
  * calls of different shapes alternating on one rasterizer object, recycled memory as the allocator hands it out;
  * words that already carry the NEXT call's frame tag under the depth-bits words (hs_common.h, kDepthBitsAt), in a child
    process on libhdrsplat_test.so, which alone exports the tag.

Not compared (the header calls them scratch, or says who may leave what there): keys_sorted after a counting / hierarchical
tile sort, the 16-byte pads between the slices of the flat gradient buffer, sort_tmp / pair_sort_tmp / depth_ws / tile_matrix
/ hier_ws / pairs_tmp / depth_pairs, and of hs_counters the one timing-dependent field, reserved[4] (look-back helps: how
often a waiting workgroup did a silent predecessor's counting -- it depends on dispatch order).  Buffers the header makes
the CALLER initialise are never poisoned: Adam's state (all-zero = t 0), hs_render_stats' counters, the three densification
accumulators (DensifyStats: torch.zeros).

Forms left out because hs_plan gives them no workspace (hs_layout.tile_matrix / hier_ws empty): `count` and `hier` on the
frames without binning capacity -- "all_culled" (R = 0, hence capacity 0) and "p0" (no Gaussian at all); they run `auto`,
`radix`, `passes_tickets` and `scan_inside` (p0: `auto` only -- no sort runs at all).  LEFT_OUT below names them; the test
asserts that hs_plan agrees.
"""
import contextlib
import ctypes as C
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import helpers as Hh
import poison
from casualhdrsplat_amd import synthetic as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
RAST = "casualhdrsplat_amd.rasterizer"
_TEST_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "casualhdrsplat_amd", "libhdrsplat_test.so")


def _lib():
    from casualhdrsplat_amd import _lib as L
    return L, L.load()


@pytest.fixture(autouse=True)
def process_defaults_stay():
    """hs_depth_sort / hs_sort_tickets are what they were, and no frame reported ranges of the counting depth sort that left
    the chip (the host would warn and move the process to the look-back passes): poison must not make a frame slow either."""
    L, lib = _lib()
    before = (lib.hs_depth_sort(-1), lib.hs_sort_tickets(-1))
    seen, warn = [], warnings.warn

    def recording_warn(message, *args, **kwargs):
        seen.append(str(message))
        return warn(message, *args, **kwargs)

    mp = pytest.MonkeyPatch()
    mp.setattr(warnings, "warn", recording_warn)
    try:
        yield
    finally:
        mp.undo()
    assert (lib.hs_depth_sort(-1), lib.hs_sort_tickets(-1)) == before
    bad = [m for m in seen if "did not fit on chip" in m or "ticket-ordered" in m]
    assert not bad, bad


@contextlib.contextmanager
def environment(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def differing(got: dict, want: dict) -> list:
    """Keys whose bytes differ (or that only one side has), with the first differing element of each."""
    bad = []
    for k in sorted(set(got) | set(want)):
        if k not in got or k not in want:
            bad.append((k, "missing on one side"))
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append((k, a.shape, b.shape, str(a.dtype), str(b.dtype)))
        elif a.tobytes() != b.tobytes():
            ra, rb = a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)
            d = np.nonzero(ra != rb)[0]
            i = int(d[0]) // max(a.dtype.itemsize, 1)
            bad.append((k, f"{np.unique(d // max(a.dtype.itemsize, 1)).size} of {a.size} elements; first at {i}: "
                           f"{a.reshape(-1)[i]!r} != {b.reshape(-1)[i]!r}"))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the stale sources: whole steps whose buffers are kept as they were left
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stale_session(which):
    """A Session (keep=True) of one whole step whose buffers a later call inherits as they were LEFT.
    "large": another scene, more instances (300 000) and more tiles (1280 x 1040: 5200) than any frame below, the
    hierarchical tile sort and the look-back depth passes (the frames below run the counting forms by default);
    "t20k": the 20 000-Gaussian frame at 500 x 300 with its default sorts, forward and backward."""
    mp = pytest.MonkeyPatch()
    try:
        with poison.poisoned(mp, "zero", keep=True) as s:
            if which == "large":
                with environment(HS_TILE_SORT="hier", HS_DEPTH_SORT="lsd"):
                    g = Hh.run_hip(S.make_scene(300_000, 1280, 1040, 1, seed=41, hdr=True), hdr=True)
                assert int(g["state"]["tile_sort"]) == 2
            else:
                Hh.run_hip(S.make_scene(20000, 500, 300, 1, seed=3))
        torch.cuda.synchronize()
    finally:
        mp.undo()
    s.require(RAST, roles=("geom", "binning", "image", "bwd", "flat_gradients", "out_color", "radii"))
    return s


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward at the C ABI
# ---------------------------------------------------------------------------------------------------------------------
FORMS = ("radix", "count", "hier", "passes_tickets", "scan_inside", "auto")
BOUNDARY_I = (255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 262143, 262144, 262145)
FRAMES = ("p1", "p257") + tuple(f"i{n}" for n in BOUNDARY_I) + ("hdr16_ldrblur", "hdr16_hdrblur", "tiles4096", "all_culled", "p0")
LEFT_OUT = {("all_culled", "count"), ("all_culled", "hier")} | {("p0", f) for f in FORMS if f != "auto"}
FULL_PATTERNS = tuple(p for p in poison.PATTERNS if p != "zero")
# (ff, random and stale, plus nan: 0x7FC00000 is also a large POSITIVE integer -- a word that an atomicMax is meant to start
# from zero keeps it, where 0xFFFFFFFF = -1 loses to every radius and a random word does half of the time)
BOUNDARY_PATTERNS = ("ff", "nan", "random", "stale")


def _form_fields(L, form):
    return dict(radix=dict(tile_sort=L.HS_TILE_SORT_RADIX), count=dict(tile_sort=L.HS_TILE_SORT_COUNT),
                hier=dict(tile_sort=L.HS_TILE_SORT_HIER),
                passes_tickets=dict(tile_sort=L.HS_TILE_SORT_RADIX, depth_sort=L.HS_DEPTH_SORT_PASSES, chain_order=L.HS_CHAIN_TICKETS),
                scan_inside=dict(emission_scan=L.HS_EMISSION_SCAN_INSIDE), auto={})[form]


def _scene_of(name):
    """(scene, cameras or None, hdr, blur domain) of a frame of FRAMES / "t20k"."""
    if name == "t20k":
        return S.make_scene(20000, 500, 300, 1, seed=3), None, False, "ldr"
    if name == "p1":
        return S.make_scene(1, 16, 16, 1, seed=1), None, False, "ldr"
    if name == "p257":
        return S.make_scene(257, 16, 16, 1, seed=2), None, False, "ldr"
    if name.startswith("i"):
        n = int(name[1:])
        return S.make_scene(n, 320, 240, 0 if n > 100000 else 1, seed=n % 97), None, False, "ldr"
    if name.startswith("hdr16_"):
        return S.make_scene(700, 256, 256, 1, seed=7, hdr=True), S.blur_poses(256, 256, 16, step=0.01), True, name[6:9]
    if name == "tiles4096":     # 64 x 64 tiles: the most the counting tile sort takes, the hierarchical sort's 64 super-tiles
        return S.make_scene(3000, 1024, 1024, 1, seed=9), None, False, "ldr"
    if name == "all_culled":
        sc = S.make_scene(1000, 160, 120, 1, seed=4)
        sc.means3D[:, 2] = -sc.means3D[:, 2]      # everything behind the camera
        return sc, None, False, "ldr"
    if name == "p0":
        return S.make_scene(0, 64, 48, 1, seed=5), None, False, "ldr"
    raise KeyError(name)


class Frame:
    """A finished forward of one frame through the Python host (synchronous mode: capacity = R), kept as the template of
    hs_fwd_args, and the zero-filled run of every form, computed when first asked for."""

    def __init__(self, name):
        from casualhdrsplat_amd import GaussianRasterizer
        self.name = name
        sc, cams, hdr, dom = _scene_of(name)
        rs, _, _ = Hh.settings_from_scene(sc, DEV, cams, hdr=hdr, blur_domain=dom)
        self.inputs = [t.clone().to(DEV) for t in (sc.means3D, torch.zeros_like(sc.means3D), sc.opacities, sc.shs, sc.scales, sc.rotations)]
        rast = GaussianRasterizer(rs, keep_state=True)
        m, m2, o, sh, s_, r = self.inputs
        with torch.no_grad():
            self.out = rast(m, m2, o, shs=sh, scales=s_, rotations=r)
        self.rast, self.st = rast, rast._last["state"]
        torch.cuda.synchronize()
        self.R = int(self.st.num_rendered)
        self.hdr = hdr
        self.zero = {}

    # -- one hs_forward into buffers of our own --
    def buffers(self):
        st = self.st
        b = dict(geom=torch.zeros_like(st.geom), binning=torch.zeros_like(st.binning), image=torch.zeros_like(st.image),
                 out_color=torch.zeros_like(self.out[0]), radii=torch.zeros_like(self.out[1]))
        if self.hdr:
            b["out_hdr"] = torch.zeros_like(self.out[2])
        return b

    def fill(self, bufs, pattern):
        stale = stale_session("large") if pattern == "stale" else None
        for i, (role, t) in enumerate(bufs.items()):
            src = stale.source_for(f"{RAST}:{role}")[1] if stale is not None else None
            poison.fill_(t, pattern, seed=i, stale=src)

    def enqueue(self, bufs, form, capacity=None):
        L, lib = _lib()
        a = L.hs_fwd_args.from_buffer_copy(self.st.fwd_args)
        a.geom, a.binning, a.image = bufs["geom"].data_ptr(), bufs["binning"].data_ptr(), bufs["image"].data_ptr()
        a.out_color, a.radii = bufs["out_color"].data_ptr(), bufs["radii"].data_ptr()
        a.out_hdr = bufs["out_hdr"].data_ptr() if self.hdr else None
        a.out_invdepth = a.counters_host = None
        a.stages = L.HS_STAGE_ALL
        if capacity is not None:
            a.dims.capacity = capacity
        a.tile_sort = a.depth_sort = a.chain_order = a.emission_scan = a.depth_range_cap = a.depth_dist_max = 0
        for k, v in _form_fields(L, form).items():
            setattr(a, k, v)
        L.check(lib.hs_forward(C.byref(a), torch.cuda.current_stream().cuda_stream), f"hs_forward[{self.name}, {form}]")
        return a

    def snapshot(self, bufs, a):
        """Everything the forward is answerable for, as numpy (module docstring: what is and is not compared)."""
        L, lib = _lib()
        torch.cuda.synchronize()
        d = a.dims
        sz, lay = L.hs_sizes(), L.hs_layout()
        L.check(lib.hs_plan(C.byref(d), C.byref(sz), C.byref(lay)), "hs_plan")
        assert sz.geom_bytes <= bufs["geom"].numel() and sz.binning_bytes <= bufs["binning"].numel() and sz.image_bytes <= bufs["image"].numel()
        I, HW = d.P * d.n_poses, d.W * d.H
        gx, gy = (d.W + 15) // 16, (d.H + 15) // 16
        vt = gx * gy * d.n_poses
        geom, binning, image = (bufs[k].cpu().numpy() for k in ("geom", "binning", "image"))

        def arr(buf, off, n, dt):
            return buf[off:off + n * np.dtype(dt).itemsize].view(dt).copy()

        ctr = arr(geom, lay.counters, 8, np.uint32)
        snap = {k: bufs[k].cpu().numpy() for k in ("out_color", "radii", "out_hdr") if k in bufs}
        snap["counters_but_helps"] = np.delete(ctr, 6)          # reserved[4] = look-back helps: timing-dependent
        R = int(ctr[2])                                         # reserved[0]: pairs actually binned (0 on overflow)
        snap["point_list"] = arr(binning, lay.point_list, R, np.uint32)
        ranges = arr(binning, lay.ranges, 2 * vt, np.uint32).reshape(vt, 2)
        snap["ranges"] = ranges
        snap["final_T"] = arr(image, lay.final_T, d.n_poses * HW, np.uint32)
        n_contrib = arr(image, lay.n_contrib, d.n_poses * HW, np.uint32)
        snap["n_contrib"] = n_contrib
        snap["tile_work"] = arr(image, lay.tile_work, vt, np.uint32)
        if vt <= 6 * 3072:                                      # (render.hip, orders_tiles: larger launches keep the strip order)
            snap["tile_order"] = arr(image, lay.tile_order, vt, np.uint32)
        F = max(d.n_frames, 1)
        if self.hdr or d.n_poses // F > 1:
            snap["pose_hdr"] = arr(image, lay.pose_hdr, (d.n_poses + (F if d.n_poses // F > 1 else 0)) * 3 * HW, np.uint32)
        # pair_act: the entries the render forward staged -- at least every entry up to the tile's deepest contributor
        # (n_contrib = position of a pixel's last contributor in its tile's list, 1-based), which is all the backward reads
        if R > 0:
            nc = n_contrib.reshape(d.n_poses, d.H, d.W).astype(np.int64)
            pad = np.zeros((d.n_poses, gy * 16, gx * 16), np.int64)
            pad[:, :d.H, :d.W] = nc
            deepest = pad.reshape(d.n_poses, gy, 16, gx, 16).max(axis=(2, 4)).reshape(vt)
            assert (deepest <= ranges[:, 1].astype(np.int64) - ranges[:, 0]).all()
            staged = np.zeros(R + 1, np.int64)
            np.add.at(staged, ranges[:, 0].astype(np.int64), 1)
            np.add.at(staged, ranges[:, 0].astype(np.int64) + deepest, -1)
            staged = np.cumsum(staged)[:R] > 0
            snap["pair_act_staged"] = arr(binning, lay.pair_act, R, np.uint8)[staged]
            snap["pair_flags"] = arr(binning, lay.pair_flags, R, np.uint8)     # cleared by the emission: the backward's segmented sum reads them
        # what the backward reads of the geometry / binning state next to the lists
        snap["rec"] = arr(geom, lay.rec, I * 16, np.uint32)
        snap["radii_inst"] = arr(geom, lay.radii, I, np.uint32)
        snap["tiles_touched"] = arr(geom, lay.tiles_touched, I, np.uint32)
        snap["clamped"] = arr(geom, lay.clamped, I, np.uint8)
        if int(ctr[1]) < 2:
            snap["inst_sorted"] = arr(binning, lay.inst_sorted, I, np.uint32)
        snap["offs_sorted"] = arr(binning, lay.offs_sorted, I, np.uint32)
        return snap, ctr

    def zero_run(self, form):
        if form not in self.zero:
            bufs = self.buffers()
            self.fill(bufs, "zero")
            self.zero[form] = self.snapshot(bufs, self.enqueue(bufs, form))
        return self.zero[form]

    def fits(self, form):
        """Does hs_plan give the form's workspace at this frame's dims (capacity = R)?"""
        L, lib = _lib()
        sz, lay = L.hs_sizes(), L.hs_layout()
        L.check(lib.hs_plan(C.byref(self.st.dims), C.byref(sz), C.byref(lay)), "hs_plan")
        if form == "count":
            return lay.hier_ws > lay.tile_matrix
        if form == "hier":
            return sz.binning_bytes > lay.hier_ws
        return True


@functools.lru_cache(maxsize=4)     # (frames are visited one after the other: a few stay, the rest make room)
def frame(name):
    return Frame(name)


def _expected_tile_sort(fr, form):
    if fr.st.dims.P == 0:
        return None
    if form in ("radix", "passes_tickets"):
        return 0
    if form == "hier":
        return 2
    return 1 if fr.fits("count") else (2 if fr.fits("hier") else 0)     # count, scan_inside, auto


def _check_forward(name, form, pattern):
    fr = frame(name)
    if (name, form) in LEFT_OUT:
        assert fr.st.dims.P == 0 or not fr.fits(form), (name, form, "is listed as not fitting, but hs_plan gives it a workspace")
        return
    assert fr.fits(form), (name, form, "hs_plan gives the form no workspace: list it in LEFT_OUT")
    want, ctr0 = fr.zero_run(form)
    assert int(ctr0[0]) == fr.R and int(ctr0[1]) == 0 and int(ctr0[4]) == 0, (name, form, ctr0)
    ts = _expected_tile_sort(fr, form)
    if ts is not None:
        assert int(ctr0[7]) == ts, (name, form, "the form asked for is not the one that ran", ctr0)
    bufs = fr.buffers()
    fr.fill(bufs, pattern)
    got, ctr = fr.snapshot(bufs, fr.enqueue(bufs, form))
    print(f"{name} {form} {pattern}: R={fr.R} counters={ctr.tolist()}")
    assert not differing(got, want), (name, form, pattern, differing(got, want))
    # ... and the Python host's own (auto) frame is this one
    if form == "auto":
        assert poison.bytes_of(fr.out[0]) == got["out_color"].tobytes() and poison.bytes_of(fr.out[1]) == got["radii"].tobytes()


@pytest.mark.parametrize("pattern", FULL_PATTERNS)
@pytest.mark.parametrize("form", FORMS)
def test_forward_template_frame_every_pattern(form, pattern):
    """20 000 Gaussians at 500 x 300, one pose (the frame of test_sort_selection_travels_in_the_call...): every form under
    every pattern."""
    _check_forward("t20k", form, pattern)


@pytest.mark.parametrize("pattern", BOUNDARY_PATTERNS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", FRAMES)
def test_forward_boundary_frames(name, form, pattern):
    _check_forward(name, form, pattern)


@pytest.mark.parametrize("pattern", BOUNDARY_PATTERNS)
@pytest.mark.parametrize("form", FORMS)
def test_forward_overflow_then_the_same_frame_at_sufficient_capacity_in_the_same_bytes(form, pattern):
    """A capacity of R / 2 renders the frame empty with hs_counters.overflow = 1 -- whatever the buffers held; the same
    frame enqueued again at capacity R into the SAME buffers, not refilled (they now hold the overflowed call's layout, cut
    for another capacity), is the clean run."""
    fr = frame("t20k")
    want, _ = fr.zero_run(form)
    bufs = fr.buffers()
    fr.fill(bufs, pattern)
    a = fr.enqueue(bufs, form, capacity=fr.R // 2)
    got, ctr = fr.snapshot(bufs, a)
    assert int(ctr[0]) == fr.R and int(ctr[1]) == 1 and int(ctr[2]) == 0, ctr
    assert not got["out_color"].any() and not got["ranges"].any() and not got["n_contrib"].any()     # background 0, nothing listed
    assert (got["final_T"].view(np.float32) == 1.0).all()
    assert got["radii"].tobytes() == want["radii"].tobytes()
    got2, ctr2 = fr.snapshot(bufs, fr.enqueue(bufs, form))
    assert int(ctr2[1]) == 0
    assert not differing(got2, want), (form, pattern, differing(got2, want))


# ---------------------------------------------------------------------------------------------------------------------
# 2. backward and the whole Python path
# ---------------------------------------------------------------------------------------------------------------------
STATE_KEYS = ("num_rendered", "tile_sort", "depth_slow_ranges", "point_list", "ranges", "final_T", "n_contrib", "radii", "depths",
              "tiles_touched", "clamped", "inst_sorted", "offs_sorted", "rec", "pose_hdr")


def _flatten(res, extra=None):
    out = {}
    for k, v in res.items():
        if k == "state":
            R = int(v["num_rendered"])
            for q in STATE_KEYS:
                if v.get(q) is not None:
                    out["state." + q] = np.asarray(v[q])[:R] if q == "point_list" else np.asarray(v[q])
        elif v is not None:
            out[k] = np.asarray(v)
    for k, v in (extra or {}).items():
        out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return out


def _leaves(sc, stored=None):
    t = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=sc.scales,
             rotations=sc.rotations)
    if stored is not None:
        t.update(opacities=stored[0], scales=stored[1], rotations=stored[2])
    return {k: v.detach().clone().to(DEV).requires_grad_(True) for k, v in t.items()}


def _call(rast, leaf):
    return rast(leaf["means3D"], leaf["means2D"], leaf["opacities"], shs=leaf["shs"], scales=leaf["scales"], rotations=leaf["rotations"])


def _grads(leaf, **more):
    out = {"d_" + k: v.grad for k, v in leaf.items() if v.grad is not None}
    out.update({k: v for k, v in more.items() if v is not None})
    return out


def _posed_settings(sc, cams, hdr=False, **kw):
    rs, expo, crf = Hh.settings_from_scene(sc, DEV, cams, hdr=hdr, requires_grad=True, **kw)
    rs = rs._replace(viewmatrices=rs.viewmatrices.clone().requires_grad_(True), projmatrices=rs.projmatrices.clone().requires_grad_(True),
                     camposes=rs.camposes.clone().requires_grad_(True))
    return rs, expo, crf


def f_ldr_deg3():
    return _flatten(Hh.run_hip(S.make_scene(2000, 160, 120, 3, seed=11))), ()


def f_fixed_capacity():
    """The single-enqueue forward (preprocess clears the binning scratch, frame tag) instead of the synchronous one."""
    return _flatten(Hh.run_hip(S.make_scene(2000, 160, 120, 1, seed=13), capacity=40000)), ()


def f_hdr_3_poses():
    sc = S.make_scene(2000, 160, 120, 2, seed=12, hdr=True)
    gh = torch.randn(3, 120, 160, generator=torch.Generator().manual_seed(1))
    return _flatten(Hh.run_hip(sc, cameras=S.blur_poses(160, 120, 3, step=0.03), hdr=True, grad_hdr=gh)), ("out_hdr",)


def f_hdr_3_poses_blur_hdr():
    sc = S.make_scene(2000, 160, 120, 1, seed=14, hdr=True)
    return _flatten(Hh.run_hip(sc, cameras=S.blur_poses(160, 120, 3, step=0.03), hdr=True, blur_domain="hdr")), ("out_hdr",)


def f_two_frames():
    """n_frames = 2, two poses each, HDR, pose gradients."""
    from casualhdrsplat_amd import GaussianRasterizer, inspect_state
    sc = S.make_scene(1500, 128, 96, 2, seed=15, hdr=True)
    rs, _, crf = _posed_settings(sc, S.blur_poses(128, 96, 4, step=0.02), hdr=True)
    expo = torch.tensor([0.5, 1.7], device=DEV).requires_grad_(True)
    rs = rs._replace(exposure=expo, n_frames=2)
    leaf = _leaves(sc)
    out = _call(GaussianRasterizer(rs), leaf)
    st = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in inspect_state(out[0]).items()}
    dL = torch.randn(2, 3, 96, 128, generator=torch.Generator().manual_seed(2)).to(DEV)
    ((out[0] * dL).sum() + (out[2] * dL.flip(0)).sum()).backward()
    torch.cuda.synchronize()
    return _flatten(dict(color=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy(), hdr=out[2].detach().cpu().numpy(), state=st),
                    _grads(leaf, d_exposure=expo.grad, d_crf=crf.grad, d_view=rs.viewmatrices.grad, d_proj=rs.projmatrices.grad,
                           d_campos=rs.camposes.grad)), ("out_hdr",)


def f_raw():
    """parameterization="raw": hs_activate into scratch tensors, hs_activate_backward in place in the flat buffer."""
    from casualhdrsplat_amd import GaussianRasterizer
    sc = S.make_scene(1500, 128, 96, 2, seed=16, hdr=True)
    gen = torch.Generator().manual_seed(3)
    x = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))
    x[0], x[1] = 30.0, -30.0
    q = sc.rotations * torch.exp(torch.empty(1500, 1).uniform_(-2.0, 2.0, generator=gen))
    q[2] = 0.0
    rs, expo, crf = Hh.settings_from_scene(sc, DEV, hdr=True, requires_grad=True)
    leaf = _leaves(sc, stored=(x, torch.log(sc.scales), q))
    out = _call(GaussianRasterizer(rs, parameterization="raw"), leaf)
    (out[0] * sc.dL_dimage.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return _flatten(dict(color=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy(), hdr=out[2].detach().cpu().numpy()),
                    _grads(leaf, d_exposure=expo.grad, d_crf=crf.grad)), ("out_hdr", "opacities", "scales", "rotations")


def f_deferred_sh():
    """defer_sh_grad: dL_dview_colors [N, P, 3] out of the backward, hs_sh_backward_views (M = 16 at degree 1: the rows
    k >= 4 are written as zeros by the kernel)."""
    from casualhdrsplat_amd import GaussianRasterizer
    from casualhdrsplat_amd.distributed import exchange_view_gradients
    sc = S.make_scene(1500, 128, 96, 3, seed=17)
    sc.sh_degree = 1
    rs, _, _ = Hh.settings_from_scene(sc, DEV, S.blur_poses(128, 96, 3, step=0.02))
    leaf = _leaves(sc)
    rast = GaussianRasterizer(rs, defer_sh_grad=True)
    out = _call(rast, leaf)
    (out[0] * sc.dL_dimage.to(DEV)).sum().backward()
    vc = rast.deferred["view_colors"].clone()
    exchange_view_gradients([v for k, v in leaf.items() if k != "shs"], leaf["shs"], rast.deferred)
    torch.cuda.synchronize()
    assert leaf["shs"].grad.shape == (1500, 16, 3) and not leaf["shs"].grad[:, 4:].any() and leaf["shs"].grad[:, :4].any()
    return _flatten(dict(color=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy()), _grads(leaf, view_colors=vc)), ("view_colors",)


def f_chunked_backward():
    """HS_BWD_PROJECT in ascending chunks [g_begin, g_end) (reduce_group on one rank: no collective, the chunks run), HDR,
    three poses, pose gradients, densification statistics (caller-initialised: zeros)."""
    from casualhdrsplat_amd import DensifyStats, GaussianRasterizer
    sc = S.make_scene(1500, 128, 96, 2, seed=18, hdr=True)
    rs, expo, crf = _posed_settings(sc, S.blur_poses(128, 96, 3, step=0.02), hdr=True)
    leaf = _leaves(sc)
    dens = DensifyStats(1500, DEV)
    rast = GaussianRasterizer(rs, densify_stats=dens, reduce_group=True, reduce_chunks=3)
    out = _call(rast, leaf)
    (out[0] * sc.dL_dimage.to(DEV)).sum().backward()
    assert rast.finish_reduce() == 0
    torch.cuda.synchronize()
    return _flatten(dict(color=out[0].detach().cpu().numpy()),
                    _grads(leaf, d_exposure=expo.grad, d_crf=crf.grad, d_view=rs.viewmatrices.grad, d_proj=rs.projmatrices.grad,
                           d_campos=rs.camposes.grad, grad_accum=dens.grad_accum, denom=dens.denom, max_radii=dens.max_radii)), ("out_hdr",)


def f_pose_gradients():
    """dL/d(viewmatrices, projmatrices, camposes): "unused entries are zero" -- written as zeros by pose_reduce2_kernel."""
    from casualhdrsplat_amd import GaussianRasterizer
    sc = S.make_scene(500, 96, 80, 2, seed=12)
    cams = [S.yaw_camera(96, 80, 2.0 * k - 1.0) for k in range(3)]
    rs, _, _ = _posed_settings(sc, cams)
    leaf = _leaves(sc)
    out = _call(GaussianRasterizer(rs), leaf)
    (out[0] * sc.dL_dimage.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    dv, dp = rs.viewmatrices.grad.reshape(3, 16), rs.projmatrices.grad.reshape(3, 16)
    assert not dv[:, [3, 7, 11, 15]].any() and not dp[:, [2, 6, 10, 14]].any() and dv.any() and dp.any()
    return _flatten(dict(color=out[0].detach().cpu().numpy()), _grads(leaf, d_view=dv, d_proj=dp, d_campos=rs.camposes.grad)), ()


def f_alpha_invdepth():
    from casualhdrsplat_amd import GaussianRasterizer
    sc = S.make_scene(800, 112, 80, 1, seed=14)
    sc.bg = torch.tensor([0.3, 0.1, 0.6])
    sc.antialias = True
    rs, _, _ = Hh.settings_from_scene(sc, DEV, S.blur_poses(112, 80, 2, step=0.02))
    leaf = _leaves(sc)
    out = _call(GaussianRasterizer(rs, return_alpha=True, return_invdepth=True), leaf)
    assert len(out) == 4 and out[2].shape == (80, 112) and out[3].shape == (80, 112)
    g = torch.Generator().manual_seed(2)
    gA, gD = torch.randn(80, 112, generator=g).to(DEV), torch.randn(80, 112, generator=g).to(DEV)
    ((out[0] * sc.dL_dimage.to(DEV)).sum() + (out[2] * gA).sum() + (out[3] * gD).sum()).backward()
    torch.cuda.synchronize()
    return _flatten(dict(color=out[0].detach().cpu().numpy(), alpha=out[2].detach().cpu().numpy(), invdepth=out[3].detach().cpu().numpy()),
                    _grads(leaf)), ("invdepth",)


def f_mostly_culled():
    """Nine Gaussians in ten behind the camera: their gradient rows (SH rows of degree 2 included) are zeros a kernel wrote."""
    sc = S.make_scene(3000, 160, 120, 2, seed=19)
    hide = torch.rand(3000, generator=torch.Generator().manual_seed(4)) < 0.9
    sc.means3D[hide, 2] = -sc.means3D[hide, 2]
    res = Hh.run_hip(sc)
    hidden = hide.numpy()
    assert (res["radii"][hidden] == 0).all() and (res["radii"][~hidden] > 0).any()
    for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations"):
        assert not res["d_" + k][hidden].any() and res["d_" + k][~hidden].any(), k
    return _flatten(res), ()


FEATURES = dict(ldr_deg3=f_ldr_deg3, fixed_capacity=f_fixed_capacity, hdr_3_poses=f_hdr_3_poses, hdr_3_poses_blur_hdr=f_hdr_3_poses_blur_hdr,
                two_frames=f_two_frames, raw=f_raw, deferred_sh=f_deferred_sh, chunked_backward=f_chunked_backward,
                pose_gradients=f_pose_gradients, alpha_invdepth=f_alpha_invdepth, mostly_culled=f_mostly_culled)
STEP_ROLES = ("geom", "binning", "image", "bwd", "flat_gradients", "out_color", "radii")
_zero_runs = {}


def _under(pattern, fn, stale=None):
    mp = pytest.MonkeyPatch()
    try:
        with poison.poisoned(mp, pattern, stale_from=stale) as s:
            res = fn()
        torch.cuda.synchronize()
    finally:
        mp.undo()
    return res, s


def _zero_of(key, fn):
    if key not in _zero_runs:
        _zero_runs[key] = _under("zero", fn)
    return _zero_runs[key]


@pytest.mark.parametrize("pattern", ["ff", "nan", "random", "stale"])
@pytest.mark.parametrize("feature", list(FEATURES))
def test_python_path_outputs_and_gradients(feature, pattern):
    (want, more_roles), s0 = _zero_of(feature, FEATURES[feature])
    (got, _), s = _under(pattern, FEATURES[feature], stale_session("t20k") if pattern == "stale" else None)
    fills = s.require(RAST, roles=STEP_ROLES + tuple(more_roles))
    assert [(f.role, f.shape, f.dtype) for f in fills] == [(f.role, f.shape, f.dtype) for f in s0.of(RAST)]
    print(f"{feature} {pattern}: {len(fills)} buffers of the rasterizer poisoned, {sum(f.nbytes for f in fills)} bytes: "
          f"{[f.role for f in fills]}; others: {sorted({(f.module, f.role) for f in s.fills if f.module != RAST})}")
    if feature == "deferred_sh":
        s.require(RAST, roles=("sh_backward_views#0",))
    assert any(k.startswith("d_") for k in got) and "color" in got
    assert not differing(got, want), (feature, pattern, differing(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the other entry points, through their Python wrappers
# ---------------------------------------------------------------------------------------------------------------------
def e_loss(shape):
    def run():
        from casualhdrsplat_amd import photometric_loss
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.rand(shape, generator=g).to(DEV).requires_grad_(True)
        y = torch.rand(shape, generator=g).to(DEV)
        loss, (l1, ssim) = photometric_loss(x, y, 0.2, return_terms=True)
        (1.5 * loss).backward()
        torch.cuda.synchronize()
        return dict(loss=loss.detach().cpu().numpy(), l1=l1.detach().cpu().numpy(), ssim=ssim.detach().cpu().numpy(), d_image=x.grad.cpu().numpy())
    return run, "casualhdrsplat_amd.losses", ("forward#0", "forward#1", "backward#0")


def e_knn(P):
    def run():
        import knn_reference as KR
        from casualhdrsplat_amd import knn_mean_dist2
        x = KR.uniform(P) if P != 4099 else KR.sfm_like(4099, seed=2)
        return dict(mean_d2=knn_mean_dist2(torch.from_numpy(np.array(x, np.float32)).to(DEV)).cpu().numpy())
    return run, "casualhdrsplat_amd.knn", ("knn_mean_dist2#0",) + (("knn_mean_dist2#1", "knn_mean_dist2#2") if P else ())


def _mcmc_optimizer(case):
    import mcmc_reference as MR
    from casualhdrsplat_amd import GaussianAdam, cloud_param_groups
    t = {k: torch.tensor(v, device=DEV).requires_grad_(True) for k, v in case["cloud"].items()}
    opt = GaussianAdam(cloud_param_groups(*[t[k] for k in MR.NAMES]), eps=1e-15)
    opt.prepare()
    for k in MR.NAMES:
        opt.state[t[k]]["exp_avg"].copy_(torch.tensor(case["moments"][k][0]))
        opt.state[t[k]]["exp_avg_sq"].copy_(torch.tensor(case["moments"][k][1]))
    return opt, t


def _cloud_of(opt, names):
    out = {}
    for g in opt.param_groups:
        p = g["params"][0]
        out[g["name"]] = p.detach().cpu().numpy()
        out[g["name"] + ".m"] = opt.state[p]["exp_avg"].cpu().numpy()
        out[g["name"] + ".v"] = opt.state[p]["exp_avg_sq"].cpu().numpy()
    return out


def e_mcmc(P, M, what):
    def run():
        import mcmc_reference as MR
        from casualhdrsplat_amd import grow, inject_noise, relocate
        case = MR.make_case(P, M, seed=MR.case_seed(P, M), raw=True)
        opt, t = _mcmc_optimizer(case)
        out = {}
        if what == "relocate":
            r = relocate(opt, min_opacity=case["min_opacity"], u=torch.tensor(case["u"][:P], device=DEV))
            out.update(counts=r.counts.cpu().numpy(), source=r.source.cpu().numpy(), cnt=r.cnt.cpu().numpy())
        elif what == "grow":
            n_new = int((2.0 if P < 100 else 1.05) * P) - P
            r = grow(opt, cap_max=10 * P, factor=2.0 if P < 100 else 1.05, min_opacity=case["min_opacity"],
                     u=torch.tensor(case["u"][:n_new], device=DEV))
            out.update(counts=r.counts.cpu().numpy(), row_map=r.row_map.cpu().numpy())
        else:
            xi = torch.randn(P, 3, generator=torch.Generator().manual_seed(6)).to(DEV)
            inject_noise(opt, lr=1.6e-4, xi=xi)
        torch.cuda.synchronize()
        out.update(_cloud_of(opt, MR.NAMES))
        return out
    roles = dict(relocate=("_sample_args#0", "_sample_args#1"), grow=("_sample_args#0", "_sample_args#1", "grow#0", "grow#15"), noise=())[what]
    return run, "casualhdrsplat_amd.mcmc", roles


def e_densify(P, M, roles):
    def run():
        import densify_reference as DR
        from casualhdrsplat_amd import DensifyStats, GaussianAdam, cloud_param_groups, densify_and_prune
        case = DR.make_case(P, M, seed=DR.case_seed(P, M))
        t = {k: torch.tensor(v, device=DEV).requires_grad_(True) for k, v in case["cloud"].items()}
        opt = GaussianAdam(cloud_param_groups(*[t[k] for k in DR.NAMES]), eps=1e-15)
        opt.prepare()
        for k in DR.NAMES:
            opt.state[t[k]]["exp_avg"].copy_(torch.tensor(case["moments"][k][0]))
            opt.state[t[k]]["exp_avg_sq"].copy_(torch.tensor(case["moments"][k][1]))
        stats = DensifyStats(case["P"], DEV)            # caller-initialised (torch.zeros), then the case's statistics
        stats.grad_accum.copy_(torch.tensor(case["grad_accum"]))
        stats.denom.copy_(torch.tensor(case["denom"]))
        stats.max_radii.copy_(torch.tensor(case["max_radii"]))
        res = densify_and_prune(opt, stats, noise=torch.tensor(case["noise"], device=DEV), **case["policy"])
        torch.cuda.synchronize()
        out = dict(row_map=res.row_map.cpu().numpy(), counts=np.array([res.counts[k] for k in sorted(res.counts)]))
        out.update(_cloud_of(opt, DR.NAMES))
        return out
    return run, "casualhdrsplat_amd.densify", tuple(f"densify_and_prune#{k}" for k in roles)


def e_spline(kind, J):
    def run():
        import spline_cases as SC
        from casualhdrsplat_amd import image_formation as IF
        case = SC.Case(kind, J, 1, "free", "randn")
        delta, base, _ = case.inputs
        lo, hi = SC.t_range(J, kind)
        t = (lo + (hi - lo) * torch.rand(13, generator=torch.Generator().manual_seed(5), dtype=torch.float64)).float().to(DEV).requires_grad_(True)
        d = delta.float().to(DEV).requires_grad_(True)
        out = IF._SplinePoses.apply(d, base.float().to(DEV), t, kind)
        jac, seg = out.grad_fn.saved_tensors
        w = torch.randn(13, 4, 4, generator=torch.Generator().manual_seed(9)).to(DEV)
        (out * w).sum().backward()
        torch.cuda.synchronize()
        return dict(w2c=out.detach().cpu().numpy(), jac=jac.cpu().numpy(), seg=seg.cpu().numpy(), d_delta=d.grad.cpu().numpy(),
                    d_t=t.grad.cpu().numpy())
    return run, "casualhdrsplat_amd.image_formation", ("forward#0", "forward#1", "forward#2")


def e_mark_visible():
    def run():
        from casualhdrsplat_amd import GaussianRasterizer
        sc = S.make_scene(1001, 96, 80, 0, seed=21)
        sc.means3D[::3, 2] = -sc.means3D[::3, 2]
        rs, _, _ = Hh.settings_from_scene(sc, DEV)
        vis = GaussianRasterizer(rs).markVisible(sc.means3D.to(DEV))
        assert vis.shape == (1001,) and vis.any() and not vis.all()
        return dict(visible=vis.cpu().numpy())
    return run, RAST, ("markVisible#0",)


def e_sh_backward_views():
    def run():
        from casualhdrsplat_amd.rasterizer import sh_backward_views
        g = torch.Generator().manual_seed(11)
        P, V = 2500, 5
        means, cams, vc = torch.randn(P, 3, generator=g) * 3, torch.randn(V, 3, generator=g) * 5 + 10, torch.randn(V, P, 3, generator=g)
        got = sh_backward_views(means.to(DEV), cams.to(DEV), vc.to(DEV), 16, 1)
        assert not got[:, 4:].any() and got[:, :4].any()          # "rows k >= (sh_degree + 1)^2 are zeroed": by the kernel
        return dict(d_shs=got.cpu().numpy())
    return run, RAST, ("sh_backward_views#0",)


ENTRY_POINTS = {
    "loss_3x37x129": e_loss((3, 37, 129)), "loss_2x3x50x70": e_loss((2, 3, 50, 70)),
    "knn_1": e_knn(1), "knn_5": e_knn(5), "knn_1025": e_knn(1025), "knn_4099": e_knn(4099), "knn_10007": e_knn(10007),
    "mcmc_relocate_1": e_mcmc(1, 1, "relocate"), "mcmc_relocate_257": e_mcmc(257, 16, "relocate"), "mcmc_relocate_10007": e_mcmc(10007, 1, "relocate"),
    "mcmc_grow_1": e_mcmc(1, 1, "grow"), "mcmc_grow_257": e_mcmc(257, 16, "grow"), "mcmc_grow_10007": e_mcmc(10007, 1, "grow"),
    "mcmc_noise_257": e_mcmc(257, 16, "noise"), "mcmc_noise_10007": e_mcmc(10007, 1, "noise"),
    # (workspace, row_map, counts; with rows coming out, the five new tensors and their ten moments: #3 .. #17)
    "densify_1": e_densify(1, 1, (0, 1, 2)), "densify_10007": e_densify(10007, 16, (0, 1, 2, 3, 17)),
    "spline_linear_3": e_spline("linear", 3), "spline_cubic_7": e_spline("cubic", 7),
    "mark_visible": e_mark_visible(), "sh_backward_views": e_sh_backward_views(),
}


@pytest.mark.parametrize("pattern", ["ff", "a5", "nan", "random", "stale"])
@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_entry_point_through_its_wrapper(name, pattern):
    """hs_activate forward and backward: the `raw` feature of test_python_path_outputs_and_gradients."""
    run, module, roles = ENTRY_POINTS[name]
    want, s0 = _zero_of("entry:" + name, run)
    got, s = _under(pattern, run, stale_session("t20k") if pattern == "stale" else None)
    if roles:
        fills = s.require(module, roles=roles)
    else:       # hs_mcmc_noise works in place: the wrapper hands the library no uninitialised buffer at all
        fills = s.of(module)
        assert fills == []
    assert [(f.role, f.shape) for f in fills] == [(f.role, f.shape) for f in s0.of(module)]
    print(f"{name} {pattern}: {len(fills)} buffers of {module} poisoned: {[(f.role, f.nbytes) for f in fills]}")
    assert not differing(got, want), (name, pattern, differing(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# 4. shapes alternating on one rasterizer object
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [None, 400000], ids=["synchronous", "fixed_capacity"])
def test_interleaved_shapes_on_one_rasterizer_object(capacity):
    """20 000 @ 500 x 300 -> 3 000 @ 160 x 120 HDR with two poses -> 257 @ 16 x 16 -> the first again, on ONE rasterizer object
    (its settings exchanged between the calls), nothing freed explicitly in between: the caching allocator hands each call the
    previous calls' buffers, cut differently.  Every call equals the same call on a fresh object in a clean allocator."""
    from casualhdrsplat_amd import GaussianRasterizer
    specs = [(S.make_scene(20000, 500, 300, 1, seed=3), None, False),
             (S.make_scene(3000, 160, 120, 2, seed=31, hdr=True), S.blur_poses(160, 120, 2, step=0.03), True),
             (S.make_scene(257, 16, 16, 1, seed=2), None, False)]
    order = [0, 1, 2, 0]

    def step(rast, spec):
        sc, cams, hdr = spec
        rs, expo, crf = Hh.settings_from_scene(sc, DEV, cams, hdr=hdr, requires_grad=hdr)
        rast.raster_settings = rs
        leaf = _leaves(sc)
        out = _call(rast, leaf)
        loss = (out[0] * sc.dL_dimage.to(DEV)).sum()
        loss.backward()
        torch.cuda.synchronize()
        res = dict(color=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy())
        if hdr:
            res.update(hdr=out[2].detach().cpu().numpy(), d_exposure=expo.grad.cpu().numpy(), d_crf=crf.grad.cpu().numpy())
        res.update({k: v.cpu().numpy() for k, v in _grads(leaf).items()})
        return res

    def fresh(spec):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        rs, _, _ = Hh.settings_from_scene(spec[0], DEV, spec[1], hdr=spec[2])
        return step(GaussianRasterizer(rs, capacity=capacity), spec)

    want = [fresh(sp) for sp in specs]
    torch.cuda.empty_cache()
    rs0, _, _ = Hh.settings_from_scene(specs[0][0], DEV)
    rast = GaussianRasterizer(rs0, capacity=capacity)
    for n, i in enumerate(order):
        got = step(rast, specs[i])
        assert not differing(got, want[i]), (n, i, differing(got, want[i]))
    assert rast.overflow_replays == 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. words that already carry the call's frame tag
# ---------------------------------------------------------------------------------------------------------------------
_TAG_CHILD = r"""
import os, sys, hashlib, ctypes as C
import numpy as np, torch
sys.path.insert(0, os.environ["HS_ROOT"]); sys.path.insert(0, os.path.join(os.environ["HS_ROOT"], "tests"))
import test_workspace_contents_gpu as T
from casualhdrsplat_amd import _lib as L
lib = L.load()
lib.hs_test_next_frame_tag.restype = C.c_uint32
fr = T.Frame("t20k")
for form in ("auto", "passes_tickets"):
    want, ctr0 = fr.zero_run(form)
    for bits in ("ones", "random"):
        bufs = fr.buffers()
        fr.fill(bufs, "a5")
        tag = int(lib.hs_test_next_frame_tag())
        words = bufs["binning"].view(torch.int64)
        if bits == "ones":
            lo = torch.full((words.numel(),), 0xFFFFFFFF, dtype=torch.int64, device=words.device)
        else:
            lo = torch.randint(0, 1 << 32, (words.numel(),), dtype=torch.int64, device=words.device, generator=torch.Generator(device=words.device).manual_seed(7))
        signed_tag = tag - (1 << 32) if tag >= (1 << 31) else tag
        words.copy_((torch.full_like(lo, signed_tag) << 32) | lo)
        assert int(lib.hs_test_next_frame_tag()) == tag
        got, ctr = fr.snapshot(bufs, fr.enqueue(bufs, form))
        assert int(lib.hs_test_next_frame_tag()) == ((tag + 1) & 0xFFFFFFFF or 1), "the call did not draw the tag that was planted"
        bad = T.differing({k: got[k] for k in ("point_list", "ranges", "out_color")}, {k: want[k] for k in ("point_list", "ranges", "out_color")})
        print("TAGGED", form, bits, "tag", hex(tag), "R", int(ctr[0]), "overflow", int(ctr[1]), "slow_ranges", int(ctr[4]),
              "slow_ranges_clean", int(ctr0[4]), "DIFFERS" if bad else "SAME", bad)
"""


def test_garbage_bits_under_a_matching_frame_tag_never_give_a_wrong_order():
    """hs_common.h, kDepthBitsAt: a depth-bits word whose tag is this call's counts as this call's -- "stale or garbage bits
    under a matching tag could only ADD varying bits, i.e. sort a constant bit too: never a wrong order".  The whole binning
    workspace is filled with 64-bit words {tag << 32 | bits}, tag = what the NEXT hs_forward will draw (exported by
    libhdrsplat_test.so only), bits all ones and seeded random; both depth sorts.  point_list, ranges and the image are
    the clean run's.  (Ranges of the counting depth sort that leave the chip under the wider digit layout would be
    "correct, slow": printed, not asserted.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HS_ROOT=root, HS_LIB_PATH=_TEST_LIB, HS_FAULT_INJECT="")
    r = subprocess.run([sys.executable, "-c", _TAG_CHILD], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("TAGGED")]
    print("\n".join(lines))
    assert len(lines) == 4 and all(" SAME " in ln and " overflow 0 " in ln for ln in lines), lines
