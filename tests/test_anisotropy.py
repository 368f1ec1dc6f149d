"""The instrument for ill-conditioned footprints, pinned on the CPU without the code under test.

Needles and discs (synthetic.anisotropic_scene, helpers.ANISO_SCENES A-E) make the power -0.5 (A dx^2 + C dy^2) - B dx dy a
difference of terms M = 0.5|A|dx^2 + 0.5|C|dy^2 + |B||dx dy| that is far larger than the power itself; the oracle's conditioned
guard band (oracle.threshold_risk(conditioned=k)) widens every decision test by k 2^-24 M.  Here, from the oracle alone:
  * k is the derived constant, and both evaluations it was derived from -- the oracle's and a restatement of the render
    kernel's pre-scaled base-2 form -- stay within (k / 2) 2^-24 M of float64 on the same conic and centre bits, on EVERY
    (pixel, entry) of the five scenes;
  * every scene holds the share caps that make it usable (conditions, never raised);
  * the default, non-conditioned calls return the bytes they returned before the conditioning existed;
  * the new exports refuse bad arguments and leave the gradients and abs_* alone.
tests/test_anisotropy_gpu.py then holds the HIP path to this instrument.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import helpers as Hh
from casualhdrsplat_amd import synthetic as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U24 = 2.0 ** -24
LOG2E_F32 = np.float32(1.4426950408889634)      # render.hip: kLog2e


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(scene, oracle forward, oracle camera, conditioned band at the derived k) of one of helpers.ANISO_SCENES."""
    from oracle import c_oracle as O
    O.build()
    kind, ratio, fraction, seed = Hh.ANISO_SCENES[name]
    sc = S.anisotropic_scene(kind, ratio, fraction, seed)
    f, _ = Hh.run_oracle(O, sc, backward=False)
    cam = Hh.oracle_camera(O, sc)
    return sc, f, cam, O.threshold_risk(cam, f, 1e-5, 5e-5, conditioned=O.K_COND)


def _walk_powers(f, W, H):
    """Every (pixel, entry) of the frame, tile by tile: the largest |fp32 power - float64 power| / (2^-24 M) of (a) the
    oracle's five-product form and (b) the render kernel's pre-scaled form -- scale_entry's three products, then
    dy*(C2*dy + B2*dx) + (A2*dx)*dx, the same operation order in numpy float32 (numpy fuses nothing), the base-2 result
    divided back by log2(e) in float64 -- both against float64 from the same fp32 conic and centre bits.  Returns
    (c_oracle, c_kernel, pairs walked, largest M of any pair)."""
    xy, co = f["xy"], f["conic_opacity"]
    gx = (W + 15) // 16
    c1, cB = np.float32(-0.5) * LOG2E_F32, -LOG2E_F32
    worst_o = worst_k = max_M = 0.0
    pairs = 0
    for t, (beg, end) in enumerate(f["ranges"].astype(np.int64)):
        if end == beg:
            continue
        ids = f["point_list"][beg:end]
        ty, tx = divmod(t, gx)
        px, py = np.meshgrid(np.arange(16 * tx, min(16 * tx + 16, W)), np.arange(16 * ty, min(16 * ty + 16, H)))
        dx = xy[ids, 0][:, None] - px.reshape(1, -1).astype(np.float32)
        dy = xy[ids, 1][:, None] - py.reshape(1, -1).astype(np.float32)
        A, B, Cc = co[ids, 0][:, None], co[ids, 1][:, None], co[ids, 2][:, None]
        assert dx.dtype == dy.dtype == A.dtype == np.float32
        p_oracle = np.float32(-0.5) * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        A2, B2, C2 = A * c1, B * cB, Cc * c1
        p_kernel = dy * (C2 * dy + B2 * dx) + (A2 * dx) * dx
        assert p_oracle.dtype == p_kernel.dtype == np.float32
        x, y = dx.astype(np.float64), dy.astype(np.float64)
        A64, B64, C64 = A.astype(np.float64), B.astype(np.float64), Cc.astype(np.float64)
        exact = -0.5 * (A64 * x * x + C64 * y * y) - B64 * x * y
        M = 0.5 * np.abs(A64) * x * x + 0.5 * np.abs(C64) * y * y + np.abs(B64) * np.abs(x * y)
        ok = M > 0
        if ok.any():
            unit = U24 * M[ok]
            worst_o = max(worst_o, float((np.abs(p_oracle.astype(np.float64) - exact)[ok] / unit).max()))
            worst_k = max(worst_k, float((np.abs(p_kernel.astype(np.float64) / np.log2(np.e) - exact)[ok] / unit).max()))
            max_M = max(max_M, float(M.max()))
        pairs += M.size
    return worst_o, worst_k, pairs, max_M


def test_k_is_the_derived_constant(oracle):
    """4 roundings per term in the oracle's form + 5.22 in the kernel's, rounded up (hs_oracle.c, HSO_COND_K): the Python
    constant, the C constant and the count are one number."""
    lib = oracle.lib()
    assert oracle.K_COND == lib.hso_cond_k() == 10.0
    assert 4 + 5.22 <= oracle.K_COND < 4 + 5.22 + 1


@pytest.mark.parametrize("name", sorted(Hh.ANISO_SCENES))
def test_both_power_evaluations_stay_within_half_k_of_float64(oracle, name):
    """Every (pixel, entry) of the scene: the oracle's fp32 power (the C walk's own figure, and the numpy restatement of
    it, which must agree on the pairs walked and on the worst case) and the numpy float32 restatement of the render
    kernel's pre-scaled form are each within (k / 2) 2^-24 M of float64.  Measured: 3.35-3.64 and 3.89-4.15 (scenes A-E)."""
    sc, f, cam, r = _scene(name)
    c_o, c_k, pairs, max_M = _walk_powers(f, sc.camera.W, sc.camera.H)
    print(f"scene {name}: pairs {pairs}, largest M of any pair {max_M:.3g}, of a contributor {r['max_M']:.3g}; "
          f"|fp32 - fp64| / (2^-24 M): oracle {r['power_c']:.3f} (numpy {c_o:.3f}), kernel form {c_k:.3f}")
    # (the C walk stops where a pixel terminates, this one does not: a superset of its pairs, the same arithmetic)
    assert pairs >= r["n_pairs"] > 1_000_000 and c_o >= r["power_c"] > 1.0
    assert r["power_c"] <= oracle.K_COND / 2
    assert c_k <= oracle.K_COND / 2
    # the scenes do what they are for: M of a contributing entry far above today's 11
    assert r["max_M"] >= {"A": 3e2, "B": 2e3, "C": 1e4, "D": 1e3, "E": 1e4}[name]


@pytest.mark.parametrize("name", sorted(Hh.ANISO_SCENES))
def test_scenes_hold_the_share_caps(oracle, name):
    """Conditions on the scene, from the oracle alone: the conditioned band covers at most 5e-3 of the pixels and at most
    1e-2 of them cannot be classified (T_tol above 1.5e-3).  E keeps a radius above 1000 px, C one above 400."""
    sc, f, cam, r = _scene(name)
    npix = sc.camera.W * sc.camera.H
    band, unclass = r["n_risky_pixels"] / npix, float((r["T_tol"] > Hh.T_TOL_CLASSIFIABLE).mean())
    print(f"scene {name}: R {f['R']}, largest radius {int(f['radii'].max())}, band {band:.2e}, unclassifiable {unclass:.2e}, "
          f"worst T_tol {r['T_tol'].max():.2e}")
    assert band <= Hh.ANISO_BAND_CAP
    assert unclass <= Hh.ANISO_UNCLASSIFIABLE_CAP
    assert int(f["radii"].max()) >= {"A": 100, "B": 200, "C": 400, "D": 200, "E": 1000}[name]
    # the conditioned band contains the fixed one, pixel by pixel and row by row
    fixed = oracle.threshold_risk(cam, f, 1e-5, 5e-5)
    assert not (fixed["pix_risk"] & ~r["pix_risk"]).any() and not (fixed["gauss_risk"] & ~r["gauss_risk"]).any()
    assert r["n_risky_pixels"] > fixed["n_risky_pixels"]
    assert (r["T_tol"] >= 0).all() and (r["color_tol"] >= 0).all() and np.isfinite(r["color_tol"]).all()
    assert (r["T_tol"][f["n_contrib"] == 0] == 0).all()


def test_default_calls_return_what_they_returned_before(oracle):
    """One unmodified make_scene frame: threshold_risk, pixel_reach, backward(bounds=True), helpers.oracle_risk and
    helpers.decision_masks WITHOUT the conditioning arguments give, byte for byte, what tests/golden/
    anisotropy_defaults.json recorded at the commit before the conditioning was added."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_anisotropy_defaults", os.path.join(GOLDEN, "make_anisotropy_defaults.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "anisotropy_defaults.json")) as fh:
        want = json.load(fh)
    got = mod.default_digests(oracle)
    assert set(got) == set(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}


def test_conditioned_backward_leaves_gradients_and_abs_terms_alone(oracle):
    """backward(conditioned=True): the gradients and every abs_* are the bits of backward(bounds=True); each cond_* has its
    abs_* twin's shape and zeros; on a contributor cond / abs = (M + T_units) / (4 + steps) can be small or large, but a
    cond_* is zero exactly where its abs_* is."""
    sc, f, cam, r = _scene("B")
    args = (cam, f, sc.dL_dimage.numpy(), sc.means3D.numpy())
    kw = dict(shs=sc.shs.numpy(), scales=sc.scales.numpy(), rotations=sc.rotations.numpy())
    b0 = oracle.backward(*args, bounds=True, **kw)
    b1 = oracle.backward(*args, bounds=True, conditioned=True, **kw)
    for k, v in b0.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v.view(np.uint8), b1[k].view(np.uint8)), k
    n = 0
    for _, rk in Hh.GRAD_KEYS:
        a, c = b1["abs_" + rk], b1["cond_" + rk]
        assert c.shape == a.shape and np.isfinite(c).all() and (c >= 0).all()
        assert np.array_equal(c == 0, a == 0), rk
        n += int((c > 0).sum())
    assert n > 10_000


def test_new_exports_check_their_arguments(oracle):
    sc, f, cam, r = _scene("A")
    for k in (0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            oracle.threshold_risk(cam, f, conditioned=k)
        with pytest.raises(ValueError):
            oracle.pixel_reach(cam, f, r["pix_risk"], whole_list=True, conditioned=k)
    with pytest.raises(ValueError):
        oracle.threshold_risk(cam, f, -1e-5, 5e-5, conditioned=oracle.K_COND)
    with pytest.raises(ValueError):
        oracle.pixel_reach(cam, f, r["pix_risk"][:-1], whole_list=True, conditioned=oracle.K_COND)
    with pytest.raises(ValueError):
        oracle.backward(cam, f, sc.dL_dimage.numpy(), sc.means3D.numpy(), shs=sc.shs.numpy(), scales=sc.scales.numpy(),
                        rotations=sc.rotations.numpy(), conditioned=True)
    # the C exports themselves: a missing array or a bad k is -1, nothing is written
    L = oracle.lib()
    c = cam.cstruct(f["radii"].shape[0], 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    pix = np.full((cam.H, cam.W), 7, np.uint8)
    mm = np.zeros(3)
    good = [C.byref(c), p(f["ranges"]), p(f["point_list"]), p(f["xy"]), p(f["conic_opacity"]), p(f["rgb"]), C.c_float(1e-5),
            C.c_float(5e-5), C.c_double(10.0), p(pix), None, p(mm), None, None, None]
    assert L.hso_threshold_risk_cond(*good) == r["n_risky_pixels"]          # every optional output may be missing
    for at, bad in ((1, None), (9, None), (11, None), (8, C.c_double(0.0)), (8, C.c_double(float("nan"))), (6, C.c_float(-1.0))):
        args = list(good)
        args[at] = bad
        pix[:] = 7
        assert L.hso_threshold_risk_cond(*args) == -1 and (pix == 7).all()
    cu = np.zeros((3, cam.H, cam.W), np.float32)
    args = list(good)
    args[5], args[13] = None, p(cu)
    assert L.hso_threshold_risk_cond(*args) == -1                            # colour bound asked for without the colours
    assert L.hso_pixel_reach_cond(C.byref(c), p(f["ranges"]), p(f["point_list"]), p(f["xy"]), p(f["conic_opacity"]), None,
                                  p(pix), C.c_int(1), C.c_float(1e-5), C.c_double(10.0)) == -1
    assert L.hso_render_bwd_cond(*([None] * 18)) == -1
