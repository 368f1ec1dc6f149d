"""Digests of what the oracle's guard band, reach and gradient bounds -- and the helpers built on them -- return when called
WITHOUT the conditioning arguments, on one unmodified make_scene frame (3000 Gaussians, 240 x 160, SH degree 1, seed 0).

tests/golden/anisotropy_defaults.json holds these digests as recorded at the commit BEFORE the conditioned guard band was
added; tests/test_anisotropy.py recomputes them and demands the same bytes.  Run this file only to record a deliberate
change of the default path:  python tests/golden/make_anisotropy_defaults.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def _digest(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(str(a.dtype).encode() + b"|" + str(a.shape).encode() + b"|")
    h.update(a.tobytes())
    return h.hexdigest()


def default_digests(O):
    import helpers as Hh
    from casualhdrsplat_amd import synthetic as S
    sc = S.make_scene(3000, 240, 160, 1, seed=0)
    f, b = Hh.run_oracle(O, sc, bounds=True)
    cam = Hh.oracle_camera(O, sc)
    out = {}
    for name, args in (("risk_default", ()), ("risk_helpers", (1e-5, 5e-5))):
        r = O.threshold_risk(cam, f, *args)
        out[name + ".pix_risk"] = _digest(r["pix_risk"])
        out[name + ".gauss_risk"] = _digest(r["gauss_risk"])
        out[name + ".margins"] = _digest(np.array([r["n_risky_pixels"], r["min_margin_alpha"], r["min_margin_T"],
                                                   r["min_abs_power"]], np.float64))
    band = O.threshold_risk(cam, f, 1e-3, 1e-3)["pix_risk"]     # a wide band, so that the reach has pixels to walk
    out["reach_own"] = _digest(O.pixel_reach(cam, f, band))
    out["reach_whole_list"] = _digest(O.pixel_reach(cam, f, band, whole_list=True))
    for k in sorted(b):
        if isinstance(b[k], np.ndarray):
            out["backward." + k] = _digest(b[k])
    pix, gs = Hh.oracle_risk(O, sc, [f])
    out["helpers.oracle_risk.pix"] = _digest(pix)
    out["helpers.oracle_risk.gauss"] = _digest(gs)
    # decision_masks against a stand-in for the HIP state: the oracle's own frame with the contributor count of the band's
    # first pixel changed (a differing decision INSIDE the band, so that `rows` has a pixel to reach from)
    nc = f["n_contrib"].copy()
    if pix[0].any():
        y, x = np.argwhere(pix[0])[0]
        nc[y, x] += 1
    m = Hh.decision_masks(O, sc, [f], dict(n_contrib=nc[None], final_T=f["final_T"][None]))
    for k in ("pix_risk", "differs", "knot", "rows", "excluded"):
        out["helpers.decision_masks." + k] = _digest(m[k])
    out["helpers.decision_masks.counts"] = [m["n_differ"], m["n_knot_pixels"]]
    return out


if __name__ == "__main__":
    from oracle import c_oracle
    c_oracle.build()
    with open(os.path.join(HERE, "anisotropy_defaults.json"), "w") as fh:
        json.dump(default_digests(c_oracle), fh, indent=1, sort_keys=True)
        fh.write("\n")
