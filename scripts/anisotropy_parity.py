"""profiles/anisotropy_parity.json: the figures of tests/test_anisotropy_gpu.py's scenes A-E (helpers.ANISO_SCENES), HIP path
against the oracle under its conditioned guard band, on the GPU this runs on.  Every assertion of the tests is made on
the way (tests/test_anisotropy_gpu.py: scene_parity); per scene: R and the largest radius, the largest M of a contributing
entry, band share, unclassifiable share, pixels with a differing decision, how much of the per-pixel image bounds was used,
and c_needed of both terms of the per-element gradient bound (each the constant its term would need with the other at its
set value: the abs term next to k 2^-24 cond, the cond term next to C_BOUND 2^-24 abs; 0 where nothing more is needed).

    python scripts/anisotropy_parity.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out):
    import torch

    import helpers as Hh
    import test_anisotropy_gpu as T
    from oracle import c_oracle as O
    O.build()
    rec = dict(device=torch.cuda.get_device_name(0), k=O.K_COND, C_BOUND=Hh.C_BOUND, frame="3000 Gaussians, 240 x 160, SH degree 1",
               caps=dict(band=Hh.ANISO_BAND_CAP, unclassifiable=Hh.ANISO_UNCLASSIFIABLE_CAP, differing=T.DIFFER_CAP), scenes={})
    for name in sorted(Hh.ANISO_SCENES):
        rec["scenes"][name] = T.scene_parity(O, name)
    for sort in ("radix", "hier"):
        rec["scenes"]["C " + sort] = T.scene_parity(O, "C", tile_sort=sort)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "anisotropy_parity.json"))
