#!/usr/bin/env python3
"""The loop a CasualHDRSplat-style trainer runs around the rasterizer, on synthetic captures (no dataset needed).

Ground truth: a synthetic Gaussian cloud, a camera moving along a cubic SE(3) B-spline, one exposure time per captured frame
(which scales the radiance AND sets the length of the exposure window, i.e. the blur), a camera response curve.  The
observations are the blurred LDR frames `image_formation.HDRBlurFormation` renders from that.  The run then starts from
perturbed radiance and opacities, wrong exposure times and a wrong trajectory, and optimises all of them jointly with
Adam against the observations -- what /root/reference/Readme.md:54 describes ("jointly estimating exposure time with
camera motion") -- through the HIP kernels: every step is frames x (N-pose forward + backward).

    python examples/train_synthetic.py --steps 300
    python examples/train_synthetic.py --steps 300 --lambda-dssim 0.2     # the published L1 + D-SSIM loss, fused
    python examples/train_synthetic.py --steps 300 --fused-adam           # the update through optim.GaussianAdam, visible rows only
    python examples/train_synthetic.py --steps 300 --fused-adam --raw     # the stored (logit) opacities go straight into the rasterizer
    python examples/train_synthetic.py --steps 300 --batch-frames         # all frames of a step in ONE rasterizer call
    python examples/train_synthetic.py --steps 300 --mcmc                 # learn the WHOLE cloud from a quarter of the points: MCMC policy
    python examples/train_synthetic.py --steps 300 --mcmc --filter-3d     # ... with the 3D smoothing filter of Mip-Splatting
    python examples/train_synthetic.py --steps 300 --mcmc --distortion 1  # ... with the depth-distortion regulariser on the blending weights
    python examples/train_synthetic.py --steps 300 --mcmc --normal 0.05   # ... with the depth-normal consistency term on the composited normals
    python examples/train_synthetic.py --steps 300 --mcmc --distortion 0.1 --normal 0.05 --mesh out.ply   # ... and the surface: TSDF fusion + mesh
    python examples/train_synthetic.py --steps 300 --mcmc --distortion 0.1 --normal 0.05 --mesh out.ply --mesh-keep-largest 1   # ... cleaned: one component
    python examples/train_synthetic.py --steps 300 --topk                 # ... grown by score to a budget, pruned by contribution
    python examples/train_synthetic.py --steps 200 --absgrad              # ... the published densify / prune on the AbsGS statistic
    python examples/train_synthetic.py --steps 300 --topk --absgrad       # ... the budgeted policy, scored by the AbsGS statistic
    python examples/train_synthetic.py --steps 300 --bilagrid             # vignetted, tinted observations; a bilateral grid per frame absorbs them
    python examples/train_synthetic.py --steps 300 --topk --vq 1024       # ... then the SH coefficients as 16-bit codes into a k-means codebook

Gauge: exposure x radiance x response is determined only up to a common factor, so the response curve and the first frame's
exposure are held at their true values (a real capture pins them with EXIF exposure ratios or a calibrated response).
"""
import argparse
import functools
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import scene_io
from casualhdrsplat_amd.bilagrid import BilateralGrid
from casualhdrsplat_amd import synthetic as S
from casualhdrsplat_amd.importance import ContributionStats, accumulate_contributions
from casualhdrsplat_amd.mcmc import grow, inject_noise, regularize, relocate
from casualhdrsplat_amd.rows import densify_top_k, keep_top_k
from casualhdrsplat_amd.densify import densify_and_prune
from casualhdrsplat_amd.distortion import distortion_loss
from casualhdrsplat_amd.features import composite_features
from casualhdrsplat_amd.normals import gaussian_normals, normal_consistency_loss
from casualhdrsplat_amd.optim import cloud_param_groups
from casualhdrsplat_amd.losses import photometric_loss
from casualhdrsplat_amd.optim import GaussianAdam
from casualhdrsplat_amd.graphs import GraphedStep
from casualhdrsplat_amd.rasterizer import DensifyStats, GaussianRasterizationSettings, GaussianRasterizer
from casualhdrsplat_amd.tsdf import TSDFVolume
from casualhdrsplat_amd.vq import dequantize_sh, quantize_sh
from casualhdrsplat_amd.image_formation import (FrameRasterizers, HDRBlurFormation, ImplicitCRF, TrajectorySpline,
                                                  knots_from_lookat)

CLOUD = ("means3D", "opacities", "shs", "scales", "rotations")


def mean_by_rows(x: torch.Tensor) -> torch.Tensor:
    """x.mean() as two small reductions (rows of 256, then the row sums).  Inside THIS captured step a plain .mean() / .sum()
    over more than a few ten thousand elements -- PyTorch's two-pass kernel -- reads a wrong value from the second replay on
    (23.6 instead of 0.0406: scripts/repro/graph_step_mean.py).  Round 5 blamed a memset node; round 6's reproducers show
    that neither HIP's memset nodes nor this reduction fail in isolation and that the step fails with a torch-only stand-in
    for the rasterizer too: the capture of the long torch step, not the reduction, not this library.  The
    gradient of a mean does not depend on its value, so training was right all along; the printed numbers were not."""
    if os.environ.get("HS_EXAMPLE_PLAIN_MEAN"):      # (scripts/repro/graph_step_mean.py: the reduction this function avoids)
        return x.mean()
    n = x.numel()
    pad = (-n) % 256
    flat = x.reshape(-1)
    if pad:
        flat = torch.cat([flat, flat.new_zeros(pad)])
    return flat.reshape(-1, 256).sum(dim=1).sum() / n


def run(P=20000, W=320, H=208, frames=4, virtual=5, steps=200, seed=0, deg=1, log_every=25, device="cuda", quiet=False,
        graph=False, capacity=None, lambda_dssim=0.0, fused_adam=False, raw=False, batch_frames=False,
        mcmc=False, cap_max=None, refine_every=25, opacity_reg=0.01, scale_reg=0.01, filter_3d=False, topk=False, absgrad=False,
        bilagrid=False, distort=None, vq=0, distortion=None, normal=None, mesh=None, mesh_min_faces=None,
        mesh_keep_largest=None):
    """Returns a dict of the run's first / last loss, PSNR and parameter errors (also what the GPU test checks).
    lambda_dssim > 0: each frame's loss is the published (1 - lambda) L1 + lambda (1 - SSIM), from the fused kernels of
    losses.photometric_loss (its scalar comes from the library's own fixed-order reduction); 0 keeps the plain L1.
    fused_adam: the update goes through optim.GaussianAdam -- one launch for all four tensors, and the per-Gaussian ones
    (radiance, opacities) only in the rows some frame of the step saw (radii > 0 in any frame).  With graph=True the update
    stays outside the captured step.
    raw: the learner's rasterizers take the cloud as it is STORED (GaussianRasterizer(..., parameterization="raw")): the
    logit opacities go in as the leaf they are -- no torch.sigmoid in front, their gradient a view of the rasterizer's flat
    buffer -- and the fixed scales / rotations as logs / quaternions.
    batch_frames: the step is ONE rasterizer call over all frames (HDRBlurFormation.forward_frames, settings.n_frames) and
    one loss call over the [frames, 3, H, W] batch instead of a call per frame: the same gradients up to fp32 summation
    order.  Eager only: together with graph=True it raises (the captured step keeps one rasterizer per frame).
    mcmc: the learner does not know the cloud.  It starts from P // 4 of the true positions, noised, as
    scene_io.init_from_points builds a cloud from points (3-NN scales, identity quaternions, opacity 0.1, DC from noised
    true colours), and learns ALL FIVE stored tensors -- leaves of one GaussianAdam(cloud_param_groups(...)) that also holds
    the exposure and trajectory groups -- under the MCMC policy: every step is gradients, regularize (the publication's
    opacity_reg mean|opacity| + scale_reg mean|scale|, added in place into the rasterizer's gradient rows), opt.step() on
    every row, inject_noise; every `refine_every` steps, from the first such step to steps - refine_every, relocate (dead
    rows onto live ones) and grow towards `cap_max` (default P) by the factor, at most 2, that reaches the budget at the
    last refinement.  Implies fused_adam and raw; eager only (P changes: not with graph=True).  The history gains P and the
    two regulariser terms, and the reported loss is the mean per-frame loss plus the two terms.
    filter_3d (with mcmc): the 3D smoothing filter of Mip-Splatting.  HDRBlurFormation.compute_filter_3D computes it from every
    virtual pose of the learner's trajectory at the start and again after every grow (the rows moved and P changed), and the
    learner's rasterizers fold it into the opacities and scales they run on (GaussianRasterizer.filter_3D); the optimizer, the
    regularisers and the relocation keep working on the stored tensors.  The history gains the filter's length.
    topk: the learner of mcmc (P // 4 noised points, all five stored tensors under one GaussianAdam, raw rasterizers) under a
    score-driven, budgeted policy instead: its rasterizers collect a DensifyStats, and every `refine_every` steps
    rows.densify_top_k clones or splits the k = min(cap - P, round(P (factor - 1))) rows with the largest mean view-space
    gradient, under the factor schedule of mcmc -- the host knows the new size, nothing is read back.  At the last refinement,
    after the growth, a no_grad pass over all frames accumulates the blending-weight statistics
    (importance.accumulate_contributions) and rows.keep_top_k keeps the P - P // 10 rows with the largest maximum weight.  No
    noise, no regularisers, no relocation.  Eager only; not together with mcmc.  The history gains P.
    absgrad: the statistics are a DensifyStats(absgrad=True) -- every backward also collects the absolute screen-gradient
    statistic of AbsGS (importance.py).  With topk the score of densify_top_k is stats.mean_abs_grad() instead of
    mean_grad(); on its own it is the same learner under the published policy, densify_and_prune(absgrad=True) every
    `refine_every` steps while the cloud is below `cap_max` (default P), with the threshold AbsGS trainers use (twice the
    default: magnitudes do not cancel).  Eager only; not together with mcmc.
    bilagrid: the observations are multiplied by a smooth per-frame gain field (a vignette times a per-frame tint: what a phone
    camera's white balance drift and lens do, and what no exposure scalar or response curve can express), and the learner
    slices every frame's LDR image through its own bilateral grid (bilagrid.BilateralGrid(frames), identity at the start)
    before the loss, adds 10 tv_loss() (gsplat's weight) to the step's loss and updates the grids with a torch.optim.Adam of
    their own.  Works with every eager mode, with and without batch_frames; not with graph=True.  The history gains the
    total variation, the reported loss includes its term, and the result the grids.  distort (default: as bilagrid) applies
    the gain field on its own -- distort=True, bilagrid=False is the learner without the correction on the same observations.
    vq = K > 0 (needs deg >= 1): after the last step the cloud's view-dependent SH coefficients are quantised to K centroids
    (vq.quantize_sh, 10 iterations) -- weighted by the blending-weight sums of a pass over all frames
    (ContributionStats.weight_sum) where the learner's rasterizers keep the state that pass needs (topk, absgrad), unweighted
    otherwise --, every frame is rendered again from the dequantised cloud, and the result gains `vq`: the PSNR between the
    two renders and the sizes of the cloud as scene_io.save_ply and as scene_io.save_vq write it.
    distortion = LAMBDA >= 0: the depth-distortion regulariser of Mip-NeRF 360 on every frame's blending weights
    (distortion.distortion_loss on the rasterizer's output, with the tensors the forward was given): LAMBDA times the mean of
    the [virtual, H, W] map is added to each frame's loss, and the history gains `distortion`, that mean averaged over the
    frames.  LAMBDA = 0 adds nothing and computes the map without a gradient: the run to compare with.  Works with every
    eager mode, with and without batch_frames; not with graph=True.
    normal = LAMBDA >= 0: the depth-normal consistency term (normals.normal_consistency_loss) on every frame.  The learner's
    rasterizers also return the accumulated opacity and the expected inverse depth; the per-Gaussian normals
    (normals.gaussian_normals, turned to the frame's mid pose) are composited with the frame's blending weights
    (features.composite_features with the geometry) and LAMBDA times the mean of the map, weighted by the detached alpha, is
    added to the frame's loss.  With more than one virtual pose per frame this is an APPROXIMATION: the term sees the pose
    average of the composited normals, of the alpha and of the inverse depth, with the mid pose's rotation -- not a term per
    pose.  The history gains `normal`, the mean of the map averaged over the frames.  LAMBDA = 0 computes the map without a
    gradient: the run to compare with.  Not with graph=True or batch_frames=True (neither delivers the optional outputs).
    mesh = PATH: after the last step every captured frame is rendered once more SHARP -- one pose, the middle of its exposure
    window -- with the accumulated opacity and the inverse depth; the frames are fused into a tsdf.TSDFVolume over the cloud's
    bounds as the frames see it (the 1 % .. 99 % range of the back-projected depth samples plus 5 %, 160 samples along the longest
    side; the means of an MCMC cloud bound nothing: its transparent Gaussians wander far off), colour from the LDR images, in one
    integrate call, and the mesh extract_mesh returns is written to PATH (scene_io.save_mesh_ply).  The result gains `mesh`:
    V, T, the volume's dims and voxel size.  Eager only (not with graph=True: the captured rasterizers return no depth).
    mesh_min_faces = N, mesh_keep_largest = N (only with mesh): between extract_mesh and save_mesh_ply the mesh goes through
    mesh.clean_mesh(min_faces=N, keep_largest=N) -- the floaters' blobs next to the surface go, with the degenerate faces and the
    vertices nothing references any more; `mesh` gains V_clean, T_clean and components (of the extracted mesh, by
    mesh.mesh_components) and components_clean."""
    if (mesh_min_faces is not None or mesh_keep_largest is not None) and mesh is None:
        raise ValueError("mesh_min_faces=N (--mesh-min-faces) and mesh_keep_largest=N (--mesh-keep-largest) clean the mesh of "
                         "mesh=PATH (--mesh): give that too")
    if mesh_min_faces is not None and mesh_min_faces < 0:
        raise ValueError("mesh_min_faces=N (--mesh-min-faces) must be >= 0")
    if mesh_keep_largest is not None and mesh_keep_largest < 1:
        raise ValueError("mesh_keep_largest=N (--mesh-keep-largest) must be >= 1")
    if mesh is not None and graph:
        raise ValueError("mesh=PATH (--mesh) is not supported together with graph=True (--graph): the surface is fused from the "
                         "rasterizer's return_alpha / return_invdepth outputs, which the captured step's rasterizers do not deliver")
    if normal is not None and (graph or batch_frames):
        raise ValueError("normal=LAMBDA (--normal) is not supported together with graph=True (--graph) or batch_frames=True "
                         "(--batch-frames): the term needs the rasterizer's return_alpha / return_invdepth outputs, which "
                         "neither delivers")
    if normal is not None and normal < 0:
        raise ValueError("normal=LAMBDA (--normal) must be >= 0")
    if distortion is not None and graph:
        raise ValueError("distortion=LAMBDA (--distortion) is not supported together with graph=True (--graph): the term is "
                         "not wired into the captured step")
    if distortion is not None and distortion < 0:
        raise ValueError("distortion=LAMBDA (--distortion) must be >= 0")
    if vq and deg < 1:
        raise ValueError("vq=K (--vq K) needs deg >= 1 (--deg): a degree-0 cloud has no view-dependent coefficients to quantise")
    if bilagrid and graph:
        raise ValueError("bilagrid=True (--bilagrid) is not supported together with graph=True (--graph): the captured step is "
                         "built around the rasterizers' parameters alone (the grids have an optimizer of their own)")
    distort = bilagrid if distort is None else distort
    if absgrad and (mcmc or graph):
        raise ValueError("absgrad=True (--absgrad) drives densify_and_prune or, with topk=True, densify_top_k: not together with "
                         "mcmc=True (--mcmc) or graph=True (--graph)")
    if topk and mcmc:
        raise ValueError("topk=True (--topk) and mcmc=True (--mcmc) are two refinement policies for the same learner: choose one")
    if topk and graph:
        raise ValueError("topk=True (--topk) is not supported together with graph=True (--graph): the number of Gaussians "
                         "changes at every refinement, a captured step is recorded for one size")
    if topk and filter_3d:
        raise ValueError("filter_3d=True (--filter-3d) needs mcmc=True (--mcmc)")
    if filter_3d and not mcmc:
        raise ValueError("filter_3d=True (--filter-3d) needs mcmc=True (--mcmc): the other modes hold the scales at the truth")
    if mcmc and graph:
        raise ValueError("mcmc=True (--mcmc) is not supported together with graph=True (--graph): the number of Gaussians "
                         "changes at every refinement, a captured step is recorded for one size")
    scored = topk or absgrad            # its rasterizers collect a DensifyStats
    whole = mcmc or scored              # the learner does not know the cloud: all five stored tensors are leaves
    if whole:
        fused_adam = raw = True
    if batch_frames and graph:
        raise ValueError("batch_frames=True (--batch-frames) is not supported together with graph=True (--graph): the captured "
                         "step is built around one persistent rasterizer per frame (image_formation.FrameRasterizers)")
    dev = torch.device(device)
    sc = S.make_scene(P, W, H, deg, seed=seed, hdr=True)
    cam = sc.camera
    torch.manual_seed(seed)
    knots = knots_from_lookat(frames + 3, radius=0.25)
    dt_true = torch.tensor([1.0, 0.5, 1.6, 0.8, 1.3, 0.6, 1.1, 0.9])[:frames]

    def formation(crf, **kw):
        traj = TrajectorySpline(knots, kind="cubic")
        return HDRBlurFormation(traj, frames, W, H, cam.tanfovx, cam.tanfovy, n_virtual=virtual, crf=crf, sh_degree=deg,
                                window_from_exposure=True, window_scale=0.6, **kw).to(dev)

    truth = formation(ImplicitCRF(K=128))
    with torch.no_grad():
        truth.log_exposure.copy_(dt_true.log())
        gen = torch.Generator().manual_seed(seed + 1)
        truth.trajectory.delta.copy_(0.004 * torch.randn(truth.trajectory.delta.shape, generator=gen))   # the true motion is not the prior
        cloud_true = {k: getattr(sc, k).to(dev) for k in CLOUD}
        targets = [truth(i, *[cloud_true[k] for k in CLOUD])[0] for i in range(frames)]
        if distort:
            # a vignette (1 at the centre, 0.65 in the corners) times one tint per frame and channel within +-15 %
            gen_gain = torch.Generator().manual_seed(seed + 4)
            yy = ((torch.arange(H) + 0.5) / H * 2 - 1)[:, None]
            xx = ((torch.arange(W) + 0.5) / W * 2 - 1)[None, :]
            vignette = 1.0 - 0.175 * (xx * xx + yy * yy)
            for i in range(frames):
                tint = 1.0 + 0.3 * (torch.rand(3, generator=gen_gain) - 0.5)
                targets[i] = (targets[i] * (tint[:, None, None] * vignette[None]).to(dev)).clamp(0.0, 1.0)

    # the learner: the response curve is given, everything else starts off
    # --graph: one persistent sync-free rasterizer per captured frame, so that the step's gradient computation can be
    # recorded once and replayed (graphs.GraphedStep): no host time for the few thousand tiny kernels of the pose arithmetic
    how = {"parameterization": "raw"} if raw else {}
    if normal is not None:
        how.update(return_alpha=True, return_invdepth=True)
    per_frame = FrameRasterizers(capacity=capacity or 40 * P * virtual, **how) if graph else None
    factory = per_frame if graph else (functools.partial(GaussianRasterizer, **how) if raw else None)
    filt = {"filter_3D": None}          # --filter-3d: the filter of the moment, handed to every rasterizer the learner makes
    if filter_3d:
        def factory(settings):
            return GaussianRasterizer(settings, filter_3D=filt["filter_3D"], **how)
    score = {"stats": None, "keep_state": False, "last": None}     # --topk: the statistics its rasterizers collect
    if scored:
        def factory(settings):
            score["last"] = GaussianRasterizer(settings, densify_stats=None if score["keep_state"] else score["stats"],
                                               keep_state=score["keep_state"], **how)
            return score["last"]
    geom_out = {}                       # --normal: the accumulated opacity and inverse depth of the learner's last forward
    if normal is not None:
        make = factory if factory is not None else functools.partial(GaussianRasterizer, **how)

        def factory(settings):
            rast = make(settings)

            def call(*args, **kw):          # (the formation unpacks colour, radii, hdr: the two extra images stay here)
                out = rast(*args, **kw)
                geom_out["alpha"], geom_out["invdepth"] = out[-2], out[-1]
                return out[:-2]
            return call
    model = formation(ImplicitCRF(K=128), **({"rasterizer_factory": factory} if factory is not None else {}))
    model.crf.load_state_dict(truth.crf.state_dict())
    for p_ in model.crf.parameters():
        p_.requires_grad_(False)
    gen = torch.Generator().manual_seed(seed + 2)
    shs0 = sc.shs.clone()
    shs0[:, 0] += 0.25 * torch.randn(shs0[:, 0].shape, generator=gen)
    raw_opac0 = torch.logit(sc.opacities.clamp(1e-3, 1 - 1e-3)) + 0.5 * torch.randn(sc.opacities.shape, generator=gen)
    shs = shs0.to(dev).requires_grad_(True)
    raw_opac = raw_opac0.to(dev).requires_grad_(True)
    fixed = {k: cloud_true[k] for k in ("means3D", "scales", "rotations")}
    if raw:                                                  # (the stored form of the fixed tensors: the quaternions as they are)
        fixed["scales"] = fixed["scales"].log()
    # what the rasterizer is given: the learnt radiance and opacities over the true geometry -- or, mcmc, five learnt tensors
    cur = {"means3D": fixed["means3D"], "opacities": raw_opac, "shs": shs, "scales": fixed["scales"], "rotations": fixed["rotations"]}
    with torch.no_grad():
        model.log_exposure[0] = truth.log_exposure[0]       # the gauge (see the module docstring)
    if whole:
        P0 = max(P // 4, 4)
        pick = torch.randperm(P, generator=gen)[:P0]
        xyz0 = sc.means3D[pick] + 0.02 * torch.randn(P0, 3, generator=gen)
        rgb0 = 255.0 * (scene_io.SH_C0 * (sc.shs[pick, 0] + 0.25 * torch.randn(P0, 3, generator=gen)) + 0.5)
        start = scene_io.init_from_points(xyz0.to(dev), rgb0.to(dev), sh_degree=deg, initial_opacity=0.1, device=dev)
        cur = {k: v.clone().requires_grad_(True) for k, v in start.stored(dev).items()}
        groups = cloud_param_groups(*[cur[k] for k in CLOUD], lr=dict(means3D=2e-4, opacities=5e-2, shs_dc=1e-2, shs_rest=5e-4,
                                                                       scales=5e-3, rotations=1e-3))
        for g_ in groups:
            g_["eps"] = 1e-15
        opt = GaussianAdam(groups + [{"params": [model.log_exposure], "lr": 1e-2}, {"params": [model.trajectory.delta], "lr": 5e-4}])
        cap = int(cap_max) if cap_max else P
        refine_at = [it for it in range(refine_every, steps - refine_every + 1, refine_every)] if refine_every > 0 else []
        gen_dev = torch.Generator(device=dev).manual_seed(seed + 3)
        if filter_3d:
            filt["filter_3D"] = model.compute_filter_3D(cur["means3D"])
        if scored:
            score["stats"] = DensifyStats(P0, dev, absgrad=absgrad)
            extent = float(sc.means3D.std(dim=0).norm())
    elif fused_adam:
        opt = GaussianAdam([
            {"params": [shs], "lr": 1e-2, "per_gaussian": True}, {"params": [raw_opac], "lr": 2e-2, "per_gaussian": True},
            {"params": [model.log_exposure], "lr": 1e-2}, {"params": [model.trajectory.delta], "lr": 5e-4}])
    else:
        opt = torch.optim.Adam([
            {"params": [shs], "lr": 1e-2}, {"params": [raw_opac], "lr": 2e-2},
            {"params": [model.log_exposure], "lr": 1e-2}, {"params": [model.trajectory.delta], "lr": 5e-4}])
    seen = torch.zeros(P, dtype=torch.bool, device=dev)      # Gaussians some frame of the step saw (written in place)

    def errors():
        with torch.no_grad():
            e_dt = float((model.log_exposure[1:] - truth.log_exposure[1:]).abs().mean()) if frames > 1 else 0.0
            e_pose = float((model.trajectory.knots()[:, :3, 3] - truth.trajectory.knots()[:, :3, 3]).norm(dim=1).mean())
            return e_dt, e_pose

    learn = [shs, raw_opac, model.log_exposure, model.trajectory.delta]
    if whole:
        learn = [cur[k] for k in CLOUD] + [model.log_exposure, model.trajectory.delta]
    grid_tv = {"value": None}              # --bilagrid: the total variation of the step (a device scalar)
    if bilagrid:
        grids = BilateralGrid(frames, device=dev)
        grid_opt = torch.optim.Adam(grids.parameters(), lr=2e-3, eps=1e-15)
        grid_ids = torch.arange(frames, dtype=torch.int32, device=dev)
        learn.append(grids.grids)

    dist_mean = {"value": None}            # --distortion: the mean of the step's distortion maps (a device scalar)

    def distortion_term(ldr, opac):
        """LAMBDA * mean(map) of the forward behind `ldr` (None for LAMBDA = 0); the mean goes to dist_mean"""
        if distortion > 0:
            geo = dict(means3D=cur["means3D"], opacities=opac, scales=cur["scales"], rotations=cur["rotations"])
            m = distortion_loss(ldr, geo).mean()
        else:
            m = distortion_loss(ldr).mean()
        dist_mean["value"] = m.detach() if dist_mean["value"] is None else dist_mean["value"] + m.detach()
        return distortion * m if distortion > 0 else None

    normal_mean = {"value": None}          # --normal: the mean of the step's normal-consistency maps (a device scalar)
    fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)

    def normal_term(ldr, opac, views, camposes):
        """LAMBDA * mean(map) of the forward behind `ldr` (None for LAMBDA = 0); the mean goes to normal_mean"""
        mid = views.shape[0] // 2
        with torch.enable_grad() if normal > 0 else torch.no_grad():
            n = gaussian_normals(cur["rotations"], cur["scales"], cur["means3D"], camposes[mid].detach().to(torch.float32))
            geo = dict(means3D=cur["means3D"], opacities=opac, scales=cur["scales"], rotations=cur["rotations"])
            N = composite_features(ldr, n, geometry=geo if normal > 0 else None).mean(dim=0)
            alpha, invd = geom_out["alpha"], geom_out["invdepth"]
            m = normal_consistency_loss(invd, N, fx, fy, alpha=alpha, weight=alpha.detach(),
                                        cam_to_world=views[mid, :3, :3].detach().to(torch.float32)).mean()
        normal_mean["value"] = m.detach() if normal_mean["value"] is None else normal_mean["value"] + m.detach()
        return normal * m if normal > 0 else None

    def backward_of(step_loss):
        """backward of the step's loss, with gsplat's 10 tv(grids) added under --bilagrid"""
        if bilagrid:
            tv = grids.tv_loss()
            grid_tv["value"] = tv.detach()
            step_loss = step_loss + 10.0 * tv
        step_loss.backward()

    def gradients():
        """Forward of every frame + backward of the summed loss; returns (per-frame losses, per-frame MSE) as tensors."""
        for p_ in learn:
            p_.grad = None
        # one pass over the spline for all frames (its few hundred tiny tensor operations are the step's host cost), one
        # rasterizer call per frame, one backward of the summed loss
        cams = model.cameras_all()
        opac = cur["opacities"] if raw else torch.sigmoid(raw_opac)
        losses, mses = [], []
        dist_mean["value"] = None
        normal_mean["value"] = None
        for i in range(frames):
            ldr, _, radii, _ = model(i, cur["means3D"], opac, cur["shs"], cur["scales"], cur["rotations"], cameras=cams)
            reg = distortion_term(ldr, opac) if distortion is not None else None
            if normal is not None:
                reg_n = normal_term(ldr, opac, cams[0][i], cams[2][i])
                reg = reg_n if reg is None else (reg if reg_n is None else reg + reg_n)
            if bilagrid:
                ldr = grids(ldr, i)
            if fused_adam and not whole:   # (kernels only, written in place: the captured step leaves no copy node behind)
                if i == 0:
                    torch.gt(radii, 0, out=seen)
                else:
                    seen.logical_or_(radii > 0)
            if lambda_dssim > 0:
                losses.append(photometric_loss(ldr, targets[i], lambda_dssim))
            else:
                losses.append(mean_by_rows((ldr - targets[i]).abs()))
            if reg is not None:
                losses[-1] = losses[-1] + reg
            mses.append(mean_by_rows((ldr.detach() - targets[i]) ** 2))
        backward_of(torch.stack(losses).sum())
        return torch.stack([l_.detach() for l_ in losses]), torch.stack(mses)

    target_batch = torch.stack(targets) if batch_frames else None

    def gradients_batched():
        """The same step as ONE rasterizer call over all frames and one backward; returns (losses, per-frame MSE) with
        losses.sum() the step's loss: per frame for the plain L1, ONE entry for the fused L1 + D-SSIM loss (a single loss call
        over the batch has no per-frame values)."""
        for p_ in learn:
            p_.grad = None
        opac = cur["opacities"] if raw else torch.sigmoid(raw_opac)
        ldr, _, radii, _ = model.forward_frames(range(frames), cur["means3D"], opac, cur["shs"], cur["scales"], cur["rotations"])
        dist_mean["value"] = None
        # (one map over every pose of every frame: its mean is the mean of the per-frame means; the step's loss is their sum)
        reg = distortion_term(ldr, opac) if distortion is not None else None
        if dist_mean["value"] is not None:
            dist_mean["value"] = dist_mean["value"] * frames
        if bilagrid:
            ldr = grids(ldr, grid_ids)
        if fused_adam and not whole:
            torch.gt(radii, 0, out=seen)      # (radii: the maximum over every frame's poses)
        if lambda_dssim > 0:
            # (one fused loss over the [frames, 3, H, W] batch: it averages over every plane, i.e. it is the MEAN of the
            # per-frame losses; the step's loss is their sum)
            losses = (photometric_loss(ldr, target_batch, lambda_dssim) * frames).reshape(1)
        else:
            losses = torch.stack([mean_by_rows((ldr[i] - targets[i]).abs()) for i in range(frames)])
        mses = torch.stack([mean_by_rows((ldr[i].detach() - targets[i]) ** 2) for i in range(frames)])
        if reg is not None:
            losses = torch.cat([losses, (reg * frames).reshape(1)])
        backward_of(losses.sum())
        return losses.detach(), mses

    step_fn = gradients_batched if batch_frames else gradients
    if graph:
        gradients()                                   # (creates the per-frame rasterizers)
        captured = GraphedStep(gradients, per_frame.rasterizers(frames), params=learn)

        def step_fn():
            out = captured.step()
            for p_, g_ in zip(learn, captured.grads):   # (the optimizer reads .grad: the graph's static gradient tensors)
                p_.grad = g_
            return out

    def contributions(q):
        """The blending-weight statistics of the cloud `q` over all frames (scored learners: their rasterizers can keep the state)"""
        cstats = ContributionStats(int(q["means3D"].shape[0]), dev)
        score["keep_state"] = True
        with torch.no_grad():
            cams = model.cameras_all()
            for i in range(frames):
                model(i, q["means3D"], q["opacities"], q["shs"], q["scales"], q["rotations"], cameras=cams)
                accumulate_contributions(score["last"], cstats)
        score["keep_state"] = False
        return cstats

    hist = []
    t0 = time.time()
    for it in range(steps + 1):
        losses, mses = step_fn()
        if graph and (it % 50 == 0 or it == steps):
            captured.check_overflow()
        total = float(losses.sum())
        ps = float((-10.0 * torch.log10(mses.clamp_min(1e-12))).sum())
        extra = {}
        if mcmc:
            # (the two terms are always computed, so that the last entry -- no update follows it -- reports the same loss)
            terms = regularize(opt, opacity_reg=opacity_reg, scale_reg=scale_reg).tolist()
            extra = dict(P=int(cur["means3D"].shape[0]), reg_opacity=terms[0], reg_scale=terms[1])
            total += frames * (terms[0] + terms[1])
            if filter_3d:
                extra["filter_len"] = int(filt["filter_3D"].shape[0])
        if scored:
            extra = dict(P=int(cur["means3D"].shape[0]))
        if bilagrid:
            extra["tv"] = float(grid_tv["value"])
            total += frames * 10.0 * extra["tv"]
        if distortion is not None:
            extra["distortion"] = float(dist_mean["value"]) / frames
        if normal is not None:
            extra["normal"] = float(normal_mean["value"]) / frames
        if it < steps:
            if bilagrid:
                grid_opt.step()
            g0 = model.log_exposure.grad
            if g0 is not None:
                g0[0] = 0.0                                    # frame 0's exposure is the gauge
            if mcmc:
                opt.step()                                     # every row: the regularisers act on unseen Gaussians too
                inject_noise(opt, generator=gen_dev)
                if it in refine_at:
                    relocate(opt, generator=gen_dev)
                    P_now, left = int(cur["means3D"].shape[0]), len(refine_at) - refine_at.index(it)
                    factor = min(2.0, max(1.0, (cap / P_now) ** (1.0 / left) * (1.0 + 1e-12)))
                    res = grow(opt, cap_max=cap, factor=factor, generator=gen_dev)
                    cur.update(res.params)
                    learn[:len(CLOUD)] = [cur[k] for k in CLOUD]
                    if filter_3d:                              # (the rows moved and P changed: the filter follows)
                        filt["filter_3D"] = model.compute_filter_3D(cur["means3D"])
            elif topk:
                opt.step()
                if it in refine_at:
                    P_now, left = int(cur["means3D"].shape[0]), len(refine_at) - refine_at.index(it)
                    factor = min(2.0, max(1.0, (cap / P_now) ** (1.0 / left) * (1.0 + 1e-12)))
                    k = min(cap - P_now, int(round(P_now * (factor - 1.0))))
                    by = score["stats"].mean_abs_grad() if absgrad else score["stats"].mean_grad()
                    res = densify_top_k(opt, by, k, extent=extent, generator=gen_dev)
                    score["stats"].resize(res.P_out)
                    if it == refine_at[-1]:                    # the final prune: by contribution, to nine tenths
                        res = keep_top_k(opt, contributions(res.params).weight_max, res.P_out - res.P_out // 10)
                        score["stats"].resize(res.P_out)
                    cur.update(res.params)
                    learn[:len(CLOUD)] = [cur[k] for k in CLOUD]
            elif absgrad:
                opt.step()
                if it in refine_at and int(cur["means3D"].shape[0]) < cap:
                    # (densify_and_prune zeroes the statistics at the new size itself)
                    res = densify_and_prune(opt, score["stats"], extent=extent, grad_threshold=4e-4, absgrad=True,
                                            generator=gen_dev)
                    cur.update(res.params)
                    learn[:len(CLOUD)] = [cur[k] for k in CLOUD]
            elif fused_adam:
                opt.step(visibility=seen)
            else:
                opt.step()
        e_dt, e_pose = errors()
        hist.append(dict(step=it, loss=total / frames, psnr=ps / frames, exposure_log_err=e_dt, knot_pos_err=e_pose, **extra))
        if not quiet and (it % log_every == 0 or it == steps):
            print(f"step {it:4d}  {'L1' if lambda_dssim == 0 else 'loss'} {total / frames:.5f}  PSNR {ps / frames:6.2f} dB  |log dt - truth| {e_dt:.4f}  "
                  f"knot position error {e_pose:.5f}  ({(time.time() - t0) / max(it, 1) * 1e3:.1f} ms/step)" +
                  (f"  P {extra['P']}  regularisers {extra['reg_opacity']:.5f} + {extra['reg_scale']:.5f}" if mcmc else "") +
                  (f"  P {extra['P']}" if scored else ""))
    out = dict(first=hist[0], last=hist[-1], history=hist)
    if vq:
        with torch.no_grad():
            q = {k: v.detach() for k, v in cur.items()}
            weights = contributions(q).weight_sum if scored else None
            book, codes = quantize_sh(q["shs"], vq, iters=10, weights=weights, generator=torch.Generator().manual_seed(seed + 5))
            shs_q = dequantize_sh(q["shs"][:, :1].contiguous(), book, codes)
            cams = model.cameras_all()
            opac = q["opacities"] if raw else torch.sigmoid(q["opacities"])
            mse = []
            for i in range(frames):
                full = model(i, q["means3D"], opac, q["shs"], q["scales"], q["rotations"], cameras=cams)[0]
                quant = model(i, q["means3D"], opac, shs_q, q["scales"], q["rotations"], cameras=cams)[0]
                mse.append(mean_by_rows((full - quant) ** 2))
            psnr = float((-10.0 * torch.log10(torch.stack(mse).clamp_min(1e-12))).mean())
            stored = scene_io.GaussianCloud(q["means3D"], q["shs"], q["opacities"], q["scales"] if raw else q["scales"].log(),
                                            q["rotations"])
            with tempfile.TemporaryDirectory() as tmp:
                scene_io.save_ply(os.path.join(tmp, "cloud.ply"), stored)
                scene_io.save_vq(os.path.join(tmp, "cloud.npz"), stored, book, codes)
                sizes = [os.path.getsize(os.path.join(tmp, n)) for n in ("cloud.ply", "cloud.npz")]
        out["vq"] = dict(K=int(vq), P=int(q["means3D"].shape[0]), weighted=weights is not None, psnr_full_vs_quantised_db=psnr,
                         ply_bytes=sizes[0], vq_bytes=sizes[1], sh_codebook=book, sh_codes=codes)
    if mesh is not None:
        with torch.no_grad():
            q = {k: v.detach() for k, v in cur.items()}
            opac = q["opacities"] if raw else torch.sigmoid(q["opacities"])
            w2c = model.trajectory.pose_at(model.frame_times.to(model.log_exposure.dtype))      # the mid-exposure pose of every frame
            full = torch.matmul(model.proj.to(w2c.dtype)[None], w2c)
            campos = -torch.matmul(w2c[:, :3, :3].transpose(1, 2), w2c[:, :3, 3:])[..., 0]
            views, projs = w2c.transpose(1, 2).contiguous(), full.transpose(1, 2).contiguous()
            images, alphas, invdepths = [], [], []
            for i in range(frames):
                settings = GaussianRasterizationSettings(
                    image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev),
                    scale_modifier=1.0, viewmatrix=views[i], projmatrix=projs[i], sh_degree=deg, campos=campos[i], prefiltered=False,
                    debug=False, exposure=torch.exp(model.log_exposure[i]), crf_table=model.crf.table(), crf_range=model.crf.u_range,
                    viewmatrices=views[i:i + 1], projmatrices=projs[i:i + 1], camposes=campos[i:i + 1], blur_domain=model.blur_domain)
                rast = GaussianRasterizer(settings, **{**how, "return_alpha": True, "return_invdepth": True},
                                          **({"filter_3D": filt["filter_3D"]} if filter_3d else {}))
                res = rast(q["means3D"], torch.zeros_like(q["means3D"]), opac, shs=q["shs"], scales=q["scales"], rotations=q["rotations"])
                images.append(res[0].reshape(3, H, W))
                alphas.append(res[-2].reshape(H, W))
                invdepths.append(res[-1].reshape(H, W))
            invdepths, alphas, views = torch.stack(invdepths), torch.stack(alphas), views.to(torch.float32)
            # the bounds of the cloud AS THE FRAMES SEE IT: the depth samples integrate will use, back-projected (the means of an
            # MCMC cloud do not bound anything: its transparent Gaussians random-walk far from the scene)
            seen = torch.isfinite(invdepths) & (invdepths > 0) & torch.isfinite(alphas) & (alphas >= 0.5)
            if not bool(seen.any()):
                raise RuntimeError("mesh=PATH (--mesh): no pixel of any frame has alpha >= 0.5: the cloud has no surface to fuse")
            z = torch.where(seen, alphas, torch.ones_like(alphas)) / torch.where(seen, invdepths, torch.ones_like(invdepths))
            xh = (torch.arange(W, device=dev, dtype=torch.float32) + 0.5 - W / 2) / fx
            yh = (torch.arange(H, device=dev, dtype=torch.float32) + 0.5 - H / 2) / fy
            p_cam = torch.stack([z * xh[None, None, :], z * yh[None, :, None], z], dim=-1)             # [frames, H, W, 3]
            p_world = torch.matmul(p_cam - views[:, None, None, 3, :3], views[:, None, :3, :3].transpose(-1, -2))[seen]
            p_world = p_world[:: max(1, p_world.shape[0] // 1_000_000)]
            lo, hi = (torch.quantile(p_world, x, dim=0) for x in (0.01, 0.99))
            pad = 0.05 * (hi - lo) + 1e-3
            lo, hi = lo - pad, hi + pad
            voxel = float((hi - lo).max()) / 159.0
            volume = TSDFVolume.from_bounds(lo.tolist(), hi.tolist(), voxel, color=True, device=dev)
            volume.integrate(invdepths, views, fx, fy, alpha=alphas, color=torch.stack(images))
            vertices, faces, colors = volume.extract_mesh()
            cleaned = None
            if mesh_min_faces is not None or mesh_keep_largest is not None:
                from casualhdrsplat_amd.mesh import clean_mesh, mesh_components
                raw = (int(vertices.shape[0]), int(faces.shape[0]), int(mesh_components(faces, vertices.shape[0])[0].unique().numel()))
                vertices, faces, colors = clean_mesh(vertices, faces, colors, min_faces=mesh_min_faces or 0,
                                                     keep_largest=mesh_keep_largest)
                cleaned = dict(V_clean=int(vertices.shape[0]), T_clean=int(faces.shape[0]), components=raw[2],
                               components_clean=int(mesh_components(faces, vertices.shape[0])[0].unique().numel()))
            scene_io.save_mesh_ply(mesh, vertices, faces, colors)
        out["mesh"] = dict(V=int(vertices.shape[0]), T=int(faces.shape[0]), dims=volume.dims, voxel_size=volume.voxel_size,
                           observed=int((volume.weight >= 1).sum()), path=mesh)
        if cleaned is not None:
            out["mesh"].update(cleaned, V=raw[0], T=raw[1])
    if bilagrid:
        out["grids"] = grids.grids.detach()
    if whole:
        out["cloud"] = {k: cur[k].detach() for k in CLOUD}
        if filter_3d:
            out["filter_3D"] = filt["filter_3D"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--P", type=int, default=20000)
    ap.add_argument("--W", type=int, default=320)
    ap.add_argument("--H", type=int, default=208)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--virtual", type=int, default=5, help="virtual poses per captured frame")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deg", type=int, default=1)
    ap.add_argument("--graph", action="store_true", help="record the gradient computation once as a HIP graph and replay it")
    ap.add_argument("--lambda-dssim", type=float, default=0.0,
                    help="weight of the D-SSIM term of the published 3DGS loss (0.2 upstream; 0 = plain L1)")
    ap.add_argument("--fused-adam", action="store_true",
                    help="update through casualhdrsplat_amd.optim.GaussianAdam (one launch; per-Gaussian tensors only in the rows "
                         "some frame of the step saw) instead of torch.optim.Adam")
    ap.add_argument("--raw", action="store_true",
                    help="pass the stored (logit) opacities to GaussianRasterizer(..., parameterization='raw') instead of "
                         "torch.sigmoid in front of the default rasterizer")
    ap.add_argument("--batch-frames", action="store_true",
                    help="render all frames of a step in ONE rasterizer call (settings.n_frames; HDRBlurFormation.forward_frames) "
                         "instead of one call per frame; eager only (not with --graph)")
    ap.add_argument("--mcmc", action="store_true",
                    help="learn the whole cloud (positions, opacities, radiance, scales, rotations) from P / 4 noised points under "
                         "the MCMC policy: regularize, step, inject_noise every step, relocate + grow every --refine-every steps; "
                         "implies --fused-adam --raw; eager only (not with --graph)")
    ap.add_argument("--filter-3d", action="store_true",
                    help="--mcmc: the 3D smoothing filter of Mip-Splatting, computed from every virtual pose at the start and after "
                         "every grow and folded into the opacities and scales the rasterizers run on")
    ap.add_argument("--topk", action="store_true",
                    help="learn the whole cloud from P / 4 noised points under a score-driven budget: every --refine-every steps "
                         "densify_top_k clones / splits the rows with the largest mean view-space gradient towards --cap-max, and the "
                         "last refinement keeps the nine tenths with the largest blending weight (keep_top_k); eager only, not "
                         "with --mcmc")
    ap.add_argument("--absgrad", action="store_true",
                    help="collect the absolute screen-gradient statistic of AbsGS in every backward: with --topk it is the score "
                         "of densify_top_k; on its own the same learner runs densify_and_prune(absgrad=True) every "
                         "--refine-every steps while the cloud is below --cap-max; eager only, not with --mcmc")
    ap.add_argument("--bilagrid", action="store_true",
                    help="multiply the observations by a smooth per-frame gain field (vignette x tint) and slice every frame's image "
                         "through its own bilateral grid before the loss (+ 10 tv_loss(), the grids under torch.optim.Adam); "
                         "eager only (not with --graph)")
    ap.add_argument("--vq", type=int, default=0, metavar="K",
                    help="after training, quantise the view-dependent SH coefficients to K centroids (needs --deg >= 1; weighted by "
                         "the blending-weight sums under --topk / --absgrad), render every frame again from the dequantised cloud and "
                         "print the PSNR between the two renders and both file sizes")
    ap.add_argument("--distortion", type=float, default=None, metavar="LAMBDA",
                    help="add LAMBDA times the mean depth-distortion map of every frame (distortion.distortion_loss) to its loss and "
                         "print that mean; 0 prints it without adding the term; eager only (not with --graph)")
    ap.add_argument("--normal", type=float, default=None, metavar="LAMBDA",
                    help="add LAMBDA times the mean depth-normal consistency map of every frame (normals.normal_consistency_loss on "
                         "the composited normals.gaussian_normals, weighted by the detached alpha) to its loss and print that mean; "
                         "0 prints it without adding the term.  With more than one virtual pose per frame this is an approximation: "
                         "the term is applied to the pose average of the composited normals, alpha and inverse depth, with the mid "
                         "pose's rotation.  Eager only: not with --graph or --batch-frames")
    ap.add_argument("--mesh", type=str, default=None, metavar="PATH",
                    help="after training, render every captured frame sharp (one pose, mid exposure) with alpha and inverse depth, "
                         "fuse them into a TSDF volume over the bounds of the cloud as those views see it (tsdf.TSDFVolume) and write the extracted triangle "
                         "mesh to PATH as PLY; prints V, T and the volume's size.  Eager only (not with --graph)")
    ap.add_argument("--mesh-min-faces", type=int, default=None, metavar="N",
                    help="--mesh: drop the connected components of the mesh with fewer than N faces (mesh.clean_mesh) before it "
                         "is written; prints the cleaned V and T and the number of components")
    ap.add_argument("--mesh-keep-largest", type=int, default=None, metavar="N",
                    help="--mesh: keep the N largest connected components of the mesh (mesh.clean_mesh) before it is written; with "
                         "--mesh-min-faces a component must pass both")
    ap.add_argument("--cap-max", type=int, default=None, help="--mcmc: the budget of Gaussians the cloud grows to (default: P)")
    ap.add_argument("--refine-every", type=int, default=25, help="--mcmc: steps between two relocate + grow")
    ap.add_argument("--opacity-reg", type=float, default=0.01, help="--mcmc: weight of mean|opacity| (0.01 upstream)")
    ap.add_argument("--scale-reg", type=float, default=0.01, help="--mcmc: weight of mean|scale| (0.01 upstream)")
    a = ap.parse_args(argv)
    if (a.mesh_min_faces is not None or a.mesh_keep_largest is not None) and not a.mesh:
        ap.error("--mesh-min-faces and --mesh-keep-largest clean the mesh of --mesh PATH: give that too")
    r = run(a.P, a.W, a.H, a.frames, a.virtual, a.steps, a.seed, a.deg, graph=a.graph, lambda_dssim=a.lambda_dssim,
            fused_adam=a.fused_adam, raw=a.raw, batch_frames=a.batch_frames, mcmc=a.mcmc, cap_max=a.cap_max,
            refine_every=a.refine_every, opacity_reg=a.opacity_reg, scale_reg=a.scale_reg, filter_3d=a.filter_3d, topk=a.topk,
            absgrad=a.absgrad, bilagrid=a.bilagrid, vq=a.vq, distortion=a.distortion, normal=a.normal, mesh=a.mesh,
            mesh_min_faces=a.mesh_min_faces, mesh_keep_largest=a.mesh_keep_largest)
    f, l = r["first"], r["last"]
    print(f"loss {f['loss']:.5f} -> {l['loss']:.5f}; PSNR {f['psnr']:.2f} -> {l['psnr']:.2f} dB; exposure error "
          f"{f['exposure_log_err']:.4f} -> {l['exposure_log_err']:.4f}; knot error {f['knot_pos_err']:.5f} -> {l['knot_pos_err']:.5f}")
    if a.distortion is not None:
        print(f"mean distortion map {f['distortion']:.6f} -> {l['distortion']:.6f} (lambda {a.distortion:g})")
    if a.normal is not None:
        print(f"mean normal-consistency map {f['normal']:.6f} -> {l['normal']:.6f} (lambda {a.normal:g})")
    if a.mesh:
        m = r["mesh"]
        print(f"mesh {m['path']}: V {m['V']}, T {m['T']}; volume {m['dims'][0]} x {m['dims'][1]} x {m['dims'][2]} samples of "
              f"{m['voxel_size']:.5f} ({m['observed']} observed)")
        if "T_clean" in m:
            print(f"mesh cleaned: V {m['V_clean']}, T {m['T_clean']}; components {m['components']} -> {m['components_clean']}")
    if a.vq:
        v = r["vq"]
        print(f"vq K {v['K']} ({'weighted by contribution' if v['weighted'] else 'unweighted'}), P {v['P']}: PSNR full vs quantised "
              f"{v['psnr_full_vs_quantised_db']:.2f} dB; save_ply {v['ply_bytes']} B, save_vq {v['vq_bytes']} B "
              f"({v['ply_bytes'] / v['vq_bytes']:.2f} x)")


if __name__ == "__main__":
    main()
