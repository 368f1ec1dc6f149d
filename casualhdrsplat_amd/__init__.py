"""casualhdrsplat_amd -- MI355X-native differentiable 3D Gaussian rasterizer for HDR splatting.

Scope: the rasterizer hot path, behind the
GaussianRasterizer / GaussianRasterizationSettings API, and the fused L1 + D-SSIM training loss
that consumes its images (losses.photometric_loss, losses.ssim) and the fused, visibility-masked
Adam step that applies the gradients (optim.GaussianAdam), and the densify / prune of the cloud that
changes the number of Gaussians under that optimizer (densify.densify_and_prune), and the neighbour
distances that size a new cloud (knn.knn_mean_dist2, scene_io.init_from_points), and the MCMC policy's
relocation, growth, position noise and regularisers (mcmc.relocate, mcmc.grow, mcmc.inject_noise, mcmc.regularize), and the
3D smoothing filter of Mip-Splatting (smoothing.compute_filter_3D, GaussianRasterizer(..., filter_3D=...)), and the per-Gaussian
blending-weight statistics contribution-based policies decide from (importance.accumulate_contributions), and the
absolute screen-gradient statistic of AbsGS (DensifyStats(absgrad=True), importance.accumulate_abs_gradients), and the
score-driven row edits that act on them (rows.prune_rows, rows.keep_top_k, rows.densify_top_k), and the per-frame
bilateral-grid colour correction between the rasterizer's image and the loss (bilagrid.BilateralGrid, bilagrid.slice_image,
bilagrid.tv_loss), and the k-means codebook compression of a finished cloud's view-dependent SH coefficients (vq.quantize_sh,
vq.kmeans, scene_io.save_vq), and the lens undistortion of captured frames, fused with the downscale to the training resolution
(undistort.undistort_map, undistort.undistort_frames, undistort.undistorted_camera), and the compositing of any number of
per-Gaussian feature channels with a finished forward's blending weights (features.composite_features), and the depth-distortion
regulariser on the blending weights of a ray (distortion.distortion_loss), and the depth-normal consistency term with the
per-Gaussian normals it composites (normals.normal_consistency_loss, normals.gaussian_normals), and the fusion of rendered
depth maps into a truncated signed distance volume with the triangle mesh extracted from it (tsdf.TSDFVolume,
scene_io.save_mesh_ply), and that mesh's clean-up by connected components (mesh.clean_mesh, mesh.mesh_components).  Compute lives in
casualhdrsplat_amd/libhdrsplat.so (hand-written HIP, gfx950) reached through the C ABI of
include/hdrsplat.h; importing the package does not load the library, calling it does, and a
missing library is a hard error (no CPU fallback).
"""
from .bilagrid import BilateralGrid, slice_image, tv_loss
from .densify import DensifyResult, densify_and_prune
from .distortion import distortion_loss
from .features import composite_features
from .importance import ContributionStats, accumulate_abs_gradients, accumulate_contributions
from .knn import knn_mean_dist2
from .losses import photometric_loss, ssim
from .mcmc import GrowResult, RelocateResult, grow, inject_noise, regularize, relocate
from .mesh import clean_mesh, mesh_components
from .normals import gaussian_normals, normal_consistency_loss
from .optim import GaussianAdam, cloud_param_groups
from .rasterizer import (BinningOverflow, DensifyStats, GaussianRasterizationSettings, GaussianRasterizer,
                         SortChainStalled, inspect_state, rasterize_gaussians)
from .rows import RowsResult, densify_top_k, keep_top_k, prune_rows
from .smoothing import apply_filter_3D, compute_filter_3D
from .tsdf import TSDFVolume
from .undistort import UndistortMap, undistort_frames, undistort_map, undistorted_camera
from .vq import VQResult, dequantize_sh, kmeans, kmeans_assign, kmeans_update, quantize_sh

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "DensifyStats", "BinningOverflow", "SortChainStalled",
           "rasterize_gaussians", "inspect_state", "photometric_loss", "ssim", "GaussianAdam", "cloud_param_groups",
           "densify_and_prune", "DensifyResult", "knn_mean_dist2",
           "relocate", "grow", "inject_noise", "regularize", "RelocateResult", "GrowResult",
           "compute_filter_3D", "apply_filter_3D", "ContributionStats", "accumulate_contributions", "accumulate_abs_gradients",
           "prune_rows", "keep_top_k", "densify_top_k", "RowsResult", "BilateralGrid", "slice_image", "tv_loss",
           "kmeans", "kmeans_assign", "kmeans_update", "quantize_sh", "dequantize_sh", "VQResult",
           "undistorted_camera", "undistort_map", "undistort_frames", "UndistortMap",
           "composite_features", "distortion_loss", "normal_consistency_loss", "gaussian_normals",
           "TSDFVolume", "clean_mesh", "mesh_components"]
__version__ = "0.1.0"
