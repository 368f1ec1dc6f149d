"""ctypes binding of libhdrsplat.so -- the C ABI declared in include/hdrsplat.h.

The shared library is built in-tree by `make -C casualhdrsplat_amd/csrc` (hipcc, gfx950) and
is the ONLY compute path of this package: there is no CPU or PyTorch fallback.  If the library
is missing or a symbol cannot be resolved, loading fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HS_LIB_PATH", os.path.join(_HERE, "libhdrsplat.so"))

HS_VERSION = 309  # the hdrsplat.h whose structs the classes below mirror: load() refuses a library of another version
HS_OK, HS_EINVAL, HS_EHIP, HS_EOVERFLOW = 0, -1, -2, -3
HS_STAGE_PREPROCESS, HS_STAGE_BIN, HS_STAGE_RENDER, HS_STAGE_ALL, HS_STAGE_OFFSETS = 1, 2, 4, 7, 8
HS_STAGE_PREPROCESS_ONLY = 16
HS_FLAG_HDR, HS_FLAG_BLUR_HDR, HS_FLAG_DEBUG, HS_FLAG_ANTIALIAS = 1, 2, 4, 8
HS_FLAG_RADIANCE_EXP, HS_FLAG_RADIANCE_SOFTPLUS = 16, 32
HS_BWD_RENDER, HS_BWD_PREPROCESS, HS_BWD_CRF, HS_BWD_ALL = 1, 2, 4, 7
HS_BWD_SEGSUM, HS_BWD_PROJECT = 8, 16
HS_TILE = 16
# hs_fwd_args.tile_sort / depth_sort / chain_order / emission_scan (0 = auto in each)
HS_TILE_SORT_RADIX, HS_TILE_SORT_COUNT, HS_TILE_SORT_HIER = 1, 2, 3
HS_DEPTH_SORT_PASSES, HS_DEPTH_SORT_COUNT = 1, 2
HS_CHAIN_BLOCKIDX, HS_CHAIN_TICKETS = 1, 2
HS_EMISSION_SCAN_AHEAD, HS_EMISSION_SCAN_INSIDE = 1, 2

_fp = C.c_void_p  # device pointers travel as plain addresses


class hs_dims(C.Structure):
    _fields_ = [("P", C.c_int32), ("M", C.c_int32), ("sh_degree", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
                ("n_poses", C.c_int32), ("capacity", C.c_int64), ("crf_K", C.c_int32), ("n_frames", C.c_int32)]


class hs_sizes(C.Structure):
    _fields_ = [("geom_bytes", C.c_int64), ("binning_bytes", C.c_int64), ("image_bytes", C.c_int64),
                ("bwd_bytes", C.c_int64)]


class hs_counters(C.Structure):
    _fields_ = [("num_rendered", C.c_uint32), ("overflow", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class hs_fwd_args(C.Structure):
    _fields_ = [
        ("dims", hs_dims),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("flags", C.c_int32), ("stages", C.c_int32), ("crf_K", C.c_int32),
        ("crf_umin", C.c_float), ("crf_umax", C.c_float),
        ("bg", _fp), ("viewmatrices", _fp), ("projmatrices", _fp), ("camposes", _fp),
        ("means3D", _fp), ("opacities", _fp), ("shs", _fp), ("colors_precomp", _fp), ("scales", _fp),
        ("rotations", _fp), ("cov3D_precomp", _fp), ("exposure", _fp), ("crf_table", _fp),
        ("geom", _fp), ("binning", _fp), ("image", _fp),
        ("out_color", _fp), ("out_hdr", _fp), ("radii", _fp), ("out_invdepth", _fp), ("counters_host", _fp),
        ("tile_sort", C.c_int32), ("depth_sort", C.c_int32), ("chain_order", C.c_int32), ("emission_scan", C.c_int32),
        ("depth_range_cap", C.c_int32), ("depth_dist_max", C.c_int32),
    ]


class hs_bwd_args(C.Structure):
    _fields_ = [
        ("dims", hs_dims),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("flags", C.c_int32), ("stages", C.c_int32), ("crf_K", C.c_int32), ("crf_umin", C.c_float),
        ("crf_umax", C.c_float),
        ("bg", _fp), ("viewmatrices", _fp), ("projmatrices", _fp), ("camposes", _fp),
        ("means3D", _fp), ("opacities", _fp), ("shs", _fp), ("colors_precomp", _fp), ("scales", _fp),
        ("rotations", _fp), ("cov3D_precomp", _fp), ("exposure", _fp), ("crf_table", _fp),
        ("geom", _fp), ("binning", _fp), ("image", _fp), ("bwd", _fp),
        ("dL_dout_color", _fp), ("dL_dout_hdr", _fp), ("dL_dout_alpha", _fp),
        ("dL_dmeans3D", _fp), ("dL_dmeans2D", _fp), ("dL_dopacities", _fp), ("dL_dshs", _fp),
        ("dL_dcolors_precomp", _fp), ("dL_dscales", _fp), ("dL_drotations", _fp), ("dL_dcov3D_precomp", _fp),
        ("dL_dexposure", _fp), ("dL_dcrf_table", _fp),
        ("dL_dviewmatrices", _fp), ("dL_dprojmatrices", _fp), ("dL_dcamposes", _fp),
        ("dL_dview_colors", _fp), ("dL_dout_invdepth", _fp),
        ("densify_grad_accum", _fp), ("densify_denom", _fp), ("densify_max_radii", _fp),
        ("g_begin", C.c_int32), ("g_end", C.c_int32),
    ]


class hs_layout(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "counters", "rec", "depth", "radii", "tiles_touched", "offsets", "cov3D", "clamped", "scan_spine", "binfo",
        "keys_sorted", "point_list", "pairs_tmp", "ranges", "sort_tmp", "depth_pairs", "inst_sorted", "offs_sorted", "pair_sort_tmp",
        "pair_flags", "pair_act",
        "final_T", "n_contrib", "pose_hdr", "tile_work", "tile_order",
        "pair_grads", "crf_partials", "inst_grads", "pose_partials",
        "tile_matrix", "hier_ws", "depth_ws")]


class hs_loss_args(C.Structure):
    _fields_ = [("planes", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("lambda_dssim", C.c_float),
                ("image", _fp), ("target", _fp), ("workspace", _fp), ("partials", _fp), ("out", _fp),
                ("dL_dloss", _fp), ("dL_dimage", _fp)]


HS_ADAM_MAX_GROUPS = 16
HS_ADAM_MASK_NONE, HS_ADAM_MASK_RADII, HS_ADAM_MASK_BYTES = 0, 1, 2


class hs_adam_group(C.Structure):
    _fields_ = [("param", _fp), ("grad", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp),
                ("rows", C.c_int64), ("row_stride", C.c_int64), ("col_begin", C.c_int64), ("col_count", C.c_int64),
                ("masked", C.c_int32), ("reserved", C.c_int32)]


class hs_adam_args(C.Structure):
    _fields_ = [("groups", C.POINTER(hs_adam_group)), ("n_groups", C.c_int32), ("mask_kind", C.c_int32),
                ("mask", _fp), ("mask_len", C.c_int64), ("state", _fp), ("hyper", _fp)]


HS_DENSIFY_MAX_MATRICES = 16
HS_DENSIFY_RAW_OPACITY, HS_DENSIFY_RAW_SCALES = 1, 2
HS_DENSIFY_COPY, HS_DENSIFY_ZERO_NEW, HS_DENSIFY_MEANS, HS_DENSIFY_SCALES = 0, 1, 2, 3
HS_DENSIFY_KIND_SURVIVOR, HS_DENSIFY_KIND_CLONE, HS_DENSIFY_KIND_CHILD0, HS_DENSIFY_KIND_CHILD1 = 0, 1, 2, 3
HS_DENSIFY_COUNTS = 8


class hs_densify_matrix(C.Structure):
    _fields_ = [("src", _fp), ("dst", _fp), ("row_stride", C.c_int64), ("role", C.c_int32), ("reserved", C.c_int32)]


class hs_densify_args(C.Structure):
    _fields_ = [("P", C.c_int64), ("P_out", C.c_int64), ("flags", C.c_int32), ("r_max", C.c_int32),
                ("tau_grad", C.c_float), ("tau_split", C.c_float), ("o_min", C.c_float), ("sigma_max", C.c_float),
                ("grad_accum", _fp), ("denom", _fp), ("max_radii", _fp), ("opacities", _fp), ("scales", _fp),
                ("rotations", _fp), ("noise", _fp), ("workspace", _fp), ("row_map", _fp), ("counts", _fp),
                ("counts_host", _fp), ("matrices", C.POINTER(hs_densify_matrix)), ("n_matrices", C.c_int32),
                ("reserved", C.c_int32)]


HS_ROWS_MASK, HS_ROWS_KEEP, HS_ROWS_DENSIFY = 0, 1, 2


class hs_rows_args(C.Structure):
    _fields_ = [("P", C.c_int64), ("k", C.c_int64), ("mode", C.c_int32), ("flags", C.c_int32), ("tau_split", C.c_float),
                ("reserved", C.c_int32), ("score", _fp), ("mask", _fp), ("scales", _fp), ("workspace", _fp), ("row_map", _fp),
                ("counts", _fp), ("counts_host", _fp)]


class hs_activate_args(C.Structure):
    _fields_ = [("P", C.c_int64), ("g_begin", C.c_int64), ("g_end", C.c_int64),
                ("opacity_raw", _fp), ("scales_raw", _fp), ("rotations_raw", _fp),
                ("opacities", _fp), ("scales", _fp), ("rotations", _fp),
                ("dL_dopacities", _fp), ("dL_dscales", _fp), ("dL_drotations", _fp)]


class hs_knn_args(C.Structure):
    _fields_ = [("P", C.c_int64), ("xyz", _fp), ("mean_d2", _fp), ("workspace", _fp), ("status", _fp)]


HS_MCMC_RELOCATE, HS_MCMC_GROW = 0, 1
HS_MCMC_COUNTS = 8


class hs_mcmc_args(C.Structure):
    _fields_ = [("P", C.c_int64), ("n_draws", C.c_int64), ("mode", C.c_int32), ("flags", C.c_int32),
                ("o_min", C.c_float), ("reserved", C.c_float), ("min_opacity", C.c_double),
                ("opacities", _fp), ("scales", _fp), ("u", _fp), ("workspace", _fp), ("row_map", _fp), ("counts", _fp),
                ("counts_host", _fp), ("matrices", C.POINTER(hs_densify_matrix)), ("n_matrices", C.c_int32),
                ("reserved2", C.c_int32)]


class hs_mcmc_noise_args(C.Structure):
    _fields_ = [("P", C.c_int64), ("flags", C.c_int32), ("scaler", C.c_float),
                ("means3D", _fp), ("opacities", _fp), ("scales", _fp), ("rotations", _fp), ("xi", _fp)]


class hs_mcmc_reg_args(C.Structure):
    _fields_ = [("P", C.c_int64), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("lambda_opacity", C.c_double), ("lambda_scale", C.c_double),
                ("opacities", _fp), ("scales", _fp), ("dL_dopacities", _fp), ("dL_dscales", _fp),
                ("loss", _fp), ("workspace", _fp)]


class hs_smoothing_filter_args(C.Structure):
    _fields_ = [("P", C.c_int64), ("C", C.c_int64), ("xyz", _fp), ("viewmatrices", _fp), ("intrinsics", _fp),
                ("filter", _fp), ("n_views", _fp), ("workspace", _fp)]


class hs_smoothing_apply_args(C.Structure):
    _fields_ = [("P", C.c_int64), ("g_begin", C.c_int64), ("g_end", C.c_int64),
                ("opacity_raw", _fp), ("scales_raw", _fp), ("filter", _fp), ("opacities", _fp), ("scales", _fp),
                ("dL_dopacities", _fp), ("dL_dscales", _fp)]


class hs_contribution_args(C.Structure):
    _fields_ = [("dims", hs_dims), ("geom", _fp), ("binning", _fp), ("image", _fp), ("ws", _fp), ("pixel_weight", _fp),
                ("weight_sum", _fp), ("weight_max", _fp), ("pixel_count", _fp)]


class hs_abs_gradient_args(C.Structure):
    _fields_ = [("dims", hs_dims), ("flags", C.c_int32), ("crf_K", C.c_int32), ("crf_umin", C.c_float), ("crf_umax", C.c_float),
                ("bg", _fp), ("exposure", _fp), ("crf_table", _fp), ("geom", _fp), ("binning", _fp), ("image", _fp), ("ws", _fp),
                ("dL_dout_color", _fp), ("dL_dout_hdr", _fp), ("dL_dout_alpha", _fp), ("dL_dout_invdepth", _fp),
                ("abs_grad_accum", _fp)]


class hs_composite_features_args(C.Structure):
    _fields_ = [("dims", hs_dims), ("geom", _fp), ("binning", _fp), ("image", _fp), ("n_channels", C.c_int32),
                ("reserved", C.c_int32), ("features", _fp), ("out", _fp)]


class hs_composite_features_bwd_args(C.Structure):
    _fields_ = [("dims", hs_dims), ("geom", _fp), ("binning", _fp), ("image", _fp), ("ws", _fp), ("n_channels", C.c_int32),
                ("reserved", C.c_int32), ("dL_dout", _fp), ("dL_dfeatures", _fp)]


class hs_composite_features_geometry_args(C.Structure):
    _fields_ = [("dims", hs_dims), ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
                ("flags", C.c_int32), ("viewmatrices", _fp), ("projmatrices", _fp), ("camposes", _fp), ("means3D", _fp),
                ("opacities", _fp), ("scales", _fp), ("rotations", _fp), ("geom", _fp), ("binning", _fp), ("image", _fp),
                ("ws", _fp), ("n_channels", C.c_int32), ("reserved", C.c_int32), ("features", _fp), ("dL_dout", _fp),
                ("dL_dmeans3D", _fp), ("dL_dopacities", _fp), ("dL_dscales", _fp), ("dL_drotations", _fp)]


class hs_distortion_args(C.Structure):
    _fields_ = [("dims", hs_dims), ("geom", _fp), ("binning", _fp), ("image", _fp), ("out_distortion", _fp), ("out_moment", _fp)]


class hs_distortion_bwd_args(C.Structure):
    _fields_ = [("dims", hs_dims), ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
                ("flags", C.c_int32), ("viewmatrices", _fp), ("projmatrices", _fp), ("camposes", _fp), ("means3D", _fp),
                ("opacities", _fp), ("scales", _fp), ("rotations", _fp), ("geom", _fp), ("binning", _fp), ("image", _fp),
                ("ws", _fp), ("moment", _fp), ("dL_ddistortion", _fp),
                ("dL_dmeans3D", _fp), ("dL_dopacities", _fp), ("dL_dscales", _fp), ("dL_drotations", _fp)]


class hs_bilagrid_args(C.Structure):
    _fields_ = [("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("G", C.c_int32), ("L", C.c_int32), ("Y", C.c_int32),
                ("X", C.c_int32), ("reserved", C.c_int32),
                ("image", _fp), ("grids", _fp), ("grid_ids", _fp), ("out", _fp), ("dL_dout", _fp), ("dL_dimage", _fp),
                ("dL_dgrids", _fp), ("workspace", _fp)]


HS_BILAGRID_TV_WORKSPACE_BYTES = 24576


class hs_bilagrid_tv_args(C.Structure):
    _fields_ = [("G", C.c_int32), ("L", C.c_int32), ("Y", C.c_int32), ("X", C.c_int32),
                ("grids", _fp), ("tv", _fp), ("dL_dtv", _fp), ("dL_dgrids", _fp), ("workspace", _fp)]


class hs_vq_args(C.Structure):
    _fields_ = [("N", C.c_int32), ("D", C.c_int32), ("K", C.c_int32),
                ("x", _fp), ("weights", _fp), ("codebook_in", _fp), ("codes", _fp), ("dist2", _fp), ("codebook_out", _fp),
                ("counts", _fp), ("workspace", _fp)]


HS_CAMERA_MODELS = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV")  # HS_CAMERA_* = index


class hs_undistort_args(C.Structure):
    _fields_ = [("model", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("Wf", C.c_int32), ("Hf", C.c_int32), ("F", C.c_int32),
                ("factor", C.c_int32), ("frames_u8", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k", C.c_float * 8),
                ("map", _fp), ("valid", _fp), ("frames", _fp), ("out", _fp)]


class hs_normal_consistency_args(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("reserved", C.c_int32), ("fx", C.c_float), ("fy", C.c_float),
                ("invdepth", _fp), ("alpha", _fp), ("normals", _fp), ("weight", _fp), ("cam_to_world", _fp),
                ("out", _fp), ("depth_normals", _fp), ("dL_dout", _fp), ("dL_dnormals", _fp), ("dL_dinvdepth", _fp),
                ("dL_dalpha", _fp), ("workspace", _fp)]


class hs_gaussian_normals_args(C.Structure):
    _fields_ = [("P", C.c_int64), ("rotations", _fp), ("scales", _fp), ("means3D", _fp), ("campos", _fp), ("normals", _fp),
                ("dL_dnormals", _fp), ("dL_drotations", _fp)]


class hs_tsdf_args(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("origin", C.c_float * 3), ("voxel_size", C.c_float), ("trunc", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("min_alpha", C.c_float), ("max_depth", C.c_float), ("min_weight", C.c_float),
                ("tsdf", _fp), ("weight", _fp), ("color", _fp), ("invdepth", _fp), ("alpha", _fp), ("frame_color", _fp),
                ("viewmatrices", _fp), ("workspace", _fp), ("totals", _fp), ("n_vertices", C.c_int64), ("n_faces", C.c_int64),
                ("vertices", _fp), ("faces", _fp), ("colors", _fp)]


class hs_mesh_args(C.Structure):
    _fields_ = [("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("min_faces", C.c_int64), ("keep_largest", C.c_int64),
                ("remove_degenerate", C.c_int32), ("reserved", C.c_int32),
                ("vertices", _fp), ("faces", _fp), ("colors", _fp), ("workspace", _fp), ("label", _fp), ("size", _fp),
                ("totals", _fp), ("n_vertices_out", C.c_int64), ("n_faces_out", C.c_int64),
                ("vertices_out", _fp), ("faces_out", _fp), ("colors_out", _fp), ("vertex_index", _fp), ("face_index", _fp)]


def _call(args):
    """int f(const args*, void* hip_stream): the shape of most entry points"""
    return C.c_int, [C.POINTER(args), C.c_void_p]


# Every export of include/hdrsplat.h: name -> (restype, argtypes; None = not declared).  load() sets the signatures from this
# table and EXPORTS is its keys: a new entry point takes one line here.
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
SIGNATURES = {
    "hs_version": (C.c_int, None),
    "hs_last_error": (C.c_char_p, None),
    "hs_plan": (C.c_int, [C.POINTER(hs_dims), C.POINTER(hs_sizes), C.POINTER(hs_layout)]),
    "hs_forward": _call(hs_fwd_args),
    "hs_backward": _call(hs_bwd_args),
    "hs_mark_visible": (C.c_int, [_i32, _vp, _vp, _vp, _vp]),
    "hs_sh_backward_views": (C.c_int, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "hs_sort_tmp_bytes": (_i64, [_i64]),
    "hs_sort_pairs": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "hs_render_stats": (C.c_int, [C.POINTER(hs_fwd_args), C.POINTER(hs_bwd_args), _vp, _vp, _vp]),
    "hs_sort_tickets": (C.c_int, [C.c_int]),
    "hs_spline_poses": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hs_depth_sort": (C.c_int, [C.c_int]),
    "hs_loss_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "hs_photometric_loss": _call(hs_loss_args),
    "hs_photometric_loss_backward": _call(hs_loss_args),
    "hs_adam_state_bytes": (_i64, [_i32]),
    "hs_adam_step": _call(hs_adam_args),
    "hs_densify_workspace_bytes": (_i64, [_i64]),
    "hs_densify_plan": _call(hs_densify_args),
    "hs_densify_apply": _call(hs_densify_args),
    "hs_activate": _call(hs_activate_args),
    "hs_activate_backward": _call(hs_activate_args),
    "hs_max_frames": (C.c_int, []),
    "hs_knn_workspace_bytes": (_i64, [_i64]),
    "hs_knn_mean_dist_sq": _call(hs_knn_args),
    "hs_mcmc_workspace_bytes": (_i64, [_i64, _i64]),
    "hs_mcmc_sample": _call(hs_mcmc_args),
    "hs_mcmc_update": _call(hs_mcmc_args),
    "hs_mcmc_noise": _call(hs_mcmc_noise_args),
    "hs_mcmc_reg_workspace_bytes": (_i64, [_i64]),
    "hs_mcmc_regularize": _call(hs_mcmc_reg_args),
    "hs_smoothing_filter_workspace_bytes": (_i64, [_i64]),
    "hs_smoothing_filter": _call(hs_smoothing_filter_args),
    "hs_smoothing_apply": _call(hs_smoothing_apply_args),
    "hs_smoothing_apply_backward": _call(hs_smoothing_apply_args),
    "hs_contribution_workspace_bytes": (_i64, [C.POINTER(hs_dims)]),
    "hs_contribution": _call(hs_contribution_args),
    "hs_abs_gradient_workspace_bytes": (_i64, [C.POINTER(hs_dims)]),
    "hs_abs_gradient": _call(hs_abs_gradient_args),
    "hs_rows_workspace_bytes": (_i64, [_i64]),
    "hs_rows_plan": _call(hs_rows_args),
    "hs_bilagrid_workspace_bytes": (_i64, [_i32] * 7),
    "hs_bilagrid_slice": _call(hs_bilagrid_args),
    "hs_bilagrid_slice_backward": _call(hs_bilagrid_args),
    "hs_bilagrid_tv": _call(hs_bilagrid_tv_args),
    "hs_bilagrid_tv_backward": _call(hs_bilagrid_tv_args),
    "hs_vq_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "hs_vq_assign": _call(hs_vq_args),
    "hs_vq_update": _call(hs_vq_args),
    "hs_undistort_map": _call(hs_undistort_args),
    "hs_undistort_remap": _call(hs_undistort_args),
    "hs_composite_features_workspace_bytes": (_i64, [C.POINTER(hs_dims)]),
    "hs_composite_features": _call(hs_composite_features_args),
    "hs_composite_features_backward": _call(hs_composite_features_bwd_args),
    "hs_composite_features_geometry_workspace_bytes": (_i64, [C.POINTER(hs_dims)]),
    "hs_composite_features_geometry_backward": _call(hs_composite_features_geometry_args),
    "hs_distortion_workspace_bytes": (_i64, [C.POINTER(hs_dims)]),
    "hs_distortion": _call(hs_distortion_args),
    "hs_distortion_backward": _call(hs_distortion_bwd_args),
    "hs_normal_consistency_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "hs_normal_consistency": _call(hs_normal_consistency_args),
    "hs_normal_consistency_backward": _call(hs_normal_consistency_args),
    "hs_gaussian_normals": _call(hs_gaussian_normals_args),
    "hs_gaussian_normals_backward": _call(hs_gaussian_normals_args),
    "hs_tsdf_integrate": _call(hs_tsdf_args),
    "hs_tsdf_mesh_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "hs_tsdf_mesh_plan": _call(hs_tsdf_args),
    "hs_tsdf_mesh_emit": _call(hs_tsdf_args),
    "hs_mesh_workspace_bytes": (_i64, [_i64, _i64]),
    "hs_mesh_components": _call(hs_mesh_args),
    "hs_mesh_clean_plan": _call(hs_mesh_args),
    "hs_mesh_clean_emit": _call(hs_mesh_args),
}
EXPORTS = tuple(SIGNATURES)
# detected by name, and a library without them still loads: it serves every call that does not need them.  hs_max_frames: a
# library without it reads hs_dims.n_frames as the reserved word it was and would render all poses into ONE image, silently
# -- max_frames() is what a request for frames is checked against
OPTIONAL_EXPORTS = ("hs_max_frames",)
HS_RENDER_STATS = 24

_lib = None


def load() -> C.CDLL:
    """Load libhdrsplat.so; raises (never falls back) when it is absent or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run `make -C casualhdrsplat_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "casualhdrsplat_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name) and name not in OPTIONAL_EXPORTS:
            raise RuntimeError(f"{LIB_PATH} does not export {name}")
    for name, (restype, argtypes) in SIGNATURES.items():
        if hasattr(lib, name):         # (only an OPTIONAL_EXPORTS name can be missing here)
            fn = getattr(lib, name)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
    if lib.hs_version() != HS_VERSION:   # (a stale variant picked by HS_LIB_PATH would read the structs short or long)
        raise RuntimeError(f"{LIB_PATH} is HS_VERSION {lib.hs_version()}, this package mirrors the structs of "
                           f"{HS_VERSION}: rebuild it (`make -C casualhdrsplat_amd/csrc`)")
    if os.environ.get("HS_SORT_TICKETS", "")[:1] == "1":   # the process default of the chain order, set once
        lib.hs_sort_tickets(1)
    _lib = lib
    return lib


def _atoi(s: str) -> int:
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group()) if m else 0


def sort_options(env) -> dict:
    """The sort selection fields of hs_fwd_args that the switches in `env` (a mapping like os.environ) ask for.  The
    library itself reads no environment: HS_TILE_SORT=radix / count / hier and HS_DEPTH_SORT=lsd / msd (first letter
    counts), HS_SCAN_IN_EMISSION=1 / anything else, HS_DEPTH_RANGE_CAP and HS_DEPTH_DIST_MAX (integers) mean what they
    meant when it did; unset = 0 = the library's own choice."""
    cap, dist = env.get("HS_DEPTH_RANGE_CAP"), env.get("HS_DEPTH_DIST_MAX")
    scan = env.get("HS_SCAN_IN_EMISSION")
    return dict(
        tile_sort={"r": HS_TILE_SORT_RADIX, "c": HS_TILE_SORT_COUNT, "h": HS_TILE_SORT_HIER}.get(env.get("HS_TILE_SORT", "")[:1], 0),
        depth_sort={"l": HS_DEPTH_SORT_PASSES, "m": HS_DEPTH_SORT_COUNT}.get(env.get("HS_DEPTH_SORT", "")[:1], 0),
        emission_scan=0 if scan is None else (HS_EMISSION_SCAN_INSIDE if scan[:1] == "1" else HS_EMISSION_SCAN_AHEAD),
        # (the fields keep 0 for "not set": a set variable is clamped here, to [64, 4096] elements -- 4096 is all the LDS
        # holds -- and to [0, 16] members with -1 for "0", as the library clamped what atoi gave it)
        depth_range_cap=0 if cap is None else min(max(_atoi(cap), 64), 4096),
        depth_dist_max=0 if dist is None else (-1 if _atoi(dist) <= 0 else min(_atoi(dist), 16)))


def forward(a: hs_fwd_args, stream, what: str = "hs_forward") -> int:
    """hs_forward(a) with the sort selection of the moment: os.environ's switches (sort_options) and, as an explicit value,
    the process-wide chain order (hs_sort_tickets) -- returned, 1 = tickets: what the call is given is what the caller
    knows it had.  Every hs_fwd_args the package hands to the library goes through here."""
    lib = load()
    for k, v in sort_options(os.environ).items():
        setattr(a, k, v)
    tickets = lib.hs_sort_tickets(-1)
    a.chain_order = HS_CHAIN_TICKETS if tickets else HS_CHAIN_BLOCKIDX
    check(lib.hs_forward(C.byref(a), stream), what)
    return tickets


def check(rc: int, what: str) -> None:
    if rc != HS_OK:
        msg = load().hs_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def max_frames() -> int:
    """The largest hs_dims.n_frames the loaded library groups poses into; 0: it has no hs_max_frames and ignores the field."""
    lib = load()
    return int(lib.hs_max_frames()) if hasattr(lib, "hs_max_frames") else 0


def require_frames(n_frames: int) -> None:
    """RuntimeError unless the loaded library renders `n_frames` frames in one call."""
    if n_frames > 1 and n_frames > max_frames():
        raise RuntimeError(f"{LIB_PATH} " + ("does not export hs_max_frames: it ignores hs_dims.n_frames and would render the "
                           f"poses of all {n_frames} frames into one image" if max_frames() == 0 else
                           f"groups at most {max_frames()} frames, {n_frames} were asked for") +
                           "; rebuild it (`make -C casualhdrsplat_amd/csrc`) or render the frames one call each")


def plan(P: int, M: int, sh_degree: int, W: int, H: int, n_poses: int, capacity: int, crf_K: int = 0, n_frames: int = 0):
    require_frames(n_frames)
    d = hs_dims(P, M, sh_degree, W, H, n_poses, capacity, crf_K, n_frames)
    sz, lay = hs_sizes(), hs_layout()
    check(load().hs_plan(C.byref(d), C.byref(sz), C.byref(lay)), "hs_plan")
    return d, sz, lay
