/*
 * hdrsplat.h -- C ABI of libhdrsplat.so, the MI355X (gfx950) differentiable Gaussian rasterizer.
 *
 * Boundary being replaced.  BASELINE.json's north_star fixes the drop-in boundary as the
 * GaussianRasterizer / GaussianRasterizationSettings Python API.  /root/reference contains no
 * code at all (Readme.md:1-58 + two figures), so there is no reference
 * FFI file:line to cite.  The interface each entry point replaces is therefore the *published*
 * binding of the third-party package that API belongs to (diff_gaussian_rasterization, not
 * vendored/pinned by the reference -- SURVEY.md 2.3, 8b):
 *
 *   hs_forward       <-> _C.rasterize_gaussians           (pybind11, torch tensors)   [SURVEY 3.2]
 *   hs_backward      <-> _C.rasterize_gaussians_backward                              [SURVEY 3.3]
 *   hs_mark_visible  <-> _C.mark_visible                                              [SURVEY 2.3 a14]
 *   hs_plan          <-> the resize-callback carving of geomBuffer/binningBuffer/imgBuffer [a13]
 *
 * Contract: plain C structs of raw DEVICE pointers and scalars; no torch types,
 * no C++ exceptions across the ABI; the caller owns every byte (the library never allocates
 * device memory and keeps no state between calls); all work is enqueued on the caller's HIP
 * stream and nothing inside synchronises; return 0 = ok, negative = error, text through
 * hs_last_error() (thread-local).
 *
 * "Instance" below means one (pose, Gaussian) pair: with n_poses = N the library renders N
 * virtual sharp images in one launch (pose id folded into the tile sort key) and averages
 * them (motion blur as N-pose render averaging, /root/reference/assets/pipeline.png "+").
 *
 * Frames (detected by name: hs_max_frames).  hs_dims.n_frames = F > 1 groups the n_poses = F * N poses of a call into F
 * consecutive runs of N: frame f owns the poses f * N .. f * N + N - 1, has its own exposure[f] and its own output image --
 * one training step over F captured frames (or a mini-batch of F plain views, N = 1) in ONE call.  Everything per pose stays
 * per pose, everything per Gaussian is summed (radii: maximised) over all F * N poses; what becomes per frame is noted next
 * to each field below.  Frame f's images carry the bits a separate call on its N poses gives.  n_frames = 0 or 1 is the
 * call without frames: the same workspace sizes and offsets, the same kernels, the same outputs.
 */
#ifndef HDRSPLAT_H
#define HDRSPLAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libhdrsplat.so is built with -fvisibility=hidden: the hs_* entry points below are its only exported symbols */
#define HS_API __attribute__((visibility("default")))

#define HS_VERSION 309 /* 309: hs_fwd_args grew the sort selection fields (tile_sort ... depth_dist_max) at its end; the
                          library reads no environment variable any more */

#define HS_OK 0
#define HS_EINVAL (-1)    /* bad argument (null pointer, bad shape, unsupported degree ...) */
#define HS_EHIP (-2)      /* a HIP runtime call failed; see hs_last_error() */
#define HS_EOVERFLOW (-3) /* binning capacity smaller than the number of (tile, instance) pairs */

#define HS_TILE 16 /* binning tile edge in pixels (BLOCK_X = BLOCK_Y = 16 upstream) */

/* hs_fwd_args.stages */
#define HS_STAGE_PREPROCESS 1 /* preprocess; when run WITHOUT HS_STAGE_BIN (the upstream-style call, host reads
                                 num_rendered before binning) also the instance-order scan of tiles_touched */
#define HS_STAGE_BIN 2        /* depth sort, duplicateWithKeys with the scan of the depth-ordered counts inside (writes
                                 num_rendered), tile sort, tile ranges */
#define HS_STAGE_RENDER 4     /* per-tile alpha blend (+ HDR epilogue, + N-pose resolve) */
#define HS_STAGE_ALL 7
#define HS_STAGE_OFFSETS 8    /* inspection only: inclusive scan of tiles_touched in instance order into the geom
                                 workspace (`offsets`; the pipeline itself scans the depth-ordered counts) and the 3-D
                                 covariances (`cov3D`; the pipeline recomputes them in the backward instead of storing);
                                 (HS_VERSION 305) with a binning workspace of a frame sorted by counting, also keys_sorted */

#define HS_STAGE_PREPROCESS_ONLY 16 /* profiling (bench.py's per-kernel roofline leg): with PREPROCESS | BIN, enqueue the
                                 preprocess kernel exactly as a single-enqueue forward does -- carrying the binning stage's
                                 prologue: depth keys, cleared scratch and ranges -- and stop before the binning kernels */

/* hs_bwd_args.stages */
#define HS_BWD_RENDER 1      /* per-pixel backward -> one gradient record per (tile, instance) pair */
#define HS_BWD_PREPROCESS 2  /* per-instance record sum + computeCov2D/projection/SH/cov3D backward */
#define HS_BWD_CRF 4         /* CRF-table and exposure gradients (HDR only) */
#define HS_BWD_ALL 7
/* the two halves of HS_BWD_PREPROCESS on their own (a caller that all-gathers dL_dview_colors over the ranks can
 * start that exchange between them) */
#define HS_BWD_SEGSUM 8      /* per-instance record sums (+ dL_dview_colors when given) */
#define HS_BWD_PROJECT 16    /* computeCov2D/projection/SH/cov3D backward from the record sums */

/* (HS_VERSION 309) hs_fwd_args.tile_sort / depth_sort / chain_order / emission_scan: 0 = auto in each */
#define HS_TILE_SORT_RADIX 1   /* stable look-back radix passes over the tile ids */
#define HS_TILE_SORT_COUNT 2   /* counting sort (small frames: hs_layout.tile_matrix); radix passes where it does not fit */
#define HS_TILE_SORT_HIER 3    /* hierarchical (hs_layout.hier_ws); the automatic choice where it does not fit */
#define HS_DEPTH_SORT_PASSES 1 /* stable look-back radix passes */
#define HS_DEPTH_SORT_COUNT 2  /* counting pass + range sorts (hs_depth_sort); look-back passes from 2^21 instances on */
#define HS_CHAIN_BLOCKIDX 1    /* chain positions of the radix passes: blockIdx ... */
#define HS_CHAIN_TICKETS 2     /* ... or tickets drawn when a block starts (hs_sort_tickets) */
#define HS_EMISSION_SCAN_AHEAD 1  /* slot offsets of the pair emission from kernels of their own ahead of it ... */
#define HS_EMISSION_SCAN_INSIDE 2 /* ... or from a chained scan inside its launch */

/* flags */
#define HS_FLAG_HDR 1          /* exposure * CRF tone-map epilogue; out_color = LDR, out_hdr = radiance */
#define HS_FLAG_BLUR_HDR 2     /* N-pose average taken on radiance before the CRF (default: on LDR) */
#define HS_FLAG_DEBUG 4         /* wait for every stage and name the failing one (the only case of a sync) */
#define HS_FLAG_ANTIALIAS 8    /* newer published rasterizer's `antialiasing`: opacity *= sqrt(max(0.000025,
                                  det(cov2D) / det(cov2D + 0.3 I))), with its gradient */
/* radiance activation (SURVEY.md 7.3 / 8a a1 `radiance_activation`; the reference reconstructs an HDR scene,
 * /root/reference/Readme.md:54): how the SH sum s of a Gaussian becomes its linear-radiance colour.  Neither bit:
 * relu_shift = max(s + 0.5, 0), the published rule (unbounded above, clamped below with the clamp mask zeroing the
 * gradient).  Precomputed colours pass through unchanged. */
#define HS_FLAG_RADIANCE_EXP 16       /* colour = e^s            (always positive; d colour / d s = colour) */
#define HS_FLAG_RADIANCE_SOFTPLUS 32  /* colour = ln(1 + e^s)    (d colour / d s = sigmoid(s) = -expm1(-colour)) */

typedef struct hs_dims {
    int32_t P;         /* Gaussians */
    int32_t M;         /* SH coefficients stored per Gaussian and channel (0 if colors_precomp) */
    int32_t sh_degree; /* active degree, (sh_degree+1)^2 <= M */
    int32_t W, H;
    int32_t n_poses;   /* N >= 1 */
    int64_t capacity;  /* binning capacity in (tile, instance) pairs */
    int32_t crf_K;     /* knots per channel of the CRF table, 0 when the call has no HDR tone-map: sizes the scratch of
                          the CRF-gradient stage (must equal hs_fwd_args.crf_K / hs_bwd_args.crf_K under HS_FLAG_HDR) */
    int32_t n_frames;  /* F: the poses form F consecutive runs of n_poses / F, each with its own exposure and output image;
                          0 means 1 (a zero-initialised struct is the call without frames).  HS_EINVAL when negative, larger
                          than n_poses, or not a divisor of n_poses.  (This field was `reserved`, 0, before hs_max_frames
                          existed: a library without that export ignores it) */
} hs_dims;

typedef struct hs_sizes {
    int64_t geom_bytes;    /* per-instance geometry state (a13 GeometryState) */
    int64_t binning_bytes; /* keys/values double buffers, histograms, ranges (BinningState) */
    int64_t image_bytes;   /* final_T, n_contrib, per-pose radiance (ImageState) */
    int64_t bwd_bytes;     /* backward scratch: per-pair gradient records, CRF partials */
} hs_sizes;

/* First bytes of the geometry workspace; the host may read them after HS_STAGE_PREPROCESS. */
typedef struct hs_counters {
    uint32_t num_rendered; /* R = sum of tiles_touched over all instances */
    uint32_t overflow;     /* HS_STAGE_BIN: 1 = R > capacity; 2 = a radix pass gave up waiting for a predecessor's status
                              word (damaged scratch).  Either way the frame is rendered empty */
    uint32_t reserved[6];  /* [0] = pairs actually binned (R, or 0 on overflow); [1] = instance count of the depth sort;
                              [2] = ranges of the counting depth sort that did not fit the LDS and were sorted through
                              memory by one workgroup (correct, slow: see hs_depth_sort); [3] = tile-queue counter of the render backward (zero between launches); [4] = times a
                              waiting workgroup of HS_STAGE_BIN had to compute a silent predecessor's counts itself
                              (non-zero: other kernels kept its blocks off the GPU -- see hs_sort_tickets); [5] = the tile
                              sort HS_STAGE_BIN ran (0 radix passes, 1 counting, 2 hierarchical); others unused */
} hs_counters;

typedef struct hs_fwd_args {
    hs_dims dims;
    float tanfovx, tanfovy, scale_modifier;
    int32_t flags;
    int32_t stages;
    int32_t crf_K;               /* knots per channel of crf_table (HDR) */
    float crf_umin, crf_umax;    /* log-exposure range spanned by the table */
    /* device inputs */
    const float* bg;             /* [3] */
    const float* viewmatrices;   /* [N,16] flat "transposed": x' = m[0]x + m[4]y + m[8]z + m[12] */
    const float* projmatrices;   /* [N,16] full view*proj, same convention */
    const float* camposes;       /* [N,3] */
    const float* means3D;        /* [P,3] */
    const float* opacities;      /* [P] */
    const float* shs;            /* [P,M,3] or NULL */
    const float* colors_precomp; /* [P,3] or NULL */
    const float* scales;         /* [P,3] or NULL */
    const float* rotations;      /* [P,4] (w,x,y,z) or NULL */
    const float* cov3D_precomp;  /* [P,6] or NULL */
    const float* exposure;       /* [F] (HDR; F = max(n_frames, 1): one exposure time per frame) or NULL */
    const float* crf_table;      /* [3,crf_K] (HDR) or NULL */
    /* caller-owned workspaces, sizes from hs_plan(), 256-byte aligned */
    void* geom;
    void* binning;
    void* image;
    /* device outputs */
    float* out_color;            /* [F,3,H,W] (one image per frame); LDR when HS_FLAG_HDR */
    float* out_hdr;              /* [F,3,H,W] linear radiance (HDR) or NULL */
    int32_t* radii;              /* [P] max over ALL poses of the call (every frame's) */
    float* out_invdepth;         /* [n_poses,H,W] or NULL: expected inverse depth sum_i alpha_i T_i / z_i per pose
                                    (the caller averages the poses); per pose, whatever n_frames is */
    void* counters_host;         /* (HS_VERSION 304) NULL, or a host address the GPU can write (page-locked, mapped: what
                                    hipHostMalloc / torch pin_memory return): HS_STAGE_BIN leaves a copy of hs_counters
                                    (32 bytes) there -- written by its last kernel, so a sync-free caller that wants to
                                    look at num_rendered / overflow LATER needs no copy of its own on the stream */
    /* (HS_VERSION 309) Which sorts HS_STAGE_BIN runs for THIS call.  All zero (a zero-initialised struct) = the library's
     * own choice, as before; the result is the same bit for bit whichever form runs (a stable sort has one result), so
     * these select speed and code path only.  hs_forward resolves them once, before it enqueues anything, together with
     * the process defaults of hs_depth_sort / hs_sort_tickets: two callers in one process may run different sorts, and
     * no kernel of a frame is chosen under other answers than the rest.  A value outside an enumeration is HS_EINVAL.
     * The library reads no environment variable: the Python host fills these fields from HS_TILE_SORT, HS_DEPTH_SORT,
     * HS_SCAN_IN_EMISSION, HS_DEPTH_RANGE_CAP and HS_DEPTH_DIST_MAX at every call (casualhdrsplat_amd/_lib.py). */
    int32_t tile_sort;       /* 0 = auto: counting where it fits (hs_layout.tile_matrix), else hierarchical where that fits
                                (hs_layout.hier_ws), else radix passes; or HS_TILE_SORT_*.  A forced form that does not
                                fit the dims falls back as noted there; hs_counters.reserved[5] tells what ran */
    int32_t depth_sort;      /* 0 = auto: hs_depth_sort()'s process-wide setting; or HS_DEPTH_SORT_* */
    int32_t chain_order;     /* 0 = auto: hs_sort_tickets()'s process-wide setting; or HS_CHAIN_* */
    int32_t emission_scan;   /* 0 = auto: inside the emission from 2^21 instances on unless the chain order is tickets,
                                ahead of it otherwise; or HS_EMISSION_SCAN_* */
    int32_t depth_range_cap; /* tests: elements a range-sort workgroup of the counting depth sort keeps in its LDS before
                                it goes through memory; 0 = 4096 (all that fit), else clamped to [64, 4096]; < 0 invalid */
    int32_t depth_dist_max;  /* tests: members of a bucket up to which such a range is sorted by distribution; 0 = 16 (the
                                default), -1 = none (every range by digit passes), else clamped to at most 16 */
} hs_fwd_args;

typedef struct hs_bwd_args {
    hs_dims dims;
    float tanfovx, tanfovy, scale_modifier;
    int32_t flags;
    int32_t stages;               /* HS_BWD_* bitmask; bench/profiling may run the two halves separately */
    int32_t crf_K;
    float crf_umin, crf_umax;
    const float* bg;
    const float* viewmatrices;
    const float* projmatrices;
    const float* camposes;
    const float* means3D;
    const float* opacities;
    const float* shs;
    const float* colors_precomp;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    const float* exposure;        /* [F], as in the forward */
    const float* crf_table;
    /* state produced by hs_forward (same buffers) */
    const void* geom;
    const void* binning;
    const void* image;
    void* bwd;                    /* scratch, hs_sizes.bwd_bytes */
    /* upstream gradients */
    const float* dL_dout_color;   /* [F,3,H,W] */
    const float* dL_dout_hdr;     /* [F,3,H,W] or NULL */
    const float* dL_dout_alpha;   /* [H,W] or NULL: gradient w.r.t. the accumulated-opacity image 1 - mean_k final_T_k
                                     (a per-image gradient: HS_EINVAL together with n_frames > 1) */
    /* outputs (each may be NULL when its input is absent) */
    float* dL_dmeans3D;           /* [P,3] */
    float* dL_dmeans2D;           /* [P,3] screen-space gradient (NDC-scaled), summed over ALL poses of the call; like it,
                                     every per-Gaussian gradient below is the sum over every frame's poses */
    float* dL_dopacities;         /* [P] */
    float* dL_dshs;               /* [P,M,3] */
    float* dL_dcolors_precomp;    /* [P,3] */
    float* dL_dscales;            /* [P,3] */
    float* dL_drotations;         /* [P,4] */
    float* dL_dcov3D_precomp;     /* [P,6] */
    float* dL_dexposure;          /* [F] (HDR): entry f from frame f's pixels only, bit for bit what a separate call gives */
    float* dL_dcrf_table;         /* [3,crf_K] (HDR), summed over the frames in a fixed order (frame-major) */
    /* camera-pose gradients (the reference optimises camera motion jointly, Readme.md:54);
     * all three or none; same flat transposed layout as the inputs, unused entries are zero */
    float* dL_dviewmatrices;      /* [n_poses,16] or NULL (per pose, whatever n_frames is) */
    float* dL_dprojmatrices;      /* [n_poses,16] or NULL */
    float* dL_dcamposes;          /* [n_poses,3]  or NULL */
    /* view-parallel exchange: when non-NULL, the colour gradient of every instance AFTER the SH clamp
     * mask (zero for culled instances) is written here, [N,P,3]; dL_dshs may then be NULL, and the SH-coefficient
     * gradient is formed later from the views of ALL ranks by hs_sh_backward_views (per pose, whatever n_frames is) */
    float* dL_dview_colors;
    const float* dL_dout_invdepth; /* [H,W] or NULL: gradient w.r.t. the pose-averaged inverse-depth image (a per-image
                                      gradient: HS_EINVAL together with n_frames > 1) */
    /* densification statistics, all three or none; updated IN PLACE for every Gaussian that was
     * rasterized in at least one pose: grad_accum += |dL/dmean2D.xy| (the NDC-scaled gradient returned in
     * dL_dmeans2D), denom += 1, max_radii = max(max_radii, radius) -- what a 3DGS trainer keeps between
     * densification rounds, without re-reading the gradient tensors.  With n_frames = F > 1 the call leaves what F calls
     * leave: for every frame in which the Gaussian was rasterized in at least one pose, grad_accum += |sum over THAT
     * frame's poses of dL/dmean2D.xy| and denom += 1, frames in ascending order; max_radii takes the maximum over all poses */
    float* densify_grad_accum;    /* [P] */
    float* densify_denom;         /* [P] */
    int32_t* densify_max_radii;   /* [P] */
    /* HS_BWD_PROJECT over the Gaussians [g_begin, g_end) only (both 0: all of them).  The per-Gaussian half of the
     * backward is one thread per Gaussian, so a view-parallel step may run it in ascending chunks and start the
     * exchange of a chunk's gradient rows while the next chunk computes (casualhdrsplat_amd.distributed.
     * chunked_all_reduce; BASELINE.json configs[4]).  g_begin must be a multiple of 128; the chunks of one backward
     * must be enqueued in ascending order, the last one ending at P (it also finishes the pose-gradient reduction). */
    int32_t g_begin, g_end;
} hs_bwd_args;

/* Byte offsets of the arrays carved out of the three state workspaces, for tests, profilers and
 * INTEGRATION.md-style bindings that want to inspect intermediates (keys, point_list, ranges...). */
typedef struct hs_layout {
    /* geom workspace; arrays are indexed by instance = pose * P + gaussian */
    int64_t counters, rec, depth, radii, tiles_touched, offsets, cov3D, clamped, scan_spine, binfo;
    /* binning workspace: keys_sorted = u32 tile id of each sorted pair, point_list = u32 instance of each sorted
     * pair (the sort key of the published algorithm is (tile << 32) | depth_bits[instance]); pairs_tmp = scratch of the
     * tile sort ((tile, instance) as 8-byte elements; keys_sorted | point_list double as its other buffer);
     * depth_pairs = scratch of the depth sort (2 x I 8-byte (depth bits, instance) elements), inst_sorted = the
     * instances in depth order (u32 x I), offs_sorted = inclusive scan of their pair counts in that order (u32 x I:
     * instance inst_sorted[i] owns the pair slots [offs_sorted[i-1], offs_sorted[i])); sort_tmp / pair_sort_tmp = scratch
     * of the depth sort / of the pair emission's scan and the tile sort (digit totals, status words).
     * keys_sorted is written by the RADIX tile sort only (its last pass; tile_ranges reads it).  The counting and the
     * hierarchical tile sort write point_list and ranges and leave keys_sorted alone (nothing in the pipeline reads it):
     * after such a frame it holds scratch until an HS_STAGE_OFFSETS call rebuilds it from the ranges for inspection.
     * hs_counters.reserved[5] tells which tile sort a frame had (0 radix, 1 counting, 2 hierarchical). */
    int64_t keys_sorted, point_list, pairs_tmp, ranges, sort_tmp, depth_pairs, inst_sorted, offs_sorted, pair_sort_tmp;
    /* pair_flags (binning workspace): u8 per pair slot, cleared by the forward's pair emission, set to 1 by the
     * render backward for the records it wrote */
    int64_t pair_flags;
    /* pair_act (binning workspace): u8 per SORTED pair, written by the render forward for every entry it staged: bit
     * 2g + w = some pixel of lane group g (the 8 x 8 block of columns 8g .. 8g+7) of half tile w (rows 8w .. 8w+7 of the
     * tile) took the entry -- four bits, one per 8 x 8 block of the 16 x 16 tile.  The render backward walks exactly
     * those entries, one list per block */
    int64_t pair_act;
    /* image workspace.  pose_hdr: one [3,H,W] radiance plane per pose (kept under HS_FLAG_HDR or with more than one pose
     * per frame), followed -- when a frame has N > 1 poses -- by one mean-radiance plane per frame: slot n_poses + f */
    int64_t final_T, n_contrib, pose_hdr;
    /* tile_work: u32 per (pose, tile): (half tile, entry) trips the render forward counted on it = what the render
     * backward will replay; tile_order: u32 per render-backward workgroup: the (pose, tile) it processes (the forward
     * orders the tiles so that each XCD's lightest ones run last, see render.hip) */
    int64_t tile_work, tile_order;
    /* bwd workspace */
    /* inst_grads: 12 floats per instance, the per-instance sum of its (flagged) pair records */
    int64_t pair_grads, crf_partials, inst_grads, pose_partials;
    /* (HS_VERSION 305) tile_matrix (binning workspace; empty unless the frame is small: <= 4096 (pose, tile) keys and
     * <= 2^21 (emission workgroup, key) entries): scratch of the counting tile sort such frames get instead of radix passes
     * -- u32 [ceil(I/256)][keys] pair counts (one byte per wave) | u32 [ceil(I/256)][keys] pairs of the key in earlier
     * workgroups | u32 [keys] totals.  Such a forward writes point_list and ranges but NOT keys_sorted (see there). */
    int64_t tile_matrix;
    /* (HS_VERSION 307) hier_ws (binning workspace; empty unless the frame has <= 2048 (pose, 8 x 8-tile super-tile) keys):
     * scratch of the hierarchical tile sort -- u32 header | element counts per super-tile | pairs per tile | first sorted
     * position per tile | first element / chunk per super-tile | chunk descriptors | per-chunk pair counts.  The default
     * for frames the counting sort does not take and that have <= 2048 (pose, super-tile) keys (hs_fwd_args.tile_sort
     * forces it on smaller ones); like the counting sort it writes point_list and ranges but not keys_sorted.
     * hs_counters.reserved[5] records which tile sort a forward ran (0 radix, 1 counting, 2 hierarchical). */
    int64_t hier_ws;
    /* (HS_VERSION 308) depth_ws (binning workspace; empty unless the frame has fewer than 2^21 instances): scratch of the
     * depth sort such frames get instead of look-back passes -- per block of 1024 / 4096 instances a row of 4096 u16 bucket
     * counts (top 12 varying key bits) | a row of u32 prefixes down the columns | u32 [4096] bucket totals.  Written before
     * it is read: nothing to clear.  See hs_depth_sort. */
    int64_t depth_ws;
} hs_layout;

HS_API int hs_version(void);
HS_API const char* hs_last_error(void);
/* Limits (HS_EINVAL beyond them): P * n_poses < 2^30 instances, capacity < 2^30 pairs, fewer than 2^22 tiles per pose
 * (a 32768 x 32768 frame), n_poses <= 21845, crf_K <= 4096, 0 <= n_frames <= n_poses with n_poses a multiple of it. */
HS_API int hs_plan(const hs_dims* dims, hs_sizes* sizes, hs_layout* layout /* may be NULL */);
HS_API int hs_forward(const hs_fwd_args* args, void* hip_stream);
HS_API int hs_backward(const hs_bwd_args* args, void* hip_stream);
/* (detected by name; HS_VERSION unchanged) The largest hs_dims.n_frames this library groups poses into (21845: the limit
 * on n_poses).  A library WITHOUT this export treats the field as the reserved word it used to be and renders every pose
 * into one image: a host asks for frames only after it has found the symbol. */
HS_API int hs_max_frames(void);
HS_API int hs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, uint8_t* visible,
                    void* hip_stream);

/* SH-coefficient gradient from per-view colour gradients (the multi-GPU exchange of SURVEY.md 8e, where ranks
 * all-gather 12 bytes per Gaussian and view instead of all-reducing the 12*M-byte SH gradient rows):
 *   dL_dshs[g, k, c] = sum_{v < V} Y_k(normalize(means3D[g] - camposes[v])) * dL_dview_colors[v, g, c],
 * views added in ascending order, k < (sh_degree+1)^2, rows k >= that are zeroed.  Same basis and per-view
 * arithmetic as the SH part of hs_backward, so V = 1 reproduces its dL_dshs bit for bit. */
HS_API int hs_sh_backward_views(int32_t P, int32_t M, int32_t sh_degree, int32_t V, const float* means3D,
                         const float* camposes /* [V,3] */, const float* dL_dview_colors /* [V,P,3] */,
                         float* dL_dshs /* [P,M,3] */, void* hip_stream);

/* (HS_VERSION 306) Camera poses along the trajectory spline of the image-formation model -- the N virtual poses inside each
 * captured frame's exposure window (/root/reference/assets/pipeline.png: "camera motion spline" through the control knots
 * T_j .. T_{j+3}; Readme.md:54) -- together with their Jacobian, in one launch (spline.hip; the tensor-operation form of the
 * same arithmetic, image_formation.TrajectorySpline.pose_at, is ~1000 tiny kernels forward + backward per call).
 *   knot_j = exp(delta[j]) * base_w2c[j]   (delta: [n_knots, 6] se(3) corrections (rho, omega); base: [n_knots, 4, 4] row-major)
 *   kind 1 (cubic cumulative B-spline): times in [1, n_knots - 2]; kind 0 (geodesic between two knots): times in [0, n_knots - 1]
 * Outputs per sample time s: w2c[s] (4 x 4 row-major world-to-camera), segment[s] = j, the first knot governing the sample, and
 * jacobian[s][o][i], o = 4 * row + column over the first three rows of w2c[s] (12 values), i < 24: d / d delta[j + i / 6][i % 6]
 * (knots beyond the two of a linear segment: zeros), i = 24: d / d times[s].  Device pointers; 25 threads per sample. */
HS_API int hs_spline_poses(int32_t n_knots, int32_t n_times, int32_t kind, const float* delta, const float* base_w2c,
                    const float* times, float* w2c /* [n_times,4,4] */, float* jacobian /* [n_times,12,25] */,
                    int32_t* segment /* [n_times] */, void* hip_stream);

/* Bench/profiling only: re-runs the render stage(s) of a finished hs_forward (and hs_backward) call -- same argument
 * structs, same buffers, so the outputs are simply rewritten -- with the diagnostic instantiation of the kernels, which
 * ADDS its counts to stats[0..HS_RENDER_STATS) (device memory, zeroed by the caller).  Either struct may be NULL.
 *   [0] backward (wave, entry) trips  [1] ... with no active lane  [2] sum of active pixels over trips (<= 128 each)
 *   [3] entries rejected by the half-tile test (per wave)  [4..9] trips by active lanes: 0, 1-4, 5-8, 9-16, 17-32, 33-64
 *   [10] entries staged (per tile)  [11] staging batches  [12..17] forward: trips, empty, active pixels, culled,
 *   staged, batches.  bench.py derives lane utilisation and the VALU roofline from them. */
#define HS_RENDER_STATS 24
HS_API int hs_render_stats(const hs_fwd_args* fwd /* or NULL */, const hs_bwd_args* bwd /* or NULL */, uint64_t* stats,
                    uint64_t* bwd_timeline /* or NULL: per workgroup of the backward launch (tiles x poses of them)
                                              {start, end} on the 100 MHz device clock and (XCC id << 32 | HW_ID) */,
                    void* hip_stream);

/* The depth sort of HS_STAGE_BIN for frames of fewer than 2^21 instances, process-wide: 1 (default) = by counting -- one
 * stable counting pass over the top 12 varying bits of the depth keys (per-block bucket counts, a column scan, one
 * scatter), then every run of buckets of about 2048 instances (512 up to 2^18 instances) sorted to the end by one workgroup
 * inside its LDS; 0 = the
 * stable look-back radix passes larger frames always get.  Same result bit for bit (a stable sort has one).  The
 * counting form assumes that no 2048 consecutive positions of the bucket order spill over 4096 instances, i.e. that no
 * depth sliver of 1 / 4096 of the key range holds more than ~2048 instances; a range that does is sorted through memory by
 * its one workgroup -- correct, but a frame dominated by such a range (a wall of Gaussians at one depth seen head-on)
 * is slower than with the passes.  hs_counters.reserved[2] counts those ranges; the Python host moves the process to 0
 * when a frame reports any.  mode < 0 only queries.  Returns the setting in force.  hs_fwd_args.depth_sort overrides
 * it per forward. */
HS_API int hs_depth_sort(int mode);

/* Chain positions of the radix passes of HS_STAGE_BIN, process-wide: 0 = blockIdx (default: relies on every XCD handing
 * its share of a grid out in increasing order), 1 = tickets drawn when a block STARTS (+3 % per step at c3; correct under
 * any dispatch order, and the faster setting when SEVERAL PROCESSES run this library on one GPU: two blockIdx-ordered
 * passes of different processes can fill the GPU with blocks that wait for blocks of their own kernel which the other
 * process' waiting blocks keep out; a waiting block then computes the silent predecessor's counts itself -- correct,
 * counted in hs_counters.reserved[4], but slower than never having to).
 * With 1 the pair emission also takes its slot offsets from kernels of their own instead of its in-launch chain.
 * enable < 0 only queries.  Returns the setting in force.  Initial value: 0; hs_fwd_args.chain_order overrides it per
 * forward.  The Python host calls hs_sort_tickets(1) when it loads the library with HS_SORT_TICKETS=1 in the environment,
 * and switches to 1 by itself once frames report helps (or, should a pass ever give up: overflow = 2, after which it asks
 * for the step again). */
HS_API int hs_sort_tickets(int enable);

/* (HS_VERSION 308, detected by name) Photometric training loss of the published 3DGS train.py, fused (loss.hip):
 *   loss = (1 - lambda_dssim) * mean|image - target| + lambda_dssim * (1 - mean SSIM(image, target))
 * SSIM as the published ssim(): 11 x 11 Gaussian window (sigma 1.5), zero padding, C1 = 0.01^2, C2 = 0.03^2, averaged over
 * every plane (one channel of one image) and pixel.  All pointers are device memory owned by the caller; 256-byte aligned
 * workspace.  Limits (HS_EINVAL): planes, H, W >= 1, planes * H * W < 2^31, 0 <= lambda_dssim <= 1. */
typedef struct hs_loss_args {
    int32_t planes, H, W;         /* images are [planes, H, W] fp32, contiguous ([B, C, H, W]: planes = B * C) */
    float lambda_dssim;
    const float* image;
    const float* target;
    void* workspace;              /* hs_loss_workspace_bytes(planes, H, W, 0) bytes: one fp64 pair per tile of the forward */
    float* partials;              /* [3, planes, H, W] per-pixel partials of SSIM that the backward reads, or NULL: forward
                                     only (evaluation, metrics) -- nothing to keep for a backward */
    float* out;                   /* [3] written by the forward: {loss, l1_mean, ssim_mean} */
    const float* dL_dloss;        /* [1] upstream gradient of the loss scalar (backward; read on the device, never the host) */
    float* dL_dimage;             /* [planes, H, W] written by the backward */
} hs_loss_args;

/* Bytes of one buffer that holds the workspace (at offset 0) and, with with_partials != 0, the partials after it (at offset
 * hs_loss_workspace_bytes(planes, H, W, 0)): align256(16 * tiles) + (with_partials ? 12 * planes * H * W : 0), tiles =
 * planes * ceil(H / 16) * ceil(W / 64).  -1 (HS_EINVAL) for shapes outside the limits above. */
HS_API int64_t hs_loss_workspace_bytes(int32_t planes, int32_t H, int32_t W, int32_t with_partials);
/* forward: writes out[3] (and the partials when non-NULL); no atomics, the same inputs give the same bits */
HS_API int hs_photometric_loss(const hs_loss_args* args, void* hip_stream);
/* backward: dL_dimage = dL_dloss[0] * d loss / d image, from the partials of the forward of the same image / target */
HS_API int hs_photometric_loss_backward(const hs_loss_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Adam update of the cloud and of any other fp32 parameters, fused into one launch
 * and optionally restricted to the Gaussians a step saw (adam.hip).  Adam as torch.optim.Adam defines it: bias-corrected, no
 * weight decay, no AMSGrad; fp32 parameters, gradients and moments.
 *
 * A GROUP is a column range [col_begin, col_begin + col_count) of a row-major fp32 matrix [rows, row_stride]: shs[P, M, 3]
 * can be two groups with two learning rates (columns 0..2 and 3..3M-1) and stay one tensor.  Group g reads row g of the
 * hyper-parameter table `hyper`, fp64 [n_groups][4] = {lr, beta1, beta2, eps}, ON THE DEVICE: a learning-rate schedule is a
 * write to that table, also between replays of a captured graph.
 *
 * hs_adam_step enqueues two kernels and nothing else.  The first advances the device-resident state: with t the step
 * count after the increment and B1 = beta1^t, B2 = beta2^t kept as RUNNING PRODUCTS in fp64 (B *= beta each step; 1 before
 * the first),
 *     step_size = (float)(lr / (1 - B1)),   bc2 = (float)sqrt(1 - B2)                      (fp64, then rounded)
 * and b1 = (float)beta1, b2 = (float)beta2, c1 = (float)(1 - beta1), c2 = (float)(1 - beta2) (the difference in fp64, rounded
 * once: an fp32 value, as torch passes it), e = (float)eps.  The second updates every element, in fp32, each operation a
 * correctly rounded IEEE operation, nothing contracted, denormals kept, in exactly this order:
 *     m' = b1 * m + c1 * g
 *     v' = b2 * v + (c2 * g) * g
 *     d  = sqrtf(v') / bc2 + e
 *     p' = p - step_size * (m' / d)
 * No atomics: the same inputs give the same bits.
 *
 * Visibility mask (optional): one entry per Gaussian, either the forward's radii (HS_ADAM_MASK_RADII: int32, visible = > 0)
 * or bytes (HS_ADAM_MASK_BYTES: uint8 / bool, visible = != 0).  In a group flagged `masked`, rows whose entry is not visible
 * are SKIPPED: param, exp_avg and exp_avg_sq keep their bits and are not read.  This is the published "sparse Adam" and is
 * not dense Adam with a zero gradient: the moments of a skipped row do not decay and its momentum does not move it.  The
 * step count is global to the call.  Groups not flagged `masked`, and every group when mask_kind is HS_ADAM_MASK_NONE, are
 * dense.
 *
 * State: hs_adam_state_bytes(n_groups) = 64 + 64 * n_groups bytes, 16-byte aligned, owned by the caller.  All-zero bytes
 * are a fresh state (t = 0).  Layout, for callers that save or restore it: u64 t at byte 0; for group g at byte 64 + 64 * g:
 * fp64 B1, fp64 B2, then the eight fp32 values the first kernel derives (rewritten by every call).
 * Pointers param / grad / exp_avg / exp_avg_sq need 4-byte alignment only (16-byte loads and stores are used where the
 * addresses allow).  Limits (HS_EINVAL): 1 <= n_groups <= 16, rows >= 0 (0 = nothing to do, pointers not looked at),
 * row_stride >= 1, col_begin >= 0, col_count >= 1, col_begin + col_count <= row_stride, rows * row_stride <= 2^40. */
#define HS_ADAM_MAX_GROUPS 16
#define HS_ADAM_MASK_NONE 0
#define HS_ADAM_MASK_RADII 1
#define HS_ADAM_MASK_BYTES 2
typedef struct hs_adam_group {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t rows, row_stride, col_begin, col_count;
    int32_t masked;               /* != 0: the mask applies to this group's rows (rows must equal mask_len) */
    int32_t reserved;
} hs_adam_group;

typedef struct hs_adam_args {
    const hs_adam_group* groups;  /* HOST array of n_groups descriptors (copied into the kernel's arguments) */
    int32_t n_groups;
    int32_t mask_kind;            /* HS_ADAM_MASK_* */
    const void* mask;             /* device, mask_len entries; NULL with HS_ADAM_MASK_NONE */
    int64_t mask_len;
    void* state;                  /* device, hs_adam_state_bytes(n_groups) bytes */
    const double* hyper;          /* device, [n_groups][4] = {lr, beta1, beta2, eps} */
} hs_adam_args;

/* -1 (HS_EINVAL) unless 1 <= n_groups <= HS_ADAM_MAX_GROUPS */
HS_API int64_t hs_adam_state_bytes(int32_t n_groups);
HS_API int hs_adam_step(const hs_adam_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Densify / prune of the cloud (densify.hip): the published densify_and_prune --
 * clone, split into N = 2 children, prune -- as a PLAN stage (which rows come out, and from which source row) and an APPLY
 * stage (one gather of every row of every array).  Between the two the caller reads P_out and allocates: the contract is the
 * file's -- the caller owns every byte, nothing here synchronises or allocates.  No atomics anywhere: the same inputs give
 * the same bits.
 *
 * Per source row i of P (fp32 throughout, every operation one correctly rounded IEEE operation, nothing contracted):
 *     g   = grad_accum[i] / denom[i];  g counts as 0 when denom[i] == 0 or the quotient is NaN
 *     sel = g >= tau_grad
 *     s   = max of the three stored scales: s = scales[3i]; if (scales[3i+1] > s) s = scales[3i+1]; the same for [3i+2]
 *     big = s > tau_split
 *     prune(o, r, s) = o < o_min || (r_max > 0 && r > r_max) || (sigma on && s > sigma_max)
 *   not sel      the row survives iff !prune(o_i, r_i, s)
 *   sel && !big  CLONE: the row survives and a bit-identical copy is appended, both iff !prune(o_i, r_i, s)
 *   sel && big   SPLIT: the source row goes; children k = 0, 1 exist, both, iff !prune(o_i, r_i, child(s)), where child(x) is
 *                x / 1.6f, or with HS_DENSIFY_RAW_SCALES x - HS_DENSIFY_LOG_1_6 (the fp32 constant logf(1.6))
 * with o_i = opacities[i], r_i = max_radii[i]: derived rows are tested with their SOURCE's radius.  Opacities and scales
 * are compared AS STORED: with HS_DENSIFY_RAW_OPACITY the stored value is a logit and o_min is one too, with
 * HS_DENSIFY_RAW_SCALES the stored values are logs and tau_split / sigma_max are logs too (sigmoid and exp are monotonic: the
 * host converts the thresholds once, in fp64, and rounds to fp32; no transcendental function decides anything).  The sigma
 * test is off when sigma_max is +INFINITY, and with stored-linear scales also when it is 0; the radius test when r_max is 0.
 *
 * Output order: survivors | clones | children k = 0 | children k = 1, each in source order.  Output row j carries
 *     row_map[j] = kind << 30 | source row      (HS_DENSIFY_KIND_*: 0 survivor, 1 clone, 2 child k = 0, 3 child k = 1)
 * and counts[HS_DENSIFY_COUNTS] (u32) = {P_out, survivors, clones, children (both k), sources that left no row at all, split
 * sources (sel && big, whether or not their children exist), P, 0}.
 *
 * hs_densify_plan enqueues three kernels: classify (a 2-bit code per row into the workspace, four counts per block of 256
 * rows), one small scan of the block counts (writes `counts`), and the map (writes row_map[0, P_out); its first thread also
 * leaves a copy of `counts` at counts_host, a page-locked host address as hs_fwd_args.counters_host is, when given).
 * Workspace: hs_densify_workspace_bytes(P) = align256(P) + 16 * ceil(P / 256) bytes, 16-byte aligned; row_map holds 2 * P
 * u32 (P_out <= 2 P).
 *
 * hs_densify_apply enqueues ONE kernel over up to 16 matrices {src [P, row_stride], dst [P_out, row_stride], role}; output
 * row j of every matrix is written from source row row_map[j] & (2^30 - 1), and nothing is written at or beyond row P_out:
 *   HS_DENSIFY_COPY      every row copied
 *   HS_DENSIFY_ZERO_NEW  survivors copied, every new row (clone, child) all zeros: Adam's moments
 *   HS_DENSIFY_SCALES    row_stride 3: children get child(x) of each stored scale, other rows are copied
 *   HS_DENSIFY_MEANS     row_stride 3: other rows copied; child k of source i gets, with (w, x, y, z) = rotations[4i..]
 *                        divided by n = sqrtf(((w w + x x) + y y) + z z), sg_j = scales[3i + j] (expf of it with
 *                        HS_DENSIFY_RAW_SCALES), v_j = sg_j * noise[6i + 3k + j], and the rotation matrix
 *                          R00 = 1 - 2 (y y + z z)   R01 = 2 (x y - w z)       R02 = 2 (x z + w y)
 *                          R10 = 2 (x y + w z)       R11 = 1 - 2 (x x + z z)   R12 = 2 (y z - w x)
 *                          R20 = 2 (x z - w y)       R21 = 2 (y z + w x)       R22 = 1 - 2 (x x + y y)
 *                        mean_c = ((Rc0 v_0 + Rc1 v_1) + Rc2 v_2) + src[3i + c], in exactly this order
 * `noise` is [P, 2, 3] standard normals indexed by the SOURCE row: the library holds no random-number generator.  The scales
 * and rotations the means read are the SOURCE arrays of the args (not a matrix's dst).  16-byte loads and stores are used
 * where the addresses allow, 4-byte accesses of exactly the owned elements otherwise: src / dst need 4-byte alignment only.
 * Limits (HS_EINVAL, reported before any HIP call): 0 <= P < 2^30, 0 <= P_out <= 2 P, 1 <= n_matrices <= 16, row_stride >= 1
 * (3 for MEANS / SCALES), P_out * row_stride < 2^40; with P == 0 (or, in apply, P_out == 0) no data pointer is looked at. */
#define HS_DENSIFY_MAX_MATRICES 16
#define HS_DENSIFY_RAW_OPACITY 1
#define HS_DENSIFY_RAW_SCALES 2
#define HS_DENSIFY_COPY 0
#define HS_DENSIFY_ZERO_NEW 1
#define HS_DENSIFY_MEANS 2
#define HS_DENSIFY_SCALES 3
#define HS_DENSIFY_KIND_SURVIVOR 0
#define HS_DENSIFY_KIND_CLONE 1
#define HS_DENSIFY_KIND_CHILD0 2
#define HS_DENSIFY_KIND_CHILD1 3
#define HS_DENSIFY_COUNTS 8
#define HS_DENSIFY_LOG_1_6 0.47000366f /* logf(1.6f) rounded to fp32: bits 0x3ef0a452 */
typedef struct hs_densify_matrix {
    const float* src;             /* [P, row_stride] */
    float* dst;                   /* [P_out, row_stride]; must not overlap src */
    int64_t row_stride;           /* floats per row */
    int32_t role;                 /* HS_DENSIFY_COPY / _ZERO_NEW / _MEANS / _SCALES */
    int32_t reserved;
} hs_densify_matrix;

typedef struct hs_densify_args {
    int64_t P;                    /* source rows */
    int64_t P_out;                /* apply: rows of every dst = counts[0] of the plan (the plan ignores it) */
    int32_t flags;                /* HS_DENSIFY_RAW_* */
    int32_t r_max;                /* prune rows whose max_radii exceeds it; 0 = off */
    float tau_grad;               /* select rows whose mean gradient reaches it */
    float tau_split;              /* stored space: split above, clone at or below */
    float o_min;                  /* stored space: prune below */
    float sigma_max;              /* stored space: prune above; +INFINITY (or 0 with linear scales) = off */
    const float* grad_accum;      /* [P]  plan */
    const float* denom;           /* [P]  plan */
    const int32_t* max_radii;     /* [P]  plan */
    const float* opacities;       /* [P]  plan */
    const float* scales;          /* [P, 3]  plan, and the apply's MEANS role */
    const float* rotations;       /* [P, 4] (w, x, y, z), not normalised: apply, MEANS role */
    const float* noise;           /* [P, 2, 3]: apply, MEANS role */
    void* workspace;              /* hs_densify_workspace_bytes(P) bytes, 16-byte aligned: plan */
    uint32_t* row_map;            /* [2 P]: written by the plan, read by the apply */
    uint32_t* counts;             /* device, [HS_DENSIFY_COUNTS]: written by the plan */
    uint32_t* counts_host;        /* NULL, or a page-locked host address the GPU can write: the plan's copy of counts */
    const hs_densify_matrix* matrices; /* HOST array of n_matrices descriptors (copied into the kernel's arguments): apply */
    int32_t n_matrices;
    int32_t reserved;
} hs_densify_args;

/* align256(P) + 16 * ceil(P / 256); -1 (HS_EINVAL) unless 0 <= P < 2^30 */
HS_API int64_t hs_densify_workspace_bytes(int64_t P);
HS_API int hs_densify_plan(const hs_densify_args* args, void* hip_stream);
HS_API int hs_densify_apply(const hs_densify_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Score-driven row plans of the cloud (rows.hip): prune by a mask, keep the k best
 * rows, or clone / split the k best rows -- the PLAN stage of a refinement whose policy is the caller's score.  The output is
 * hs_densify_plan's, so the unchanged hs_densify_apply gathers from it.  In KEEP and DENSIFY mode the host knows P_out before
 * any kernel runs (k, and P + k: a clone adds one row, a split removes one and adds two), so nothing has to be read back.  The
 * caller owns every byte; nothing here synchronises, allocates, sets or copies memory.  No float arithmetic and no float or
 * global atomics: the same inputs give the same bits.
 *
 * THE ORDER ON SCORES (fp32 `score`, [P]):
 *   1. NaN ranks below every number, and all NaNs are equal;
 *   2. -0 equals +0;
 *   3. everything else is in numeric order, +-infinity and denormals in their places.
 * "The k best rows" are the first k rows when all rows are listed by (score descending, row index ascending): among equal
 * scores the lower row wins.  T = the number of rows whose score equals the k-th best one (0 when k == 0).
 *
 *   HS_ROWS_MASK     rows with mask[i] != 0 leave, the others survive; P_out = counts[0], which the caller reads
 *   HS_ROWS_KEEP     the k best rows survive, the others leave; P_out = k
 *   HS_ROWS_DENSIFY  every selected row i, with s the maximum of its three stored scales by hs_densify_plan's comparisons
 *                    (s = scales[3i]; if (scales[3i+1] > s) s = scales[3i+1]; the same for [3i+2]), is SPLIT when
 *                    s > tau_split (the source goes, children k = 0, 1) and CLONED otherwise (the row survives and a copy is
 *                    appended); rows not selected survive; nothing is pruned; P_out = P + k.  tau_split is compared AS STORED
 *                    (a log with HS_DENSIFY_RAW_SCALES; the flag is what the caller hands hs_densify_apply with the plan)
 *
 * Output, exactly hs_densify_plan's: row_map[j] = kind << 30 | source row for j < P_out, segments survivors | clones | children
 * k = 0 | children k = 1, each in source order, and counts[HS_DENSIFY_COUNTS] (u32) = {P_out, survivors, clones, children (both
 * k), sources that left no row, split sources, P, T}; a copy at counts_host (NULL, or a page-locked host address as
 * hs_densify_args.counts_host is), written by the call's last kernel.  row_map holds P u32 in MASK and KEEP mode, P + k in
 * DENSIFY mode; nothing is written at or beyond row P_out.
 *
 * Kernels: with k > 0 an exact radix select over the 32-bit key of the order (four passes of a histogram over contiguous
 * chunks of rows and a one-workgroup pick, most significant byte first) finds the k-th best key and the number of rows strictly
 * above it; one classify pass (a row is selected above the threshold, or at it while its rank among the threshold rows, in
 * source order, is below k - above); then the scan and the map of the densify plan.  3 launches in MASK mode, 12 otherwise.
 * Workspace: hs_rows_workspace_bytes(P) = align256(P) + align256(16 * ceil(P / 256)) + 263424 bytes, 16-byte aligned; every
 * word is written before it is read.
 * Limits (HS_EINVAL, reported before any HIP call): 0 <= P < 2^30; 0 <= k <= P; mode one of HS_ROWS_*; flags within
 * HS_DENSIFY_RAW_SCALES; tau_split not NaN (DENSIFY); the pointers the mode reads non-null and 4-byte aligned (mask: any
 * address; workspace: 16 bytes); with P == 0 no data pointer is looked at (counts is still written). */
#define HS_ROWS_MASK 0
#define HS_ROWS_KEEP 1
#define HS_ROWS_DENSIFY 2
typedef struct hs_rows_args {
    int64_t P;                    /* rows */
    int64_t k;                    /* KEEP: rows that stay; DENSIFY: rows cloned or split; MASK: 0 */
    int32_t mode;                 /* HS_ROWS_MASK / _KEEP / _DENSIFY */
    int32_t flags;                /* HS_DENSIFY_RAW_SCALES only */
    float tau_split;              /* DENSIFY, stored space: split above, clone at or below */
    int32_t reserved;
    const float* score;           /* [P]     KEEP, DENSIFY */
    const uint8_t* mask;          /* [P]     MASK */
    const float* scales;          /* [P, 3]  DENSIFY: clone or split */
    void* workspace;              /* hs_rows_workspace_bytes(P) bytes, 16-byte aligned */
    uint32_t* row_map;            /* [P] (MASK, KEEP) or [P + k] (DENSIFY): hs_densify_apply's row_map */
    uint32_t* counts;             /* device, [HS_DENSIFY_COUNTS] */
    uint32_t* counts_host;        /* NULL, or a page-locked host address the GPU can write: the copy of counts */
} hs_rows_args;

/* the formula above; -1 (HS_EINVAL) unless 0 <= P < 2^30 */
HS_API int64_t hs_rows_workspace_bytes(int64_t P);
HS_API int hs_rows_plan(const hs_rows_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) MCMC refinement of the cloud (mcmc.hip): the relocation, the growth and the
 * position noise of "3D Gaussian Splatting as Markov Chain Monte Carlo".  A fixed row budget, a size the host knows before
 * any kernel runs, and dead rows moved onto live ones in place: nothing here is read back, nothing synchronises, allocates,
 * sets or copies memory; the caller owns every byte.  The library holds no random-number generator: every random input is a
 * caller-drawn tensor, and the same inputs give the same bits.
 *
 * SAMPLING BY OPACITY (hs_mcmc_sample), per row i of P:
 *     dead_i = !(opacities[i] > o_min)         compared AS STORED (o_min is a logit with HS_DENSIFY_RAW_OPACITY: the host
 *                                              converts min_opacity once, in fp64, and rounds to fp32); a NaN is dead
 *     w_i    = (uint64) rint(2^24 / (1 + exp(-(double)opacities[i])))     exp in fp64, rint to nearest-even
 *              without HS_DENSIFY_RAW_OPACITY: rint(2^24 * min(max((double)opacities[i], 0), 1))
 *              0 for a NaN; HS_MCMC_RELOCATE: 0 for a dead row; HS_MCMC_GROW: every other row keeps its weight
 *     C_i    = w_0 + ... + w_i   (uint64, exact whatever the order; S = C_{P-1} < 2^54)
 * A draw takes a 64-bit word u (the int64 tensor `u` read as uint64): t = floor(u S / 2^64) (the high word of the 128-bit
 * product), and its source is the first i with C_i > t: a row of weight zero is never chosen.  With S == 0 no draw is made,
 * cnt stays zero and hs_mcmc_update changes nothing.
 *   HS_MCMC_RELOCATE  n_draws == P: every DEAD row i draws with u[i] (its own row: no compaction); sources[i] = its source, -1
 *                     for rows that are not dead (and for every row when S == 0)
 *   HS_MCMC_GROW      draw k of n_draws <= P uses u[k]; sources[k] = its source (-1 when S == 0), and
 *                     row_map[j] = j for j < P, row_map[P + k] = HS_DENSIFY_KIND_CLONE << 30 | sources[k]: hs_densify_apply's
 *                     format, survivors then clones in draw order (when S == 0 the clones name row k mod P, so that the
 *                     gather stays inside the cloud)
 * cnt[src] = the number of draws that chose src (u32, integer atomic adds: order-free).
 * counts[HS_MCMC_COUNTS] (u32) = {P, dead rows, draws made, sources (rows with cnt >= 1), S == 0, 0, 0, 0}, and a copy at
 * counts_host (NULL, or a page-locked host address as hs_densify_args.counts_host is; written by the call's last kernel).
 * Three kernels (four with counts_host): weights with their prefix inside each block of 256 rows and the block sums, ONE
 * small scan of the block sums, the draws (two binary searches: blocks, then rows of the block).
 * Workspace: hs_mcmc_workspace_bytes(P, n_draws) = align256(8 P) + align256(16 (ceil(P / 256) + 1)) + align256(4 P) +
 * align256(4 n_draws) bytes, 16-byte aligned, in that order: u64 inner prefixes [P] (row i: w of its block up to and
 * including i) | per block {u64 exclusive prefix, u32 dead rows, u32 0}, then {S, dead rows, 0} | u32 cnt [P] | i32 sources
 * [n_draws].  hs_mcmc_update reads cnt and sources there: both calls take the same struct.
 *
 * UPDATE (hs_mcmc_update), in place, two kernels.  Every row with c = cnt[i] >= 1, in fp64, each result rounded once to fp32:
 *     r = min(c + 1, 51);  o = 1 / (1 + exp(-opacities[i]))  (the stored value without HS_DENSIFY_RAW_OPACITY)
 *     x = 1 - pow(1 - o, 1 / r)
 *     D = sum_{n = 1..r} sum_{k = 0..n-1} C(n-1, k) (-1)^k x^(k+1) / sqrt(k + 1)     in this loop order, x^(k+1) a running
 *                                                                                   product, the binomials exact
 *     x_c = min(max(x, min_opacity), 1 - 2^-23)
 *     opacities[i] <- log(x_c / (1 - x_c))     (x_c without HS_DENSIFY_RAW_OPACITY)
 *     scales[3i+j] <- scales[3i+j] + log(o / D)     (scales[3i+j] * (o / D) without HS_DENSIFY_RAW_SCALES)
 * Then, HS_MCMC_RELOCATE only, over the matrices {dst [P, row_stride], role; src NULL or dst}: in HS_DENSIFY_COPY matrices
 * (the parameters) every dead row i becomes a bit-exact copy of row sources[i] as the first kernel left it; in
 * HS_DENSIFY_ZERO_NEW matrices (Adam's moments) every row with cnt >= 1 becomes zeros.  The moments of dead rows, and every
 * row that is neither dead nor a source, keep their bits.  HS_MCMC_GROW runs the first kernel only (the moments of a grown
 * source are kept); the new rows are hs_densify_apply's gather over row_map (roles COPY / ZERO_NEW, P_out = P + n_draws).
 *
 * POSITION NOISE (hs_mcmc_noise), one kernel, one row per thread, fp32, every operation one correctly rounded IEEE operation
 * plus the library expf, nothing contracted, no atomics:
 *     o   = 1 / (1 + expf(-opacities[i]))      (the stored value without HS_DENSIFY_RAW_OPACITY)
 *     g   = 1 / (1 + expf(-100 * ((1 - o) - 0.995f)));   gs = g * scaler;   gs == 0: the row is not written
 *     (w, x, y, z) = rotations[4i..] / sqrtf(((w w + x x) + y y) + z z),  R as in hs_densify_apply's MEANS role
 *     s_j = expf(scales[3i+j])   (the stored value without HS_DENSIFY_RAW_SCALES);   v_j = xi[3i+j] * gs
 *     b_j = (s_j s_j) * ((R0j v_0 + R1j v_1) + R2j v_2)
 *     means3D[3i+c] <- ((Rc0 b_0 + Rc1 b_1) + Rc2 b_2) + means3D[3i+c]
 * i.e. mu + R diag(s^2) R^T (xi g scaler), with `xi` [P, 3] standard normals and scaler = lr_xyz * noise_lr a host scalar.
 * Pointers need 4-byte alignment only (the quaternion is one 16-byte load where its address allows), u 8 bytes.
 * Limits (HS_EINVAL, reported before any HIP call): 0 <= P < 2^30; mode one of HS_MCMC_*; flags within HS_DENSIFY_RAW_*;
 * n_draws == P (RELOCATE) or 0 <= n_draws <= P (GROW); o_min not NaN; 0 <= min_opacity <= 1; 0 <= n_matrices <= 16, roles
 * COPY / ZERO_NEW, row_stride >= 1, P * row_stride < 2^40; scaler finite.  With P == 0 no data pointer is looked at (the
 * sample still writes its counts: {0, 0, 0, 0, 1, 0, 0, 0} -- an empty cloud has S == 0). */
#define HS_MCMC_RELOCATE 0
#define HS_MCMC_GROW 1
#define HS_MCMC_COUNTS 8
typedef struct hs_mcmc_args {
    int64_t P;                    /* rows */
    int64_t n_draws;              /* RELOCATE: P (one slot per row); GROW: the new rows */
    int32_t mode;                 /* HS_MCMC_RELOCATE / HS_MCMC_GROW */
    int32_t flags;                /* HS_DENSIFY_RAW_* */
    float o_min;                  /* stored space: rows not above it are dead: sample */
    float reserved;
    double min_opacity;           /* activated space: lower clamp of a source's new opacity: update */
    float* opacities;             /* [P]     read by the sample, updated in place by the update */
    float* scales;                /* [P, 3]  updated in place by the update */
    const int64_t* u;             /* [n_draws] random 64-bit words, read as uint64: sample */
    void* workspace;              /* hs_mcmc_workspace_bytes(P, n_draws) bytes, 16-byte aligned: both */
    uint32_t* row_map;            /* GROW: [P + n_draws], written by the sample (NULL for RELOCATE) */
    uint32_t* counts;             /* device, [HS_MCMC_COUNTS]: written by the sample */
    uint32_t* counts_host;        /* NULL, or a page-locked host address the GPU can write: the sample's copy of counts */
    const hs_densify_matrix* matrices; /* HOST array of n_matrices descriptors (copied into the kernel's arguments): update */
    int32_t n_matrices;
    int32_t reserved2;
} hs_mcmc_args;

typedef struct hs_mcmc_noise_args {
    int64_t P;
    int32_t flags;                /* HS_DENSIFY_RAW_* */
    float scaler;                 /* lr_xyz * noise_lr */
    float* means3D;               /* [P, 3]  in place */
    const float* opacities;       /* [P] */
    const float* scales;          /* [P, 3] */
    const float* rotations;       /* [P, 4] (w, x, y, z), not normalised */
    const float* xi;              /* [P, 3] standard normals */
} hs_mcmc_noise_args;

/* the formula above; -1 (HS_EINVAL) unless 0 <= P < 2^30 and 0 <= n_draws < 2^30 */
HS_API int64_t hs_mcmc_workspace_bytes(int64_t P, int64_t n_draws);
HS_API int hs_mcmc_sample(const hs_mcmc_args* args, void* hip_stream);
HS_API int hs_mcmc_update(const hs_mcmc_args* args, void* hip_stream);
HS_API int hs_mcmc_noise(const hs_mcmc_noise_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) The regularisers of the MCMC policy (mcmc_reg.hip): the publication adds
 *     lambda_o mean|opacity| + lambda_s mean|scale|        (activated values; 0.01 each upstream)
 * to every step's loss, so that Gaussians die and the relocation has rows to move.  hs_mcmc_regularize is called after
 * hs_backward and before hs_adam_step: it ADDS the gradient of the two terms, with respect to the values AS STORED, in place
 * to the gradient rows that exist already -- the rows keep their address -- and optionally writes the two terms to the
 * device.  No host wait, no allocation, no memset or copy, no atomics; the caller owns every byte.
 *
 * fp32 throughout, every operation one correctly rounded IEEE operation plus the library expf, nothing contracted, denormals
 * kept.  The host computes, in double and rounded once,  ko = (float)(lambda_opacity / P),  ks = (float)(lambda_scale / (3 P)).
 * Per element (x the stored value, g its gradient):
 *     opacities, HS_DENSIFY_RAW_OPACITY:   o = 1 / (1 + expf(-x));   g <- g + ko * ((1 - o) * o)     (torch's sigmoid backward)
 *     opacities, stored linear:            g <- g + ko * sign(x)      sign(+-0) = 0, sign(NaN) = NaN
 *     scales, HS_DENSIFY_RAW_SCALES:       s = expf(x);              g <- g + ks * s
 *     scales, stored linear:               g <- g + ks * sign(x)
 * A gradient array whose lambda is 0 is NOT WRITTEN (its bits stay, -0.0 and NaN included) and may be NULL; with both lambdas
 * 0 and loss == NULL nothing is launched.  A NaN input gives a NaN in its own element only.
 * loss (device, [2], or NULL): each element's o or |x| (s or |x| for the scales) -- the fp32 value above -- is converted to
 * double; a workgroup of 256 Gaussians adds its 256 opacity terms and 768 scale terms (thread t: scale floats t, t + 256,
 * t + 512 of the block, in that order; then a halving tree over the threads) into one {S_o, S_s} record of the workspace; ONE
 * workgroup of a second kernel adds the records: thread t those of [t c, (t + 1) c), c = ceil(blocks / 256), ascending, then
 * thread 0 the 256 thread sums, ascending.
 *     loss[0] = (float)(lambda_opacity * (S_o / P)),   loss[1] = (float)(lambda_scale * (S_s / (3 P)))
 * The order is a function of P alone and every record is written before it is read: the same bits on every run, whatever
 * the workspace held.  Workspace: hs_mcmc_reg_workspace_bytes(P) = align256(16 ceil(P / 256)) bytes, 16-byte aligned, only
 * read / written when loss != NULL.
 * One thread covers one opacity and three scale floats; the map is elementwise, so a wave's loads and stores are contiguous.
 * Limits (HS_EINVAL, reported before any HIP call): 0 <= P < 2^30; flags within HS_DENSIFY_RAW_*; both lambdas finite and
 * >= 0; opacities / scales non-NULL when their lambda is not 0 or loss is given, a gradient array non-NULL when its lambda is
 * not 0, workspace non-NULL with loss.  Pointers need 4-byte alignment only (the workspace 16).  With P == 0 loss receives
 * {0, 0} and no data pointer is looked at. */
typedef struct hs_mcmc_reg_args {
    int64_t P;
    int32_t flags;                /* HS_DENSIFY_RAW_* */
    int32_t reserved;
    double lambda_opacity;        /* >= 0, finite */
    double lambda_scale;          /* >= 0, finite */
    const float* opacities;       /* [P]     as stored */
    const float* scales;          /* [P, 3]  as stored */
    float* dL_dopacities;         /* [P]     in place; may be NULL when lambda_opacity == 0 */
    float* dL_dscales;            /* [P, 3]  in place; may be NULL when lambda_scale == 0 */
    float* loss;                  /* device [2] or NULL: {lambda_o mean|o|, lambda_s mean|s|} */
    void* workspace;              /* hs_mcmc_reg_workspace_bytes(P) bytes, 16-byte aligned; only read / written when loss != NULL */
} hs_mcmc_reg_args;

/* the formula above; -1 (HS_EINVAL) unless 0 <= P < 2^30 */
HS_API int64_t hs_mcmc_reg_workspace_bytes(int64_t P);
HS_API int hs_mcmc_regularize(const hs_mcmc_reg_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Activations of the STORED cloud (activate.hip).  A trainer stores logit opacities,
 * log scales and unnormalised quaternions -- what hs_adam_step updates and hs_densify_* compact -- while hs_forward /
 * hs_backward take opacities, scales and unit quaternions.  hs_activate computes the second from the first; hs_activate_backward
 * turns the gradients hs_backward wrote into gradients with respect to the stored values, IN PLACE.  One kernel each; the
 * caller owns every byte, nothing is allocated, nothing synchronises.  fp32, every operation one correctly rounded IEEE
 * operation plus the library expf, nothing contracted, denormals kept, no atomics: the same inputs give the same bits.
 *
 * hs_activate, rows [0, P) of every tensor whose STORED pointer is not NULL (its activated pointer must then be given):
 *     opacities[i]   = 1 / (1 + expf(-opacity_raw[i]))
 *     scales[j]      = expf(scales_raw[j])                                     j in [0, 3 P)
 *     n              = max(sqrtf(((q0 q0 + q1 q1) + q2 q2) + q3 q3), 1e-12f)   q = rotations_raw[4 i ..]
 *     rotations[4 i + k] = q_k / n                                             (torch.nn.functional.normalize's clamp)
 * hs_activate_backward, rows [g_begin, g_end) of every tensor whose GRADIENT pointer is not NULL (its activated pointer, and
 * for the rotations the stored one, must then be given), with o / s / q^ the activated values hs_activate wrote:
 *     dL_dopacities[i] <- (g o) (1 - o)
 *     dL_dscales[j]    <- g s
 *     d = ((q^0 g0 + q^1 g1) + q^2 g2) + q^3 g3;   dL_drotations[4 i + k] <- (g_k - q^_k d) / n
 *     with n recomputed from the stored q as above; where the clamp was active (|q| < 1e-12f) g_k <- g_k / 1e-12f
 * Each element is read and written by the same thread.  The map is linear in g: converting the rows of a chunk before they are
 * summed over ranks that hold the same parameters gives the sum's conversion.
 * Every pointer needs 4-byte alignment only (16-byte accesses are used where the addresses allow, 4-byte accesses of exactly
 * the rows' elements otherwise).  Limits (HS_EINVAL, reported before any HIP call): 0 <= P < 2^30, 0 <= g_begin <= g_end <= P.
 * P == 0, an empty range and a call with no tensor present are successful no-ops. */
typedef struct hs_activate_args {
    int64_t P;                    /* rows of every tensor */
    int64_t g_begin, g_end;       /* hs_activate_backward: the rows to convert (hs_activate ignores them) */
    const float* opacity_raw;     /* [P]     logits          NULL = absent */
    const float* scales_raw;      /* [P, 3]  logs            NULL = absent */
    const float* rotations_raw;   /* [P, 4]  (w, x, y, z), any length */
    float* opacities;             /* [P]     written by hs_activate, read by hs_activate_backward */
    float* scales;                /* [P, 3] */
    float* rotations;             /* [P, 4] */
    float* dL_dopacities;         /* [P]     hs_activate_backward, in place   NULL = absent */
    float* dL_dscales;            /* [P, 3] */
    float* dL_drotations;         /* [P, 4] */
} hs_activate_args;

HS_API int hs_activate(const hs_activate_args* args, void* hip_stream);
HS_API int hs_activate_backward(const hs_activate_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) The 3D smoothing filter of Mip-Splatting (smoothing.hip).  HS_FLAG_ANTIALIAS is the
 * publication's 2D screen-space filter; this is its per-Gaussian half: a radius, from the training cameras, below which no
 * camera resolves a Gaussian (hs_smoothing_filter), and the activations of the stored cloud with that radius folded into the
 * scales and opacities (hs_smoothing_apply / hs_smoothing_apply_backward, in place of hs_activate / hs_activate_backward for
 * those two tensors).  Kernels only, on the caller's stream: no memset, no copy, no allocation, no synchronisation, no
 * floating-point atomics; the caller owns every byte.  fp32, every operation one correctly rounded IEEE operation plus the
 * library expf, nothing contracted, denormals kept: the same inputs give the same bits on every run.
 *
 * hs_smoothing_filter.  Per Gaussian i (x, y, z its position) and camera c, with m the camera's 16 floats (the transposed
 * convention of hs_fwd_args.viewmatrices) and (fx, fy, W, H) its intrinsics in pixels:
 *     xc = ((m0 x + m4 y) + m8 z) + m12;   yc = ((m1 x + m5 y) + m9 z) + m13;   zc = ((m2 x + m6 y) + m10 z) + m14
 *     u  = (xc / zc) * fx + 0.5f * W;      v  = (yc / zc) * fy + 0.5f * H
 *     valid = zc > 0.2f && u >= -0.15f * W && u <= 1.15f * W && v >= -0.15f * H && v <= 1.15f * H       (a NaN: not valid)
 * (the published margin and near plane; 0.2 is also the rasterizer's cull).  d_i = the minimum of zc over the valid cameras,
 * n_i = their number; D = the maximum of d_i over the Gaussians with n_i > 0; fmax = the maximum of fx over all cameras (a NaN
 * fx is passed over).  Then
 *     filter[i] = ((n_i > 0 ? d_i : D) / fmax) * 0.4472135901451111f          (sqrt(0.2) in fp32, bits 0x3ee4f92e)
 * -- a Gaussian no camera sees takes the largest seen distance, as published.  If no Gaussian is seen at all, or C == 0, every
 * filter[i] is 0.0f and every n_i is 0.  Minimum and maximum are exact in any order, so the result does not depend on how the
 * kernels divide the work.  Two launches: one thread per Gaussian with the cameras staged through LDS 64 at a time, one
 * {D_b, fmax} pair of workspace words per workgroup; then every workgroup folds the pairs and writes the radii.  Nothing at
 * or beyond row P of filter / n_views and nothing beyond hs_smoothing_filter_workspace_bytes(P) bytes of the workspace is
 * written, and no workspace word is read that this call has not written: the result is the same whatever the workspace held.
 * Limits (HS_EINVAL, reported before any HIP call): 0 <= P < 2^30; 0 <= C < 2^20; xyz, filter and workspace non-NULL, and with
 * C > 0 viewmatrices and intrinsics; every pointer 4-byte aligned, the workspace 256-byte aligned.  P == 0 is a successful
 * no-op: no data pointer is looked at and nothing is launched. */
typedef struct hs_smoothing_filter_args {
    int64_t P;                    /* Gaussians */
    int64_t C;                    /* cameras */
    const float* xyz;             /* [P, 3] */
    const float* viewmatrices;    /* [C, 16] transposed convention, as hs_fwd_args.viewmatrices; may be NULL when C == 0 */
    const float* intrinsics;      /* [C, 4]  (fx, fy, W, H) in pixels, per camera; may be NULL when C == 0 */
    float* filter;                /* [P] out: the radius */
    int32_t* n_views;             /* [P] out or NULL: cameras that see the Gaussian */
    void* workspace;              /* hs_smoothing_filter_workspace_bytes(P) bytes, 256-byte aligned */
} hs_smoothing_filter_args;

/* align256(8 min(ceil(P / 256), 2048)): a multiple of 256, non-decreasing in P; -1 (HS_EINVAL) unless 0 <= P < 2^30 */
HS_API int64_t hs_smoothing_filter_workspace_bytes(int64_t P);
HS_API int hs_smoothing_filter(const hs_smoothing_filter_args* args, void* hip_stream);

/* hs_smoothing_apply, rows [0, P), with x = opacity_raw[i], l_k = scales_raw[3 i + k], f = filter[i]:
 *     o  = 1 / (1 + expf(-x));   s_k = expf(l_k);   q_k = s_k s_k;   f2 = f f
 *     v_k = q_k + f2;   s'_k = sqrtf(v_k);   r_k = q_k / v_k;   t_k = f2 / v_k;        where v_k == 0:  r_k = 1, t_k = 0
 *     c  = sqrtf((r_0 r_1) r_2);   o' = o c
 *     scales[3 i + k] = s'_k;   opacities[i] = o'
 * c is the published sqrt(det(S^2) / det(S^2 + f^2 I)) as a product of per-axis ratios, so that tiny scales do not underflow;
 * t_k is 1 - r_k without the cancellation.  A filter of zeros gives hs_activate's opacities and scales bit for bit.
 * hs_smoothing_apply_backward, rows [g_begin, g_end), IN PLACE on the gradient rows hs_backward wrote (g_o, g_k the values
 * found there; every element is read and written by the same thread); o, s', r, t, c and o' are recomputed from the stored
 * values with the forward's own operations and carry its bits -- opacities / scales are not read:
 *     dL_dopacities[i]   <- ((g_o c) o) (1 - o)
 *     dL_dscales[3i + k] <- (g_k s'_k) r_k + (g_o o') t_k          where t_k == 0 the second term is not added
 * (with a zero filter the rows are hs_activate_backward's bit for bit, a -0.0 included).  The filter is a constant and gets no gradient.  The map is linear in g: converting the rows of a chunk before they are summed
 * over ranks that hold the same parameters gives the sum's conversion.  A thread takes four consecutive rows; 16-byte accesses
 * are used where every pointer is 16-byte aligned and the four rows lie inside the range, 4-byte accesses of exactly the rows'
 * elements otherwise.  Limits (HS_EINVAL, reported before any HIP call): 0 <= P < 2^30, 0 <= g_begin <= g_end <= P; forward:
 * opacity_raw, scales_raw, filter, opacities, scales non-NULL; backward: opacity_raw, scales_raw, filter, dL_dopacities,
 * dL_dscales non-NULL; 4-byte alignment.  P == 0 and an empty range are successful no-ops (no pointer is looked at). */
typedef struct hs_smoothing_apply_args {
    int64_t P;                    /* rows of every tensor */
    int64_t g_begin, g_end;       /* hs_smoothing_apply_backward: the rows to convert (hs_smoothing_apply ignores them) */
    const float* opacity_raw;     /* [P]     logits */
    const float* scales_raw;      /* [P, 3]  logs */
    const float* filter;          /* [P]     what hs_smoothing_filter wrote (any non-negative radius) */
    float* opacities;             /* [P]     written by hs_smoothing_apply */
    float* scales;                /* [P, 3]  written by hs_smoothing_apply */
    float* dL_dopacities;         /* [P]     hs_smoothing_apply_backward, in place */
    float* dL_dscales;            /* [P, 3]  hs_smoothing_apply_backward, in place */
} hs_smoothing_apply_args;

HS_API int hs_smoothing_apply(const hs_smoothing_apply_args* args, void* hip_stream);
HS_API int hs_smoothing_apply_backward(const hs_smoothing_apply_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Mean squared distance to the three nearest neighbours of every point (knn.hip):
 * the isotropic scale of the published SfM initialisation (upstream: simple_knn.distCUDA2).  For every point i of xyz [P, 3],
 * over all j != i -- excluded BY INDEX, not by distance --
 *     d2(i, j)   = ((dx dx) + (dy dy)) + (dz dz)                 dx = x_i - x_j ...
 *     mean_d2[i] = ((b0 + b1) + b2) / (float)k                   b0 <= b1 <= b2 the k = min(3, P - 1) smallest d2(i, .)
 * (fewer addends for k < 3; 0.0f for P = 1).  fp32, every operation one correctly rounded IEEE operation, nothing
 * contracted, denormals kept; coincident points give exact zeros.  Only values are returned, never neighbour indices: the
 * result is unique whatever order the candidates are visited in, and the same inputs give the same bits.  The search is
 * exact: Morton order (30-bit codes, sorted by the radix passes of HS_STAGE_BIN), boxes of 64 consecutive points pruned by a
 * lower bound that never exceeds a computed distance.  Cost grows to O(P^2 / 64) for clouds whose boxes prune nothing
 * (DESIGN.md section 4.19).  Coordinates must be finite (the Python front end checks; here they only decide the values).
 * Kernels only, on the caller's stream: no memset, no copy, no allocation, no synchronisation, no floating-point atomics.
 * `status` (device) reads 0 afterwards, or 2 when a radix pass gave up waiting on its look-back chain: mean_d2 is then
 * invalid (every access still stays inside the arrays).  Nothing at or beyond row P of mean_d2 and nothing beyond
 * hs_knn_workspace_bytes(P) bytes of the workspace is written.
 * Limits (HS_EINVAL, reported before any HIP call): 0 <= P < 2^30; no null pointer; xyz, mean_d2, status 4-byte aligned,
 * workspace 256-byte aligned.  P == 0 is a successful no-op (nothing is launched, status is not written). */
typedef struct hs_knn_args {
    int64_t P;              /* points */
    const float* xyz;       /* [P, 3] */
    float* mean_d2;         /* [P] out */
    void* workspace;        /* hs_knn_workspace_bytes(P) bytes, 256-byte aligned; carved inside */
    uint32_t* status;       /* device word, out: 0 ok, 2 the sort gave up (results invalid) */
} hs_knn_args;

/* non-decreasing in P, a multiple of 256; -1 (HS_EINVAL) unless 0 <= P < 2^30.  ("dist_sq": the Python front end is
 * knn_mean_dist2; exported names of this header carry no digits) */
HS_API int64_t hs_knn_workspace_bytes(int64_t P);
HS_API int hs_knn_mean_dist_sq(const hs_knn_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Per-Gaussian blending-weight statistics (contrib.hip): how much each Gaussian
 * contributes to the images of a finished hs_forward call -- what contribution-based pruning (maximum alpha * T over the
 * training rays), global significance scores (hit count, summed weight) and error-driven densification (sum over pixels of
 * error * weight) decide from.  The quantity exists only inside the compositing loop: this is a front-to-back replay of the
 * forward from the state it left in the three workspaces (rec, point_list, ranges, n_contrib, pair_act).  WHICH policy to
 * run on the statistics stays with the trainer.
 *
 * Definition.  For one finished hs_forward call (HS_STAGE_ALL, or its stages in separate calls) with n_poses poses in
 * F = max(n_frames, 1) frames: take every pose k, every pixel p and every entry g that the published rule composites at
 * (k, p) -- power <= 0, alpha = min(0.99, o * e^power) >= 1 / 255, and the entry comes before the one at which
 * T * (1 - alpha) < 1e-4 terminates the pixel -- with w = alpha * T_before and e = pixel_weight[frame(k), p] (1 when no weight
 * image is given).  A pixel whose weight is exactly 0 takes part in nothing.  The call updates, IN PLACE like the
 * densification statistics of hs_bwd_args:
 *     weight_sum[g]  += sum of e * w                            (fp32)
 *     weight_max[g]   = max(weight_max[g], max of e * w)        (fp32: starts from what the array holds)
 *     pixel_count[g] += number of (k, p) with e * w > 0         (int32)
 * No 1 / N normalisation.  Poses are folded into the running values one at a time in ascending pose order: a call over N poses
 * leaves, bit for bit, what N single-pose calls leave.  A Gaussian no term reached keeps its three values bit for bit.  A
 * call whose binning overflowed (hs_counters.overflow != 0) adds nothing -- decided on the device: nothing waits for the host.
 *
 * Three kernels on the caller's stream, no atomics: the replay (one 16-byte record {sum, max, count, 0} per (tile, instance)
 * pair at the pair's duplicateWithKeys slot; the decisions are the forward's own -- the same alpha expressions, pair_act and
 * n_contrib), a fixed-order sum of every instance's contiguous slots, the fold over the poses.  The same inputs give the same
 * bits.  The workspace is separate from the four of hs_plan: hs_contribution_workspace_bytes(dims) = align256(16 * capacity)
 * + align256(16 * P * n_poses) (256 when that is 0), 256-byte aligned; every word is written before it is read, so the result
 * does not depend on what it held.  The three state workspaces are only read.
 * HS_EINVAL (reported before any HIP call): null args; dims that hs_plan refuses; with P > 0 a null geom, binning, image, ws,
 * weight_sum, weight_max or pixel_count (workspaces 256-byte, arrays 4-byte aligned).  P == 0 is a successful no-op. */
typedef struct hs_contribution_args {
    hs_dims dims;                 /* the dims of the hs_forward call */
    const void* geom;             /* state produced by hs_forward (same buffers) */
    const void* binning;
    const void* image;
    void* ws;                     /* hs_contribution_workspace_bytes(&dims) bytes, 256-byte aligned */
    const float* pixel_weight;    /* [F,H,W] or NULL: every weight 1 */
    float* weight_sum;            /* [P] */
    float* weight_max;            /* [P] */
    int32_t* pixel_count;         /* [P] */
} hs_contribution_args;

/* a positive multiple of 256, non-decreasing in capacity; -1 (HS_EINVAL) for dims that hs_plan refuses */
HS_API int64_t hs_contribution_workspace_bytes(const hs_dims* dims);
HS_API int hs_contribution(const hs_contribution_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Per-Gaussian absolute screen-gradient statistic (absgrad.hip): the refinement
 * signal of AbsGS (gsplat's absgrad=True).  densify_grad_accum above holds |sum over pixels of ...|: the signed per-pixel
 * terms of dL/dmean2D cancel across a large blurry Gaussian, which is the one that most needs splitting.  The terms exist
 * only inside the backward's compositing loop, so this is a back-to-front replay of a finished hs_forward from the state it
 * left in the three workspaces, under the upstream gradients hs_backward takes.  The threshold and the schedule stay with
 * the trainer.
 *
 * Definition.  For one finished hs_forward call with n_poses poses in F = max(n_frames, 1) frames: take every pose k of frame
 * f, every pixel p and every entry g that the published rule composites at (k, p) -- the decisions of hs_contribution's
 * definition above.  Let w = dL/dG_{k,p,g} * G be the factor by which the backward multiplies dx = x_g - p_x and dy = y_g -
 * p_y (G = e^power; dL is the upstream gradient with respect to pose k's radiance at p: the 1 / N of the pose average, the
 * CRF chain through the stored radiance in either blur domain, dL_dout_hdr, the frame's exposure; dL_dout_alpha enters the
 * background term, dL_dout_invdepth as a fourth channel -- all exactly as in hs_backward), and (A, B, C) the conic.  The
 * per-pixel terms are
 *     t_x = -(A dx + B dy) w * 0.5 W          t_y = -(C dy + B dx) w * 0.5 H
 * -- the NDC-scaled units of dL_dmeans2D: the sum over p of t_x is the x entry hs_backward returns for that instance.  With
 *     a_x[f,g] = sum over k in f (ascending) of sum over p of |t_x|          a_y likewise
 * the call updates IN PLACE, frames ascending:  abs_grad_accum[g] += sqrt(a_x^2 + a_y^2)   (fp32).
 * No normalisation beyond the 1 / N inside dL; the denominator a trainer divides by is densify_denom, which this call never
 * touches.  A Gaussian with no term in a frame keeps its bits.  A call over F frames leaves, bit for bit, what F single-frame
 * calls leave.  A call whose binning overflowed (hs_counters.overflow != 0) adds nothing -- decided on the device.
 *
 * Three kernels on the caller's stream, no atomics: the replay (one 8-byte record {sum |t_x|, sum |t_y|} per (tile,
 * instance) pair at the pair's duplicateWithKeys slot), a fixed-order sum of every instance's contiguous slots, the fold over
 * the poses of each frame.  The same inputs give the same bits.  The workspace is its own:
 * hs_abs_gradient_workspace_bytes(dims) = align256(8 * capacity) + align256(8 * P * n_poses) (256 when that is 0), 256-byte
 * aligned; every word is written before it is read.  The three state workspaces are only read.
 * HS_EINVAL (reported before any HIP call): null args; dims that hs_plan refuses; dL_dout_alpha or dL_dout_invdepth with
 * n_frames > 1; HS_FLAG_HDR without exposure, crf_table and dims.crf_K == crf_K; with P > 0 a null bg, geom, binning, image,
 * ws, dL_dout_color or abs_grad_accum (workspaces 256-byte, arrays 4-byte aligned).  P == 0 is a successful no-op. */
typedef struct hs_abs_gradient_args {
    hs_dims dims;                 /* the dims of the hs_forward call */
    int32_t flags;                /* the HS_FLAG_* of the call */
    int32_t crf_K;
    float crf_umin, crf_umax;
    const float* bg;              /* [3] */
    const float* exposure;        /* [F] (HDR) */
    const float* crf_table;       /* [3,crf_K] (HDR) */
    const void* geom;             /* state produced by hs_forward (same buffers), read only */
    const void* binning;
    const void* image;
    void* ws;                     /* hs_abs_gradient_workspace_bytes(&dims) bytes, 256-byte aligned */
    const float* dL_dout_color;   /* [F,3,H,W] */
    const float* dL_dout_hdr;     /* [F,3,H,W] or NULL */
    const float* dL_dout_alpha;   /* [H,W] or NULL */
    const float* dL_dout_invdepth; /* [H,W] or NULL */
    float* abs_grad_accum;        /* [P] */
} hs_abs_gradient_args;

/* a positive multiple of 256, non-decreasing in capacity and in P * n_poses; -1 (HS_EINVAL) for dims that hs_plan refuses */
HS_API int64_t hs_abs_gradient_workspace_bytes(const hs_dims* dims);
HS_API int hs_abs_gradient(const hs_abs_gradient_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Per-Gaussian feature compositing (features.hip): C extra channels stored per
 * Gaussian -- a semantic or language feature field, a depth or a normal, a per-Gaussian statistic to look at -- composited
 * per pixel with the blending weights of a finished hs_forward call.  The forward composites three channels (the SH
 * radiance) plus accumulated opacity and inverse depth; this is a front-to-back replay of it from the state it left in the
 * three workspaces (rec, point_list, ranges, n_contrib, pair_act), for any number of further channels, without another
 * preprocess, binning, sort or render pass.  WHAT the features hold stays with the trainer.
 *
 * Definition.  For one finished hs_forward call with n_poses poses and a feature matrix features[P, C] (fp32, row-major,
 * 1 <= C <= 512): take every pose k, every pixel p and every entry g that the published rule composites at (k, p) -- the
 * decisions of hs_contribution's definition above; the forward's own answer to them is pair_act and n_contrib -- with
 * w = alpha * T_before.
 *   Forward.   out[k, c, p] = sum of w * features[g, c] over those entries in list order (front to back), accumulated by
 *     fp32 fma.  Layout [n_poses, C, H, W]; pose k of frame f is index f * N + k.  No background term, no 1 / N, no pose
 *     average (the blur average of a frame is the mean over its N images, taken by the caller).  A pixel nothing reaches is
 *     +0.  EVERY element of out is written, also in tiles with an empty list and for a call whose binning overflowed
 *     (hs_counters.overflow != 0: all zeros, decided on the device).  An entry that is not composited at a pixel adds nothing
 *     there -- it is selected out, not multiplied by zero: a non-finite feature of a Gaussian reaches only the pixels the
 *     Gaussian is composited on.
 *   Backward.  dL_dfeatures[g, c] = sum over k, p of w * dL_dout[k, c, p].  WRITTEN, not accumulated, every element; a
 *     Gaussian nothing reached gets +0, an overflowed frame gives all zeros.  Per instance the (tile, instance) pair records
 *     are summed in slot order; per Gaussian the sum starts at +0 and adds the poses' rows in ascending pose order.  No
 *     atomics: the same inputs give the same bits.  A non-finite dL_dout at a pixel reaches only the Gaussians composited
 *     there.
 * w is a constant of both calls: the gradient these two deliver reaches the features.  The gradient of the same loss with
 * respect to the GEOMETRY (means, covariances, opacities) through the channels is a call of its own,
 * hs_composite_features_geometry_backward below.
 *
 * The forward is one kernel and needs no workspace.  The backward runs passes of three kernels (the replay: one record of
 * the pass's channel sums per (tile, instance) pair at the pair's duplicateWithKeys slot; a fixed-order sum of every
 * instance's contiguous slots; the fold over the poses) -- eight channels per pass (32-byte records) while more than four
 * are left, then four (16-byte records) -- over one workspace of its own, whose size does not depend on C:
 * hs_composite_features_workspace_bytes(dims) = align256(32 * capacity) + align256(32 * P * n_poses) (256 when that is 0),
 * 256-byte aligned; every word is written before it is read.  The three state workspaces are only read.
 * HS_EINVAL (reported before any HIP call): null args; dims that hs_plan refuses; n_channels outside [1, 512]; a null out
 * (forward); with P > 0 a null geom, binning, image, features (forward) or ws, dL_dout, dL_dfeatures (backward) (workspaces
 * 256-byte, arrays 4-byte aligned).  P == 0: the forward writes out (zeros), the backward is a successful no-op. */
typedef struct hs_composite_features_args {
    hs_dims dims;                 /* the dims of the hs_forward call */
    const void* geom;             /* state produced by hs_forward (same buffers), read only */
    const void* binning;
    const void* image;
    int32_t n_channels;           /* C */
    int32_t reserved;
    const float* features;        /* [P,C]; rows are read 16 bytes at a time when C % 4 == 0 and this is 16-byte aligned */
    float* out;                   /* [n_poses,C,H,W] */
} hs_composite_features_args;

typedef struct hs_composite_features_bwd_args {
    hs_dims dims;                 /* the dims of the hs_forward call */
    const void* geom;             /* state produced by hs_forward (same buffers), read only */
    const void* binning;
    const void* image;
    void* ws;                     /* hs_composite_features_workspace_bytes(&dims) bytes, 256-byte aligned */
    int32_t n_channels;           /* C */
    int32_t reserved;
    const float* dL_dout;         /* [n_poses,C,H,W] */
    float* dL_dfeatures;          /* [P,C] */
} hs_composite_features_bwd_args;

/* (backward only) a positive multiple of 256, non-decreasing in capacity; -1 (HS_EINVAL) for dims that hs_plan refuses */
HS_API int64_t hs_composite_features_workspace_bytes(const hs_dims* dims);
HS_API int hs_composite_features(const hs_composite_features_args* args, void* hip_stream);
HS_API int hs_composite_features_backward(const hs_composite_features_bwd_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Gradients to the GEOMETRY through the composited channels (featgeo.hip): what a
 * loss on the output of hs_composite_features asks of the means, scales, rotations and opacities of the forward behind it --
 * the render backward for C channels instead of three.
 *
 * Definition.  Input: a finished hs_forward, features[P, C] and dL_dout[n_poses, C, H, W] (the gradient with respect to the
 * output of hs_composite_features).  At pose k, pixel p and entry i composited there -- the decisions hs_composite_features
 * uses -- let d_i = sum over c of features[g_i, c] * dL_dout[k, c, p].  No background term, no 1 / N and no CRF: the output of
 * hs_composite_features has none.  Back to front, with q = 0 behind the deepest contributor and T from the forward's final
 * transmittance (T_i = T_{i+1} / (1 - alpha_i)):
 *     dL/dalpha_i = T_i (d_i - q_i),    q_{i-1} = q_i + alpha_i (d_i - q_i)
 * -- the render backward's recurrence with c_i . dL replaced by d_i and the background, accumulated-opacity and
 * inverse-depth terms absent.  From dL/dalpha on everything is the render backward's: the terms of the 2-D mean, the conic and
 * the opacity, operand for operand, and the projection of hs_backward (HS_BWD_PROJECT) from there to the 3-D mean, the
 * scales, the rotations and the opacities (HS_FLAG_ANTIALIAS as in the forward).  The 0.99 cap on alpha behaves as in
 * hs_backward: the gradient passes through it.
 * Outputs.  dL_dmeans3D [P,3], dL_dopacities [P], dL_dscales [P,3], dL_drotations [P,4]: WRITTEN, not accumulated, every
 * element, summed over all poses of the call (every frame's).  They are the gradients with respect to the arrays the forward
 * took (the activated ones); a caller that also ran hs_backward adds the two.  An overflowed frame
 * (hs_counters.overflow != 0) gives all zeros, decided on the device.
 * Order.  Channels go in passes of sixteen (the last pass: the narrowest of 4, 8, 16 that holds the rest); d is linear in the
 * channels, so the passes' pair records add, in ascending pass order, each by the one thread that owns the record; per
 * instance the records are summed in slot order (as hs_backward's), per Gaussian the poses in ascending order.  No atomics:
 * the same inputs give the same bits.
 * State.  The three workspaces of the forward are only READ -- in particular the pair flags hs_backward keeps in the
 * binning workspace are not written: hs_backward may run before or after this call on the same state.  The records
 * (hs_backward's 64-byte pair records, colour and inverse-depth slots zero), their flags and the per-instance rows live in
 * a workspace of the call's own: hs_composite_features_geometry_workspace_bytes(dims) = align256(64 * capacity) +
 * align256(64 * P * n_poses) + align256(capacity) (256 when that is 0), 256-byte aligned, its size independent of C; every
 * word the call reads from it is one the call wrote.
 * HS_EINVAL (reported before any HIP call): null args; dims that hs_plan refuses; n_channels outside [1, 512]; with P > 0 a
 * null scales / rotations (a forward with cov3D_precomp is NOT supported) or any other null pointer; a misaligned one
 * (workspaces 256-byte, rotations and dL_drotations 16-byte, the other arrays 4-byte).  P == 0: a successful no-op.
 * Out of scope, each a later change: camera-pose gradients through the channels (the projection could deliver them);
 * dL_dmeans2D and the densification statistics through the channels; cov3D_precomp; normalisation of the channels by the
 * accumulated opacity; the wiring into a captured step (graphs.GraphedStep). */
typedef struct hs_composite_features_geometry_args {
    hs_dims dims;                 /* the dims of the hs_forward call */
    float tanfovx, tanfovy, scale_modifier;   /* as in the forward */
    int32_t flags;                /* the forward's HS_FLAG_* (HS_FLAG_ANTIALIAS is the one that is read) */
    const float* viewmatrices;    /* [n_poses,16], as in the forward */
    const float* projmatrices;    /* [n_poses,16] */
    const float* camposes;        /* [n_poses,3] */
    const float* means3D;         /* [P,3], as the forward took them */
    const float* opacities;       /* [P] */
    const float* scales;          /* [P,3] */
    const float* rotations;       /* [P,4], 16-byte aligned */
    const void* geom;             /* state produced by hs_forward (same buffers), read only */
    const void* binning;
    const void* image;
    void* ws;                     /* hs_composite_features_geometry_workspace_bytes(&dims) bytes, 256-byte aligned */
    int32_t n_channels;           /* C */
    int32_t reserved;
    const float* features;        /* [P,C]; rows are read 16 bytes at a time when C % 4 == 0 and this is 16-byte aligned */
    const float* dL_dout;         /* [n_poses,C,H,W] */
    float* dL_dmeans3D;           /* [P,3] */
    float* dL_dopacities;         /* [P] */
    float* dL_dscales;            /* [P,3] */
    float* dL_drotations;         /* [P,4], 16-byte aligned */
} hs_composite_features_geometry_args;

/* a positive multiple of 256, non-decreasing in capacity and in P * n_poses; -1 (HS_EINVAL) for dims that hs_plan refuses */
HS_API int64_t hs_composite_features_geometry_workspace_bytes(const hs_dims* dims);
HS_API int hs_composite_features_geometry_backward(const hs_composite_features_geometry_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Depth-distortion loss (distort.hip): the regulariser of Mip-NeRF 360 on the
 * blending weights of a ray (2DGS uses it, gsplat ships it as distloss), per pixel of a finished hs_forward call.  It pulls
 * the weights of a ray together and starves floaters and semi-transparent haze.  Quadratic in the weights and built from
 * prefix sums along the ray, it exists only inside the compositing loop: a front-to-back replay of the forward's state for the
 * map, a back-to-front replay for its gradient to the geometry.
 *
 * Definition.  At pose k and pixel p take the entries i = 1..n the forward composited there -- the decisions
 * hs_composite_features uses (pair_act, n_contrib) -- front to back, with w_i = alpha_i * T_i, s_i = 1 / z_i (the instance's
 * view-space depth as stored in the render record: the 1 / z that out_invdepth composites), A_i = sum over j <= i of w_j and
 * D_i = sum over j <= i of w_j s_j:
 *     distortion[k, p] = 2 * sum over i of w_i * (D_{i-1} - s_i * A_{i-1})
 *     moment[k, p]     = D_n                   (sum w s: the expected inverse depth of that pose)
 * A list is sorted by the fp32 bits of z and a correctly rounded reciprocal is monotone, so s is non-increasing along the
 * list and the sum equals sum_i sum_j w_i w_j |s_i - s_j| >= 0.  No background term, no 1 / N, no pose average, no
 * normalisation.  Layout [n_poses, H, W]; pose k of frame f is index f * N + k.  A pixel with fewer than two contributors
 * gives exactly +0.  EVERY element of both outputs is written; a call whose binning overflowed (hs_counters.overflow != 0)
 * gives all zeros, decided on the device.  s is the inverse depth, not z: it is bounded (z > 0.2 gives s < 5), it is what the
 * library already composites, and its gradient path to the mean exists.  The loss is invariant under s -> s - s0, and the
 * kernels carry their sums relative to a workgroup-uniform s0 (1 / z of the tile's first entry); moment is sum w s.
 * Backward.  With gamma = dL/d distortion[k, p], back to front with A_n = 1 - final_T, D_n = moment, q = 0 behind the deepest
 * contributor, T rebuilt from the forward's final transmittance (T_i = T_{i+1} / (1 - alpha_i)), A+_i and D+_i the sums over
 * j > i:
 *     v_i        = 2 * [ (D_{i-1} - s_i A_{i-1}) + (s_i A+_i - D+_i) ]      (= dL_p / dw_i)
 *     dL/dalpha_i = gamma * T_i * (v_i - q_i),    q_{i-1} = q_i + alpha_i (v_i - q_i)
 *     dL/ds_i   += gamma * 2 * w_i * (A+_i - A_{i-1})
 * -- hs_composite_features_geometry_backward's recurrence with d_i = gamma v_i (L_p depends on alpha only through w).  From
 * dL/dalpha on the terms of the 2-D mean, the conic and the opacity are the render backward's, operand for operand; the sum
 * over the pixels of dL/ds_i goes into the inverse-depth slot of the pair record and reaches the 3-D mean through z in the
 * projection of hs_backward (HS_BWD_PROJECT).  The 0.99 cap on alpha passes the gradient through.
 * Outputs of the backward.  dL_dmeans3D [P,3], dL_dopacities [P], dL_dscales [P,3], dL_drotations [P,4]: WRITTEN, not
 * accumulated, every element, summed over all poses of the call, with respect to the arrays the forward took (the activated
 * ones).  An overflowed frame gives all zeros.  Per instance the pair records are summed in slot order, per Gaussian the
 * poses in ascending order.  No atomics: the same inputs give the same bits.
 * State.  The three workspaces of the forward are only READ: hs_backward may run before or after on the same state.  The
 * backward's records, flags and rows live in a workspace of the call's own: hs_distortion_workspace_bytes(dims) =
 * align256(64 * capacity) + align256(64 * P * n_poses) + align256(capacity) (256 when that is 0), 256-byte aligned; every
 * word the call reads from it is one the call wrote.  The forward needs no workspace.
 * HS_EINVAL (reported before any HIP call): null args; dims that hs_plan refuses; a null or misaligned out_distortion /
 * out_moment (forward); with P > 0 a null scales / rotations (a forward with cov3D_precomp is NOT supported) or any other
 * null pointer; a misaligned one (workspaces 256-byte, rotations and dL_drotations 16-byte, the other arrays 4-byte).
 * P == 0: the forward writes zeros, the backward is a successful no-op that looks at no pointer.
 * Out of scope, each a later change: distortion in linear z or a near / far normalisation; the per-frame pose average;
 * camera-pose gradients, dL_dmeans2D and the densification statistics through the term; the wiring into a captured step. */
typedef struct hs_distortion_args {
    hs_dims dims;                 /* the dims of the hs_forward call */
    const void* geom;             /* state produced by hs_forward (same buffers), read only */
    const void* binning;
    const void* image;
    float* out_distortion;        /* [n_poses,H,W] */
    float* out_moment;            /* [n_poses,H,W] */
} hs_distortion_args;

typedef struct hs_distortion_bwd_args {
    hs_dims dims;                 /* the dims of the hs_forward call */
    float tanfovx, tanfovy, scale_modifier;   /* as in the forward */
    int32_t flags;                /* the forward's HS_FLAG_* (HS_FLAG_ANTIALIAS is the one that is read) */
    const float* viewmatrices;    /* [n_poses,16], as in the forward */
    const float* projmatrices;    /* [n_poses,16] */
    const float* camposes;        /* [n_poses,3] */
    const float* means3D;         /* [P,3], as the forward took them */
    const float* opacities;       /* [P] */
    const float* scales;          /* [P,3] */
    const float* rotations;       /* [P,4], 16-byte aligned */
    const void* geom;             /* state produced by hs_forward (same buffers), read only */
    const void* binning;
    const void* image;
    void* ws;                     /* hs_distortion_workspace_bytes(&dims) bytes, 256-byte aligned */
    const float* moment;          /* [n_poses,H,W], what hs_distortion wrote into out_moment */
    const float* dL_ddistortion;  /* [n_poses,H,W] */
    float* dL_dmeans3D;           /* [P,3] */
    float* dL_dopacities;         /* [P] */
    float* dL_dscales;            /* [P,3] */
    float* dL_drotations;         /* [P,4], 16-byte aligned */
} hs_distortion_bwd_args;

/* (backward only) a positive multiple of 256, non-decreasing in capacity and in P * n_poses; -1 (HS_EINVAL) for dims that
 * hs_plan refuses */
HS_API int64_t hs_distortion_workspace_bytes(const hs_dims* dims);
HS_API int hs_distortion(const hs_distortion_args* args, void* hip_stream);
HS_API int hs_distortion_backward(const hs_distortion_bwd_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Bilateral-grid image correction ("Bilateral Guided Radiance Field Processing",
 * SIGGRAPH 2024), fused (bilagrid.hip): every frame owns a small 3-D lattice of 3 x 4 affine colour matrices addressed by pixel
 * position and luma; the rendered image is sliced through it between the rasterizer and the loss, and a total-variation term
 * keeps the lattice smooth.
 *
 * Shapes.  grids [G, 12, L, Y, X] fp32: coefficient c = 4 i + k is entry (row i, column k) of the matrix, the identity has
 * c = 0, 5, 10 equal to 1.  Images [F, 3, H, W] fp32 planar (the rasterizer's output).  grid_ids int32 [F] IN DEVICE MEMORY.
 * Axis rule, for an axis of n lattice points and a value v: n == 1: i0 = i1 = 0, f = 0; else t = min(max(v, 0), 1) (n - 1),
 * i0 = min(floor(t), n - 2), i1 = i0 + 1, f = t - i0 (a NaN v counts as 0).
 * Forward, per pixel (px, py) of frame fr with colour (r, g, b): x = (px + 0.5) / W on X, y = (py + 0.5) / H on Y,
 * z = 0.299 r + 0.587 g + 0.114 b on L; A[c] = the sum over the eight corners of w_x w_y w_z grids[grid_ids[fr], c, l, yy, xx]
 * (1 - f at the i0 side, f at the i1 side); out_i = A[4i] r + A[4i+1] g + A[4i+2] b + A[4i+3].  This is grid_sample(grids,
 * 2 (x, y, z) - 1, bilinear, padding border, align_corners) followed by the affine.  The fp32 operation ORDER is stated at
 * the top of bilagrid.hip and restated by tests/bilagrid_reference.py: forward and dL_dimage are compared bit for bit.
 * A frame whose id is outside [0, G) (-1: "no grid", an evaluation view) is the identity: out is bit for bit image, dL_dimage
 * bit for bit dL_dout, and the frame adds nothing to dL_dgrids.
 * Backward.  dL_dgrids[g, c = 4i + k, l, yy, xx] = the sum, over the frames with grid_ids[fr] == g in ascending fr and their
 * pixels, of w_x w_y w_z dL_dout_i v_k, v = (r, g, b, 1) -- a gather per destination in a fixed order, no atomics: the same
 * inputs give the same bits.  EVERY element is written, by a kernel; a grid no frame used gets exact zeros.
 * dL_dimage_k = sum_i A[4i+k] dL_dout_i, plus, where 0 < z < 1 strictly and L > 1, luma_k (L - 1) sum_i dL_dout_i
 * sum_k' (dA[4i+k'] / df_z) v_k'.  The pixel position carries no gradient.
 * Limits (HS_EINVAL): F, H, W, G >= 1, 1 <= L <= 16, 1 <= X, Y <= 64, 3 F H W < 2^31, 12 G L Y X < 2^31; float and id
 * pointers 4-byte aligned, the workspace 256-byte aligned.  The caller owns every byte, nothing is allocated, the work is
 * enqueued on the caller's stream, nothing synchronises, and no word of the workspace is read before it is written. */
typedef struct hs_bilagrid_args {
    int32_t F, H, W, G, L, Y, X;
    int32_t reserved;
    const float* image;           /* [F, 3, H, W] */
    const float* grids;           /* [G, 12, L, Y, X] */
    const int32_t* grid_ids;      /* [F], device memory */
    float* out;                   /* [F, 3, H, W] written by hs_bilagrid_slice */
    const float* dL_dout;         /* [F, 3, H, W] (backward) */
    float* dL_dimage;             /* [F, 3, H, W] written by the backward, or NULL: skipped */
    float* dL_dgrids;             /* [G, 12, L, Y, X] written by the backward, or NULL: skipped */
    void* workspace;              /* hs_bilagrid_workspace_bytes(...) bytes; only read / written when dL_dgrids != NULL */
} hs_bilagrid_args;

/* align256(4 F chunks 12 L Y X): one record of the 12 L sums of every lattice column per frame and chunk of 32 rows of the
 * column's pixel footprint.  chunks = ceil(tallest / 32), tallest = the most rows hi - lo + 1 any lattice row yy has, with
 * (Y == 1: lo = 0, hi = H - 1)  m = 2 + H / 2^20, lo = max(0, yy == 0 ? 0 : floor((yy - 1) H / (Y - 1)) - m),
 * hi = min(H - 1, ceil((yy + 1) H / (Y - 1)) + m).  -1 (HS_EINVAL) outside the limits above. */
HS_API int64_t hs_bilagrid_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t G, int32_t L, int32_t Y, int32_t X);
HS_API int hs_bilagrid_slice(const hs_bilagrid_args* args, void* hip_stream);
HS_API int hs_bilagrid_slice_backward(const hs_bilagrid_args* args, void* hip_stream);

/* Total variation of the grids: over the three lattice axes of size > 1, the mean over all grids, coefficients and positions
 * of (grids[.., j + 1] - grids[.., j])^2 along that axis; an axis of size 1 adds nothing.  Differences and sums in fp64, the
 * blocks added in a fixed order: the same bits on every run.  The backward writes dL_dgrids = dL_dtv[0] * d tv / d grids
 * (every element; dL_dtv is read on the device).  Limits: those of the lattice above. */
#define HS_BILAGRID_TV_WORKSPACE_BYTES 24576 /* 1024 blocks x 3 fp64 sums */
typedef struct hs_bilagrid_tv_args {
    int32_t G, L, Y, X;
    const float* grids;           /* [G, 12, L, Y, X] */
    float* tv;                    /* [1] written by hs_bilagrid_tv */
    const float* dL_dtv;          /* [1] upstream gradient (backward) */
    float* dL_dgrids;             /* [G, 12, L, Y, X] written by the backward */
    void* workspace;              /* HS_BILAGRID_TV_WORKSPACE_BYTES bytes, 256-byte aligned (forward only) */
} hs_bilagrid_tv_args;

HS_API int hs_bilagrid_tv(const hs_bilagrid_tv_args* args, void* hip_stream);
HS_API int hs_bilagrid_tv_backward(const hs_bilagrid_tv_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) k-means vector quantisation of the rows of a matrix (vq.hip): the codebook compression
 * of a finished cloud's view-dependent SH coefficients (LightGaussian's VecTree step, gsplat's PngCompression on shN,
 * Compact3D).  Lloyd's two steps; the loop, the initialisation and what is quantised are the caller's.
 *
 * Assign.  x [N, D] fp32 row-major, codebook_in [K, D] fp32.  d2(i, k): acc = 0; for d ascending: t = x[i,d] - c[k,d],
 * acc = acc + t * t -- fp32, every operation rounded once, no contraction.  codes[i] = the k of the smallest d2, scanning k
 * ascending with a strict < against a running best that starts at +inf: ties go to the lower k; a row whose distances are all
 * NaN gets code 0 and dist2 = +inf.  dist2[i] = the winning value.  tests/vq_reference.py restates it; compared bit for bit.
 * Update.  For each cluster k: S_w = sum of (double)weights[i] over its members (weights NULL: all 1), S_d = sum of
 * (double)weights[i] (double)x[i,d]; codebook_out[k,d] = (float)(S_d / S_w) when S_w > 0, else codebook_in[k,d] bit for bit (an
 * empty cluster, or one whose weights are all zero); counts[k] = the members of k whatever their weights.  A code outside
 * [0, K) belongs to no cluster.  Negative weights are undefined; nothing reads them on the host.  The fp64 sums are added in a
 * fixed order that depends on (N, K, codes) alone -- the top of vq.hip states it -- with no atomics: the same inputs give
 * the same bits, whatever the workspace held.  codebook_out must not alias codebook_in.
 * Limits (HS_EINVAL, before any HIP call): 0 <= N <= 2^30, 1 <= D <= 48, 1 <= K <= 65536; pointers 4-byte aligned, the
 * workspace 256-byte aligned; N = 0 is valid (assign writes nothing; update copies codebook_in and zeroes counts; x, codes and
 * the workspace may then be NULL).  The caller owns every byte, nothing is allocated, the work is enqueued on the caller's
 * stream and nothing synchronises. */
typedef struct hs_vq_args {
    int32_t N, D, K;
    const float* x;               /* [N, D] */
    const float* weights;         /* [N] >= 0, or NULL: all 1 (update) */
    const float* codebook_in;     /* [K, D] */
    int32_t* codes;               /* [N]: written by the assignment, read by the update */
    float* dist2;                 /* [N] written by the assignment, or NULL: skipped */
    float* codebook_out;          /* [K, D] written by the update */
    int32_t* counts;              /* [K] written by the update */
    void* workspace;              /* hs_vq_workspace_bytes(N, D, K) bytes (update only) */
} hs_vq_args;

/* a positive multiple of 256, non-decreasing in N; -1 (HS_EINVAL) outside the limits above.  No HIP call. */
HS_API int64_t hs_vq_workspace_bytes(int32_t N, int32_t D, int32_t K);
/* reads x, codebook_in; writes codes, dist2 (may be NULL) */
HS_API int hs_vq_assign(const hs_vq_args* args, void* hip_stream);
/* reads x, weights (may be NULL), codes, codebook_in; writes codebook_out, counts */
HS_API int hs_vq_update(const hs_vq_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Lens undistortion of captured frames, fused with the area-filtered downscale to the
 * training resolution (undistort.hip): the step between a COLMAP camera with distortion and the pinhole rasterizer.  One map
 * per camera (hs_undistort_map), then every frame of that camera through it (hs_undistort_remap).
 *
 * Cameras.  model = COLMAP's model id (HS_CAMERA_*); fx, fy, cx, cy and k[8] are the source camera's parameters rounded to
 * fp32 by the host, k in COLMAP's order after the intrinsics (SIMPLE_RADIAL: k; RADIAL: k1 k2; OPENCV: k1 k2 p1 p2;
 * FULL_OPENCV: k1 k2 p1 p2 k3 k4 k5 k6; OPENCV_FISHEYE: k1 k2 k3 k4; unused entries are ignored).  Pixel coordinates are
 * COLMAP's: the centre of pixel (i, j) is at (i + 0.5, j + 0.5).
 * Map.  The undistorted full-resolution grid is Wf x Hf with the source's fx, fy and its principal point at (Wf / 2, Hf / 2).
 * For its pixel (x, y): u = ((x + 0.5) - Wf / 2) / fx, v = ((y + 0.5) - Hf / 2) / fy; (ud, vd) = the model's forward mapping
 * of (u, v); map[y, x] = (sx, sy) = (ud * fx + cx, vd * fy + cy); valid[y, x] = 1 when 0.5 <= sx <= W - 0.5 and
 * 0.5 <= sy <= H - 0.5, else 0 (a NaN gives 0).  All in fp32, every operation rounded once, in the order stated at the top of
 * undistort.hip and restated by tests/undistort_reference.py: compared bit for bit (OPENCV_FISHEYE calls the library atanf
 * and is compared in pixels instead).
 * Remap.  frames: uint8 [F, H, W, 3] (frames_u8 != 0; what a decoder delivers) or fp32 [F, 3, H, W]; factor S in {1, 2, 3, 4,
 * 8}, Wf and Hf multiples of S; out fp32 [F, 3, Hf / S, Wf / S].  out[f, c, yo, xo] = the sum, over j = 0 .. S-1 and inside
 * that i = 0 .. S-1 ascending and starting from 0, of the bilinear sample of channel c of frame f at map[yo S + j, xo S + i],
 * divided by (float)(S S), and for uint8 frames then divided by 255.  Bilinear sample at (sx, sy): a NaN coordinate samples as
 * 0; px = min(max(sx - 0.5, 0), W - 1), x0 = min((int)floor(px), W - 2), wx = px - x0, likewise py, y0, wy with H;
 * top = (1 - wx) t00 + wx t01, bottom = (1 - wx) t10 + wx t11, sample = (1 - wy) top + wy bottom, t_ab = the tap at
 * (x0 + b, y0 + a): exact on every pixel centre.  EVERY element of map / valid / out is written, by a kernel, whatever the
 * buffers held.  No atomics.
 * Limits (HS_EINVAL, reported before any HIP call): args non-null; model one of the seven HS_CAMERA_* below; 2 <= W, H <=
 * 16384; 0 <= Wf, Hf <= 16384; remap: factor in {1, 2, 3, 4, 8} dividing Wf and Hf, F >= 0, 3 F H W < 2^31 and
 * 3 F (Hf / S) (Wf / S) < 2^31; map: fx, fy finite and > 0, cx, cy and k finite.  Pointers: map non-null and 8-byte aligned,
 * valid non-null (map), frames non-null and 4-byte aligned when fp32, out non-null and 4-byte aligned (remap) -- except that
 * F = 0 or an empty grid (Wf = 0 or Hf = 0) is a valid call that launches nothing and returns HS_OK, with or without
 * pointers (those given must still be aligned).  The caller owns every byte, nothing is allocated, the work is enqueued on
 * the caller's stream and nothing synchronises. */
#define HS_CAMERA_SIMPLE_PINHOLE 0
#define HS_CAMERA_PINHOLE 1
#define HS_CAMERA_SIMPLE_RADIAL 2
#define HS_CAMERA_RADIAL 3
#define HS_CAMERA_OPENCV 4
#define HS_CAMERA_OPENCV_FISHEYE 5
#define HS_CAMERA_FULL_OPENCV 6
typedef struct hs_undistort_args {
    int32_t model;                /* HS_CAMERA_* (map) */
    int32_t W, H;                 /* source frame */
    int32_t Wf, Hf;               /* undistorted full-resolution grid = the map */
    int32_t F;                    /* frames (remap) */
    int32_t factor;               /* S (remap) */
    int32_t frames_u8;            /* != 0: frames are uint8 [F, H, W, 3]; 0: fp32 [F, 3, H, W] (remap) */
    float fx, fy, cx, cy;         /* source intrinsics (map) */
    float k[8];                   /* distortion coefficients (map) */
    float* map;                   /* [Hf, Wf, 2]: written by hs_undistort_map, read by hs_undistort_remap */
    uint8_t* valid;               /* [Hf, Wf] written by hs_undistort_map */
    const void* frames;           /* (remap) */
    float* out;                   /* [F, 3, Hf / S, Wf / S] written by hs_undistort_remap */
} hs_undistort_args;

/* reads the camera; writes map, valid */
HS_API int hs_undistort_map(const hs_undistort_args* args, void* hip_stream);
/* reads map, frames; writes out */
HS_API int hs_undistort_remap(const hs_undistort_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Depth-normal consistency (normals.hip): the regulariser 2DGS, GOF, RaDe-GS, PGSR
 * and dn-splatter pair with the distortion term -- the composited per-Gaussian normals must agree with the normals of the
 * surface the composited depth describes.
 *
 * Shapes.  invdepth, alpha, weight, out, dL_dout, dL_dinvdepth, dL_dalpha: [B, H, W] fp32; normals, depth_normals,
 * dL_dnormals: [B, 3, H, W] fp32 planar; cam_to_world [B, 3, 3] fp32 row-major IN DEVICE MEMORY.  The principal point is the
 * centre of the frame.
 * Forward, per frame b and pixel (x, y).  d = invdepth (sum w / z, what out_invdepth holds), a = alpha (NULL: 1).  A sample is
 * VALID when d and a are finite and > 0; its depth is z = a / d.  P(x, y) = z ((x + 0.5 - W / 2) / fx, (y + 0.5 - H / 2) / fy, 1).
 * A pixel is INTERIOR when 1 <= x <= W - 2, 1 <= y <= H - 2 and it and its four axis neighbours are valid.  There
 * c = (P(x, y+1) - P(x, y-1)) x (P(x+1, y) - P(x-1, y)), n_d = c / |c|, n = R_b n_d (cam_to_world NULL: n = n_d), and
 * out[b, y, x] = w (1 - sum_k normals[b, k, y, x] n_k) with w = weight (NULL: 1); depth_normals[b, :, y, x] = n.  Elsewhere
 * out and depth_normals are exactly 0; a frame with W < 3 or H < 3 is a valid call that gives zeros.  With positive depths
 * c . P < 0: the normal faces the camera and |c| > 0.  The kernel evaluates fx fy c / (s_x s_y) (s = the sum of the two
 * depths of an axis, a positive factor) from r = (difference) / (sum) per axis: (fx r_x, fy r_y, -(r_y yh + r_x xh + 1)) --
 * the same direction without the cancellation in a difference of z u and without overflow; the fp32 operation order is
 * stated at the top of normals.hip and restated, with a rounding bound per element, by tests/normals_reference.py.
 * `normals` is used as given (no normalisation: sum w n of composite_features has length <= alpha).
 * Range.  Validity is decided on d and a alone, as stated: a valid sample whose quotient a / d underflows to 0 or overflows to
 * infinity in fp32 (a / d outside about [1e-38, 3e38]) stays valid, and NaN then reaches out and the gradients of the pixels
 * whose stencil it sits in.  Depths a renderer produces are far inside; nothing clamps them here.
 * Backward.  dL_dnormals_k = -dL_dout w n_k at interior pixels; dL_dinvdepth and dL_dalpha collect, per sample, the
 * contributions of the four pixels whose stencil the sample sits in (through z = a / d: dz/dd = -z / d, dz/da = 1 / d) -- a
 * gather in a fixed order, no atomics: the same inputs give the same bits.  Each of the three is written only when its
 * pointer is given, and then EVERY element is written: exactly 0 at invalid samples and at samples (pixels) that feed no
 * interior pixel.  weight, fx, fy and cam_to_world are constants.  All three NULL: a no-op.
 * Limits (HS_EINVAL, reported before any HIP call): args non-null; B, H, W >= 1, 3 B H W < 2^31; fx, fy finite and > 0;
 * invdepth non-null; forward: out or depth_normals given, normals non-null when out is; backward: normals and dL_dout
 * non-null, dL_dalpha only with alpha; every pointer given 4-byte aligned.  The caller owns every byte, nothing is allocated,
 * cleared or copied, the work is enqueued on the caller's stream and nothing synchronises: one launch each way. */
typedef struct hs_normal_consistency_args {
    int32_t B, H, W;
    int32_t reserved;
    float fx, fy;
    const float* invdepth;        /* [B, H, W] */
    const float* alpha;           /* [B, H, W], or NULL: 1 */
    const float* normals;         /* [B, 3, H, W] */
    const float* weight;          /* [B, H, W], or NULL: 1 */
    const float* cam_to_world;    /* [B, 3, 3] row-major, device memory, or NULL: the identity */
    float* out;                   /* [B, H, W] written by the forward, or NULL: skipped */
    float* depth_normals;         /* [B, 3, H, W] written by the forward, or NULL: skipped */
    const float* dL_dout;         /* [B, H, W] (backward) */
    float* dL_dnormals;           /* [B, 3, H, W] written by the backward, or NULL: skipped */
    float* dL_dinvdepth;          /* [B, H, W] written by the backward, or NULL: skipped */
    float* dL_dalpha;             /* [B, H, W] written by the backward, or NULL: skipped (NULL when alpha is) */
    void* workspace;              /* hs_normal_consistency_workspace_bytes(B, H, W) bytes: none today, may be NULL, never touched */
} hs_normal_consistency_args;

/* 0: the backward keeps the halo of its gather in LDS.  -1 (HS_EINVAL) outside the limits above.  No HIP call. */
HS_API int64_t hs_normal_consistency_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* reads invdepth, alpha, normals, weight, cam_to_world; writes out, depth_normals */
HS_API int hs_normal_consistency(const hs_normal_consistency_args* args, void* hip_stream);
/* reads the same and dL_dout; writes dL_dnormals, dL_dinvdepth, dL_dalpha */
HS_API int hs_normal_consistency_backward(const hs_normal_consistency_args* args, void* hip_stream);

/* The per-Gaussian normal that is composited (normals.hip): the shortest axis of the ellipsoid, turned to the camera.
 * q = rotations[i] = (w, x, y, z), qh = q / |q|, R(qh) the rotation the rasterizer builds; k = the index of the smallest of
 * scales[i] (the lowest index on a tie; any monotone map of the scales gives the same k: stored log-scales may be passed);
 * n0 = column k of R; normals[i] = n0 when n0 . (campos - means3D[i]) >= 0, else -n0.  |q| = 0: normals[i] = 0.
 * |q| is sqrt of the fp32 sum of squares: a quaternion with a NaN or infinite component, or one whose sum of squares
 * overflows (|q| above about 1e19) or underflows to 0 (|q| below about 1e-23), counts as |q| = 0: zeros both ways; between
 * 1e-23 and 1e-19 the squares are subnormal and the normal loses precision.  Stored quaternions are of order 1.
 * Backward: dL_drotations through R and the normalisation, k and the sign constants; |q| = 0: 0.  scales, means3D and
 * campos receive nothing.  One thread per Gaussian, one launch each way.
 * Limits (HS_EINVAL, before any HIP call): args non-null, 0 <= P < 2^30; P > 0: rotations and dL_drotations non-null and
 * 16-byte aligned, scales, means3D, campos (3 floats IN DEVICE MEMORY), normals / dL_dnormals non-null and 4-byte aligned.
 * P = 0 is a valid call that launches nothing and looks at no pointer. */
typedef struct hs_gaussian_normals_args {
    int64_t P;
    const float* rotations;       /* [P, 4] */
    const float* scales;          /* [P, 3] */
    const float* means3D;         /* [P, 3] */
    const float* campos;          /* [3], device memory */
    float* normals;               /* [P, 3] written by the forward */
    const float* dL_dnormals;     /* [P, 3] (backward) */
    float* dL_drotations;         /* [P, 4] written by the backward */
} hs_gaussian_normals_args;

HS_API int hs_gaussian_normals(const hs_gaussian_normals_args* args, void* hip_stream);
HS_API int hs_gaussian_normals_backward(const hs_gaussian_normals_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) TSDF fusion of rendered depth maps and mesh extraction (tsdf.hip): what the
 * surface regularisers above are for -- depth from all training views fused into a truncated signed distance volume, and a
 * triangle mesh extracted from it.  No gradients.
 *
 * The volume.  tsdf, weight: [nz, ny, nx] fp32; color: [3, nz, ny, nx] fp32 planar or NULL.  Sample (i, j, k) sits at
 * origin + voxel_size (i, j, k) and has the linear index q = (k ny + j) nx + i.  An empty volume holds tsdf = 1, weight = 0,
 * color = 0; the caller fills it.
 *
 * hs_tsdf_integrate: ONE launch; every sample walks the frames f = 0 .. F-1 in order, so that two calls over frames 0 .. a
 * and a .. F leave the bits of one call over 0 .. F.  invdepth, alpha: [F, H, W] (what out_invdepth and the alpha output
 * hold; alpha NULL: 1); frame_color: [F, 3, H, W]; viewmatrices: [F, 4, 4] IN DEVICE MEMORY, world to camera in the
 * rasterizer's transposed convention (hs_fwd_args.viewmatrices).  The principal point is the centre of the frame.  Per frame:
 *   (xc, yc, zc) = p V (xc = p.x V[0][0] + p.y V[1][0] + p.z V[2][0] + V[3][0], ...); skipped unless zc > 0;
 *   u = fx xc / zc + W / 2, v = fy yc / zc + H / 2; skipped unless 0 <= u < W and 0 <= v < H (a NaN skips); the pixel is
 *   (floor u, floor v) -- the nearest pixel centre;
 *   the sample d = invdepth, a = alpha of that pixel is VALID when both are finite and > 0 (hs_normal_consistency's rule) and
 *   a >= min_alpha; skipped unless valid; depth = a / d; skipped unless depth <= max_depth (infinity: no limit);
 *   sdf = depth - zc; skipped when sdf < -trunc; t = min(1, sdf / trunc);
 *   tsdf = (tsdf w + t) / (w + 1), every colour channel the same with the frame's colour at that pixel, then w = w + 1.
 * The fp32 operation order is stated at the top of tsdf.hip and restated by tests/tsdf_reference.py.  A workgroup skips a frame
 * that its whole brick of samples misses; the test is exact (tsdf.hip), the result the same bits.  Traffic: one read and one
 * write of tsdf and weight (and color): 16 B per sample, 40 B with colour, whatever F, plus the pixels the volume projects to.
 *
 * hs_tsdf_mesh_plan, hs_tsdf_mesh_emit: marching tetrahedra on the lattice.  A sample is OBSERVED when weight >= min_weight and
 * INSIDE when tsdf < 0 (exactly 0 is outside).  Every cell is cut into the six tetrahedra 000 -> e_a -> e_a + e_b -> 111, one
 * per permutation (a, b, c) of the axes, in lexicographic order.  Their edges are the translates of the seven directions 100,
 * 010, 001, 110, 101, 011, 111 (edge numbers 0 .. 6, x first), each owned by its lower end.  An owned edge carries a VERTEX
 * when both ends are observed and exactly one is inside, at pa + (a / (a - b)) (pb - pa) with a, pa at the owner and b, pb at
 * the other end; colours interpolate the same way.  The formula depends on the edge alone: the mesh is watertight.  A
 * tetrahedron emits 0, 1 or 2 TRIANGLES by the signs of its corners, only when all four are observed, wound so that the normal
 * points to the outside (free space).  Vertices are ordered by (q, edge number), triangles by (q, tetrahedron, position in the
 * case table of tsdf.hip).  Zero-area triangles (a value of exactly 0) stay; a vertex at the rim of the observed region may
 * be referenced by no triangle and stays too.
 *   plan: three launches (count, scan, vertex bases); writes the workspace and totals = {V, T} as two int64 IN DEVICE MEMORY.
 *         The workspace may hold anything before.
 *   emit: one launch; n_vertices = V and n_faces = T as read from totals by the caller (the one host read of the feature);
 *         writes vertices [V, 3] fp32, faces [T, 3] int32 and, for a volume with colour, colors [V, 3] fp32 -- every element.
 *         Between plan and emit the volume, min_weight and the workspace must not change.  V = T = 0: no launch.
 * Limits (HS_EINVAL, reported before any HIP call): args non-null; nx, ny, nz >= 2, nx ny nz <= 2^30; origin finite;
 * voxel_size finite and > 0; tsdf, weight non-null; every pointer given 4-byte aligned (workspace 16, totals 8).
 * integrate: F >= 1, 1 <= H, W <= 65536, 3 F H W < 2^31; fx, fy, trunc finite and > 0; min_alpha not a NaN; max_depth > 0; invdepth and
 * viewmatrices non-null; frame_color given exactly when color is.  mesh: min_weight not a NaN; workspace non-null; plan:
 * totals non-null; emit: 0 <= n_vertices, n_faces < 2^31, vertices / faces non-null when their count is not 0, colors given
 * exactly when color is.  The caller owns every byte, nothing is allocated, cleared or copied, the work is enqueued on the
 * caller's stream and nothing synchronises. */
typedef struct hs_tsdf_args {
    int32_t nx, ny, nz;           /* the volume */
    int32_t F, H, W;              /* integrate: the frames */
    float origin[3];              /* the position of sample (0, 0, 0) */
    float voxel_size;
    float trunc;                  /* integrate */
    float fx, fy;                 /* integrate */
    float min_alpha, max_depth;   /* integrate */
    float min_weight;             /* mesh */
    float* tsdf;                  /* [nz, ny, nx]: read and written by integrate, read by the mesh calls */
    float* weight;                /* [nz, ny, nx]: likewise */
    float* color;                 /* [3, nz, ny, nx] likewise, or NULL: a volume without colour */
    const float* invdepth;        /* [F, H, W] */
    const float* alpha;           /* [F, H, W], or NULL: 1 */
    const float* frame_color;     /* [F, 3, H, W]; given exactly when color is */
    const float* viewmatrices;    /* [F, 4, 4], device memory */
    void* workspace;              /* mesh: hs_tsdf_mesh_workspace_bytes(nx, ny, nz) bytes, written by plan, read by emit */
    int64_t* totals;              /* plan: {V, T} written, device memory */
    int64_t n_vertices, n_faces;  /* emit: V and T of the plan */
    float* vertices;              /* emit: [V, 3] written */
    int32_t* faces;               /* emit: [T, 3] written */
    float* colors;                /* emit: [V, 3] written; given exactly when color is */
} hs_tsdf_args;

HS_API int hs_tsdf_integrate(const hs_tsdf_args* args, void* hip_stream);
/* 5 bytes per sample and 16 per 256 samples, rounded to 16.  -1 (HS_EINVAL) outside the limits above.  No HIP call. */
HS_API int64_t hs_tsdf_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
HS_API int hs_tsdf_mesh_plan(const hs_tsdf_args* args, void* hip_stream);
HS_API int hs_tsdf_mesh_emit(const hs_tsdf_args* args, void* hip_stream);

/* (detected by name; HS_VERSION unchanged) Mesh clean-up by connected components (mesh.hip): what ends every published
 * surface pipeline -- cluster the triangles, keep the large clusters, drop the vertices nothing references.  The mesh
 * hs_tsdf_mesh_emit writes is raw: every floater of the cloud is a closed blob of its own next to the surface.  Integers and
 * copies only: every result is exact, and the same bits on every run.
 *
 * The mesh.  vertices [V, 3] fp32, faces [T, 3] int32, colors [V, 3] fp32 or NULL; V = n_vertices, T = n_faces.
 *   A face is VALID when its three indices are in [0, V).  An invalid face belongs to nothing, is never kept, and is counted.
 *   Two valid faces are CONNECTED when they share a vertex INDEX (equal positions connect nothing: nothing is welded); a
 *   COMPONENT is a class of the transitive closure, its LABEL the smallest vertex index its faces reference, its SIZE the
 *   number of valid faces in it, degenerate ones included (the slivers around a sample of exactly 0 are what stitches the
 *   marching-tetrahedra mesh together).
 *   A face is DEGENERATE when two of its indices are equal or two of its corners compare equal in all three coordinates with
 *   fp32 == (-0 = +0, a NaN equals nothing).  Collinear corners that are distinct are not looked for.
 *   SELECTION.  The components ordered by (size descending, label ascending): keep_largest = n > 0 keeps the first
 *   min(n, components), min_faces = m keeps those of size >= m, both given: a component must pass both.  0 = no limit.
 *   OUTPUT.  The kept faces = the faces of kept components, minus the degenerate ones when remove_degenerate = 1, in input
 *   order; the kept vertices = those a kept face references, in input order; face indices remapped, colours gathered with the
 *   vertices, floats copied bit for bit.
 *
 * hs_mesh_components: label [T] and size [T] int32 of every face's component (-1 and 0 for an invalid face).  Five launches
 *   (init, hook, flatten, sizes, write), no host read.  T = 0: no launch.
 * hs_mesh_clean_plan: the components as above; with keep_largest > 0 an exact select of the n-th largest (size, ~label) over
 *   the components in sixteen launches; then flags, two exclusive scans and totals = {V', T', components of the input, invalid
 *   faces of the input} as four int64 IN DEVICE MEMORY.  The number of launches depends on the arguments only; nothing is read
 *   on the host.  The workspace may hold anything before.  vertices may be NULL when remove_degenerate = 0.
 * hs_mesh_clean_emit: n_vertices_out = V' and n_faces_out = T' as read from totals by the caller (the one host read of the
 *   feature); writes vertices_out [V', 3], faces_out [T', 3] and, when given, colors_out [V', 3] (exactly when colors is),
 *   vertex_index [V'] and face_index [T'] int32 (the input index of every output element) -- every element.  Between plan and
 *   emit the mesh and the workspace must not change.  V' = T' = 0: no launch.
 * The union-find is lock-free: no wave ever waits for another (mesh.hip argues it); integer atomics only.
 * Traffic of the plan, in bytes: 12 T (faces) x 4 passes + 36 T gathered corners when remove_degenerate + about 40 V + 12 T of
 *   workspace; + 8 V per select pass.  Emit: 24 T + 4 T gathered + 28 V (+ 24 V' colours, + 4 V' + 4 T' indices).
 * Limits (HS_EINVAL, reported before any HIP call): args non-null; 0 <= n_vertices, n_faces < 2^31; faces non-null when
 * n_faces > 0; workspace non-null, 16-byte aligned; every other pointer given 4-byte aligned (totals 8).  components: label,
 * size non-null when n_faces > 0.  plan: min_faces, keep_largest >= 0; remove_degenerate 0 or 1, and then vertices non-null
 * when both counts are not 0; totals non-null.  emit: 0 <= n_vertices_out <= n_vertices, 0 <= n_faces_out <= n_faces;
 * vertices, vertices_out non-null when n_vertices_out > 0, faces_out when n_faces_out > 0; colors_out given exactly when colors
 * is.  The caller owns every byte, nothing is allocated, cleared or copied, the work is enqueued on the caller's stream and
 * nothing synchronises. */
typedef struct hs_mesh_args {
    int64_t n_vertices, n_faces;  /* V, T of the input */
    int64_t min_faces;            /* plan: keep components of at least this many faces; 0: all */
    int64_t keep_largest;         /* plan: keep the first n components by (size descending, label ascending); 0: all */
    int32_t remove_degenerate;    /* plan: 1 = degenerate faces are not kept */
    int32_t reserved;
    const float* vertices;        /* [V, 3]: plan (the degenerate test), emit */
    const int32_t* faces;         /* [T, 3] */
    const float* colors;          /* [V, 3] or NULL: emit */
    void* workspace;              /* hs_mesh_workspace_bytes(V, T) bytes: written by components and plan, read by emit */
    int32_t* label;               /* components: [T] written */
    int32_t* size;                /* components: [T] written */
    int64_t* totals;              /* plan: {V', T', components, invalid faces} written, device memory */
    int64_t n_vertices_out, n_faces_out;   /* emit: V' and T' of the plan */
    float* vertices_out;          /* emit: [V', 3] written */
    int32_t* faces_out;           /* emit: [T', 3] written */
    float* colors_out;            /* emit: [V', 3] written; given exactly when colors is */
    int32_t* vertex_index;        /* emit: [V'] written, or NULL */
    int32_t* face_index;          /* emit: [T'] written, or NULL */
} hs_mesh_args;

/* 12 bytes per vertex (parent / label, size, flag / new index) and 4 per face (flag / new index), 8 per 256 vertices and 8 per
 * 256 faces (the scans' sums), each of the six parts rounded up to 16, + 8192 (the select's histograms) + 64 (its state):
 *   3 r(4 V) + r(4 T) + r(8 ceil(V / 256)) + r(8 ceil(T / 256)) + 8256,   r(x) = 16 ceil(x / 16).
 * -1 (HS_EINVAL) outside the limits above.  No HIP call. */
HS_API int64_t hs_mesh_workspace_bytes(int64_t n_vertices, int64_t n_faces);
HS_API int hs_mesh_components(const hs_mesh_args* args, void* hip_stream);
HS_API int hs_mesh_clean_plan(const hs_mesh_args* args, void* hip_stream);
HS_API int hs_mesh_clean_emit(const hs_mesh_args* args, void* hip_stream);

/* Bench/test only: stable LSD radix sort of (u64 key, u32 value) pairs on bits [0, nbits), n < 2^30, using the
 * same pass kernel as HS_STAGE_BIN.  tmp must hold hs_sort_tmp_bytes(n).  Result in keys_out/vals_out.  The u32 at
 * byte 4 of tmp reads 2 afterwards if a pass gave up waiting (results invalid), else 0.  (The tests provoke exactly
 * that with HS_FAULT_INJECT=sort_ticket, which only libhdrsplat_test.so -- built with -DHS_TESTING -- reads.) */
HS_API int64_t hs_sort_tmp_bytes(int64_t n);
HS_API int hs_sort_pairs(const uint64_t* keys_in, const uint32_t* vals_in, uint64_t* keys_out, uint32_t* vals_out,
                  int64_t n, int32_t nbits, void* tmp, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HDRSPLAT_H */
