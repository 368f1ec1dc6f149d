// Depth-distortion loss of a finished forward (hs_distortion, hs_distortion_backward; include/hdrsplat.h): the regulariser of
// Mip-NeRF 360 on the blending weights of a ray, per pixel L_p = sum_i sum_j w_i w_j |s_i - s_j| with w = alpha * T and
// s = 1 / z, the inverse view-space depth of the entry (what out_invdepth composites).  Quadratic in the weights and built
// from prefix sums along the ray: it exists only inside the compositing loop, so it is a replay of the forward under the
// forward's own decisions (pair_act, n_contrib), as features.hip, and its backward a back-to-front replay, as featgeo.hip.
//
// Both kernels carry s RELATIVE to a workgroup-uniform s0 (1 / z of the tile's first entry; the loss is invariant under
// s -> s - s0): the sums D - s A then cancel numbers of the size of the tile's depth SPREAD, not of its depth.  `moment`
// goes to memory as sum w s.
//
//   distort_fwd_kernel         one 128-thread workgroup per (pose, tile), the render forward's pixel mapping and XCD strip
//                              map, two pixels per lane, features_fwd_kernel's staging plus s - s0 of each entry.  Per
//                              pixel T, A = sum w, D = sum w (s - s0) and the running loss in packed fp32:
//                                  loss += w_i (D_{i-1} - (s_i - s0) A_{i-1}),  D += w_i (s_i - s0),  A += w_i
//                              An entry that is not composited at a pixel is SELECTED out.  The epilogue stores
//                              distortion = 2 loss and moment = D + s0 A for every in-image pixel, whatever the list held
//                              (an overflowed frame: the walk is empty, zeros).
//   distort_bwd_replay_kernel  featgeo_replay_kernel's structure: batches of 64 deepest first, per-block taker lists, one
//                              LDS plane per block.  Per pixel gamma, T (from final_T), q, the suffix sums A+ and D+, and
//                              the two totals A_n = 1 - final_T and M0 = moment - s0 A_n.  With s' = s_i - s0:
//                                  v_i / 2 = (M0 - s' A_n) + 2 (s' A+ - D+)        (the prefix part is the total minus the
//                                            suffix part; the entry's own w (s_i - s_i) is zero and drops out)
//                                  d_i = gamma v_i,  dL/dalpha_i = T_i (d_i - q_i),  q_{i-1} = q_i + alpha_i (d_i - q_i)
//                                  dL/ds_i = 2 gamma w_i (A+ - A_{i-1}) = 2 gamma w_i (2 A+ + w_i - A_n)
//                              Seven sums per entry and block by the fixed DPP tree (featgeo's six and dL/ds); the thread
//                              that staged the entry adds the planes in plane order and WRITES the pair's record
//                              (render_bwd_kernel's format: colour slots zero, the inverse-depth slot filled) and flag at
//                              the pair's duplicateWithKeys slot in the call's OWN workspace.  One pass: no read-modify-write.
//   distort_segsum_kernel      pair_segsum_body (hs_common.h) over the call's records and flags into the call's rows.
//   preprocess_bwd_kernel      launch_preprocess_bwd(project only): the rows to dL_dmeans3D (the inverse-depth slot reaches
//                              the mean through z), dL_dopacities, dL_dscales, dL_drotations, every element written.
// No atomics anywhere: the same inputs give the same bits.  The forward's three workspaces are only read.
//
// Compiled like render.hip (FMA contraction on: the Makefile's FAST_TUS); the forward's decisions, the staging of an entry,
// both walks, the six geometry sums and the pair record's arithmetic are hs_replay.h's.
#include "hs_replay.h"

namespace hs {
namespace {

constexpr int kDThreads = 128;       // threads per workgroup: two waves, one per half tile
constexpr int kDFwdBatch = 128;      // staged entries per batch of the forward = threads per workgroup
constexpr int kDBwdBatch = 64;       // ... of the backward (featgeo.hip: one ballot per list)
constexpr int kDistSums = 7;         // reduced values per (tile, entry): featgeo's six and dL/ds

// 1 / z of the tile's first entry (0 for an empty list): uniform over the workgroup
__device__ __forceinline__ float tile_s0(const ReplayFrame& p, const TileCtx& tc) {
    if (tc.n <= 0) return 0.f;
    return 1.f / reinterpret_cast<const float*>(p.rec + kRecF4 * (int64_t)entry_id(p, tc, 0) + 2)[1];
}

struct DistFwd : ReplayFrame {
    float* out_distortion;            // [n_poses, H, W]
    float* out_moment;                // [n_poses, H, W]
};

struct DistBwd : ReplayFrame {
    const float* moment;              // [n_poses, H, W], as the forward wrote it
    const float* dL_ddistortion;      // [n_poses, H, W]
    const float* final_T;
    float4* pair_rec;                 // the call's records, kPairF4 float4 per pair slot
    uint8_t* pair_flags;              // the call's flags, one per pair slot
};

__global__ void __launch_bounds__(kDThreads) distort_fwd_kernel(DistFwd p) {
    constexpr int KB = kDFwdBatch;
    __shared__ float4 s_a[KB];            // {x, y, A2, B2}
    __shared__ float4 s_b[KB];            // {C2, opacity, s - s0, -}
    __shared__ uint8_t s_actb[KB];        // activity byte of each staged entry (bit 2g + w)
    __shared__ uint32_t s_max[2];

    const TileCtx tc = tile_context(p);
    const int64_t HW = (int64_t)p.H * p.W;

    uint32_t last0 = 0, last1 = 0;        // per pixel: the number of its last contributor (the forward stopped it there)
    if (tc.in0) last0 = p.n_contrib[(int64_t)tc.pose * HW + (int64_t)tc.py0 * p.W + tc.px];
    if (tc.in1) last1 = p.n_contrib[(int64_t)tc.pose * HW + (int64_t)tc.py1 * p.W + tc.px];
    post_wave_depth(s_max, tc, last0, last1);
    __syncthreads();
    // an overflowed frame was rendered empty: nothing is walked, the epilogue stores zeros
    const int n_proc = p.counters->overflow ? 0 : walk_bound(s_max, tc);
    const float s0 = n_proc > 0 ? tile_s0(p, tc) : 0.f;

    f2 T = {1.f, 1.f}, A = {0.f, 0.f}, D = {0.f, 0.f}, loss = {0.f, 0.f};

    for (int base = 0; base < n_proc; base += KB) {
        const int cnt = min(KB, n_proc - base);
        __syncthreads();   // the previous batch has been walked
        uint32_t act = 0;
        if ((int)threadIdx.x < cnt) {
            const Staged e(p, tc, base);
            act = e.act;
            s_a[threadIdx.x] = e.ra;
            s_b[threadIdx.x] = make_float4(e.rb.x, e.rb.y, 1.f / e.rc.y - s0, 0.f);
        }
        s_actb[threadIdx.x] = (uint8_t)act;
        __syncthreads();
        walk_front<KB>(tc, s_a, s_b, s_actb, base, last0, last1, T, [&](int j, bool, bool act0, bool act1, f2 w) {
            const f2 sr = splat(s_b[j].z);
            const f2 term = D - sr * A;                     // D_{i-1} - (s_i - s0) A_{i-1}
            const f2 nloss = w * term + loss;               // (contracted: packed fmas)
            const f2 nD = w * sr + D;
            const f2 nA = A + w;
            loss = f2{act0 ? nloss.x : loss.x, act1 ? nloss.y : loss.y};
            D = f2{act0 ? nD.x : D.x, act1 ? nD.y : D.y};
            A = f2{act0 ? nA.x : A.x, act1 ? nA.y : A.y};
        });
    }
    // every in-image pixel of both planes is stored, whatever the list held
    const f2 dist = loss + loss;
    const f2 mom = splat(s0) * A + D;
    if (tc.in0) {
        const int64_t o = (int64_t)tc.pose * HW + (int64_t)tc.py0 * p.W + tc.px;
        p.out_distortion[o] = dist.x; p.out_moment[o] = mom.x;
    }
    if (tc.in1) {
        const int64_t o = (int64_t)tc.pose * HW + (int64_t)tc.py1 * p.W + tc.px;
        p.out_distortion[o] = dist.y; p.out_moment[o] = mom.y;
    }
}

// an empty cloud has no state to replay: every element of both planes is +0
__global__ void __launch_bounds__(256) distort_zero_kernel(float* a, float* b, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { a[i] = 0.f; b[i] = 0.f; }
}

struct alignas(16) DistPart { float v[8]; };   // (seven used)

__global__ void __launch_bounds__(kDThreads) distort_bwd_replay_kernel(DistBwd p) {
    constexpr int KB = kDBwdBatch;
    // (record KB of the staging arrays: the back-to-front walk's sentinel)
    __shared__ float4 s_a[KB + 1];              // {x, y, A2, B2}
    __shared__ float4 s_b[KB + 1];              // {C2, opacity, radius (int bits), slot start (uint bits)}
    __shared__ float s_s[KB + 1];               // s - s0
    __shared__ DistPart s_part[KB + 1][4];      // plane 2g + w: the totals of lane group g of wave w, stored by that group alone
    __shared__ uint8_t s_actb[kDThreads];       // activity byte of each staged entry (bit 2g + w)
    __shared__ uint16_t s_list[2][2][KB + 8];   // [wave][lane group]: the group's takers among the staged entries, back to front
    __shared__ uint32_t s_max[2];

    if (p.counters->overflow) return;     // (ReplayFrame: the segmented sum reads no record and no flag of an overflowed frame)
    const TileCtx tc = tile_context(p);
    const int lane = tc.lane, plane = act_plane(tc.grp, tc.wave);
    const float s0 = tile_s0(p, tc);

    // per pixel: the forward's final transmittance and last contributor, twice the upstream gradient, the totals
    const int64_t HW = (int64_t)p.H * p.W;
    uint32_t last0 = 0, last1 = 0;
    f2 T = {0.f, 0.f}, q = {0.f, 0.f}, g2 = {0.f, 0.f}, An = {0.f, 0.f}, M0 = {0.f, 0.f};
    if (tc.in0) {
        const int64_t pix = (int64_t)tc.pose * HW + (int64_t)tc.py0 * p.W + tc.px;
        last0 = p.n_contrib[pix];
        T.x = p.final_T[pix];
        g2.x = 2.f * p.dL_ddistortion[pix];
        An.x = 1.f - T.x;
        M0.x = p.moment[pix] - s0 * An.x;
    }
    if (tc.in1) {
        const int64_t pix = (int64_t)tc.pose * HW + (int64_t)tc.py1 * p.W + tc.px;
        last1 = p.n_contrib[pix];
        T.y = p.final_T[pix];
        g2.y = 2.f * p.dL_ddistortion[pix];
        An.y = 1.f - T.y;
        M0.y = p.moment[pix] - s0 * An.y;
    }
    f2 Ap = {0.f, 0.f}, Dp = {0.f, 0.f};     // the sums over the contributors behind the current entry
    post_wave_depth(s_max, tc, last0, last1);
    if (threadIdx.x == 0) {
        s_a[KB] = make_float4(0.f, 0.f, 0.f, 0.f); s_b[KB] = make_float4(0.f, 0.f, 0.f, 0.f); s_s[KB] = 0.f;
    }
    __syncthreads();
    const int n_proc = walk_bound(s_max, tc);

    const int nb = (n_proc + KB - 1) / KB;
    for (int bi = nb - 1; bi >= 0; --bi) {
        const int base = bi * KB;
        const int cnt = min(KB, n_proc - base);
        __syncthreads();   // the previous batch's write-out has read its records
        uint32_t act = 0;
        if ((int)threadIdx.x < cnt) {
            const Staged e(p, tc, base);
            act = e.act;
            s_a[threadIdx.x] = e.ra;
            s_b[threadIdx.x] = make_float4(e.rb.x, e.rb.y, e.rc.z, e.rc.w);
            s_s[threadIdx.x] = 1.f / e.rc.y - s0;
        }
        s_actb[threadIdx.x] = (uint8_t)act;
        __syncthreads();
        // back to front over the entries this wave's blocks took (hs_replay.h: the back-to-front walk)
        const int trips = take_lists<KB>(tc, s_actb, s_list);
        const uint16_t* const my_list = s_list[tc.wave][tc.grp];
#pragma unroll 1
        for (int ti = 0; ti < trips; ++ti) {
            const BackEntry e = back_entry(tc, s_a, s_b, (int)my_list[ti], base, last0, last1);
            const f2 sr = splat(s_s[e.j]);
            // ---- the backward's step (render.hip, step_bwd_pair): inactive pixels keep their state exactly ----
            const BackStep st = e.step(T);
            T = st.T;
            const f2 w = st.ae * T;                              // (0 where the pixel does not composite the entry)
            // ---- d_i = gamma v_i: the total about s_i, and twice the part behind the entry ----
            const f2 suf = sr * Ap - Dp;                         // sum over j > i of w_j (s_i - s_j)
            const f2 tot = M0 - sr * An;                         // sum over all j of w_j (s_j - s_i)
            const f2 cd = g2 * (tot + (suf + suf));
            // dL/ds_i = 2 gamma w_i (A+ - A_{i-1}),  A_{i-1} = A_n - A+ - w_i
            const f2 ds = (g2 * w) * ((Ap + Ap) + (w - An));
            Ap += w;
            Dp += w * sr;
            const f2 diff = cd - q;
            const f2 gd = e.G * (diff * T);
            q += st.ae * diff;
            const f2 dop = {e.act0 ? gd.x : 0.f, e.act1 ? gd.y : 0.f};  // select AFTER the product (G may be inf at a skipped pixel)
            const f2 sw = splat(e.b.y) * dop;
            DistPart tot7;
            geo_sums(tot7, e, sw, dop);
            tot7.v[6] = group_sum(ds.x + ds.y);                  // (w = 0 where not composited: ds is 0 there)
            tot7.v[7] = 0.f;
            // one lane per group, a plain LDS store into the group's own plane of its own entry (the sentinel's is scratch)
            if ((lane & 31) == 31) s_part[e.j][plane] = tot7;
        }
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const float4 a = s_a[threadIdx.x], b = s_b[threadIdx.x];
            const int64_t slot = pair_slot(p, a.x, a.y, __float_as_int(b.z), __float_as_uint(b.w), tc.tx, tc.ty);
            if (slot >= 0 && slot < p.capacity) {
                p.pair_flags[slot] = act != 0 ? 1 : 0;
                if (act != 0) {
                    const GeoAcc<kDistSums> sums = planes_combined<GeoAcc<kDistSums>>(act, s_part[threadIdx.x]);
                    float4* o = p.pair_rec + kPairF4 * slot;
                    write_geo_record(o, geo_record(p, a, b.x, sums.v));
                    write_geo_record_tail(o, sums.v[6]);   // (the inverse depth's slot is filled)
                }
            }
        }
    }
    // the entries behind the tile's deepest contributor: nobody took them
    write_untaken(p, tc, n_proc, kDThreads, p.pair_flags, (uint8_t)0);
}

__global__ void __launch_bounds__(256) distort_segsum_kernel(SegsumArgs sg) {
    pair_segsum_body(sg, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// the call's workspace: pair records [capacity] | per-instance rows [P * n_poses] (both as hs_layout's pair_grads /
// inst_grads: kPairFloats / kInstFloats fp32 each) | pair flags [capacity], each 256-byte aligned
struct DistWs { int64_t rec, rows, flags, bytes; };
static inline DistWs dist_workspace(const hs_dims& d) {
    DistWs w;
    w.rec = 0;
    w.rows = align_up(d.capacity * kPairFloats * 4, 256);
    w.flags = w.rows + align_up((int64_t)d.P * d.n_poses * kInstFloats * 4, 256);
    w.bytes = w.flags + align_up(d.capacity, 256);
    if (w.bytes <= 0) w.bytes = 256;
    return w;
}

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

HS_API int64_t hs_distortion_workspace_bytes(const hs_dims* dims) {
    const char* fn = "hs_distortion_workspace_bytes";
    hs_sizes sz;
    if (check_args(fn, dims) || hs_plan(dims, &sz, nullptr) != HS_OK) return HS_EINVAL;
    return dist_workspace(*dims).bytes;
}

HS_API int hs_distortion(const hs_distortion_args* a, void* hip_stream) {
    const char* fn = "hs_distortion";
    if (check_args(fn, a)) return HS_EINVAL;
    hs_sizes sz; hs_layout L;
    if (hs_plan(&a->dims, &sz, &L) != HS_OK) return HS_EINVAL;   // (the text names what hs_plan refused)
    const hs_dims& d = a->dims;
    const Field o[] = {{a->out_distortion, "out_distortion", 4}, {a->out_moment, "out_moment", 4}};
    int rc = check_fields(fn, o, 2);
    if (rc != HS_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    if (d.P == 0) {   // no state: both planes are all zeros
        const int64_t n = (int64_t)d.n_poses * d.H * d.W;
        distort_zero_kernel<<<ceil_div(n, 256), 256, 0, s>>>(a->out_distortion, a->out_moment, n);
        HS_LAUNCH_CHECK();
        return HS_OK;
    }
    const Field f[] = {{a->geom, "geom", 256}, {a->binning, "binning", 256}, {a->image, "image", 256}};
    if ((rc = check_fields(fn, f, 3)) != HS_OK) return rc;

    DistFwd p;
    static_cast<ReplayFrame&>(p) = replay_frame(d, L, a->geom, a->binning, a->image);
    p.out_distortion = a->out_distortion; p.out_moment = a->out_moment;
    distort_fwd_kernel<<<p.ntiles * d.n_poses, kDThreads, 0, s>>>(p);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

HS_API int hs_distortion_backward(const hs_distortion_bwd_args* a, void* hip_stream) {
    const char* fn = "hs_distortion_backward";
    if (check_args(fn, a)) return HS_EINVAL;
    hs_sizes sz; hs_layout L;
    if (hs_plan(&a->dims, &sz, &L) != HS_OK) return HS_EINVAL;   // (the text names what hs_plan refused)
    const hs_dims& d = a->dims;
    if (d.P == 0) return HS_OK;   // (the gradients have no elements: no pointer is looked at, nothing is launched)
    const Field cov[] = {{a->scales, "scales", 4}, {a->rotations, "rotations", 16}};
    int rc = check_fields(fn, cov, 2, " (the forward's scales and rotations: a cov3D_precomp forward is not supported)");
    if (rc != HS_OK) return rc;
    const Field f[] = {{a->geom, "geom", 256}, {a->binning, "binning", 256}, {a->image, "image", 256}, {a->ws, "ws", 256},
                       {a->viewmatrices, "viewmatrices", 4}, {a->projmatrices, "projmatrices", 4}, {a->camposes, "camposes", 4},
                       {a->means3D, "means3D", 4}, {a->opacities, "opacities", 4},
                       {a->moment, "moment", 4}, {a->dL_ddistortion, "dL_ddistortion", 4},
                       {a->dL_dmeans3D, "dL_dmeans3D", 4}, {a->dL_dopacities, "dL_dopacities", 4},
                       {a->dL_dscales, "dL_dscales", 4}, {a->dL_drotations, "dL_drotations", 16}};
    if ((rc = check_fields(fn, f, (int)(sizeof f / sizeof f[0]))) != HS_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const DistWs w = dist_workspace(d);
    char* ws = (char*)a->ws;

    DistBwd p;
    static_cast<ReplayFrame&>(p) = replay_frame(d, L, a->geom, a->binning, a->image);
    p.moment = a->moment; p.dL_ddistortion = a->dL_ddistortion;
    p.final_T = (const float*)((const char*)a->image + L.final_T);
    p.pair_rec = (float4*)(ws + w.rec); p.pair_flags = (uint8_t*)(ws + w.flags);
    distort_bwd_replay_kernel<<<p.ntiles * d.n_poses, kDThreads, 0, s>>>(p);
    HS_LAUNCH_CHECK();

    const int64_t I = p.I;
    const char* bin = (const char*)a->binning;
    SegsumArgs sg;
    sg.I = I; sg.inst_sorted = (const uint32_t*)(bin + L.inst_sorted); sg.offs_sorted = (const uint32_t*)(bin + L.offs_sorted);
    sg.pair_grads = p.pair_rec; sg.pair_flags = p.pair_flags; sg.inst_grads = (float4*)(ws + w.rows); sg.counters = p.counters;
    sg.radii_inst = nullptr; sg.clamped = nullptr; sg.view_colors = nullptr; sg.rec = nullptr; sg.act = 0;
    distort_segsum_kernel<<<ceil_div(4 * I, 256), 256, 0, s>>>(sg);
    HS_LAUNCH_CHECK();

    // the projection of hs_backward (HS_BWD_PROJECT) from the call's rows, as featgeo.hip hands it over: the layout places
    // inst_grads in the call's workspace, the colours are declared precomputed (their slots are zero; the pointer only says
    // so), M = 0 sizes its LDS.  The inverse-depth slot of a row reaches the mean through z there.
    hs_layout G = L;
    G.inst_grads = w.rows;
    hs_bwd_args b = {};
    b.dims = d; b.dims.M = 0;
    b.tanfovx = a->tanfovx; b.tanfovy = a->tanfovy; b.scale_modifier = a->scale_modifier;
    b.flags = a->flags & HS_FLAG_ANTIALIAS;
    b.viewmatrices = a->viewmatrices; b.projmatrices = a->projmatrices; b.camposes = a->camposes;
    b.means3D = a->means3D; b.opacities = a->opacities; b.scales = a->scales; b.rotations = a->rotations;
    b.colors_precomp = a->means3D;
    b.geom = a->geom; b.binning = a->binning; b.image = a->image; b.bwd = a->ws;
    b.dL_dmeans3D = a->dL_dmeans3D; b.dL_dopacities = a->dL_dopacities; b.dL_dscales = a->dL_dscales;
    b.dL_drotations = a->dL_drotations;
    return launch_preprocess_bwd(b, G, s, false, true, nullptr);
}

}  // extern "C"
