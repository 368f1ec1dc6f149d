// Gradients to the GEOMETRY through the composited feature channels (hs_composite_features_geometry_backward,
// include/hdrsplat.h): what a loss on hs_composite_features' output asks of the means, covariances and opacities of the
// forward behind it -- render_bwd_kernel for C channels instead of three.  A back-to-front replay of the finished forward,
// as absgrad.hip, with the backward's one-number recurrence: d_i = sum_c features[g_i, c] * dL_dout[k, c, p] takes the place
// of c_i . dL, there is no background, no 1 / N and no CRF (the compositing has none), q starts at 0 behind the deepest
// contributor, dL/dalpha_i = T_i (d_i - q_i), q_{i-1} = q_i + alpha_i (d_i - q_i), T_i = T_{i+1} / (1 - alpha_i) from final_T.
// From dL/dalpha on the terms of the 2-D mean, the conic and the opacity are render_bwd_kernel's, operand for operand.
//
//   featgeo_replay_kernel  one 128-thread workgroup per (pose, tile), the render forward's pixel mapping and XCD strip map.
//                          A launch takes a PASS of K channels (K = 16 while more than eight are left, then the narrowest of
//                          4, 8, 16 that holds the rest): the pass's dL_dout values of the lane's two pixels stay in registers
//                          (2 K of them), the pass's K feature values of each staged entry in LDS beside its record.  Stages
//                          the tile's list 64 entries at a time, deepest batch first; each 8 x 8 block walks its own list of
//                          takers (pair_act) back to front, reduces its six sums {w dx, w dy, w dx^2, w dx dy, w dy^2, G dL/dalpha}
//                          by a fixed DPP tree and STORES them into its own plane of the entry's LDS record; the thread that
//                          staged an entry adds the planes in plane order and owns the pair's record (render_bwd_kernel's
//                          format, kPairFloats, colour and inverse-depth slots zero) at the pair's duplicateWithKeys slot in the
//                          call's OWN workspace.  d is linear in the channels, so the passes' records add: the first pass
//                          WRITES the record and the pair's flag (1: some block took the entry; 0 for every other pair of
//                          the frame, also behind the tile's deepest contributor), every later pass adds its terms to the
//                          record it finds -- ascending pass order, one owner per record, no atomics: the same bits every run.
//   featgeo_segsum_kernel  pair_segsum_body (hs_common.h) over the call's records and flags into the call's per-instance rows.
//   preprocess_bwd_kernel  launch_preprocess_bwd(project only) from those rows: dL_dmeans3D, dL_dopacities, dL_dscales,
//                          dL_drotations, every element written.
// The forward's three workspaces are only read -- the pair flags of hs_backward in the binning workspace are not touched, so
// the rasterizer's own backward may run before or after this call on the same state.  Every word read from the call's
// workspace is one the call wrote.  An overflowed frame: the replay returns at once, the segmented sum writes zero rows.
//
// Compiled like render.hip (FMA contraction on: the Makefile's FAST_TUS); the forward's decisions, the staging of an entry and
// of its feature row, the back-to-front walk, the six geometry sums and the pair record's arithmetic are hs_replay.h's.
#include "hs_replay.h"

// A/B switch of scripts/time_features_geometry.py (make variant TUS=featgeo DEFS=...).  0, what ships: chosen per pass.
#ifndef HS_TUNE_GEO_PASS
#define HS_TUNE_GEO_PASS 0       // channels per pass: 4, 8 or 16 for every pass
#endif

namespace hs {
namespace {

constexpr int kGThreads = 128;       // threads per workgroup: two waves, one per half tile
// staged entries per batch: 64 keeps the workgroup's LDS at 12.7 KB with sixteen channels (96 bytes of plane sums and 64 of
// feature values per entry beside the 32-byte record); absgrad.hip measured 64 against 128 entries as a wash
constexpr int kGBatch = 64;
// channels per pass (K).  A pass costs one walk of the lists (the exp, the rcp, six tree sums per trip) whatever K is, and
// K fmas and K / 4 LDS reads per trip on top.  Measured, the whole call (passes + segmented sum + projection), medians of 20,
// alternated: at 1 M Gaussians / 1080p and C = 16, K = 4 in every pass 2.629 ms, K = 8 1.454 ms, K = 16 0.862 ms (100 k /
// 800 x 800: 0.867 / 0.468 / 0.252 ms); at C = 3, K = 4 0.768 ms, K = 8 0.808 ms (0.259 / 0.254 ms).  The kernel alone: one
// walk with K = 16 0.730 ms, with K = 4 0.670 ms (62 against 86 registers, eight against five waves per SIMD).  K = 32 would
// hold 64 registers of dL_dout and was not built.  (profiles/features_geometry_timing.json)
constexpr int kGeoPass = 16;
constexpr int kGeoForce = HS_TUNE_GEO_PASS;
constexpr int kMaxChannels = 512;
constexpr int kGeoSums = 6;          // reduced values per (tile, entry)
static_assert(kGBatch % 64 == 0 && kGBatch <= kGThreads, "the lists are built from whole ballots, one entry is staged per thread");
static_assert(kGeoForce == 0 || kGeoForce == 4 || kGeoForce == 8 || kGeoForce == 16, "channels per pass");

static inline int geo_pass(int left) { return kGeoForce ? kGeoForce : left > 8 ? kGeoPass : left > 4 ? 8 : 4; }

struct GeoReplay : ReplayFrame {
    int C, c0, P;                     // channels; the pass's first; Gaussians
    bool vec4;                        // C % 4 == 0 and a 16-byte aligned base: feature rows are read as float4
    const float* features;            // [P, C]
    const float* dL_dout;             // [n_poses, C, H, W]
    const float* final_T;
    float4* pair_rec;                 // the call's records, kPairF4 float4 per pair slot
    uint8_t* pair_flags;              // the call's flags, one per pair slot
};

struct alignas(8) GeoPart { float v[kGeoSums]; };

template <int K>
__global__ void __launch_bounds__(kGThreads) featgeo_replay_kernel(GeoReplay p) {
    constexpr int KB = kGBatch;
    // (record KB of the staging arrays: the back-to-front walk's sentinel, features 0)
    __shared__ float4 s_a[KB + 1];              // {x, y, A2, B2}
    __shared__ float4 s_b[KB + 1];              // {C2, opacity, radius (int bits), slot start (uint bits)}
    __shared__ alignas(16) float s_f[KB + 1][K];   // the pass's feature values of each staged entry
    __shared__ GeoPart s_part[KB + 1][4];       // plane 2g + w: the totals of lane group g of wave w, stored by that group alone
    __shared__ uint8_t s_actb[kGThreads];       // activity byte of each staged entry (bit 2g + w)
    __shared__ uint16_t s_list[2][2][KB + 8];   // [wave][lane group]: the group's takers among the staged entries, back to front
    __shared__ uint32_t s_max[2];

    if (p.counters->overflow) return;     // (ReplayFrame: the segmented sum reads no record and no flag of an overflowed frame)
    const TileCtx tc = tile_context(p);
    const int lane = tc.lane, plane = act_plane(tc.grp, tc.wave);
    const bool first = p.c0 == 0;         // the pass that writes the records and the flags

    // per pixel: the forward's final transmittance and last contributor, the pass's channels of the upstream gradient (0 past
    // the last channel and outside the image)
    const int64_t HW = (int64_t)p.H * p.W;
    uint32_t last0 = 0, last1 = 0;
    f2 T = {0.f, 0.f}, q = {0.f, 0.f};
    f2 e[K];
#pragma unroll
    for (int c = 0; c < K; ++c) e[c] = f2{0.f, 0.f};
    const float* dl = p.dL_dout + ((int64_t)tc.pose * p.C + p.c0) * HW;
    if (tc.in0) {
        const int64_t pix = (int64_t)tc.py0 * p.W + tc.px;
        last0 = p.n_contrib[(int64_t)tc.pose * HW + pix];
        T.x = p.final_T[(int64_t)tc.pose * HW + pix];
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (p.c0 + c < p.C) e[c].x = dl[c * HW + pix];
    }
    if (tc.in1) {
        const int64_t pix = (int64_t)tc.py1 * p.W + tc.px;
        last1 = p.n_contrib[(int64_t)tc.pose * HW + pix];
        T.y = p.final_T[(int64_t)tc.pose * HW + pix];
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (p.c0 + c < p.C) e[c].y = dl[c * HW + pix];
    }
    post_wave_depth(s_max, tc, last0, last1);
    if (threadIdx.x == 0) { s_a[KB] = make_float4(0.f, 0.f, 0.f, 0.f); s_b[KB] = make_float4(0.f, 0.f, 0.f, 0.f); }
    if ((int)threadIdx.x < K) s_f[KB][threadIdx.x] = 0.f;
    __syncthreads();
    const int n_proc = walk_bound(s_max, tc);

    const int nb = (n_proc + KB - 1) / KB;
    for (int bi = nb - 1; bi >= 0; --bi) {
        const int base = bi * KB;
        const int cnt = min(KB, n_proc - base);
        __syncthreads();   // the previous batch's write-out has read its records
        uint32_t act = 0;
        if ((int)threadIdx.x < cnt) {
            const Staged s(p, tc, base);
            act = s.act;
            s_a[threadIdx.x] = s.ra;
            s_b[threadIdx.x] = make_float4(s.rb.x, s.rb.y, s.rc.z, s.rc.w);
            stage_feature_row(s_f[threadIdx.x], p.features, p.P, p.C, p.c0, p.vec4, s.id, tc.pose);
        }
        s_actb[threadIdx.x] = (uint8_t)act;
        __syncthreads();
        // back to front over the entries this wave's blocks took (hs_replay.h: the back-to-front walk)
        const int trips = take_lists<KB>(tc, s_actb, s_list);
        const uint16_t* const my_list = s_list[tc.wave][tc.grp];
#pragma unroll 1
        for (int ti = 0; ti < trips; ++ti) {
            const BackEntry en = back_entry(tc, s_a, s_b, (int)my_list[ti], base, last0, last1);
            // ---- d_i of the pass: the entry's K feature values against the pixel pair's K gradients ----
            f2 cd = {0.f, 0.f};
#pragma unroll
            for (int c4 = 0; c4 < K / 4; ++c4) {
                const float4 f = reinterpret_cast<const float4*>(s_f[en.j])[c4];
                cd += splat(f.x) * e[4 * c4 + 0];
                cd += splat(f.y) * e[4 * c4 + 1];
                cd += splat(f.z) * e[4 * c4 + 2];
                cd += splat(f.w) * e[4 * c4 + 3];
            }
            // ---- the backward's step (render.hip, step_bwd_pair): inactive pixels keep their state exactly ----
            const BackStep st = en.step(T);
            T = st.T;
            const f2 diff = cd - q;
            const f2 gd = en.G * (diff * T);
            q += st.ae * diff;
            const f2 dop = {en.act0 ? gd.x : 0.f, en.act1 ? gd.y : 0.f};  // select AFTER the product (G may be inf at a skipped pixel)
            const f2 sw = splat(en.b.y) * dop;
            GeoPart tot;
            geo_sums(tot, en, sw, dop);
            // one lane per group, a plain LDS store into the group's own plane of its own entry (the sentinel's is scratch)
            if ((lane & 31) == 31) s_part[en.j][plane] = tot;
        }
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const float4 a = s_a[threadIdx.x], b = s_b[threadIdx.x];
            const int64_t slot = pair_slot(p, a.x, a.y, __float_as_int(b.z), __float_as_uint(b.w), tc.tx, tc.ty);
            if (slot >= 0 && slot < p.capacity) {
                if (first) p.pair_flags[slot] = act != 0 ? 1 : 0;
                if (act != 0) {
                    const GeoAcc<kGeoSums> sums = planes_combined<GeoAcc<kGeoSums>>(act, s_part[threadIdx.x]);
                    GeoRec r = geo_record(p, a, b.x, sums.v);
                    float4* o = p.pair_rec + kPairF4 * slot;
                    if (!first) {   // this thread's own record of the earlier passes
                        const float4 o0 = o[0];
                        const float2 o1 = reinterpret_cast<const float2*>(o + 1)[0];
                        r.r0 = make_float4(o0.x + r.r0.x, o0.y + r.r0.y, o0.z + r.r0.z, o0.w + r.r0.w);
                        r.r1 = make_float2(o1.x + r.r1.x, o1.y + r.r1.y);
                    }
                    write_geo_record(o, r);
                    if (first) write_geo_record_tail(o, 0.f);
                }
            }
        }
    }
    // the entries behind the tile's deepest contributor: nobody took them
    if (first) write_untaken(p, tc, n_proc, kGThreads, p.pair_flags, (uint8_t)0);
}

__global__ void __launch_bounds__(256) featgeo_segsum_kernel(SegsumArgs sg) {
    pair_segsum_body(sg, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

template <int K>
int replay_pass(const GeoReplay& p, int n_poses, hipStream_t s) {
    featgeo_replay_kernel<K><<<p.ntiles * n_poses, kGThreads, 0, s>>>(p);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

// the call's workspace: pair records [capacity] | per-instance rows [P * n_poses] (both as hs_layout's pair_grads /
// inst_grads: kPairFloats / kInstFloats fp32 each) | pair flags [capacity], each 256-byte aligned
struct GeoWs { int64_t rec, rows, flags, bytes; };
static inline GeoWs geo_workspace(const hs_dims& d) {
    GeoWs w;
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

HS_API int64_t hs_composite_features_geometry_workspace_bytes(const hs_dims* dims) {
    const char* fn = "hs_composite_features_geometry_workspace_bytes";
    hs_sizes sz;
    if (check_args(fn, dims) || hs_plan(dims, &sz, nullptr) != HS_OK) return HS_EINVAL;
    return geo_workspace(*dims).bytes;
}

HS_API int hs_composite_features_geometry_backward(const hs_composite_features_geometry_args* a, void* hip_stream) {
    const char* fn = "hs_composite_features_geometry_backward";
    if (check_args(fn, a)) return HS_EINVAL;
    hs_sizes sz; hs_layout L;
    if (hs_plan(&a->dims, &sz, &L) != HS_OK) return HS_EINVAL;   // (the text names what hs_plan refused)
    const hs_dims& d = a->dims;
    if (a->n_channels < 1 || a->n_channels > kMaxChannels) {
        set_error("%s: n_channels=%d outside [1, %d]", fn, a->n_channels, kMaxChannels);
        return HS_EINVAL;
    }
    if (d.P == 0) return HS_OK;   // (the gradients have no elements: no pointer is looked at, nothing is launched)
    const Field cov[] = {{a->scales, "scales", 4}, {a->rotations, "rotations", 16}};
    int rc = check_fields(fn, cov, 2, " (the forward's scales and rotations: a cov3D_precomp forward is not supported)");
    if (rc != HS_OK) return rc;
    const Field f[] = {{a->geom, "geom", 256}, {a->binning, "binning", 256}, {a->image, "image", 256}, {a->ws, "ws", 256},
                       {a->viewmatrices, "viewmatrices", 4}, {a->projmatrices, "projmatrices", 4}, {a->camposes, "camposes", 4},
                       {a->means3D, "means3D", 4}, {a->opacities, "opacities", 4},
                       {a->features, "features", 4}, {a->dL_dout, "dL_dout", 4},
                       {a->dL_dmeans3D, "dL_dmeans3D", 4}, {a->dL_dopacities, "dL_dopacities", 4},
                       {a->dL_dscales, "dL_dscales", 4}, {a->dL_drotations, "dL_drotations", 16}};
    if ((rc = check_fields(fn, f, (int)(sizeof f / sizeof f[0]))) != HS_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const GeoWs w = geo_workspace(d);
    char* ws = (char*)a->ws;

    GeoReplay p;
    static_cast<ReplayFrame&>(p) = replay_frame(d, L, a->geom, a->binning, a->image);
    p.C = a->n_channels; p.P = d.P;
    p.vec4 = p.C % 4 == 0 && aligned_to(a->features, 16);
    p.features = a->features; p.dL_dout = a->dL_dout;
    p.final_T = (const float*)((const char*)a->image + L.final_T);
    p.pair_rec = (float4*)(ws + w.rec); p.pair_flags = (uint8_t*)(ws + w.flags);
    // passes in ascending channel order over the one set of records: the stream orders a pass behind the one before it
    for (int c0 = 0; c0 < p.C;) {
        const int K = geo_pass(p.C - c0);
        p.c0 = c0;
        rc = K == 16 ? replay_pass<16>(p, d.n_poses, s) : K == 8 ? replay_pass<8>(p, d.n_poses, s) : replay_pass<4>(p, d.n_poses, s);
        if (rc != HS_OK) return rc;
        c0 += K;
    }

    const int64_t I = p.I;
    const char* bin = (const char*)a->binning;
    SegsumArgs sg;
    sg.I = I; sg.inst_sorted = (const uint32_t*)(bin + L.inst_sorted); sg.offs_sorted = (const uint32_t*)(bin + L.offs_sorted);
    sg.pair_grads = p.pair_rec; sg.pair_flags = p.pair_flags; sg.inst_grads = (float4*)(ws + w.rows); sg.counters = p.counters;
    sg.radii_inst = nullptr; sg.clamped = nullptr; sg.view_colors = nullptr; sg.rec = nullptr; sg.act = 0;
    featgeo_segsum_kernel<<<ceil_div(4 * I, 256), 256, 0, s>>>(sg);
    HS_LAUNCH_CHECK();

    // the projection of hs_backward (HS_BWD_PROJECT) from the call's rows: the layout it is handed places inst_grads in the
    // call's workspace.  The colour slots of the rows are zero, so the colours are declared precomputed (the pointer only
    // says so: the projection never reads it) -- no SH row is staged, no view direction formed; M = 0 sizes its LDS.
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
