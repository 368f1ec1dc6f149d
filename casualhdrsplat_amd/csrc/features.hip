// Per-Gaussian feature compositing (hs_composite_features, hs_composite_features_backward; include/hdrsplat.h): C extra
// channels stored per Gaussian, composited per pixel with the blending weights w = alpha * T of a FINISHED forward -- a third
// replay beside contrib.hip and absgrad.hip, front to back, under the forward's own decisions (pair_act, n_contrib).  The
// render kernels are not involved.  No atomics of any kind, the same inputs give the same bits.
//
//   features_fwd_kernel         one 128-thread workgroup per (pose, tile) and channel group (blockIdx.y: 4, 8 or 16 channels),
//                               the render forward's pixel mapping and XCD strip map, two pixels per lane.  Stages the tile's
//                               list 128 entries at a time ({x, y, A2, B2 | C2, opacity}) together with the group's feature
//                               values of each entry (row instance - pose * P; float4 reads where C % 4 == 0 and the base is
//                               16-byte aligned), walks only the entries one of the wave's blocks took up to the tile's
//                               deepest contributor, keeps T per pixel and acc[c] = fma(w, f[c], acc[c]) for both pixels
//                               (every lane reads the same LDS word: a broadcast).  An entry that is not composited at a pixel
//                               is SELECTED out, not multiplied by zero.  The epilogue stores every in-image pixel of the
//                               group's channels -- also for an empty list and for an overflowed frame (zeros).
//   features_bwd_replay_kernel  contrib_replay_kernel with the pass's 4 or 8 channels of dL_dout[pose, c, pix] as signed
//                               pixel weights: sums only, one record per pair slot, for every pair, taken or not.
//   features_segsum_kernel      segsum_rows over a sum-only accumulator.
//   features_fold_kernel        per Gaussian and channel of the pass: +0, plus the poses' rows in ascending pose order, WRITTEN
//                               into the pass's columns of dL_dfeatures[P, C].
// The backward runs its passes (eight channels while more than four are left, then four) over one workspace sized for the
// 32-byte records of an eight-channel pass: twice hs_contribution's, whatever C is.
//
// The gradient these kernels deliver reaches the features; the gradient to the geometry (means, covariances, opacities)
// through the channels -- a C-channel generalisation of render_bwd_kernel -- is featgeo.hip's.
//
// Compiled like render.hip (FMA contraction on: the Makefile's FAST_TUS); the forward's decisions, the staging of an entry and
// of its feature row, the front-to-back walk and the combination of the planes are hs_replay.h's.
#include "hs_replay.h"

// A/B switches of scripts/time_features.py (make variant TUS=features DEFS=...).  0, what ships: chosen per call from C, as
// measured -- the forward takes the narrowest group that holds all channels (one walk of the lists), the
// backward takes eight channels per pass while more than four are left, then four
#ifndef HS_TUNE_FEAT_GROUP
#define HS_TUNE_FEAT_GROUP 0     // channels per forward workgroup: 4, 8 or 16 for every call
#endif
#ifndef HS_TUNE_FEAT_REC
#define HS_TUNE_FEAT_REC 0       // channels per backward pass: 4 (16-byte records) or 8 (32-byte records) for every pass
#endif

namespace hs {
namespace {

constexpr int kFBatch = 128;                  // staged entries per batch = threads per workgroup
constexpr int kFeatGroup = HS_TUNE_FEAT_GROUP;
constexpr int kFeatRec = HS_TUNE_FEAT_REC;
constexpr int kMaxChannels = 512;
static_assert(kFeatGroup == 0 || kFeatGroup == 4 || kFeatGroup == 8 || kFeatGroup == 16, "channel group of the forward");
static_assert(kFeatRec == 0 || kFeatRec == 4 || kFeatRec == 8, "channels per backward record");
constexpr int kFeatRecBytes = kFeatRec == 4 ? 16 : 32;   // the workspace holds the widest record that can be asked for

static inline int feature_group(int C) { return kFeatGroup ? kFeatGroup : C <= 4 ? 4 : C <= 8 ? 8 : 16; }
static inline int feature_pass(int left) { return kFeatRec ? kFeatRec : left > 4 ? 8 : 4; }

struct FeatFwd : ReplayFrame {
    int C, P;
    bool vec4;                        // C % 4 == 0 and a 16-byte aligned base: rows are read as float4
    const float* features;            // [P, C]
    float* out;                       // [n_poses, C, H, W]
};

struct FeatBwd : ReplayFrame {
    int C, c0;                        // channels; the pass's first
    const float* dL_dout;             // [n_poses, C, H, W]
};

// the sums of the R channels of a backward pass, and their record; nothing taken: +0 in every channel -- the record of a pair nobody took
template <int R>
struct alignas(16) FeatRecT { float v[R]; };

template <int R>
struct SumAcc {
    typedef FeatRecT<R> Rec;
    float s[R];
    __device__ __forceinline__ SumAcc() {
#pragma unroll
        for (int q = 0; q < R; ++q) s[q] = 0.f;
    }
    __device__ __forceinline__ void take(const Rec r) {
#pragma unroll
        for (int q = 0; q < R; ++q) s[q] += r.v[q];
    }
    __device__ __forceinline__ void meet(int d) {
#pragma unroll
        for (int q = 0; q < R; ++q) s[q] += __shfl_xor(s[q], d);
    }
    __device__ __forceinline__ Rec row() const {
        Rec r;
#pragma unroll
        for (int q = 0; q < R; ++q) r.v[q] = s[q];
        return r;
    }
};

template <int G>
__global__ void __launch_bounds__(kFBatch) features_fwd_kernel(FeatFwd p) {
    constexpr int KB = kFBatch;
    __shared__ float4 s_a[KB];            // {x, y, A2, B2}
    __shared__ float2 s_b[KB];            // {C2, opacity}
    __shared__ alignas(16) float s_f[KB][G];   // the group's feature values of each staged entry
    __shared__ uint8_t s_actb[KB];        // activity byte of each staged entry (bit 2g + w)
    __shared__ uint32_t s_max[2];

    const TileCtx tc = tile_context(p);
    const int c0 = blockIdx.y * G;       // the group's first channel (c0 < C: the grid)
    const int64_t HW = (int64_t)p.H * p.W;

    uint32_t last0 = 0, last1 = 0;        // per pixel: the number of its last contributor (the forward stopped it there)
    if (tc.in0) last0 = p.n_contrib[(int64_t)tc.pose * HW + (int64_t)tc.py0 * p.W + tc.px];
    if (tc.in1) last1 = p.n_contrib[(int64_t)tc.pose * HW + (int64_t)tc.py1 * p.W + tc.px];
    post_wave_depth(s_max, tc, last0, last1);
    __syncthreads();
    // an overflowed frame was rendered empty: nothing is walked, the epilogue stores zeros
    const int n_proc = p.counters->overflow ? 0 : walk_bound(s_max, tc);

    f2 T = {1.f, 1.f};
    f2 acc[G];
#pragma unroll
    for (int c = 0; c < G; ++c) acc[c] = f2{0.f, 0.f};

    for (int base = 0; base < n_proc; base += KB) {
        const int cnt = min(KB, n_proc - base);
        __syncthreads();   // the previous batch has been walked
        uint32_t act = 0;
        if ((int)threadIdx.x < cnt) {
            const Staged e(p, tc, base);
            act = e.act;
            s_a[threadIdx.x] = e.ra;
            s_b[threadIdx.x] = make_float2(e.rb.x, e.rb.y);
            stage_feature_row(s_f[threadIdx.x], p.features, p.P, p.C, c0, p.vec4, e.id, tc.pose);
        }
        s_actb[threadIdx.x] = (uint8_t)act;
        __syncthreads();
        walk_front<KB>(tc, s_a, s_b, s_actb, base, last0, last1, T, [&](int j, bool, bool act0, bool act1, f2 w) {
#pragma unroll
            for (int c = 0; c < G; ++c) {
                const float f = s_f[j][c];
                const f2 next = w * f2{f, f} + acc[c];          // (contracted: one packed fma)
                acc[c] = f2{act0 ? next.x : acc[c].x, act1 ? next.y : acc[c].y};
            }
        });
    }
    // every in-image pixel of the group's channels is stored, whatever the list held
    float* o = p.out + ((int64_t)tc.pose * p.C + c0) * HW;
#pragma unroll
    for (int c = 0; c < G; ++c) {
        if (c0 + c < p.C) {
            if (tc.in0) o[c * HW + (int64_t)tc.py0 * p.W + tc.px] = acc[c].x;
            if (tc.in1) o[c * HW + (int64_t)tc.py1 * p.W + tc.px] = acc[c].y;
        }
    }
}

// an empty cloud has no state to replay: every element of `out` is +0
__global__ void __launch_bounds__(256) features_zero_kernel(float* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 0.f;
}

template <int R>
__global__ void __launch_bounds__(kFBatch) features_bwd_replay_kernel(FeatBwd p, FeatRecT<R>* pair_rec) {
    constexpr int KB = kFBatch;
    typedef SumAcc<R> FeatAcc;
    typedef FeatRecT<R> FeatRec;
    __shared__ float4 s_a[KB];            // {x, y, A2, B2}
    __shared__ float4 s_b[KB];            // {C2, opacity, radius (int bits), slot start (uint bits)}
    __shared__ FeatRec s_part[KB][4];     // plane 2g + w: the totals of lane group g of wave w, stored by that group alone
    __shared__ uint8_t s_actb[KB];
    __shared__ uint32_t s_max[2];

    if (p.counters->overflow) return;     // (ReplayFrame: the segmented sum reads no record of an overflowed frame)
    const TileCtx tc = tile_context(p);
    const int lane = tc.lane, plane = act_plane(tc.grp, tc.wave);

    // per pixel: the number of its last contributor, and the pass's channels of the upstream gradient (0 past the last
    // channel and outside the image)
    const int64_t HW = (int64_t)p.H * p.W;
    uint32_t last0 = 0, last1 = 0;
    f2 e[R];
#pragma unroll
    for (int q = 0; q < R; ++q) e[q] = f2{0.f, 0.f};
    const float* dl = p.dL_dout + ((int64_t)tc.pose * p.C + p.c0) * HW;
    if (tc.in0) {
        const int64_t pix = (int64_t)tc.py0 * p.W + tc.px;
        last0 = p.n_contrib[(int64_t)tc.pose * HW + pix];
#pragma unroll
        for (int q = 0; q < R; ++q)
            if (p.c0 + q < p.C) e[q].x = dl[q * HW + pix];
    }
    if (tc.in1) {
        const int64_t pix = (int64_t)tc.py1 * p.W + tc.px;
        last1 = p.n_contrib[(int64_t)tc.pose * HW + pix];
#pragma unroll
        for (int q = 0; q < R; ++q)
            if (p.c0 + q < p.C) e[q].y = dl[q * HW + pix];
    }
    post_wave_depth(s_max, tc, last0, last1);
    __syncthreads();
    const int n_proc = walk_bound(s_max, tc);

    f2 T = {1.f, 1.f};

    for (int base = 0; base < n_proc; base += KB) {
        const int cnt = min(KB, n_proc - base);
        __syncthreads();   // the previous batch's write-out has read its records
        uint32_t act = 0;
        if ((int)threadIdx.x < cnt) {
            const Staged s(p, tc, base);
            act = s.act;
            s_a[threadIdx.x] = s.ra;
            s_b[threadIdx.x] = make_float4(s.rb.x, s.rb.y, s.rc.z, s.rc.w);
        }
        s_actb[threadIdx.x] = (uint8_t)act;
        __syncthreads();
        walk_front<KB>(tc, s_a, s_b, s_actb, base, last0, last1, T, [&](int j, bool on, bool act0, bool act1, f2 w) {
            // a pixel that does not composite the entry is selected out: its gradient, finite or not, adds nothing
            FeatRec tot;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const f2 v = w * e[q];
                tot.v[q] = group_sum((act0 ? v.x : 0.f) + (act1 ? v.y : 0.f));
            }
            if ((lane & 31) == 31 && on) s_part[j][plane] = tot;
        });
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const FeatAcc o = planes_combined<FeatAcc>(act, s_part[threadIdx.x]);
            const float4 a = s_a[threadIdx.x], b = s_b[threadIdx.x];
            const int64_t slot = pair_slot(p, a.x, a.y, __float_as_int(b.z), __float_as_uint(b.w), tc.tx, tc.ty);
            if (slot >= 0 && slot < p.capacity) pair_rec[slot] = o.row();
        }
    }
    write_untaken(p, tc, n_proc, KB, pair_rec, FeatAcc().row());
}

template <int R>
__global__ void __launch_bounds__(256) features_segsum_kernel(Segsum<FeatRecT<R>> a) { segsum_rows<SumAcc<R>>(a); }

// One thread per (Gaussian, channel of the pass): +0, plus the rows of its instances in ascending pose order, written.  (The
// segmented sum writes every row, an all-zero one for every instance of an overflowed frame.)
template <int R>
__global__ void __launch_bounds__(256) features_fold_kernel(int P, int n_poses, int C, int c0, const FeatRecT<R>* inst_rows,
                                                            float* dL_dfeatures) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t g = t / R;
    const int q = (int)(t - g * R);
    if (g >= P || c0 + q >= C) return;
    float s = 0.f;
    for (int k = 0; k < n_poses; ++k) s += inst_rows[(int64_t)k * P + g].v[q];
    dL_dfeatures[g * C + c0 + q] = s;
}

// one pass of the backward: the R channels from p.c0 on, over the one workspace
template <int R>
int backward_pass(const FeatBwd& p, const hs_dims& d, const hs_layout& L, const hs_composite_features_bwd_args* a, hipStream_t s) {
    const Segsum<FeatRecT<R>> sg = replay_segsum<FeatRecT<R>>(p, d, L, a->binning, a->ws);
    features_bwd_replay_kernel<R><<<p.ntiles * d.n_poses, kFBatch, 0, s>>>(p, sg.pair_rec);
    HS_LAUNCH_CHECK();
    features_segsum_kernel<R><<<ceil_div(4 * p.I, 256), 256, 0, s>>>(sg);
    HS_LAUNCH_CHECK();
    features_fold_kernel<R><<<ceil_div((int64_t)d.P * R, 256), 256, 0, s>>>(d.P, d.n_poses, p.C, p.c0, sg.inst_rows, a->dL_dfeatures);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

template <int G>
int forward_launch(const FeatFwd& p, int n_poses, hipStream_t s) {
    const dim3 grid(p.ntiles * n_poses, ceil_div(p.C, G));
    features_fwd_kernel<G><<<grid, kFBatch, 0, s>>>(p);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

int check_channels(const char* fn, int n_channels) {
    if (n_channels < 1 || n_channels > kMaxChannels) {
        set_error("%s: n_channels=%d outside [1, %d]", fn, n_channels, kMaxChannels);
        return HS_EINVAL;
    }
    return HS_OK;
}

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

HS_API int64_t hs_composite_features_workspace_bytes(const hs_dims* dims) {
    const char* fn = "hs_composite_features_workspace_bytes";
    hs_sizes sz;
    if (check_args(fn, dims) || hs_plan(dims, &sz, nullptr) != HS_OK) return HS_EINVAL;
    return replay_workspace_bytes(*dims, kFeatRecBytes);
}

HS_API int hs_composite_features(const hs_composite_features_args* a, void* hip_stream) {
    const char* fn = "hs_composite_features";
    if (check_args(fn, a)) return HS_EINVAL;
    hs_sizes sz; hs_layout L;
    if (hs_plan(&a->dims, &sz, &L) != HS_OK) return HS_EINVAL;   // (the text names what hs_plan refused)
    const hs_dims& d = a->dims;
    int rc = check_channels(fn, a->n_channels);
    if (rc != HS_OK) return rc;
    if ((rc = check_field(fn, a->out, "out", 4)) != HS_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const int C = a->n_channels;
    if (d.P == 0) {   // no state, no features: out is all zeros
        const int64_t n = (int64_t)d.n_poses * C * d.H * d.W;
        features_zero_kernel<<<ceil_div(n, 256), 256, 0, s>>>(a->out, n);
        HS_LAUNCH_CHECK();
        return HS_OK;
    }
    const Field f[] = {{a->geom, "geom", 256}, {a->binning, "binning", 256}, {a->image, "image", 256}, {a->features, "features", 4}};
    if ((rc = check_fields(fn, f, 4)) != HS_OK) return rc;

    FeatFwd p;
    static_cast<ReplayFrame&>(p) = replay_frame(d, L, a->geom, a->binning, a->image);
    p.C = C; p.P = d.P;
    p.vec4 = C % 4 == 0 && aligned_to(a->features, 16);
    p.features = a->features; p.out = a->out;
    switch (feature_group(C)) {
        case 4: return forward_launch<4>(p, d.n_poses, s);
        case 8: return forward_launch<8>(p, d.n_poses, s);
        default: return forward_launch<16>(p, d.n_poses, s);
    }
}

HS_API int hs_composite_features_backward(const hs_composite_features_bwd_args* a, void* hip_stream) {
    const char* fn = "hs_composite_features_backward";
    if (check_args(fn, a)) return HS_EINVAL;
    hs_sizes sz; hs_layout L;
    if (hs_plan(&a->dims, &sz, &L) != HS_OK) return HS_EINVAL;
    const hs_dims& d = a->dims;
    int rc = check_channels(fn, a->n_channels);
    if (rc != HS_OK) return rc;
    if (d.P == 0) return HS_OK;   // (dL_dfeatures has no elements: no pointer is looked at, nothing is launched)
    const Field f[] = {{a->geom, "geom", 256}, {a->binning, "binning", 256}, {a->image, "image", 256}, {a->ws, "ws", 256},
                       {a->dL_dout, "dL_dout", 4}, {a->dL_dfeatures, "dL_dfeatures", 4}};
    if ((rc = check_fields(fn, f, 6)) != HS_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;

    FeatBwd p;
    static_cast<ReplayFrame&>(p) = replay_frame(d, L, a->geom, a->binning, a->image);
    p.C = a->n_channels; p.dL_dout = a->dL_dout;
    // passes of eight or four channels, all over the one workspace: the stream orders a pass's fold before the next replay
    for (int c0 = 0; c0 < p.C;) {
        const int R = feature_pass(p.C - c0);
        p.c0 = c0;
        rc = R == 8 ? backward_pass<8>(p, d, L, a, s) : backward_pass<4>(p, d, L, a, s);
        if (rc != HS_OK) return rc;
        c0 += R;
    }
    return HS_OK;
}

}  // extern "C"
