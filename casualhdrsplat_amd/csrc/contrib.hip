// Per-Gaussian blending-weight statistics (hs_contribution, include/hdrsplat.h): a front-to-back REPLAY of a finished
// forward that keeps, per Gaussian, the sum, the maximum and the number of its blending weights w = alpha * T over the
// pixels -- the quantity contribution-based pruning and error-driven densification decide from, which exists only inside
// the compositing loop.  Three kernels, no atomics of any kind, the same inputs give the same bits:
//
//   contrib_replay_kernel  one 128-thread workgroup per (pose, tile), the render forward's pixel mapping and XCD strip map.
//                          Stages the tile's list 128 entries at a time ({x, y, A2, B2 | C2, opacity, radius, slot start}),
//                          evaluates alpha with the forward's expressions in the forward's operand order, walks only the
//                          entries some 8 x 8 block took (pair_act) up to the tile's deepest contributor (n_contrib), reduces
//                          each block's 64 pixels by a fixed DPP tree, STORES the block's totals into its own plane of the
//                          entry's LDS record (a (wave, group) visits an entry once), adds the planes in plane order and
//                          writes ONE 16-byte record {sum, max, count, 0} per (tile, instance) pair at the pair's
//                          duplicateWithKeys slot -- for EVERY pair of the frame, taken or not: nothing to clear.
//   contrib_segsum_kernel  per instance (in depth order), its contiguous slots combined in a fixed order: four lanes per
//                          instance, a fixed butterfly; one row per instance, every row written.
//   contrib_fold_kernel    per Gaussian, the rows of the poses folded into the caller's arrays in ascending pose order.
//
// A binning overflow (hs_counters.overflow != 0) is seen ON THE DEVICE: the fold then writes nothing.
//
// This unit is compiled like render.hip (FMA contraction on: the Makefile's FAST_TUS), so that the threshold tests below
// see the bits the forward's saw.  The forward's decisions a replay repeats (pixel mapping, XCD strip map, staged conic, alpha
// and thresholds, pair_act bits, walk bound, pair slots), the staging of an entry, the front-to-back walk (walk_front), the
// combination of the planes, the tile context, the segmented sum and the workspace layout are hs_replay.h's; this unit keeps
// what it alone computes from an entry's blending weights.
#include "hs_replay.h"

namespace hs {
namespace {

constexpr int kCBatch = 128;         // staged entries per batch = threads per workgroup

// ---- max / count over the 32 lanes of a lane group: group_sum's tree (hs_replay.h), valid in the same lanes ----
__device__ __forceinline__ float group_max(float v) {
    v = fmaxf(v, dpp_f32<0xB1>(v));
    v = fmaxf(v, dpp_f32<0x4E>(v));
    v = fmaxf(v, dpp_f32<0x141>(v));
    v = fmaxf(v, dpp_f32<0x140>(v));
    // (rows 0 and 2 are masked out of this step and read 0 from it: they are scratch from here on)
    v = fmaxf(v, dpp_f32<0x142, 0xA>(v));
    return v;
}
__device__ __forceinline__ uint32_t group_add_u32(uint32_t v) {
    v += dpp_u32<0xB1>(v);
    v += dpp_u32<0x4E>(v);
    v += dpp_u32<0x141>(v);
    v += dpp_u32<0x140>(v);
    v += dpp_u32<0x142, 0xA>(v);
    return v;
}

struct Replay : ReplayFrame {
    const float* pixel_weight;        // [F,H,W] or null (every weight 1)
    float4* pair_rec;                 // out: one record per pair slot
};

// The statistics of a set of blending weights, and their 16-byte record {sum, max, count (uint bits), 0}.  Nothing taken: the
// identities of sum, max and count -- the record of a pair nobody took.
struct WeightAcc {
    typedef float4 Rec;
    float sum = 0.f, mx = -INFINITY;
    uint32_t c = 0;
    __device__ __forceinline__ void take(const float4 v) { sum += v.x; mx = fmaxf(mx, v.y); c += __float_as_uint(v.z); }
    __device__ __forceinline__ void meet(int d) {
        sum += __shfl_xor(sum, d); mx = fmaxf(mx, __shfl_xor(mx, d)); c += (uint32_t)__shfl_xor((int)c, d);
    }
    __device__ __forceinline__ float4 row() const { return make_float4(sum, mx, __uint_as_float(c), 0.f); }
};

__global__ void __launch_bounds__(kCBatch) contrib_replay_kernel(Replay p) {
    constexpr int KB = kCBatch;
    __shared__ float4 s_a[KB];            // {x, y, A2, B2}
    __shared__ float4 s_b[KB];            // {C2, opacity, radius (int bits), slot start (uint bits)}
    __shared__ float4 s_part[KB][4];      // plane 2g + w: the totals of lane group g of wave w, stored by that group alone
    __shared__ uint8_t s_actb[KB];        // activity byte of each staged entry (bit 2g + w)
    __shared__ uint32_t s_max[2];

    if (p.counters->overflow) return;     // (ReplayFrame: the frame adds nothing)
    const TileCtx tc = tile_context(p);
    const int lane = tc.lane, plane = act_plane(tc.grp, tc.wave);

    // per pixel: the number of its last contributor (the forward stopped the pixel there) and its weight.  A pixel outside
    // the image, or whose weight is exactly 0, takes part in nothing: its bound is 0
    const int64_t HW = (int64_t)p.H * p.W;
    uint32_t last0 = 0, last1 = 0;
    float e0 = 1.f, e1 = 1.f;
    if (tc.in0) {
        const int64_t pix = (int64_t)tc.py0 * p.W + tc.px;
        last0 = p.n_contrib[(int64_t)tc.pose * HW + pix];
        if (p.pixel_weight) e0 = p.pixel_weight[(int64_t)tc.frame * HW + pix];
    }
    if (tc.in1) {
        const int64_t pix = (int64_t)tc.py1 * p.W + tc.px;
        last1 = p.n_contrib[(int64_t)tc.pose * HW + pix];
        if (p.pixel_weight) e1 = p.pixel_weight[(int64_t)tc.frame * HW + pix];
    }
    post_wave_depth(s_max, tc, last0, last1);   // (the walk's bound is the deepest contributor whatever the weights are)
    if (e0 == 0.f) last0 = 0;
    if (e1 == 0.f) last1 = 0;
    __syncthreads();
    const int n_proc = walk_bound(s_max, tc);

    f2 T = {1.f, 1.f};

    for (int base = 0; base < n_proc; base += KB) {
        const int cnt = min(KB, n_proc - base);
        __syncthreads();   // the previous batch's write-out has read its records
        uint32_t act = 0;
        if ((int)threadIdx.x < cnt) {
            const Staged e(p, tc, base);
            act = e.act;
            s_a[threadIdx.x] = e.ra;
            s_b[threadIdx.x] = make_float4(e.rb.x, e.rb.y, e.rc.z, e.rc.w);
        }
        s_actb[threadIdx.x] = (uint8_t)act;
        __syncthreads();
        walk_front<KB>(tc, s_a, s_b, s_actb, base, last0, last1, T, [&](int j, bool on, bool act0, bool act1, f2 w) {
            const float v0 = e0 * w.x, v1 = e1 * w.y;
            float sum = (act0 ? v0 : 0.f) + (act1 ? v1 : 0.f);
            float mx = fmaxf(act0 ? v0 : -INFINITY, act1 ? v1 : -INFINITY);
            uint32_t c = (act0 && v0 > 0.f ? 1u : 0u) + (act1 && v1 > 0.f ? 1u : 0u);
            sum = group_sum(sum);
            mx = group_max(mx);
            c = group_add_u32(c);
            if ((lane & 31) == 31 && on) s_part[j][plane] = make_float4(sum, mx, __uint_as_float(c), 0.f);
        });
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const WeightAcc o = planes_combined<WeightAcc>(act, s_part[threadIdx.x]);
            const float4 a = s_a[threadIdx.x], b = s_b[threadIdx.x];
            const int64_t slot = pair_slot(p, a.x, a.y, __float_as_int(b.z), __float_as_uint(b.w), tc.tx, tc.ty);
            if (slot >= 0 && slot < p.capacity) p.pair_rec[slot] = o.row();
        }
    }
    write_untaken(p, tc, n_proc, KB, p.pair_rec, WeightAcc().row());
}

__global__ void __launch_bounds__(256) contrib_segsum_kernel(Segsum<float4> a) { segsum_rows<WeightAcc>(a); }

// One thread per Gaussian: the rows of its instances folded into the running values one pose at a time, in ascending pose
// order -- a call over N poses leaves what N single-pose calls leave.  A pose in which no term took part (max = -inf)
// leaves the three values alone, bit for bit; an overflowed frame adds nothing at all.
__global__ void __launch_bounds__(256) contrib_fold_kernel(int P, int n_poses, const hs_counters* counters, const float4* inst_rows,
                                                           float* weight_sum, float* weight_max, int32_t* pixel_count) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P || counters->overflow) return;
    float s = weight_sum[g], m = weight_max[g];
    int32_t c = pixel_count[g];
    bool any = false;
    for (int k = 0; k < n_poses; ++k) {
        const float4 v = inst_rows[(int64_t)k * P + g];
        if (v.y > -INFINITY || v.y != v.y) {
            s += v.x;
            m = fmaxf(m, v.y);
            c += (int32_t)__float_as_uint(v.z);
            any = true;
        }
    }
    if (any) { weight_sum[g] = s; weight_max[g] = m; pixel_count[g] = c; }
}

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

HS_API int64_t hs_contribution_workspace_bytes(const hs_dims* dims) {
    const char* fn = "hs_contribution_workspace_bytes";
    hs_sizes sz;
    if (check_args(fn, dims) || hs_plan(dims, &sz, nullptr) != HS_OK) return HS_EINVAL;
    return replay_workspace_bytes(*dims, sizeof(WeightAcc::Rec));
}

HS_API int hs_contribution(const hs_contribution_args* a, void* hip_stream) {
    const char* fn = "hs_contribution";
    if (check_args(fn, a)) return HS_EINVAL;
    hs_sizes sz; hs_layout L;
    if (hs_plan(&a->dims, &sz, &L) != HS_OK) return HS_EINVAL;   // (the text names what hs_plan refused)
    const hs_dims& d = a->dims;
    if (d.P == 0) return HS_OK;   // (no pointer is looked at, nothing is launched)
    const Field f[] = {{a->geom, "geom", 256}, {a->binning, "binning", 256}, {a->image, "image", 256}, {a->ws, "ws", 256},
                       {a->weight_sum, "weight_sum", 4}, {a->weight_max, "weight_max", 4}, {a->pixel_count, "pixel_count", 4}};
    int rc = check_fields(fn, f, 7);
    if (rc != HS_OK) return rc;
    if ((rc = check_aligned(fn, a->pixel_weight, "pixel_weight", 4)) != HS_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;

    Replay p;
    static_cast<ReplayFrame&>(p) = replay_frame(d, L, a->geom, a->binning, a->image);
    const Segsum<float4> sg = replay_segsum<float4>(p, d, L, a->binning, a->ws);
    p.pixel_weight = a->pixel_weight;
    p.pair_rec = sg.pair_rec;
    contrib_replay_kernel<<<p.ntiles * d.n_poses, kCBatch, 0, s>>>(p);
    HS_LAUNCH_CHECK();

    contrib_segsum_kernel<<<ceil_div(4 * p.I, 256), 256, 0, s>>>(sg);
    HS_LAUNCH_CHECK();

    contrib_fold_kernel<<<ceil_div(d.P, 256), 256, 0, s>>>(d.P, d.n_poses, p.counters, sg.inst_rows, a->weight_sum, a->weight_max,
                                                           a->pixel_count);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
