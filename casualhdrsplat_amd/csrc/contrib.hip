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
// see the bits the forward's saw; the expressions are the forward's, operand for operand.  The helpers marked "as
// render.hip" are restated here because that unit keeps them in its anonymous namespace and must not change.  Of
// hs_cloud.h only the host-side argument checks are used.
#include "hs_cloud.h"

namespace hs {
namespace {

constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr float kAlphaMax = 0.99f;
constexpr float kLog2e = 1.4426950408889634f;
constexpr int kCBatch = 128;         // staged entries per batch = threads per workgroup
constexpr int kRowF4 = 1;            // float4 per pair record / per instance row: {sum, max, count (int bits), 0}

typedef float f2 __attribute__((ext_vector_type(2)));

// ---- as render.hip ----
__device__ __forceinline__ void scale_entry(float4& a, float4& b) {
    a.z *= -0.5f * kLog2e; a.w *= -kLog2e; b.x *= -0.5f * kLog2e;
}
__device__ __forceinline__ void lane_pixels(int lane, int sx, int sy, int& px, int& py0) {
    px = sx + 8 * (lane >> 5) + (lane & 7);
    py0 = sy + 2 * ((lane >> 3) & 3);
}
__device__ __forceinline__ int xcd_strip_tile(int b, int nb, int gx) {
    constexpr int kXcd = 8, kRows = 2;
    const int x = b % kXcd, k = b / kXcd;
    const int per = nb / kXcd, rem = nb % kXcd;
    int p = x * per + min(x, rem) + k;
    const int rows = nb / gx;
    const int nstrips = (rows + kRows - 1) / kRows;
    const int strip_tiles = kRows * gx;
    const int last_short = nstrips * strip_tiles - nb;
    int c = 0;
    for (; c < kXcd - 1; ++c) {
        const int ns = (nstrips - c + kXcd - 1) / kXcd;
        const int nt = ns * strip_tiles - (((nstrips - 1) % kXcd) == c ? last_short : 0);
        if (p < nt) break;
        p -= nt;
    }
    const int s_local = p / strip_tiles, r = p - s_local * strip_tiles;
    return (c + kXcd * s_local) * strip_tiles + r;
}
__device__ __forceinline__ float hs_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

// ---- sum / max / count over the 32 lanes of a lane group (rows 2g, 2g + 1 of the wave): a fixed DPP tree -- the four
// in-row steps leave every lane of a row with the row's total, row_bcast:15 then brings the first row's into the second.
// Valid in lanes 16..31 (group 0) and 48..63 (group 1); the other rows hold scratch.  Needs a full exec mask.
__device__ __forceinline__ float group_sum(float v) {
    v += dpp_f32<0xB1>(v);        // quad_perm [1,0,3,2]
    v += dpp_f32<0x4E>(v);        // quad_perm [2,3,0,1]
    v += dpp_f32<0x141>(v);       // row_half_mirror
    v += dpp_f32<0x140>(v);       // row_mirror
    v += dpp_f32<0x142, 0xA>(v);  // row_bcast:15 -> rows 1,3
    return v;
}
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

struct Replay {
    int W, H, gx, gy, ntiles, N, F;   // N: poses per FRAME, F: frames (the launch covers F x N poses)
    int64_t capacity, I;              // pair slots; instances (poses x Gaussians)
    const hs_counters* counters;
    const uint2* ranges; const uint32_t* point_list; const float4* rec;
    const uint32_t* n_contrib; const uint8_t* pair_act;
    const float* pixel_weight;        // [F,H,W] or null (every weight 1)
    float4* pair_rec;                 // out: one record per pair slot
};

// the record of a pair nobody took: the identities of sum, max and count
__device__ __forceinline__ float4 empty_record() { return make_float4(0.f, -INFINITY, __int_as_float(0), 0.f); }

// slot of the (tile, instance) pair in duplicateWithKeys order: the arithmetic of render_bwd_kernel's write-out (integer
// adds and float divides by a power of two: contraction cannot change it)
__device__ __forceinline__ int64_t pair_slot(const Replay& p, float x, float y, int rad, uint32_t off, int tx, int ty) {
    const int rminx = min(p.gx, max(0, (int)((x - (float)rad) / (float)kTile)));
    const int rminy = min(p.gy, max(0, (int)((y - (float)rad) / (float)kTile)));
    const int rmaxx = min(p.gx, max(0, (int)((x + (float)rad + (float)(kTile - 1)) / (float)kTile)));
    return (int64_t)off + (int64_t)(ty - rminy) * (rmaxx - rminx) + (tx - rminx);
}

__global__ void __launch_bounds__(kCBatch) contrib_replay_kernel(Replay p) {
    constexpr int KB = kCBatch;
    __shared__ float4 s_a[KB];            // {x, y, A2, B2}
    __shared__ float4 s_b[KB];            // {C2, opacity, radius (int bits), slot start (uint bits)}
    __shared__ float4 s_part[KB][4];      // plane 2g + w: the totals of lane group g of wave w, stored by that group alone
    __shared__ uint8_t s_actb[KB];        // activity byte of each staged entry (bit 2g + w)
    __shared__ uint32_t s_max[2];

    // an overflowed frame was rendered empty (its ranges are cleared) and adds nothing: the later kernels read no record
    if (p.counters->overflow) return;
    const int vt = xcd_strip_tile(blockIdx.x, gridDim.x, p.gx);  // virtual tile = pose * ntiles + tile
    const int pose = vt / p.ntiles;
    const int tile = vt - pose * p.ntiles;
    const int tx = tile % p.gx, ty = tile / p.gx;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane >> 5;
    const int sx = tx * kTile, sy = ty * kTile + wave * 8;
    int px, py0;
    lane_pixels(lane, sx, sy, px, py0);
    const int py1 = py0 + 1;
    const bool in0 = px < p.W && py0 < p.H, in1 = px < p.W && py1 < p.H;
    const float pxf = (float)px;
    const f2 pyf = {(float)py0, (float)py1};

    const uint2 range = p.ranges[vt];
    // (a list lies inside the sorted pairs; anything else is not a state hs_forward left, and is walked as empty)
    const int n = (range.y >= range.x && (int64_t)range.y <= p.capacity) ? (int)(range.y - range.x) : 0;

    // per pixel: the number of its last contributor (the forward stopped the pixel there) and its weight.  A pixel outside
    // the image, or whose weight is exactly 0, takes part in nothing: its bound is 0
    const int64_t HW = (int64_t)p.H * p.W;
    const int frame = p.F > 1 ? pose / p.N : 0;
    uint32_t last0 = 0, last1 = 0;
    float e0 = 1.f, e1 = 1.f;
    if (in0) {
        const int64_t pix = (int64_t)py0 * p.W + px;
        last0 = p.n_contrib[(int64_t)pose * HW + pix];
        if (p.pixel_weight) e0 = p.pixel_weight[(int64_t)frame * HW + pix];
    }
    if (in1) {
        const int64_t pix = (int64_t)py1 * p.W + px;
        last1 = p.n_contrib[(int64_t)pose * HW + pix];
        if (p.pixel_weight) e1 = p.pixel_weight[(int64_t)frame * HW + pix];
    }
    // the walk's bound: the tile's deepest contributor, whatever the weights are (pair_act is written for the entries the
    // forward staged, and it staged at least these); never more than the list holds
    const uint32_t wave_max = wave_max_u32(max(last0, last1));
    if (lane == 0) s_max[wave] = wave_max;
    if (e0 == 0.f) last0 = 0;
    if (e1 == 0.f) last1 = 0;
    __syncthreads();
    const int n_proc = min(n, (int)max(s_max[0], s_max[1]));

    f2 T = {1.f, 1.f};
    const uint32_t gbit = 1u << (2 * grp + wave);
    const uint32_t wbits = 5u << wave;

    for (int base = 0; base < n_proc; base += KB) {
        const int cnt = min(KB, n_proc - base);
        __syncthreads();   // the previous batch's write-out has read its records
        uint32_t act = 0;
        if ((int)threadIdx.x < cnt) {
            const uint32_t id = min(p.point_list[range.x + base + threadIdx.x], (uint32_t)(p.I - 1));
            act = p.pair_act[(int64_t)range.x + base + threadIdx.x];
            const float4* r = p.rec + kRecF4 * (int64_t)id;
            float4 ra = r[0], rb = r[1];
            const float4 rc = r[2];
            scale_entry(ra, rb);
            s_a[threadIdx.x] = ra;
            s_b[threadIdx.x] = make_float4(rb.x, rb.y, rc.z, rc.w);
        }
        s_actb[threadIdx.x] = (uint8_t)act;
        __syncthreads();
        // every entry one of this wave's two blocks took, front to back; the loop is uniform over the wave (exec stays full:
        // the DPP steps read every lane)
#pragma unroll 1
        for (int k = 0; k < KB / 64; ++k) {
            uint64_t m = __ballot((s_actb[k * 64 + lane] & wbits) != 0);
            while (m) {
                const int j = k * 64 + __builtin_ctzll(m);
                m &= m - 1;
                const float4 a = s_a[j];
                const float4 b = s_b[j];
                const bool on = (s_actb[j] & gbit) != 0;   // this lane's block took the entry (the forward evaluated it there)
                // ---- the forward's alpha: same expressions, same operand order ----
                const float dx = a.x - pxf;
                const f2 dy = a.y - pyf;
                const float t = a.z * dx * dx, u = a.w * dx;
                const f2 pw = dy * (b.x * dy + u) + t;
                const float al0 = fminf(kAlphaMax, b.y * hs_exp2(pw.x));
                const float al1 = fminf(kAlphaMax, b.y * hs_exp2(pw.y));
                // ---- the three tests of blend_fwd_pair: power <= 0, alpha >= 1/255, and "before the entry at which
                // T (1 - alpha) < 1e-4 ends the pixel" -- the forward's own answer to the third is n_contrib
                const uint32_t idx = (uint32_t)(base + j);
                const bool act0 = on && idx < last0 && pw.x <= 0.f && al0 >= kAlphaMin;
                const bool act1 = on && idx < last1 && pw.y <= 0.f && al1 >= kAlphaMin;
                const f2 alpha = {al0, al1};
                const f2 one = {1.f, 1.f};
                const f2 test_T = T * (one - alpha);
                const f2 aT = alpha * T;
                T = f2{act0 ? test_T.x : T.x, act1 ? test_T.y : T.y};
                const float v0 = e0 * aT.x, v1 = e1 * aT.y;
                float sum = (act0 ? v0 : 0.f) + (act1 ? v1 : 0.f);
                float mx = fmaxf(act0 ? v0 : -INFINITY, act1 ? v1 : -INFINITY);
                uint32_t c = (act0 && v0 > 0.f ? 1u : 0u) + (act1 && v1 > 0.f ? 1u : 0u);
                sum = group_sum(sum);
                mx = group_max(mx);
                c = group_add_u32(c);
                if ((lane & 31) == 31 && on) s_part[j][2 * grp + wave] = make_float4(sum, mx, __uint_as_float(c), 0.f);
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            // the planes the entry's takers wrote (its activity bits), combined in plane order
            float4 o = empty_record();
            uint32_t c = 0;
#pragma unroll
            for (int pl = 0; pl < 4; ++pl) {
                if ((act >> pl) & 1u) {
                    const float4 v = s_part[threadIdx.x][pl];
                    o.x += v.x;
                    o.y = fmaxf(o.y, v.y);
                    c += __float_as_uint(v.z);
                }
            }
            o.z = __uint_as_float(c);
            const float4 a = s_a[threadIdx.x], b = s_b[threadIdx.x];
            const int64_t slot = pair_slot(p, a.x, a.y, __float_as_int(b.z), __float_as_uint(b.w), tx, ty);
            if (slot >= 0 && slot < p.capacity) p.pair_rec[kRowF4 * slot] = o;
        }
    }
    // the entries behind the tile's deepest contributor: nobody took them
    for (int i = n_proc + (int)threadIdx.x; i < n; i += KB) {
        const uint32_t id = min(p.point_list[range.x + i], (uint32_t)(p.I - 1));
        const float4* r = p.rec + kRecF4 * (int64_t)id;
        const float4 ra = r[0], rc = r[2];
        const int64_t slot = pair_slot(p, ra.x, ra.y, __float_as_int(rc.z), __float_as_uint(rc.w), tx, ty);
        if (slot >= 0 && slot < p.capacity) p.pair_rec[kRowF4 * slot] = empty_record();
    }
}

struct Segsum {
    int64_t I, capacity;
    const uint32_t* inst_sorted; const uint32_t* offs_sorted; const hs_counters* counters;
    const float4* pair_rec; float4* inst_rows;
};

// Thread t: instance t >> 2 (in depth order), quad lane t & 3 -- lane q combines records beg + q, beg + q + 4, ... in slot
// order, the four partial results meet in a fixed butterfly (as pair_segsum_kernel).
__global__ void __launch_bounds__(256) contrib_segsum_kernel(Segsum a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = t >> 2;
    const int q = (int)(t & 3);
    // binning overflow: nothing was emitted or rendered, and slots past the capacity do not exist
    const bool valid = i < a.I && !a.counters->overflow;
    const uint32_t beg = valid ? (i == 0 ? 0u : a.offs_sorted[i - 1]) : 0u;
    uint32_t end = valid ? a.offs_sorted[i] : 0u;
    if ((int64_t)end > a.capacity) end = (uint32_t)a.capacity;
    float sum = 0.f, mx = -INFINITY;
    uint32_t c = 0;
    for (uint32_t s = beg + q; s < end; s += 4) {
        const float4 v = a.pair_rec[kRowF4 * (int64_t)s];
        sum += v.x;
        mx = fmaxf(mx, v.y);
        c += __float_as_uint(v.z);
    }
    sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2);
    mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2));
    c += (uint32_t)__shfl_xor((int)c, 1); c += (uint32_t)__shfl_xor((int)c, 2);
    if (i < a.I && q == 0) {
        // (a depth sort that gave up -- overflow = 2 -- left no instance list: the identities go to row i)
        const int64_t inst = a.counters->overflow ? i : (int64_t)a.inst_sorted[i];
        if (inst < a.I) a.inst_rows[kRowF4 * inst] = make_float4(sum, mx, __uint_as_float(c), 0.f);
    }
}

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
        const float4 v = inst_rows[kRowF4 * ((int64_t)k * P + g)];
        if (v.y > -INFINITY || v.y != v.y) {
            s += v.x;
            m = fmaxf(m, v.y);
            c += (int32_t)__float_as_uint(v.z);
            any = true;
        }
    }
    if (any) { weight_sum[g] = s; weight_max[g] = m; pixel_count[g] = c; }
}

// workspace: pair records [capacity] | instance rows [P * n_poses], 16 bytes each, both 256-byte aligned
int64_t pair_rec_bytes(const hs_dims& d) { return align_up(d.capacity * 16 * kRowF4, 256); }
int64_t inst_row_bytes(const hs_dims& d) { return align_up((int64_t)d.P * d.n_poses * 16 * kRowF4, 256); }

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

HS_API int64_t hs_contribution_workspace_bytes(const hs_dims* dims) {
    const char* fn = "hs_contribution_workspace_bytes";
    hs_sizes sz;
    if (check_args(fn, dims) || hs_plan(dims, &sz, nullptr) != HS_OK) return HS_EINVAL;
    const int64_t bytes = pair_rec_bytes(*dims) + inst_row_bytes(*dims);
    return bytes > 0 ? bytes : 256;
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
    const char* geom = (const char*)a->geom; const char* bin = (const char*)a->binning; const char* img = (const char*)a->image;
    const hs_counters* counters = (const hs_counters*)(geom + L.counters);
    float4* pair_rec = (float4*)a->ws;
    float4* inst_rows = (float4*)((char*)a->ws + pair_rec_bytes(d));
    const int64_t I = (int64_t)d.P * d.n_poses;

    Replay p;
    p.W = d.W; p.H = d.H; p.gx = (d.W + kTile - 1) / kTile; p.gy = (d.H + kTile - 1) / kTile;
    p.ntiles = p.gx * p.gy; p.F = frames_of(d); p.N = d.n_poses / p.F;
    p.capacity = d.capacity; p.I = I; p.counters = counters;
    p.ranges = (const uint2*)(bin + L.ranges); p.point_list = (const uint32_t*)(bin + L.point_list);
    p.rec = (const float4*)(geom + L.rec);
    p.n_contrib = (const uint32_t*)(img + L.n_contrib);
    p.pair_act = (const uint8_t*)bin + L.pair_act;
    p.pixel_weight = a->pixel_weight;
    p.pair_rec = pair_rec;
    contrib_replay_kernel<<<p.ntiles * d.n_poses, kCBatch, 0, s>>>(p);
    HS_LAUNCH_CHECK();

    Segsum sg;
    sg.I = I; sg.capacity = d.capacity;
    sg.inst_sorted = (const uint32_t*)(bin + L.inst_sorted); sg.offs_sorted = (const uint32_t*)(bin + L.offs_sorted);
    sg.counters = counters; sg.pair_rec = pair_rec; sg.inst_rows = inst_rows;
    contrib_segsum_kernel<<<ceil_div(4 * I, 256), 256, 0, s>>>(sg);
    HS_LAUNCH_CHECK();

    contrib_fold_kernel<<<ceil_div(d.P, 256), 256, 0, s>>>(d.P, d.n_poses, counters, inst_rows, a->weight_sum, a->weight_max,
                                                           a->pixel_count);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
