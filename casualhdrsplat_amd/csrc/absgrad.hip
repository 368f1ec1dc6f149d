// Per-Gaussian absolute screen-gradient statistic (hs_abs_gradient, include/hdrsplat.h): a back-to-front REPLAY of a
// finished forward under the upstream gradients hs_backward takes, which keeps, per Gaussian, the sum over the pixels of the
// MAGNITUDE of each pixel's term of dL/dmean2D -- the AbsGS refinement signal.  render_bwd_kernel sums the signed terms over
// the tile before a sign can be dropped, so the quantity exists only inside the compositing loop.  Three kernels, no atomics
// of any kind, the same inputs give the same bits:
//
//   absgrad_replay_kernel  one 128-thread workgroup per (pose, tile), the render forward's pixel mapping and XCD strip map.
//                          Stages the tile's list 128 entries at a time, deepest batch first; each 8 x 8 block (lane group)
//                          walks its OWN list of the entries it took (pair_act), back to front, the two groups of a wave in
//                          lock step, from the tile's deepest contributor (n_contrib) to the front with T
//                          starting at final_T and the one-number recurrence of render.hip's backward (q starts at bg . dL,
//                          dL/dalpha_i = T_i (c_i . dL - q_i), q_{i-1} = q_i + alpha_i (c_i . dL - q_i)), evaluates alpha with
//                          the forward's expressions, forms |t_x| and |t_y| PER PIXEL, reduces each block's 64 pixels by a
//                          fixed DPP tree, STORES the block's two totals into its own plane of the entry's LDS record (a (wave,
//                          group) visits an entry once), adds the planes in plane order and writes ONE 8-byte record
//                          {sum |t_x|, sum |t_y|} per (tile, instance) pair at the pair's duplicateWithKeys slot -- for
//                          EVERY pair of the frame, taken or not: nothing to clear.  A pair no pixel composited holds {-1, -1}.
//   absgrad_segsum_kernel  per instance (in depth order), its contiguous slots combined in a fixed order: four lanes per
//                          instance, a fixed butterfly; one row per instance, every row written.
//   absgrad_fold_kernel    per Gaussian, frames ascending: the rows of the frame's poses added in ascending pose order, then
//                          abs_grad_accum += sqrt(a_x^2 + a_y^2).
//
// A binning overflow (hs_counters.overflow != 0) is seen ON THE DEVICE: the fold then writes nothing.
//
// This unit is compiled like render.hip (FMA contraction on: the Makefile's FAST_TUS), so that the threshold tests below
// see the bits the forward's saw.  The forward's decisions a replay repeats (pixel mapping, XCD strip map, staged conic, alpha
// and thresholds, pair_act bits, walk bound, pair slots), the staging of an entry, the back-to-front walk (take lists,
// sentinel, T recursion), the combination of the planes, the tile context, the segmented sum and the workspace layout are
// hs_replay.h's; the rest of the backward's step is render.hip's step_bwd_pair, operand for operand.
#include "hs_replay.h"

namespace hs {
namespace {

constexpr float kLogEps = 1e-8f;
constexpr int kAThreads = 128;       // threads per workgroup: two waves, one per half tile
// staged entries per batch (a multiple of 64, at most the threads).  Measured, whole call, two runs each: 128 entries 0.482 /
// 0.481 ms at 1 M Gaussians / 1080p and 0.157 / 0.159 ms at 100 k / 800 x 800; 64 entries (half the LDS) 0.469 / 0.471 and
// 0.163 / 0.164 ms -- a wash.  Reading the next trip's record a trip ahead costs 14 registers and a wave per SIMD: 0.494 ms.
constexpr int kABatch = 128;

static_assert(kABatch % 64 == 0 && kABatch <= kAThreads, "the lists are built from whole ballots, one entry is staged per thread");

struct Crf {
    const float* table;  // [3,K]
    int K;
    float umin, umax, dt;
};
__device__ __forceinline__ void crf_locate(const Crf& c, float Hv, int& i, float& f, float& xv, bool& interior) {
    xv = Hv * c.dt;
    const float u = __logf(fmaxf(xv, kLogEps));
    float s = (u - c.umin) / (c.umax - c.umin) * (float)(c.K - 1);
    bool in = true;
    if (!(s > 0.f)) { s = 0.f; in = false; }
    if (s >= (float)(c.K - 1)) { s = (float)(c.K - 1); in = false; }
    i = (int)floorf(s);
    if (i > c.K - 2) i = c.K - 2;
    f = s - (float)i;
    interior = in && (xv > kLogEps);
}
// dL/dH given dL/dLDR
__device__ __forceinline__ float crf_grad_H(const Crf& c, int ch, float Hv, float g) {
    int i; float f, xv; bool in;
    crf_locate(c, Hv, i, f, xv, in);
    if (!in) return 0.f;
    const float* t = c.table + ch * c.K;
    const float scale = (float)(c.K - 1) / (c.umax - c.umin);
    return g * (t[i + 1] - t[i]) * scale / xv * c.dt;
}

struct Replay : ReplayFrame {
    const float* bg; const float* final_T; const float* pose_hdr;
    const float* dL_dcolor; const float* dL_dhdr; const float* dL_dalpha; const float* dL_dinvdepth;
    Crf crf;
    // (here, beside the words the prologue loads anyway: as the first word behind the frame part it was fetched by a late
    // scalar load of its own in front of the pixel loads, 0.5 % of the call at both measured sizes)
    int flags;
    const float* exposure;
    float2* pair_rec;                        // out: one record per pair slot
};

// The sums of a set of |t_x|, |t_y| terms, and their 8-byte record.  The record of a pair (the row of an instance) no pixel
// composited is {-1, -1}: sums of magnitudes are never negative.
__device__ __forceinline__ float2 empty_record() { return make_float2(-1.f, -1.f); }
__device__ __forceinline__ bool has_term(float2 v) { return !(v.x < 0.f); }
struct AbsAcc {
    typedef float2 Rec;
    float sx = 0.f, sy = 0.f;
    int any = 0;
    __device__ __forceinline__ void take(const float2 v) { if (has_term(v)) { sx += v.x; sy += v.y; any = 1; } }
    __device__ __forceinline__ void meet(int d) { sx += __shfl_xor(sx, d); sy += __shfl_xor(sy, d); any |= __shfl_xor(any, d); }
    __device__ __forceinline__ float2 row() const { return any ? make_float2(sx, sy) : empty_record(); }
};

// Upstream gradient w.r.t. this pose's radiance H_ch at one pixel (as render.hip's pixel_grad).
__device__ __forceinline__ float pixel_grad(const Replay& p, const Crf& c, int pose, int frame, int ch, int64_t pix, int64_t HW) {
    const float invN = 1.f / (float)p.N;
    const int64_t gpl = ((int64_t)frame * 3 + ch) * HW + pix;
    float g = p.dL_dcolor[gpl];
    if (!(p.flags & HS_FLAG_HDR)) return g * invN;
    float out = 0.f;
    if (p.N == 1 || !(p.flags & HS_FLAG_BLUR_HDR)) {
        const float Hv = p.pose_hdr[((int64_t)pose * 3 + ch) * HW + pix];
        out = crf_grad_H(c, ch, Hv, g * invN);
    } else {
        const float Hm = p.pose_hdr[((int64_t)(p.F * p.N + frame) * 3 + ch) * HW + pix];
        out = crf_grad_H(c, ch, Hm, g) * invN;
    }
    if (p.dL_dhdr) out += p.dL_dhdr[gpl] * invN;
    return out;
}

// Per-pixel state of the replay (as render.hip's PixB / load_pixel_bwd).
struct PixB {
    float T, dL0, dL1, dL2, q, dLd;
    uint32_t last;
};
__device__ __forceinline__ void load_pixel_bwd(const Replay& p, PixB& s, bool inside, int pose, int frame, int px, int py) {
    const int64_t HW = (int64_t)p.H * p.W;
    const int64_t pix = (int64_t)py * p.W + px;
    s.T = 0.f; s.dL0 = s.dL1 = s.dL2 = 0.f; s.last = 0;
    if (inside) {
        s.T = p.final_T[(int64_t)pose * HW + pix];
        s.last = p.n_contrib[(int64_t)pose * HW + pix];
        Crf c = p.crf;
        if (p.flags & HS_FLAG_HDR) c.dt = p.exposure[frame];
        s.dL0 = pixel_grad(p, c, pose, frame, 0, pix, HW);
        s.dL1 = pixel_grad(p, c, pose, frame, 1, pix, HW);
        s.dL2 = pixel_grad(p, c, pose, frame, 2, pix, HW);
    }
    float bg_dot = (p.bg[0] * s.dL0 + p.bg[1] * s.dL1) + p.bg[2] * s.dL2;
    if (p.dL_dalpha && inside) bg_dot -= p.dL_dalpha[pix] / (float)p.N;
    s.q = bg_dot;
    s.dLd = (p.dL_dinvdepth && inside) ? p.dL_dinvdepth[pix] / (float)p.N : 0.f;
}

template <bool DEPTH>
__global__ void __launch_bounds__(kAThreads) absgrad_replay_kernel(Replay p) {
    constexpr int KB = kABatch;
    // (record KB of the staging arrays: the back-to-front walk's sentinel)
    __shared__ float4 s_a[KB + 1];        // {x, y, A2, B2}
    __shared__ float4 s_b[KB + 1];        // {C2, opacity, r, g}
    __shared__ float4 s_c[KB + 1];        // {b, 1 / depth (DEPTH) or depth, radius (int bits), slot start (uint bits)}
    __shared__ float2 s_part[KB + 1][4];  // plane 2g + w: the totals of lane group g of wave w, stored by that group alone
    __shared__ uint8_t s_actb[kAThreads]; // activity byte of each staged entry (bit 2g + w)
    __shared__ uint16_t s_list[2][2][KB + 8];     // [wave][lane group]: the group's takers among the staged entries, back to front
    __shared__ uint32_t s_max[2];

    if (p.counters->overflow) return;     // (ReplayFrame: the frame adds nothing)
    const TileCtx tc = tile_context(p);
    const int lane = tc.lane, plane = act_plane(tc.grp, tc.wave);

    PixB s0, s1;
    load_pixel_bwd(p, s0, tc.in0, tc.pose, tc.frame, tc.px, tc.py0);
    load_pixel_bwd(p, s1, tc.in1, tc.pose, tc.frame, tc.px, tc.py1);
    f2 T = {s0.T, s1.T}, q = {s0.q, s1.q};
    const f2 dL0 = {s0.dL0, s1.dL0}, dL1 = {s0.dL1, s1.dL1}, dL2 = {s0.dL2, s1.dL2}, dLd = {s0.dLd, s1.dLd};
    const uint32_t last0 = s0.last, last1 = s1.last;

    post_wave_depth(s_max, tc, last0, last1);
    if (threadIdx.x == 0) {
        s_a[KB] = make_float4(0.f, 0.f, 0.f, 0.f); s_b[KB] = make_float4(0.f, 0.f, 0.f, 0.f); s_c[KB] = make_float4(0.f, 1.f, 0.f, 0.f);
    }
    __syncthreads();
    const int n_proc = walk_bound(s_max, tc);

    // |t_x| = |A dx + B dy| |w| W / 2 with A = -2 A2 / log2(e), B = -B2 / log2(e): the sums are kept in the staged (scaled)
    // conic's units, the positive factor is applied once per pair at write-out
    const float kx = 0.5f * (float)p.W / kLog2e, ky = 0.5f * (float)p.H / kLog2e;

    const int nb = (n_proc + KB - 1) / KB;
    for (int bi = nb - 1; bi >= 0; --bi) {
        const int base = bi * KB;
        const int cnt = min(KB, n_proc - base);
        __syncthreads();   // the previous batch's write-out has read its records
        uint32_t act = 0;
        if ((int)threadIdx.x < cnt) {
            Staged e(p, tc, base);
            act = e.act;
            if constexpr (DEPTH) e.rc.y = 1.f / e.rc.y;  // depth -> inverse depth
            s_a[threadIdx.x] = e.ra;
            s_b[threadIdx.x] = e.rb;
            s_c[threadIdx.x] = e.rc;
        }
        s_actb[threadIdx.x] = (uint8_t)act;
        __syncthreads();
        // back to front over the entries this wave's blocks took (hs_replay.h: the back-to-front walk)
        const int trips = take_lists<KB>(tc, s_actb, s_list);
        const uint16_t* const my_list = s_list[tc.wave][tc.grp];
#pragma unroll 1
        for (int ti = 0; ti < trips; ++ti) {
            const BackEntry e = back_entry(tc, s_a, s_b, (int)my_list[ti], base, last0, last1);
            const float4 a = e.a, b = e.b, c = s_c[e.j];
            // ---- the backward's step (render.hip, step_bwd_pair): inactive pixels keep their state exactly ----
            const BackStep st = e.step(T);
            T = st.T;
            f2 cd = (splat(b.z) * dL0 + splat(b.w) * dL1) + splat(c.x) * dL2;  // c_i . dL
            if constexpr (DEPTH) cd += splat(c.y) * dLd;
            const f2 diff = cd - q;
            const f2 gd = e.G * (diff * T);
            q += st.ae * diff;
            const f2 dop = {e.act0 ? gd.x : 0.f, e.act1 ? gd.y : 0.f};  // select AFTER the product (G may be inf at a skipped pixel)
            const f2 sw = splat(b.y) * dop;
            // ---- the pixel's terms, in the staged conic's units: 2 A2 dx + B2 dy and 2 C2 dy + B2 dx ----
            const f2 vx = splat(2.f * a.z * e.dx) + splat(a.w) * e.dy;
            const f2 vy = splat(2.f * b.x) * e.dy + splat(e.u);
            const f2 mx = vx * sw, my = vy * sw;
            float ax = (e.act0 ? fabsf(mx.x) : 0.f) + (e.act1 ? fabsf(mx.y) : 0.f);
            float ay = (e.act0 ? fabsf(my.x) : 0.f) + (e.act1 ? fabsf(my.y) : 0.f);
            ax = group_sum(ax);
            ay = group_sum(ay);
            // did a pixel of this lane group composite the entry?  (the forward's activity bit also covers the entry that
            // terminated a pixel, which is not composited)
            const uint64_t anym = __ballot(e.act0 || e.act1);
            const bool any = (uint32_t)(anym >> (32 * tc.grp)) != 0u;
            // one lane per group, a plain LDS store into the group's own plane of its own entry (the sentinel's is scratch)
            if ((lane & 31) == 31) s_part[e.j][plane] = any ? make_float2(ax, ay) : empty_record();
        }
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            AbsAcc o = planes_combined<AbsAcc>(act, s_part[threadIdx.x]);
            o.sx *= kx; o.sy *= ky;
            const float4 a = s_a[threadIdx.x], c = s_c[threadIdx.x];
            const int64_t slot = pair_slot(p, a.x, a.y, __float_as_int(c.z), __float_as_uint(c.w), tc.tx, tc.ty);
            if (slot >= 0 && slot < p.capacity) p.pair_rec[slot] = o.row();
        }
    }
    write_untaken(p, tc, n_proc, kAThreads, p.pair_rec, empty_record());
}

__global__ void __launch_bounds__(256) absgrad_segsum_kernel(Segsum<float2> a) { segsum_rows<AbsAcc>(a); }

// One thread per Gaussian, frames in ascending order: the rows of the frame's poses added in ascending pose order, then
// abs_grad_accum += sqrt(a_x^2 + a_y^2) -- a call over F frames leaves what F single-frame calls leave.  A frame in which no
// term took part leaves the value alone, bit for bit; an overflowed call adds nothing at all.
__global__ void __launch_bounds__(256) absgrad_fold_kernel(int P, int N, int F, const hs_counters* counters, const float2* inst_rows,
                                                           float* abs_grad_accum) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P || counters->overflow) return;
    float acc = abs_grad_accum[g];
    bool wrote = false;
    for (int f = 0; f < F; ++f) {
        float ax = 0.f, ay = 0.f;
        bool any = false;
        for (int k = 0; k < N; ++k) {
            const float2 v = inst_rows[(int64_t)(f * N + k) * P + g];
            if (has_term(v)) { ax += v.x; ay += v.y; any = true; }
        }
        if (any) { acc += sqrtf(ax * ax + ay * ay); wrote = true; }
    }
    if (wrote) abs_grad_accum[g] = acc;
}

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

HS_API int64_t hs_abs_gradient_workspace_bytes(const hs_dims* dims) {
    const char* fn = "hs_abs_gradient_workspace_bytes";
    hs_sizes sz;
    if (check_args(fn, dims) || hs_plan(dims, &sz, nullptr) != HS_OK) return HS_EINVAL;
    return replay_workspace_bytes(*dims, sizeof(AbsAcc::Rec));
}

HS_API int hs_abs_gradient(const hs_abs_gradient_args* a, void* hip_stream) {
    const char* fn = "hs_abs_gradient";
    if (check_args(fn, a)) return HS_EINVAL;
    hs_sizes sz; hs_layout L;
    if (hs_plan(&a->dims, &sz, &L) != HS_OK) return HS_EINVAL;   // (the text names what hs_plan refused)
    const hs_dims& d = a->dims;
    if (frames_of(d) > 1 && (a->dL_dout_alpha || a->dL_dout_invdepth)) {
        set_error("%s: dL_dout_alpha / dL_dout_invdepth are per-image gradients and are not supported with n_frames=%d", fn,
                  d.n_frames);
        return HS_EINVAL;
    }
    if ((a->flags & HS_FLAG_HDR) && (!a->exposure || !a->crf_table || a->crf_K < 2 || a->crf_K > 4096 || d.crf_K != a->crf_K)) {
        set_error("%s: HDR needs exposure, crf_table and dims.crf_K == crf_K", fn);
        return HS_EINVAL;
    }
    if (d.P == 0) return HS_OK;   // (no pointer is looked at, nothing is launched)
    const Field f[] = {{a->bg, "bg", 4}, {a->geom, "geom", 256}, {a->binning, "binning", 256}, {a->image, "image", 256},
                       {a->ws, "ws", 256}, {a->dL_dout_color, "dL_dout_color", 4}, {a->abs_grad_accum, "abs_grad_accum", 4}};
    int rc = check_fields(fn, f, 7);
    if (rc != HS_OK) return rc;
    if ((rc = check_aligned(fn, a->dL_dout_hdr, "dL_dout_hdr", 4)) != HS_OK) return rc;
    if ((rc = check_aligned(fn, a->dL_dout_alpha, "dL_dout_alpha", 4)) != HS_OK) return rc;
    if ((rc = check_aligned(fn, a->dL_dout_invdepth, "dL_dout_invdepth", 4)) != HS_OK) return rc;
    if ((rc = check_aligned(fn, a->exposure, "exposure", 4)) != HS_OK) return rc;
    if ((rc = check_aligned(fn, a->crf_table, "crf_table", 4)) != HS_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;

    Replay p;
    static_cast<ReplayFrame&>(p) = replay_frame(d, L, a->geom, a->binning, a->image);
    const Segsum<float2> sg = replay_segsum<float2>(p, d, L, a->binning, a->ws);
    p.flags = a->flags; p.bg = a->bg;
    p.final_T = (const float*)((const char*)a->image + L.final_T); p.pose_hdr = (const float*)((const char*)a->image + L.pose_hdr);
    p.dL_dcolor = a->dL_dout_color; p.dL_dhdr = a->dL_dout_hdr; p.dL_dalpha = a->dL_dout_alpha;
    p.dL_dinvdepth = a->dL_dout_invdepth;
    p.crf.table = a->crf_table; p.crf.K = a->crf_K; p.crf.umin = a->crf_umin; p.crf.umax = a->crf_umax; p.crf.dt = 1.f;
    p.exposure = a->exposure;
    p.pair_rec = sg.pair_rec;
    if (a->dL_dout_invdepth) absgrad_replay_kernel<true><<<p.ntiles * d.n_poses, kAThreads, 0, s>>>(p);
    else absgrad_replay_kernel<false><<<p.ntiles * d.n_poses, kAThreads, 0, s>>>(p);
    HS_LAUNCH_CHECK();

    absgrad_segsum_kernel<<<ceil_div(4 * p.I, 256), 256, 0, s>>>(sg);
    HS_LAUNCH_CHECK();

    absgrad_fold_kernel<<<ceil_div(d.P, 256), 256, 0, s>>>(d.P, p.N, p.F, p.counters, sg.inst_rows, a->abs_grad_accum);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
