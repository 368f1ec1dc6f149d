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
// see the bits the forward's saw; the expressions are the forward's and the backward's, operand for operand.  The helpers
// marked "as render.hip" are restated here because that unit keeps them in its anonymous namespace and must not change.  Of
// hs_cloud.h only the host-side argument checks are used.
#include "hs_cloud.h"

namespace hs {
namespace {

constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr float kAlphaMax = 0.99f;
constexpr float kLogEps = 1e-8f;
constexpr float kLog2e = 1.4426950408889634f;
constexpr int kAThreads = 128;       // threads per workgroup: two waves, one per half tile
// staged entries per batch (a multiple of 64, at most the threads).  Measured, whole call, two runs each: 128 entries 0.482 /
// 0.481 ms at 1 M Gaussians / 1080p and 0.157 / 0.159 ms at 100 k / 800 x 800; 64 entries (half the LDS) 0.469 / 0.471 and
// 0.163 / 0.164 ms -- a wash.  Reading the next trip's record a trip ahead costs 14 registers and a wave per SIMD: 0.494 ms.
constexpr int kABatch = 128;

static_assert(kABatch % 64 == 0 && kABatch <= kAThreads, "the lists are built from whole ballots, one entry is staged per thread");

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
__device__ __forceinline__ f2 splat(float v) { f2 r = {v, v}; return r; }
// number of set bits of a wave-uniform 64-bit mask below this lane
__device__ __forceinline__ int mask_prefix(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

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

// ---- sum over the 32 lanes of a lane group (rows 2g, 2g + 1 of the wave): a fixed DPP tree -- the four in-row steps leave
// every lane of a row with the row's total, row_bcast:15 then brings the first row's into the second.  Valid in lanes
// 16..31 (group 0) and 48..63 (group 1); the other rows hold scratch.  Needs a full exec mask.  (As contrib.hip.)
__device__ __forceinline__ float group_sum(float v) {
    v += dpp_f32<0xB1>(v);        // quad_perm [1,0,3,2]
    v += dpp_f32<0x4E>(v);        // quad_perm [2,3,0,1]
    v += dpp_f32<0x141>(v);       // row_half_mirror
    v += dpp_f32<0x140>(v);       // row_mirror
    v += dpp_f32<0x142, 0xA>(v);  // row_bcast:15 -> rows 1,3
    return v;
}

struct Replay {
    int W, H, gx, gy, ntiles, N, F, flags;   // N: poses per FRAME, F: frames (the launch covers F x N poses)
    int64_t capacity, I;                     // pair slots; instances (poses x Gaussians)
    const hs_counters* counters;
    const uint2* ranges; const uint32_t* point_list; const float4* rec; const float* bg;
    const float* final_T; const uint32_t* n_contrib; const float* pose_hdr;
    const float* dL_dcolor; const float* dL_dhdr; const float* dL_dalpha; const float* dL_dinvdepth;
    const uint8_t* pair_act;
    Crf crf;
    const float* exposure;
    float2* pair_rec;                        // out: one record per pair slot
};

// the record of a pair (the row of an instance) no pixel composited: sums of magnitudes are never negative
__device__ __forceinline__ float2 empty_record() { return make_float2(-1.f, -1.f); }
__device__ __forceinline__ bool has_term(float2 v) { return !(v.x < 0.f); }

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

// slot of the (tile, instance) pair in duplicateWithKeys order: the arithmetic of render_bwd_kernel's write-out (integer
// adds and float divides by a power of two: contraction cannot change it)
__device__ __forceinline__ int64_t pair_slot(const Replay& p, float x, float y, int rad, uint32_t off, int tx, int ty) {
    const int rminx = min(p.gx, max(0, (int)((x - (float)rad) / (float)kTile)));
    const int rminy = min(p.gy, max(0, (int)((y - (float)rad) / (float)kTile)));
    const int rmaxx = min(p.gx, max(0, (int)((x + (float)rad + (float)(kTile - 1)) / (float)kTile)));
    return (int64_t)off + (int64_t)(ty - rminy) * (rmaxx - rminx) + (tx - rminx);
}

template <bool DEPTH>
__global__ void __launch_bounds__(kAThreads) absgrad_replay_kernel(Replay p) {
    constexpr int KB = kABatch;
    constexpr int kListLen = KB + 8;
    // (record KB of the staging arrays: the sentinel, opacity 0 -- nobody composites it; it pads the shorter list of a wave)
    __shared__ float4 s_a[KB + 1];        // {x, y, A2, B2}
    __shared__ float4 s_b[KB + 1];        // {C2, opacity, r, g}
    __shared__ float4 s_c[KB + 1];        // {b, 1 / depth (DEPTH) or depth, radius (int bits), slot start (uint bits)}
    __shared__ float2 s_part[KB + 1][4];  // plane 2g + w: the totals of lane group g of wave w, stored by that group alone
    __shared__ uint8_t s_actb[kAThreads]; // activity byte of each staged entry (bit 2g + w)
    __shared__ uint16_t s_list[2][2][kListLen];   // [wave][lane group]: the group's takers among the staged entries, back to front
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

    const int frame = p.F > 1 ? pose / p.N : 0;
    PixB s0, s1;
    load_pixel_bwd(p, s0, in0, pose, frame, px, py0);
    load_pixel_bwd(p, s1, in1, pose, frame, px, py1);
    f2 T = {s0.T, s1.T}, q = {s0.q, s1.q};
    const f2 dL0 = {s0.dL0, s1.dL0}, dL1 = {s0.dL1, s1.dL1}, dL2 = {s0.dL2, s1.dL2}, dLd = {s0.dLd, s1.dLd};
    const uint32_t last0 = s0.last, last1 = s1.last;

    // the walk's bound: the tile's deepest contributor (pair_act is written for the entries the forward staged, and it
    // staged at least these); never more than the list holds
    const uint32_t wave_max = wave_max_u32(max(last0, last1));
    if (lane == 0) s_max[wave] = wave_max;
    if (threadIdx.x == 0) {
        s_a[KB] = make_float4(0.f, 0.f, 0.f, 0.f); s_b[KB] = make_float4(0.f, 0.f, 0.f, 0.f); s_c[KB] = make_float4(0.f, 1.f, 0.f, 0.f);
    }
    __syncthreads();
    const int n_proc = min(n, (int)max(s_max[0], s_max[1]));

    const uint16_t* const my_list = s_list[wave][grp];
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
            const uint32_t id = min(p.point_list[range.x + base + threadIdx.x], (uint32_t)(p.I - 1));
            act = p.pair_act[(int64_t)range.x + base + threadIdx.x];
            const float4* r = p.rec + kRecF4 * (int64_t)id;
            float4 ra = r[0], rb = r[1];
            float4 rc = r[2];
            if constexpr (DEPTH) rc.y = 1.f / rc.y;  // depth -> inverse depth
            scale_entry(ra, rb);
            s_a[threadIdx.x] = ra;
            s_b[threadIdx.x] = rb;
            s_c[threadIdx.x] = rc;
        }
        s_actb[threadIdx.x] = (uint8_t)act;
        __syncthreads();
        // The two lists of this wave (as render_bwd_kernel): group g's takers among the staged entries (bit 2g + wave of the
        // activity bytes), back to front, then sentinels up to the longer list's length.  The two 32-lane groups walk their
        // lists in lock step, each reading its OWN entry: one trip serves up to two different entries, and an entry is
        // visited only by the blocks that took it.  Wave-private LDS rows: no barrier needed.  The loop is uniform over the
        // wave (exec stays full: the DPP steps read every lane).
        int maxn = 0;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint32_t gbit = 1u << (2 * g + wave);
            uint16_t* lst = s_list[wave][g];
            int n_g = 0;
#pragma unroll
            for (int k = KB / 64 - 1; k >= 0; --k) {   // upper half of the batch first: it is deeper
                const uint64_t m = __ballot((s_actb[k * 64 + lane] & gbit) != 0);
                const int c = __popcll(m);
                if ((m >> lane) & 1ull) lst[n_g + c - 1 - mask_prefix(m)] = (uint16_t)(k * 64 + lane);
                n_g += c;
            }
#pragma unroll
            for (int t = lane; t < kListLen; t += 64)
                if (t >= n_g) lst[t] = (uint16_t)KB;
            maxn = max(maxn, n_g);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int ti = 0; ti < maxn; ++ti) {
            const int j = (int)my_list[ti];            // (two addresses per wave: one per group)
            const float4 a = s_a[j];
            const float4 b = s_b[j];
            const float4 c = s_c[j];
            // ---- the forward's alpha: same expressions, same operand order ----
            const float dx = a.x - pxf;
            const f2 dy = a.y - pyf;
            const float t = a.z * dx * dx, u = a.w * dx;
            const f2 pw = dy * (b.x * dy + u) + t;
            const f2 G = {hs_exp2(pw.x), hs_exp2(pw.y)};
            const f2 alpha = {fminf(kAlphaMax, b.y * G.x), fminf(kAlphaMax, b.y * G.y)};
            // (the sentinel passes the index test for pixels that reach past the batch: its opacity 0 is what keeps it out)
            const uint32_t idx = (uint32_t)(base + j);
            const bool act0 = idx < last0 && pw.x <= 0.f && alpha.x >= kAlphaMin;
            const bool act1 = idx < last1 && pw.y <= 0.f && alpha.y >= kAlphaMin;
            // ---- the backward's step (render.hip, step_bwd_pair): inactive pixels keep their state exactly ----
            const f2 ae = {act0 ? alpha.x : 0.f, act1 ? alpha.y : 0.f};
            const f2 one_m = splat(1.f) - ae;
            const f2 rcp = {__builtin_amdgcn_rcpf(one_m.x), __builtin_amdgcn_rcpf(one_m.y)};
            T *= rcp;  // T_i = T_{i+1} / (1 - alpha_i)
            f2 cd = (splat(b.z) * dL0 + splat(b.w) * dL1) + splat(c.x) * dL2;  // c_i . dL
            if constexpr (DEPTH) cd += splat(c.y) * dLd;
            const f2 diff = cd - q;
            const f2 gd = G * (diff * T);
            q += ae * diff;
            const f2 dop = {act0 ? gd.x : 0.f, act1 ? gd.y : 0.f};  // select AFTER the product (G may be inf at a skipped pixel)
            const f2 sw = splat(b.y) * dop;
            // ---- the pixel's terms, in the staged conic's units: 2 A2 dx + B2 dy and 2 C2 dy + B2 dx ----
            const f2 vx = splat(2.f * a.z * dx) + splat(a.w) * dy;
            const f2 vy = splat(2.f * b.x) * dy + splat(u);
            const f2 mx = vx * sw, my = vy * sw;
            float ax = (act0 ? fabsf(mx.x) : 0.f) + (act1 ? fabsf(mx.y) : 0.f);
            float ay = (act0 ? fabsf(my.x) : 0.f) + (act1 ? fabsf(my.y) : 0.f);
            ax = group_sum(ax);
            ay = group_sum(ay);
            // did a pixel of this lane group composite the entry?  (the forward's activity bit also covers the entry that
            // terminated a pixel, which is not composited)
            const uint64_t anym = __ballot(act0 || act1);
            const bool any = (uint32_t)(anym >> (32 * grp)) != 0u;
            // one lane per group, a plain LDS store into the group's own plane of its own entry (the sentinel's is scratch)
            if ((lane & 31) == 31) s_part[j][2 * grp + wave] = any ? make_float2(ax, ay) : empty_record();
        }
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            // the planes the entry's takers wrote (its activity bits), added in plane order
            float2 o = make_float2(0.f, 0.f);
            bool any = false;
#pragma unroll
            for (int pl = 0; pl < 4; ++pl) {
                if ((act >> pl) & 1u) {
                    const float2 v = s_part[threadIdx.x][pl];
                    if (has_term(v)) { o.x += v.x; o.y += v.y; any = true; }
                }
            }
            o.x *= kx; o.y *= ky;
            if (!any) o = empty_record();
            const float4 a = s_a[threadIdx.x], c = s_c[threadIdx.x];
            const int64_t slot = pair_slot(p, a.x, a.y, __float_as_int(c.z), __float_as_uint(c.w), tx, ty);
            if (slot >= 0 && slot < p.capacity) p.pair_rec[slot] = o;
        }
    }
    // the entries behind the tile's deepest contributor: nobody took them
    for (int i = n_proc + (int)threadIdx.x; i < n; i += kAThreads) {
        const uint32_t id = min(p.point_list[range.x + i], (uint32_t)(p.I - 1));
        const float4* r = p.rec + kRecF4 * (int64_t)id;
        const float4 ra = r[0], rc = r[2];
        const int64_t slot = pair_slot(p, ra.x, ra.y, __float_as_int(rc.z), __float_as_uint(rc.w), tx, ty);
        if (slot >= 0 && slot < p.capacity) p.pair_rec[slot] = empty_record();
    }
}

struct Segsum {
    int64_t I, capacity;
    const uint32_t* inst_sorted; const uint32_t* offs_sorted; const hs_counters* counters;
    const float2* pair_rec; float2* inst_rows;
};

// Thread t: instance t >> 2 (in depth order), quad lane t & 3 -- lane q combines records beg + q, beg + q + 4, ... in slot
// order, the four partial results meet in a fixed butterfly (as contrib_segsum_kernel).
__global__ void __launch_bounds__(256) absgrad_segsum_kernel(Segsum a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = t >> 2;
    const int q = (int)(t & 3);
    // binning overflow: nothing was emitted or rendered, and slots past the capacity do not exist
    const bool valid = i < a.I && !a.counters->overflow;
    const uint32_t beg = valid ? (i == 0 ? 0u : a.offs_sorted[i - 1]) : 0u;
    uint32_t end = valid ? a.offs_sorted[i] : 0u;
    if ((int64_t)end > a.capacity) end = (uint32_t)a.capacity;
    float sx = 0.f, sy = 0.f;
    int any = 0;
    for (uint32_t s = beg + q; s < end; s += 4) {
        const float2 v = a.pair_rec[(int64_t)s];
        if (has_term(v)) { sx += v.x; sy += v.y; any = 1; }
    }
    sx += __shfl_xor(sx, 1); sx += __shfl_xor(sx, 2);
    sy += __shfl_xor(sy, 1); sy += __shfl_xor(sy, 2);
    any |= __shfl_xor(any, 1); any |= __shfl_xor(any, 2);
    if (i < a.I && q == 0) {
        // (a depth sort that gave up -- overflow = 2 -- left no instance list: the empty row goes to row i)
        const int64_t inst = a.counters->overflow ? i : (int64_t)a.inst_sorted[i];
        if (inst < a.I) a.inst_rows[inst] = any ? make_float2(sx, sy) : empty_record();
    }
}

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

// workspace: pair records [capacity] | instance rows [P * n_poses], 8 bytes each, both 256-byte aligned
int64_t pair_rec_bytes(const hs_dims& d) { return align_up(d.capacity * 8, 256); }
int64_t inst_row_bytes(const hs_dims& d) { return align_up((int64_t)d.P * d.n_poses * 8, 256); }

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

HS_API int64_t hs_abs_gradient_workspace_bytes(const hs_dims* dims) {
    const char* fn = "hs_abs_gradient_workspace_bytes";
    hs_sizes sz;
    if (check_args(fn, dims) || hs_plan(dims, &sz, nullptr) != HS_OK) return HS_EINVAL;
    const int64_t bytes = pair_rec_bytes(*dims) + inst_row_bytes(*dims);
    return bytes > 0 ? bytes : 256;
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
    const char* geom = (const char*)a->geom; const char* bin = (const char*)a->binning; const char* img = (const char*)a->image;
    const hs_counters* counters = (const hs_counters*)(geom + L.counters);
    float2* pair_rec = (float2*)a->ws;
    float2* inst_rows = (float2*)((char*)a->ws + pair_rec_bytes(d));
    const int64_t I = (int64_t)d.P * d.n_poses;

    Replay p;
    p.W = d.W; p.H = d.H; p.gx = (d.W + kTile - 1) / kTile; p.gy = (d.H + kTile - 1) / kTile;
    p.ntiles = p.gx * p.gy; p.F = frames_of(d); p.N = d.n_poses / p.F; p.flags = a->flags;
    p.capacity = d.capacity; p.I = I; p.counters = counters;
    p.ranges = (const uint2*)(bin + L.ranges); p.point_list = (const uint32_t*)(bin + L.point_list);
    p.rec = (const float4*)(geom + L.rec); p.bg = a->bg;
    p.final_T = (const float*)(img + L.final_T); p.n_contrib = (const uint32_t*)(img + L.n_contrib);
    p.pose_hdr = (const float*)(img + L.pose_hdr);
    p.dL_dcolor = a->dL_dout_color; p.dL_dhdr = a->dL_dout_hdr; p.dL_dalpha = a->dL_dout_alpha;
    p.dL_dinvdepth = a->dL_dout_invdepth;
    p.pair_act = (const uint8_t*)bin + L.pair_act;
    p.crf.table = a->crf_table; p.crf.K = a->crf_K; p.crf.umin = a->crf_umin; p.crf.umax = a->crf_umax; p.crf.dt = 1.f;
    p.exposure = a->exposure;
    p.pair_rec = pair_rec;
    if (a->dL_dout_invdepth) absgrad_replay_kernel<true><<<p.ntiles * d.n_poses, kAThreads, 0, s>>>(p);
    else absgrad_replay_kernel<false><<<p.ntiles * d.n_poses, kAThreads, 0, s>>>(p);
    HS_LAUNCH_CHECK();

    Segsum sg;
    sg.I = I; sg.capacity = d.capacity;
    sg.inst_sorted = (const uint32_t*)(bin + L.inst_sorted); sg.offs_sorted = (const uint32_t*)(bin + L.offs_sorted);
    sg.counters = counters; sg.pair_rec = pair_rec; sg.inst_rows = inst_rows;
    absgrad_segsum_kernel<<<ceil_div(4 * I, 256), 256, 0, s>>>(sg);
    HS_LAUNCH_CHECK();

    absgrad_fold_kernel<<<ceil_div(d.P, 256), 256, 0, s>>>(d.P, p.N, p.F, counters, inst_rows, a->abs_grad_accum);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
