// Shared by the units that REPLAY a finished render to compute something that exists only inside the compositing loop:
// contrib.hip (blending-weight statistics), absgrad.hip (AbsGS), features.hip (feature compositing, forward and backward to
// the features), featgeo.hip (its backward to the geometry) and distort.hip (depth-distortion loss, forward and backward).
// A replay has to reproduce the forward's decisions bit for bit, and this header is the ONE restatement of them outside
// render.hip.  It owns
//   - the pixel mapping, the XCD strip map, the staged conic (scale_entry), the alpha expression and the thresholds
//     (pair_alpha, composited), the pair_act bits, the walk bound and the pair slots;
//   - how a replay reads the tile's list: entry_id (the id clamp) and Staged (id, activity byte, record);
//   - the two walks of a staged batch: walk_front (front to back: every entry one of the wave's blocks took, alpha, the tests,
//     T and the blending weight, then the unit's callable) and the back-to-front walk (take_lists: the wave's two take-lists
//     and the sentinel; back_entry: alpha and the tests; BackEntry::step: the T recursion); a unit computes what it alone keeps;
//   - what becomes of a block's totals: planes_combined (the LDS planes of an entry's takers, in plane order), and for the
//     units that deliver gradients to the geometry geo_sums / geo_record / write_geo_record (the six sums and the backward's
//     pair record);
//   - stage_feature_row, and around them what every replay is built from: the frame part of the kernel argument, the
//     per-workgroup tile context, the records behind the deepest contributor, the per-instance segmented sum and the
//     workspace layout.
// A unit keeps its kernels, its LDS arrays (the layouts differ), its batch loop and what it computes per entry.
//
// render.hip is the ORIGINAL of everything marked "as render.hip" below and keeps its own copy in its anonymous namespace: a
// change there must be mirrored here, expression for expression, in the same operand order.  (render.hip could include this
// header instead in a change that also re-collects the profiles tied to its source hash.)
//
// The including units are compiled like render.hip (FMA contraction on: the Makefile's FAST_TUS), so that the threshold
// tests see the bits the forward's saw.  Of hs_cloud.h only the host-side argument checks are used.
#pragma once
#include "hs_cloud.h"

namespace hs {

// ---- as render.hip ----
constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr float kAlphaMax = 0.99f;
constexpr float kLog2e = 1.4426950408889634f;

typedef float f2 __attribute__((ext_vector_type(2)));

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

// ---- sum over the 32 lanes of a lane group (rows 2g, 2g + 1 of the wave): a fixed DPP tree -- the four in-row steps leave
// every lane of a row with the row's total, row_bcast:15 then brings the first row's into the second.  Valid in lanes
// 16..31 (group 0) and 48..63 (group 1); the other rows hold scratch.  Needs a full exec mask.
__device__ __forceinline__ float group_sum(float v) {
    v += dpp_f32<0xB1>(v);        // quad_perm [1,0,3,2]
    v += dpp_f32<0x4E>(v);        // quad_perm [2,3,0,1]
    v += dpp_f32<0x141>(v);       // row_half_mirror
    v += dpp_f32<0x140>(v);       // row_mirror
    v += dpp_f32<0x142, 0xA>(v);  // row_bcast:15 -> rows 1,3
    return v;
}

// ---- pair_act (hdrsplat.h, hs_layout): bit 2g + w of an entry's byte = the 8 x 8 block of lane group g of wave w took it.
// A replay keeps one LDS plane per block under the same number.
__device__ __forceinline__ int act_plane(int grp, int wave) { return 2 * grp + wave; }
__device__ __forceinline__ uint32_t wave_act_bits(int wave) { return 5u << wave; }   // the two blocks of a wave

// ---- the frame part of a replay's kernel argument; a unit's own struct derives from it and adds what it alone reads ----
struct ReplayFrame {
    int W, H, gx, gy, ntiles, N, F;   // N: poses per FRAME, F: frames (the launch covers F x N poses)
    int64_t capacity, I;              // pair slots; instances (poses x Gaussians)
    // overflow != 0: the frame was rendered empty (its ranges are cleared) and adds NOTHING -- the replay kernel returns at
    // once, the segmented sum reads no record and the unit's fold leaves the caller's arrays alone
    const hs_counters* counters;
    const uint2* ranges; const uint32_t* point_list; const float4* rec;
    const uint32_t* n_contrib; const uint8_t* pair_act;
};

static inline ReplayFrame replay_frame(const hs_dims& d, const hs_layout& L, const void* geom_ws, const void* binning_ws,
                                       const void* image_ws) {
    const char* geom = (const char*)geom_ws; const char* bin = (const char*)binning_ws; const char* img = (const char*)image_ws;
    ReplayFrame p;
    p.W = d.W; p.H = d.H; p.gx = (d.W + kTile - 1) / kTile; p.gy = (d.H + kTile - 1) / kTile;
    p.ntiles = p.gx * p.gy; p.F = frames_of(d); p.N = d.n_poses / p.F;
    p.capacity = d.capacity; p.I = (int64_t)d.P * d.n_poses;
    p.counters = (const hs_counters*)(geom + L.counters);
    p.ranges = (const uint2*)(bin + L.ranges); p.point_list = (const uint32_t*)(bin + L.point_list);
    p.rec = (const float4*)(geom + L.rec);
    p.n_contrib = (const uint32_t*)(img + L.n_contrib);
    p.pair_act = (const uint8_t*)bin + L.pair_act;
    return p;
}

// ---- what a workgroup of a replay kernel (128 threads, one per (pose, tile), the forward's grid) knows about its tile ----
struct TileCtx {
    int vt, pose, frame;      // virtual tile = pose * ntiles + tile
    int tx, ty, wave, lane, grp;
    int px, py0, py1;         // the lane's pixel pair
    bool in0, in1;            // ... inside the image
    float pxf; f2 pyf;
    uint2 range; int n;       // the tile's list in point_list / pair_act, its length
};

__device__ __forceinline__ TileCtx tile_context(const ReplayFrame& p) {
    TileCtx c;
    c.vt = xcd_strip_tile(blockIdx.x, gridDim.x, p.gx);
    c.pose = c.vt / p.ntiles;
    const int tile = c.vt - c.pose * p.ntiles;
    c.tx = tile % p.gx; c.ty = tile / p.gx;
    c.wave = threadIdx.x >> 6; c.lane = threadIdx.x & 63;
    c.grp = c.lane >> 5;
    const int sx = c.tx * kTile, sy = c.ty * kTile + c.wave * 8;
    lane_pixels(c.lane, sx, sy, c.px, c.py0);
    c.py1 = c.py0 + 1;
    c.in0 = c.px < p.W && c.py0 < p.H; c.in1 = c.px < p.W && c.py1 < p.H;
    c.pxf = (float)c.px;
    c.pyf = f2{(float)c.py0, (float)c.py1};
    c.range = p.ranges[c.vt];
    // (a list lies inside the sorted pairs; anything else is not a state hs_forward left, and is walked as empty)
    c.n = (c.range.y >= c.range.x && (int64_t)c.range.y <= p.capacity) ? (int)(c.range.y - c.range.x) : 0;
    c.frame = p.F > 1 ? c.pose / p.N : 0;
    return c;
}

// ---- how a replay reads its tile's list ----
// the instance of entry i of the list (an id past the instances is not one hs_forward left: it reads the last record)
__device__ __forceinline__ uint32_t entry_id(const ReplayFrame& p, const TileCtx& c, int i) {
    return min(p.point_list[c.range.x + i], (uint32_t)(p.I - 1));
}
// Entry base + threadIdx.x as a batch stages it: the three float4 of its render record with the conic scaled (ra = {x, y, A2,
// B2}, rb = {C2, opacity, r, g}, rc = {b, depth, radius (int bits), slot start (uint bits)}), its activity byte and its
// instance.  What goes where in LDS is the unit's; a part it does not store is not loaded.
struct Staged {
    float4 ra, rb, rc;
    uint32_t act, id;
    __device__ __forceinline__ Staged(const ReplayFrame& p, const TileCtx& c, int base) {
        id = entry_id(p, c, base + (int)threadIdx.x);
        act = p.pair_act[(int64_t)c.range.x + base + threadIdx.x];
        const float4* r = p.rec + kRecF4 * (int64_t)id;
        ra = r[0]; rb = r[1]; rc = r[2];
        scale_entry(ra, rb);
    }
};
// The channels [c0, c0 + K) of the entry's Gaussian staged into `dst` (0 past channel C).  vec4: C % 4 == 0 and a 16-byte
// aligned base, rows are read as float4.
template <int K>
__device__ __forceinline__ void stage_feature_row(float (&dst)[K], const float* features, int P, int C, int c0, bool vec4,
                                                  uint32_t id, int pose) {
    // the Gaussian of the instance: instance - pose * P (inside [0, P) for every list hs_forward left)
    const int g = min(max((int)((int64_t)id - (int64_t)pose * P), 0), P - 1);
    const float* row = features + (int64_t)g * C + c0;
    if (vec4) {
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const float4 v = c0 + 4 * q < C ? reinterpret_cast<const float4*>(row)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4*>(dst)[q] = v;
        }
    } else {
#pragma unroll
        for (int c = 0; c < K; ++c) dst[c] = c0 + c < C ? row[c] : 0.f;
    }
}

// ---- the forward's alpha of a staged entry (a = {x, y, A2, B2}, C2, opacity, after scale_entry) at the lane's pixel pair:
// the expressions of render.hip's forward and backward loops in their operand order (as render.hip), with the terms a
// backward step needs beside alpha.  The ONE statement of it in the replay units: both walks call it ----
struct PairAlpha { float dx, u; f2 dy, pw, G, alpha; };

__device__ __forceinline__ PairAlpha pair_alpha(const TileCtx& c, const float4 a, float C2, float opacity) {
    PairAlpha r;
    r.dx = a.x - c.pxf;
    r.dy = a.y - c.pyf;
    const float t = a.z * r.dx * r.dx;
    r.u = a.w * r.dx;
    r.pw = r.dy * (C2 * r.dy + r.u) + t;
    r.G = f2{hs_exp2(r.pw.x), hs_exp2(r.pw.y)};
    r.alpha = f2{fminf(kAlphaMax, opacity * r.G.x), fminf(kAlphaMax, opacity * r.G.y)};
    return r;
}
// The three tests of render.hip's blend_fwd_pair at one pixel: power <= 0, alpha >= 1/255, and "before the entry at which
// T (1 - alpha) < 1e-4 ends the pixel" -- the forward's own answer to the third is n_contrib (`last`).
__device__ __forceinline__ bool composited(uint32_t idx, uint32_t last, float pw, float al) {
    return idx < last && pw <= 0.f && al >= kAlphaMin;
}

// ---- the front-to-back walk of a staged batch of KB entries (s_a = {x, y, A2, B2}, s_b = {C2, opacity, ...}, s_actb the
// activity bytes; entry j of the batch is entry base + j of the list): every entry one of this wave's two blocks took, in
// list order.  Per entry the forward's alpha and tests, the blending weight w = alpha * T and the forward's update of T
// (kept where the pixel does not composite the entry); then f(j, on, act0, act1, w) -- on: this lane's block took the
// entry (the forward evaluated it there), act0 / act1: the lane's two pixels composited it.  f MUST NOT READ T: T is
// updated behind f, so inside f it is still the transmittance in FRONT of the entry (w is all a unit needs of it).  The
// loop is uniform over the wave: exec stays full for the DPP trees of f, LDS reads at j are broadcasts.
template <int KB, class B, class F>
__device__ __forceinline__ void walk_front(const TileCtx& c, const float4* s_a, const B* s_b, const uint8_t* s_actb, int base,
                                           uint32_t last0, uint32_t last1, f2& T, F&& f) {
    const uint32_t gbit = 1u << act_plane(c.grp, c.wave);
    const uint32_t wbits = wave_act_bits(c.wave);
#pragma unroll 1
    for (int k = 0; k < KB / 64; ++k) {
        uint64_t m = __ballot((s_actb[k * 64 + c.lane] & wbits) != 0);
        while (m) {
            const int j = k * 64 + __builtin_ctzll(m);
            m &= m - 1;
            const bool on = (s_actb[j] & gbit) != 0;
            const PairAlpha al = pair_alpha(c, s_a[j], s_b[j].x, s_b[j].y);
            const uint32_t idx = (uint32_t)(base + j);
            const bool act0 = on && composited(idx, last0, al.pw.x, al.alpha.x);
            const bool act1 = on && composited(idx, last1, al.pw.y, al.alpha.y);
            const f2 one = {1.f, 1.f};
            const f2 test_T = T * (one - al.alpha);
            const f2 w = al.alpha * T;
            f(j, on, act0, act1, w);
            // (behind f, not in front: where this select stands among the unit's own statements decides the registers the
            // compiler needs -- DESIGN.md 4.23 has the figures)
            T = f2{act0 ? test_T.x : T.x, act1 ? test_T.y : T.y};
        }
    }
}

// ---- the back-to-front walk of a staged batch.  Each 8 x 8 block (lane group) walks its OWN list of the entries it took
// (bit 2g + wave of the activity bytes), deepest first; the two groups of a wave walk in lock step, each reading its own
// entry, so one trip serves up to two different entries and an entry is visited only by the blocks that took it.  This
// two-lists-per-wave form is the replay's (render.hip's backward walks four lists with one wave).
// THE SENTINEL: record KB of the unit's staging arrays, which the unit fills once with zeros -- opacity 0, so nobody
// composites it (it passes the index test for pixels that reach past the batch) and every sum it adds is zero; whatever
// else the unit reads at an entry needs a value there too.  It pads the shorter list of a wave up to the longer one's
// length; the totals a group stores at j = KB are scratch.
// A unit walks a staged batch like this (T: its per-pixel transmittance, from final_T):
//     const int trips = take_lists<KB>(tc, s_actb, s_list);
//     const uint16_t* const my_list = s_list[tc.wave][tc.grp];
// #pragma unroll 1
//     for (int ti = 0; ti < trips; ++ti) {
//         const BackEntry e = back_entry(tc, s_a, s_b, my_list[ti], base, last0, last1);   // alpha and the three tests
//         const BackStep st = e.step(T);  T = st.T;                                         // the T recursion
//         ... what the unit alone computes; group_sum trees; one lane per group stores into s_part[e.j][plane]
//     }
// THE RULE: the loop statement and the step's call stand in the unit, and every piece takes and returns VALUES.  Per-pixel
// state handed to shared code by reference (a callable that captures it, a step(T&)) is promoted to registers only after
// that code is inlined, and WHERE the step stands among the unit's own statements decides its schedule; either costs
// featgeo.hip's widest kernel registers (DESIGN.md 4.23 has the figures).  The loop is uniform over the wave (exec stays
// full: the DPP trees read every lane).
struct BackStep { f2 ae, T; };   // alpha where the pixel composited the entry, else 0; T in front of the entry
struct BackEntry {
    int j;             // the entry of the batch, KB: the sentinel
    float4 a, b;       // s_a[j], s_b[j]
    float dx, u;       // x - px, B2 dx
    f2 dy, G, alpha;   // y - py; the falloff; the forward's alpha
    bool act0, act1;   // the lane's two pixels composited the entry
    // the step of render.hip's step_bwd_pair on T: T_i = T_{i+1} / (1 - alpha_i) where the pixel composited the entry;
    // elsewhere alpha counts as 0 and T is kept exactly
    __device__ __forceinline__ BackStep step(f2 T) const {
        BackStep s;
        s.ae = f2{act0 ? alpha.x : 0.f, act1 ? alpha.y : 0.f};
        const f2 one_m = splat(1.f) - s.ae;
        const f2 rcp = {__builtin_amdgcn_rcpf(one_m.x), __builtin_amdgcn_rcpf(one_m.y)};
        s.T = T * rcp;
        return s;
    }
};

// The two lists of this wave in s_list[wave]: group g's takers among the KB staged entries, back to front, then sentinels up
// to the row's end.  Returns the trips of the wave: the length of its longer list.  Wave-private LDS rows: a wavefront
// fence, no barrier.
template <int KB>
__device__ __forceinline__ int take_lists(const TileCtx& c, const uint8_t* s_actb, uint16_t (&s_list)[2][2][KB + 8]) {
    constexpr int kListLen = KB + 8;
    int maxn = 0;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const uint32_t gbit = 1u << act_plane(g, c.wave);
        uint16_t* lst = s_list[c.wave][g];
        int n_g = 0;
#pragma unroll
        for (int k = KB / 64 - 1; k >= 0; --k) {   // upper half of the batch first: it is deeper
            const uint64_t m = __ballot((s_actb[k * 64 + c.lane] & gbit) != 0);
            const int n = __popcll(m);
            if ((m >> c.lane) & 1ull) lst[n_g + n - 1 - mask_prefix(m)] = (uint16_t)(k * 64 + c.lane);
            n_g += n;
        }
#pragma unroll
        for (int t = c.lane; t < kListLen; t += 64)
            if (t >= n_g) lst[t] = (uint16_t)KB;
        maxn = max(maxn, n_g);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return maxn;
}
// entry j of the batch (entry base + j of the list; two addresses per wave, one per group) at the lane's pixel pair
__device__ __forceinline__ BackEntry back_entry(const TileCtx& c, const float4* s_a, const float4* s_b, int j, int base,
                                                uint32_t last0, uint32_t last1) {
    BackEntry e;
    e.j = j;
    e.a = s_a[j];
    e.b = s_b[j];
    const PairAlpha al = pair_alpha(c, e.a, e.b.x, e.b.y);
    e.dx = al.dx; e.u = al.u; e.dy = al.dy; e.G = al.G; e.alpha = al.alpha;
    const uint32_t idx = (uint32_t)(base + j);
    e.act0 = composited(idx, last0, al.pw.x, al.alpha.x);
    e.act1 = composited(idx, last1, al.pw.y, al.alpha.y);
    return e;
}

// ---- what becomes of the blocks' totals: the planes the entry's takers wrote (its activity bits; plane 2g + w was stored
// by lane group g of wave w alone), combined in plane order.  Acc: a default-constructed one is empty, take(Part) adds.
template <class Acc, class Part>
__device__ __forceinline__ Acc planes_combined(uint32_t act, const Part (&planes)[4]) {
    Acc o;
#pragma unroll
    for (int pl = 0; pl < 4; ++pl)
        if ((act >> pl) & 1u) o.take(planes[pl]);
    return o;
}

// ---- gradients to the geometry (featgeo.hip, distort.hip): from sw = opacity * dop and dop = G dL/dalpha of the pixel pair
// the six sums of render.hip's backward, S1 = sum w dx, S2 = sum w dy, S3 = sum w dx^2, S4 = sum w dx dy, S5 = sum w dy^2
// and sum dop -- in-lane over the pair (dx is shared), then over the block's 64 pixels by the fixed tree -- into v[0..5]
template <class Part>
__device__ __forceinline__ void geo_sums(Part& tot, const BackEntry& e, f2 sw, f2 dop) {
    const f2 m = sw * e.dy;
    const f2 m2 = m * e.dy;
    const float g0 = (sw.x + sw.y) * e.dx, g1 = m.x + m.y;
    tot.v[0] = group_sum(g0);
    tot.v[1] = group_sum(g1);
    tot.v[2] = group_sum(g0 * e.dx);
    tot.v[3] = group_sum(g1 * e.dx);
    tot.v[4] = group_sum(m2.x + m2.y);
    tot.v[5] = group_sum(dop.x + dop.y);
}
// N sums of an entry over the tile: the accumulator of planes_combined for such parts
template <int N>
struct GeoAcc {
    float v[N];
    __device__ __forceinline__ GeoAcc() {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = 0.f;
    }
    template <class Part>
    __device__ __forceinline__ void take(const Part s) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += s.v[k];
    }
};
// The first six floats of the backward's pair record (hs_layout's pair_grads: kPairF4 float4) from the six sums of a staged
// entry (a = s_a, C2 = s_b.x): the arithmetic of render_bwd_kernel's write-out.
struct GeoRec { float4 r0; float2 r1; };   // {dL/dmean2D x, y, dL/dconic a, b} {dL/dconic c, dL/dopacity}

__device__ __forceinline__ GeoRec geo_record(const ReplayFrame& p, const float4 a, float C2, const float* v) {
    // un-scale the conic: A = A2 * (-2/L), B = B2 * (-1/L), C = C2 * (-2/L)
    const float A = a.z * (-2.f / kLog2e), B = a.w * (-1.f / kLog2e), Cc = C2 * (-2.f / kLog2e);
    const float ddelx_dx = 0.5f * (float)p.W, ddely_dy = 0.5f * (float)p.H;
    // dL/dmean2D = -(A S1 + B S2, C S2 + B S1) (NDC-scaled); dL/dconic = (-0.5 S3, -S4, -0.5 S5)
    const float gmx = -(A * v[0] + B * v[1]) * ddelx_dx;
    const float gmy = -(Cc * v[1] + B * v[0]) * ddely_dy;
    GeoRec r;
    r.r0 = make_float4(gmx, gmy, -0.5f * v[2], -v[3]);
    r.r1 = make_float2(-0.5f * v[4], v[5]);
    return r;
}
// the record at o: the six floats, then no colour gradient (the slots of r, g ...
__device__ __forceinline__ void write_geo_record(float4* o, const GeoRec& r) {
    o[0] = r.r0;
    o[1] = make_float4(r.r1.x, r.r1.y, 0.f, 0.f);
}
// ... and b stay zero) and the inverse depth's slot
__device__ __forceinline__ void write_geo_record_tail(float4* o, float dL_dinvdepth) {
    o[2] = make_float4(0.f, dL_dinvdepth, 0.f, 0.f);
    if constexpr (kPairF4 == 4) o[3] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- the walk's bound: the tile's deepest contributor (n_contrib of its pixels: pair_act is written for the entries the
// forward staged, and it staged at least these); never more than the list holds.  Two halves, a __syncthreads() of the
// caller's between them.
__device__ __forceinline__ void post_wave_depth(uint32_t (&s_max)[2], const TileCtx& c, uint32_t last0, uint32_t last1) {
    const uint32_t wave_max = wave_max_u32(max(last0, last1));
    if (c.lane == 0) s_max[c.wave] = wave_max;
}
__device__ __forceinline__ int walk_bound(const uint32_t (&s_max)[2], const TileCtx& c) {
    return min(c.n, (int)max(s_max[0], s_max[1]));
}

// slot of the (tile, instance) pair in duplicateWithKeys order: the arithmetic of render_bwd_kernel's write-out (integer
// adds and float divides by a power of two: contraction cannot change it)
__device__ __forceinline__ int64_t pair_slot(const ReplayFrame& p, float x, float y, int rad, uint32_t off, int tx, int ty) {
    const int rminx = min(p.gx, max(0, (int)((x - (float)rad) / (float)kTile)));
    const int rminy = min(p.gy, max(0, (int)((y - (float)rad) / (float)kTile)));
    const int rmaxx = min(p.gx, max(0, (int)((x + (float)rad + (float)(kTile - 1)) / (float)kTile)));
    return (int64_t)off + (int64_t)(ty - rminy) * (rmaxx - rminx) + (tx - rminx);
}

// the entries behind the tile's deepest contributor: nobody took them (`stride`: the workgroup's threads)
template <class Rec>
__device__ __forceinline__ void write_untaken(const ReplayFrame& p, const TileCtx& c, int n_proc, int stride, Rec* pair_rec,
                                              Rec empty) {
    for (int i = n_proc + (int)threadIdx.x; i < c.n; i += stride) {
        const float4* r = p.rec + kRecF4 * (int64_t)entry_id(p, c, i);
        const float4 ra = r[0], rc = r[2];
        const int64_t slot = pair_slot(p, ra.x, ra.y, __float_as_int(rc.z), __float_as_uint(rc.w), c.tx, c.ty);
        if (slot >= 0 && slot < p.capacity) pair_rec[slot] = empty;
    }
}

// ---- workspace of a replay: pair records [capacity] | instance rows [P * n_poses], both 256-byte aligned ----
static inline int64_t pair_rec_bytes(const hs_dims& d, int64_t rec_size) { return align_up(d.capacity * rec_size, 256); }
static inline int64_t inst_row_bytes(const hs_dims& d, int64_t rec_size) { return align_up((int64_t)d.P * d.n_poses * rec_size, 256); }
static inline int64_t replay_workspace_bytes(const hs_dims& d, int64_t rec_size) {
    const int64_t bytes = pair_rec_bytes(d, rec_size) + inst_row_bytes(d, rec_size);
    return bytes > 0 ? bytes : 256;
}

// ---- the per-instance segmented sum: the records of an instance's contiguous slots combined into its row ----
template <class Rec>
struct Segsum {
    int64_t I, capacity;
    const uint32_t* inst_sorted; const uint32_t* offs_sorted; const hs_counters* counters;
    Rec* pair_rec; Rec* inst_rows;
};

template <class Rec>
static inline Segsum<Rec> replay_segsum(const ReplayFrame& p, const hs_dims& d, const hs_layout& L, const void* binning_ws, void* ws) {
    const char* bin = (const char*)binning_ws;
    Segsum<Rec> sg;
    sg.I = p.I; sg.capacity = p.capacity;
    sg.inst_sorted = (const uint32_t*)(bin + L.inst_sorted); sg.offs_sorted = (const uint32_t*)(bin + L.offs_sorted);
    sg.counters = p.counters;
    sg.pair_rec = (Rec*)ws; sg.inst_rows = (Rec*)((char*)ws + pair_rec_bytes(d, sizeof(Rec)));
    return sg;
}

// The body of a unit's segsum kernel (256 threads, ceil(4 I / 256) workgroups).  Thread t: instance t >> 2 (in depth order),
// quad lane t & 3 -- lane q combines records beg + q, beg + q + 4, ... in slot order, the four partial results meet in a fixed
// butterfly (as pair_segsum_kernel); one row per instance, every row written.  Acc is the unit's accumulator: Acc::Rec the
// record, a default-constructed Acc the empty one, take(Rec) adds a record, meet(d) the lane's partner across xor d, row()
// gives the record of what was taken.
template <class Acc>
__device__ __forceinline__ void segsum_rows(const Segsum<typename Acc::Rec>& a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = t >> 2;
    const int q = (int)(t & 3);
    // binning overflow: nothing was emitted or rendered, and slots past the capacity do not exist
    const bool valid = i < a.I && !a.counters->overflow;
    const uint32_t beg = valid ? (i == 0 ? 0u : a.offs_sorted[i - 1]) : 0u;
    uint32_t end = valid ? a.offs_sorted[i] : 0u;
    if ((int64_t)end > a.capacity) end = (uint32_t)a.capacity;
    Acc acc;
    for (uint32_t s = beg + q; s < end; s += 4) acc.take(a.pair_rec[(int64_t)s]);
    acc.meet(1); acc.meet(2);
    if (i < a.I && q == 0) {
        // (a depth sort that gave up -- overflow = 2 -- left no instance list: the empty row goes to row i)
        const int64_t inst = a.counters->overflow ? i : (int64_t)a.inst_sorted[i];
        if (inst < a.I) a.inst_rows[inst] = acc.row();
    }
}

}  // namespace hs
