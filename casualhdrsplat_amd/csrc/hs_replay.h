// Shared by the units that REPLAY a finished render to keep a per-Gaussian statistic that exists only inside the compositing
// loop: contrib.hip (blending weights, front to back) and absgrad.hip (AbsGS, back to front) -- and by features.hip, which
// composites further per-Gaussian channels with those weights, and featgeo.hip, the backward of that compositing to the
// geometry (back to front), and distort.hip, the depth-distortion loss of the blending weights (both directions).  A replay has to reproduce the
// forward's decisions bit for bit, and this header is the ONE restatement of them outside render.hip: the pixel mapping, the
// XCD strip map, the staged conic, the alpha expressions and thresholds, the pair_act bits, the walk bound, the pair slots, and around them
// what every replay is built from -- the frame part of the kernel argument, the per-workgroup tile context, the records
// behind the deepest contributor, the per-instance segmented sum and the workspace layout.
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

// ---- the forward's alpha of a staged entry (a = {x, y, A2, B2}, b.x = C2, b.y = opacity, after scale_entry) at the lane's
// pixel pair: the forward's expressions in the forward's operand order (as render.hip's blend_fwd_pair) ----
struct PairAlpha { f2 pw; float al0, al1; };

__device__ __forceinline__ PairAlpha pair_alpha(const TileCtx& c, const float4 a, const float4 b) {
    PairAlpha r;
    const float dx = a.x - c.pxf;
    const f2 dy = a.y - c.pyf;
    const float t = a.z * dx * dx, u = a.w * dx;
    r.pw = dy * (b.x * dy + u) + t;
    r.al0 = fminf(kAlphaMax, b.y * hs_exp2(r.pw.x));
    r.al1 = fminf(kAlphaMax, b.y * hs_exp2(r.pw.y));
    return r;
}
// The three tests of blend_fwd_pair at one pixel: power <= 0, alpha >= 1/255, and "before the entry at which
// T (1 - alpha) < 1e-4 ends the pixel" -- the forward's own answer to the third is n_contrib (`last`); `on`: the lane's
// block took the entry (pair_act: the forward evaluated it there)
__device__ __forceinline__ bool composited(bool on, uint32_t idx, uint32_t last, float pw, float al) {
    return on && idx < last && pw <= 0.f && al >= kAlphaMin;
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
        const uint32_t id = min(p.point_list[c.range.x + i], (uint32_t)(p.I - 1));
        const float4* r = p.rec + kRecF4 * (int64_t)id;
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
