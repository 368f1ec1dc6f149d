// Activations of the STORED cloud (hs_activate, hs_activate_backward; include/hdrsplat.h states the contract): a trainer keeps
// logit opacities, log scales and unnormalised quaternions; the rasterizer takes opacities, scales and unit quaternions.
//
// Two kernels, one launch each, nothing else:
//
//   activate_fwd_kernel   rows [0, P) of whichever of the three tensors are present.  fp32, every operation one correctly
//                         rounded IEEE operation plus the library expf, nothing contracted (this file is compiled with
//                         -ffp-contract=off), denormals kept:
//                             o  = 1 / (1 + expf(-x))
//                             s  = expf(l)                                       per component
//                             n  = max(sqrtf(((q0 q0 + q1 q1) + q2 q2) + q3 q3), 1e-12f)
//                             q^ = q / n                                         four divides
//   activate_bwd_kernel   rows [g_begin, g_end), IN PLACE on the gradient slices: reads the gradient with respect to the
//                         activated value, writes the gradient with respect to the stored one:
//                             g <- (g o) (1 - o)
//                             g <- g s
//                             d  = ((q^0 g0 + q^1 g1) + q^2 g2) + q^3 g3
//                             g <- (g - q^ d) / n        n from the stored q exactly as above;
//                             g <- g / 1e-12f            where the clamp was active (the gradient of q / 1e-12f)
//                         Every element is read and written by the same thread.
//
// Both are streams.  A work item is a QUAD: four consecutive floats of the opacities, four of the scales' 3 P floats, or one
// quaternion.  Where every pointer a tensor's quads touch is 16-byte aligned a quad is one 16-byte access per array, placed on
// the 16-byte grid of the arrays; a quad that lies only partly inside the rows' floats (the two ends of a range), and every
// quad of a tensor with a pointer that is only 4-byte aligned, uses 4-byte accesses of exactly the elements it owns -- no
// byte outside the rows asked for is read or written.  The three tensors are three SEGMENTS of one grid: a workgroup takes
// virtual blocks of 256 quads, finds the segment of each from a prefix table in the kernel arguments, and strides over them
// (the grid is capped at 2048 workgroups).  No LDS, no atomics, no scratch: the same inputs give the same bits.
#include "hs_cloud.h"

#include <math.h>
#include <string.h>

namespace hs {
namespace {

constexpr int kActThreads = 256;
constexpr int kActMaxGrid = 2048;            // 256 CUs x 8 workgroups; larger problems stride
constexpr float kNormEps = 1e-12f;           // torch.nn.functional.normalize's clamp

enum { kActOpacity = 0, kActScale = 1, kActRotation = 2 };

struct ActSeg {
    const float* raw;    // stored values (backward: the rotations only)
    float* act;          // activated values: written by the forward, read by the backward
    float* grad;         // backward: the gradient slice, updated in place
    int64_t lo, hi;      // the floats [lo, hi) of the arrays belong to the rows asked for
    int64_t first;       // first quad: floats [4 first, 4 first + 4)
    int32_t kind, vec;   // vec: 16-byte accesses for quads that lie wholly inside [lo, hi)
};

struct ActLaunch {
    ActSeg seg[3];
    uint32_t first_block[4];   // prefix table of virtual blocks
    int32_t n_seg;
};

// the quad of work item `w` of segment S: its first float e0 and which of its four floats belong to the rows asked for
__device__ __forceinline__ bool quad_of(const ActSeg& S, int64_t w, int64_t& e0, bool ok[4]) {
    e0 = 4 * (S.first + w);
#pragma unroll
    for (int i = 0; i < 4; ++i) ok[i] = e0 + i >= S.lo && e0 + i < S.hi;
    return ok[0] && ok[1] && ok[2] && ok[3];
}

__global__ void __launch_bounds__(kActThreads) activate_fwd_kernel(const ActLaunch L) {
    const uint32_t n_blocks = L.first_block[L.n_seg];
    for (uint32_t vb = blockIdx.x; vb < n_blocks; vb += gridDim.x) {
        HS_BLOCK_OWNER(si, vb, L.first_block, L.n_seg);
        const ActSeg& S = L.seg[si];
        const int64_t w = (int64_t)(vb - L.first_block[si]) * kActThreads + threadIdx.x;
        int64_t e0;
        bool ok[4];
        const bool all = quad_of(S, w, e0, ok);
        if (e0 >= S.hi) continue;
        if (S.kind == kActRotation) {                 // (a quaternion is wholly inside or wholly outside)
            const f4 q = load_quad(S.raw + e0, S.vec != 0);
            const float len = quat_length(q.x, q.y, q.z, q.w);        // before the clamp
            const float n = len < kNormEps ? kNormEps : len;        // max(len, eps); a NaN stays one, as in torch
            f4 r;
            r.x = q.x / n; r.y = q.y / n; r.z = q.z / n; r.w = q.w / n;
            store_quad(S.act + e0, r, S.vec != 0);
        } else if (all) {
            f4 x = load_quad(S.raw + e0, S.vec != 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = S.kind == kActOpacity ? sigmoid_of(x[i]) : expf(x[i]);
            store_quad(S.act + e0, x, S.vec != 0);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!ok[i]) continue;
                const float x = S.raw[e0 + i];
                S.act[e0 + i] = S.kind == kActOpacity ? sigmoid_of(x) : expf(x);
            }
        }
    }
}

__global__ void __launch_bounds__(kActThreads) activate_bwd_kernel(const ActLaunch L) {
    const uint32_t n_blocks = L.first_block[L.n_seg];
    for (uint32_t vb = blockIdx.x; vb < n_blocks; vb += gridDim.x) {
        HS_BLOCK_OWNER(si, vb, L.first_block, L.n_seg);
        const ActSeg& S = L.seg[si];
        const int64_t w = (int64_t)(vb - L.first_block[si]) * kActThreads + threadIdx.x;
        int64_t e0;
        bool ok[4];
        const bool all = quad_of(S, w, e0, ok);
        if (e0 >= S.hi) continue;
        if (S.kind == kActRotation) {
            const f4 q = load_quad(S.raw + e0, S.vec != 0);
            const f4 u = load_quad(S.act + e0, S.vec != 0);
            f4 g = load_quad(S.grad + e0, S.vec != 0);
            const float n = quat_length(q.x, q.y, q.z, q.w);          // (n < eps: the clamp was active)
            if (n < kNormEps) {
                g.x = g.x / kNormEps; g.y = g.y / kNormEps; g.z = g.z / kNormEps; g.w = g.w / kNormEps;
            } else {
                const float d = ((u.x * g.x + u.y * g.y) + u.z * g.z) + u.w * g.w;
                g.x = (g.x - u.x * d) / n;
                g.y = (g.y - u.y * d) / n;
                g.z = (g.z - u.z * d) / n;
                g.w = (g.w - u.w * d) / n;
            }
            store_quad(S.grad + e0, g, S.vec != 0);
        } else if (all) {
            const f4 a = load_quad(S.act + e0, S.vec != 0);
            f4 g = load_quad(S.grad + e0, S.vec != 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = S.kind == kActOpacity ? (g[i] * a[i]) * (1.0f - a[i]) : g[i] * a[i];
            store_quad(S.grad + e0, g, S.vec != 0);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!ok[i]) continue;
                const float a = S.act[e0 + i], g = S.grad[e0 + i];
                S.grad[e0 + i] = S.kind == kActOpacity ? (g * a) * (1.0f - a) : g * a;
            }
        }
    }
}

// rows [r0, r1) of a tensor of `cols` floats per row as a segment; returns its quads
int64_t make_segment(ActSeg& s, int kind, int64_t cols, int64_t r0, int64_t r1, const float* raw, float* act, float* grad) {
    memset(&s, 0, sizeof(s));
    s.kind = kind;
    s.raw = raw; s.act = act; s.grad = grad;
    s.lo = r0 * cols; s.hi = r1 * cols;
    s.vec = aligned_to(raw, 16) && aligned_to(act, 16) && aligned_to(grad, 16) ? 1 : 0;      // (a null pointer is one not given)
    s.first = s.lo / 4;
    return (s.hi + 3) / 4 - s.first;
}

int enqueue(ActLaunch& L, const int64_t* quads, bool backward, hipStream_t s) {
    uint64_t blocks = 0;
    for (int k = 0; k < L.n_seg; ++k) {
        L.first_block[k] = (uint32_t)blocks;
        blocks += (uint64_t)((quads[k] + kActThreads - 1) / kActThreads);
    }
    for (int k = L.n_seg; k < 4; ++k) L.first_block[k] = (uint32_t)blocks;
    if (blocks == 0) return HS_OK;
    const unsigned grid = (unsigned)(blocks < (uint64_t)kActMaxGrid ? blocks : (uint64_t)kActMaxGrid);
    if (backward) activate_bwd_kernel<<<grid, kActThreads, 0, s>>>(L);
    else activate_fwd_kernel<<<grid, kActThreads, 0, s>>>(L);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // namespace

// (P < 2^30 -- checked by the caller, api.hip: at most 2^20 + 3 * 2^20 + 2^22 virtual blocks)
int launch_activate_fwd(const hs_activate_args& a, hipStream_t s) {
    ActLaunch L;
    memset(&L, 0, sizeof(L));
    int64_t quads[3];
    int n = 0;
    if (a.opacity_raw) { quads[n] = make_segment(L.seg[n], kActOpacity, 1, 0, a.P, a.opacity_raw, a.opacities, nullptr); ++n; }
    if (a.scales_raw) { quads[n] = make_segment(L.seg[n], kActScale, 3, 0, a.P, a.scales_raw, a.scales, nullptr); ++n; }
    if (a.rotations_raw) { quads[n] = make_segment(L.seg[n], kActRotation, 4, 0, a.P, a.rotations_raw, a.rotations, nullptr); ++n; }
    L.n_seg = n;
    return enqueue(L, quads, false, s);
}

int launch_activate_bwd(const hs_activate_args& a, hipStream_t s) {
    ActLaunch L;
    memset(&L, 0, sizeof(L));
    int64_t quads[3];
    int n = 0;
    const int64_t r0 = a.g_begin, r1 = a.g_end;
    if (a.dL_dopacities) { quads[n] = make_segment(L.seg[n], kActOpacity, 1, r0, r1, nullptr, a.opacities, a.dL_dopacities); ++n; }
    if (a.dL_dscales) { quads[n] = make_segment(L.seg[n], kActScale, 3, r0, r1, nullptr, a.scales, a.dL_dscales); ++n; }
    if (a.dL_drotations) { quads[n] = make_segment(L.seg[n], kActRotation, 4, r0, r1, a.rotations_raw, a.rotations, a.dL_drotations); ++n; }
    L.n_seg = n;
    return enqueue(L, quads, true, s);
}

}  // namespace hs
