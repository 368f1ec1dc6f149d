// The 3D smoothing filter of Mip-Splatting (hs_smoothing_filter_workspace_bytes, hs_smoothing_filter, hs_smoothing_apply,
// hs_smoothing_apply_backward; include/hdrsplat.h states the arithmetic).  The rasterizer's HS_FLAG_ANTIALIAS is the
// publication's 2D screen-space filter; this is its other half: a per-Gaussian radius below which no training camera can
// resolve the Gaussian, and the activations of the stored cloud with that radius folded in.
//
//   smoothing_depth_kernel   one thread per Gaussian, 256 per workgroup, a grid of at most 2048 workgroups that stride.  The
//                            cameras pass through LDS a chunk of 64 at a time, 20 floats each: the twelve matrix entries the
//                            projection reads and fx, fy, 0.5 W, 0.5 H, -0.15 W, 1.15 W, -0.15 H, 1.15 H (each ONE fp32
//                            operation on the camera's own numbers, so staging them changes no bit).  Every lane reads the
//                            same LDS address: a broadcast.  A thread keeps the minimum depth d over the cameras that see
//                            its Gaussian and their count; it writes d (0.0f for "seen by none": a seen depth exceeds 0.2f)
//                            to filter[i] and the count to n_views[i].  The workgroup folds the maximum of its d and, from
//                            the staging loads, the maximum fx, and writes {D_b, fmax} to ITS word pair of the workspace.
//   smoothing_radius_kernel  the same grid.  Every workgroup folds the word pairs of the first launch (at most 2048) into D,
//                            takes fmax from the first, and turns filter[i] from d into the radius -- read and written by
//                            the same thread.
//   smoothing_apply_kernel   forward and backward of the activations with the filter.  A thread takes FOUR consecutive rows:
//                            one 16-byte access of the opacities, of the filter, and three of the scales' twelve floats, where
//                            every pointer is 16-byte aligned and the four rows lie inside the rows asked for; 4-byte
//                            accesses of exactly the rows' elements otherwise.  The backward recomputes the forward from the
//                            stored values with the forward's own code: the same bits.
// Minimum and maximum are exact in any order, so the decomposition changes no bit.  No atomics, no memset, no copy, no
// synchronisation; every workspace word read was written by the first launch of the same call.  Compiled with
// -ffp-contract=off; denormals kept.
#include "hs_cloud.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

namespace hs {
namespace {

constexpr int kSmThreads = 256;
constexpr int kSmMaxGrid = 2048;              // 256 CUs x 8 workgroups; larger clouds stride
constexpr int kSmCamChunk = 64;               // cameras staged at a time
constexpr int kSmCamFloats = 20;
constexpr int64_t kSmMaxC = 1ll << 20;
constexpr float kSmNear = 0.2f;               // the published near plane (also the rasterizer's cull)
constexpr float kSmLo = -0.15f, kSmHi = 1.15f;
constexpr float kSmSqrtFifth = 0.4472135901451111f;   // sqrt(0.2) rounded to fp32, bits 0x3ee4f92e

inline int64_t sm_blocks(int64_t P) {
    const int64_t b = (P + kSmThreads - 1) / kSmThreads;
    return b < kSmMaxGrid ? b : kSmMaxGrid;
}

// max of the workgroup's values; every thread calls it, the result is valid in thread 0 (and all of s[] is free afterwards)
__device__ __forceinline__ float block_max(float v, float* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = kSmThreads / 2; off > 0; off >>= 1) {
        if (t < off) s[t] = s[t + off] > s[t] ? s[t + off] : s[t];
        __syncthreads();
    }
    const float r = s[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kSmThreads) smoothing_depth_kernel(int64_t P, int32_t C, const float* __restrict__ xyz,
                                                                      const float* __restrict__ views,
                                                                      const float* __restrict__ intr, float* __restrict__ filter,
                                                                      int32_t* __restrict__ n_views, float* __restrict__ words) {
    __shared__ f4 cam[kSmCamChunk * (kSmCamFloats / 4)];
    __shared__ float red[kSmThreads];
    const int t = threadIdx.x;
    float dmax = 0.f;                          // over this workgroup's seen rows
    float fmax = -INFINITY;                    // over the fx this thread staged (every workgroup stages every camera)
    const int64_t nvb = (P + kSmThreads - 1) / kSmThreads;
    for (int64_t vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
        const int64_t i = vb * kSmThreads + t;
        const bool live = i < P;
        float x = 0.f, y = 0.f, z = 0.f;
        if (live) { x = xyz[3 * i]; y = xyz[3 * i + 1]; z = xyz[3 * i + 2]; }
        float d = INFINITY;
        int32_t n = 0;
        for (int32_t c0 = 0; c0 < C; c0 += kSmCamChunk) {
            const int32_t nc = C - c0 < kSmCamChunk ? C - c0 : kSmCamChunk;
            __syncthreads();                   // the previous chunk has been read
            if (t < nc) {
                const float* m = views + 16 * (int64_t)(c0 + t);
                const float* k = intr + 4 * (int64_t)(c0 + t);
                const float fx = k[0], fy = k[1], W = k[2], H = k[3];
                f4* o = cam + t * (kSmCamFloats / 4);
                f4 v;
                v.x = m[0]; v.y = m[4]; v.z = m[8]; v.w = m[12]; o[0] = v;
                v.x = m[1]; v.y = m[5]; v.z = m[9]; v.w = m[13]; o[1] = v;
                v.x = m[2]; v.y = m[6]; v.z = m[10]; v.w = m[14]; o[2] = v;
                v.x = fx; v.y = fy; v.z = 0.5f * W; v.w = 0.5f * H; o[3] = v;
                v.x = kSmLo * W; v.y = kSmHi * W; v.z = kSmLo * H; v.w = kSmHi * H; o[4] = v;
                fmax = fx > fmax ? fx : fmax;
            }
            __syncthreads();
            if (!live) continue;               // (uniform barriers above: every thread reaches them)
            for (int32_t c = 0; c < nc; ++c) {
                const f4* q = cam + c * (kSmCamFloats / 4);
                const f4 r0 = q[0], r1 = q[1], r2 = q[2], k = q[3], b = q[4];
                const float xc = ((r0.x * x + r0.y * y) + r0.z * z) + r0.w;
                const float yc = ((r1.x * x + r1.y * y) + r1.z * z) + r1.w;
                const float zc = ((r2.x * x + r2.y * y) + r2.z * z) + r2.w;
                const float u = (xc / zc) * k.x + k.z;
                const float v = (yc / zc) * k.y + k.w;
                const bool valid = zc > kSmNear && u >= b.x && u <= b.y && v >= b.z && v <= b.w;    // a NaN: false
                if (valid) {
                    d = zc < d ? zc : d;
                    ++n;
                }
            }
        }
        if (live) {
            const float di = n > 0 ? d : 0.f;
            filter[i] = di;
            if (n_views) n_views[i] = n;
            dmax = di > dmax ? di : dmax;
        }
    }
    const float D = block_max(dmax, red);
    const float f = block_max(fmax, red);
    if (t == 0) {
        words[2 * blockIdx.x] = D;
        words[2 * blockIdx.x + 1] = f;
    }
}

__global__ void __launch_bounds__(kSmThreads) smoothing_radius_kernel(int64_t P, int32_t n_words, const float* __restrict__ words,
                                                                       float* __restrict__ filter) {
    __shared__ float red[kSmThreads];
    const int t = threadIdx.x;
    float m = 0.f;
    for (int32_t b = t; b < n_words; b += kSmThreads) {
        const float w = words[2 * b];
        m = w > m ? w : m;
    }
    __shared__ float s_D;
    const float Dm = block_max(m, red);
    if (t == 0) s_D = Dm;
    __syncthreads();
    const float D = s_D;
    const float fmax = words[1];               // every workgroup of the first launch staged every camera
    const int64_t nvb = (P + kSmThreads - 1) / kSmThreads;
    for (int64_t vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
        const int64_t i = vb * kSmThreads + t;
        if (i >= P) continue;
        const float d = filter[i];
        // D == 0: no Gaussian is seen by any camera (or there is no camera) -- zeros, not 0 / fmax
        filter[i] = D > 0.f ? ((d > 0.f ? d : D) / fmax) * kSmSqrtFifth : 0.f;
    }
}

// ---- applying the filter ----

struct SmApply {
    const float* x; const float* l; const float* f;      // stored logits [P], log scales [P, 3], filter [P]
    float* o; float* s;                                   // forward: opacities [P], scales [P, 3]
    float* g_o; float* g_s;                               // backward: the gradient rows, in place
    int64_t lo, hi;                                       // rows [lo, hi)
    int64_t first;                                        // first group of four rows: rows [4 first, 4 first + 4)
    int32_t vec;                                          // 16-byte accesses for groups wholly inside [lo, hi)
};

struct SmRow { float o, c, oc; float sp[3], r[3], t[3]; };

// the forward of one row; the backward calls it too, so both carry the same bits
__device__ __forceinline__ SmRow sm_row(float x, const float l[3], float f) {
    SmRow R;
    R.o = sigmoid_of(x);
    const float f2 = f * f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float s = expf(l[k]);
        const float q = s * s;
        const float v = q + f2;
        R.sp[k] = sqrtf(v);
        const bool zero = v == 0.0f;
        R.r[k] = zero ? 1.0f : q / v;
        R.t[k] = zero ? 0.0f : f2 / v;
    }
    R.c = sqrtf((R.r[0] * R.r[1]) * R.r[2]);
    R.oc = R.o * R.c;
    return R;
}

// the scale gradient of one axis.  Where t_k == 0 (a zero filter) nothing is added: the row is hs_activate_backward's g s bit
// for bit -- a -0.0 stays, and an infinite g_o o' makes no NaN out of 0
__device__ __forceinline__ float sm_scale_grad(float gk, float g, const SmRow& R, int k) {
    const float a = (gk * R.sp[k]) * R.r[k];
    return R.t[k] == 0.0f ? a : a + (g * R.oc) * R.t[k];
}

template <bool kBackward>
__global__ void __launch_bounds__(kSmThreads) smoothing_apply_kernel(const SmApply a) {
    const int64_t w = (int64_t)blockIdx.x * kSmThreads + threadIdx.x;
    const int64_t r0 = 4 * (a.first + w);
    if (r0 >= a.hi) return;
    const bool all = r0 >= a.lo && r0 + 4 <= a.hi;
    if (all && a.vec) {
        const f4 x = *reinterpret_cast<const f4*>(a.x + r0);
        const f4 f = *reinterpret_cast<const f4*>(a.f + r0);
        float l[12];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const f4 v = *reinterpret_cast<const f4*>(a.l + 3 * r0 + 4 * j);
            l[4 * j] = v.x; l[4 * j + 1] = v.y; l[4 * j + 2] = v.z; l[4 * j + 3] = v.w;
        }
        f4 go;
        float gs[12];
        if (kBackward) {
            go = *reinterpret_cast<const f4*>(a.g_o + r0);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const f4 v = *reinterpret_cast<const f4*>(a.g_s + 3 * r0 + 4 * j);
                gs[4 * j] = v.x; gs[4 * j + 1] = v.y; gs[4 * j + 2] = v.z; gs[4 * j + 3] = v.w;
            }
        }
        f4 oo;
        float so[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const SmRow R = sm_row(x[i], l + 3 * i, f[i]);
            if (kBackward) {
                const float g = go[i];
                oo[i] = ((g * R.c) * R.o) * (1.0f - R.o);
#pragma unroll
                for (int k = 0; k < 3; ++k) so[3 * i + k] = sm_scale_grad(gs[3 * i + k], g, R, k);
            } else {
                oo[i] = R.oc;
#pragma unroll
                for (int k = 0; k < 3; ++k) so[3 * i + k] = R.sp[k];
            }
        }
        float* po = kBackward ? a.g_o : a.o;
        float* ps = kBackward ? a.g_s : a.s;
        *reinterpret_cast<f4*>(po + r0) = oo;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            f4 v;
            v.x = so[4 * j]; v.y = so[4 * j + 1]; v.z = so[4 * j + 2]; v.w = so[4 * j + 3];
            *reinterpret_cast<f4*>(ps + 3 * r0 + 4 * j) = v;
        }
        return;
    }
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const int64_t r = r0 + i;
        if (r < a.lo || r >= a.hi) continue;
        const float l[3] = {a.l[3 * r], a.l[3 * r + 1], a.l[3 * r + 2]};
        const SmRow R = sm_row(a.x[r], l, a.f[r]);
        if (kBackward) {
            const float g = a.g_o[r];
            const float g0 = a.g_s[3 * r], g1 = a.g_s[3 * r + 1], g2 = a.g_s[3 * r + 2];
            a.g_o[r] = ((g * R.c) * R.o) * (1.0f - R.o);
            a.g_s[3 * r] = sm_scale_grad(g0, g, R, 0);
            a.g_s[3 * r + 1] = sm_scale_grad(g1, g, R, 1);
            a.g_s[3 * r + 2] = sm_scale_grad(g2, g, R, 2);
        } else {
            a.o[r] = R.oc;
            a.s[3 * r] = R.sp[0]; a.s[3 * r + 1] = R.sp[1]; a.s[3 * r + 2] = R.sp[2];
        }
    }
}

int check_filter_args(const hs_smoothing_filter_args* a) {
    const char* fn = "hs_smoothing_filter";
    if (check_args(fn, a) || check_rows(fn, "P", a->P)) return HS_EINVAL;
    if (a->C < 0 || a->C >= kSmMaxC) { set_error("%s: C=%lld outside [0, 2^20)", fn, (long long)a->C); return HS_EINVAL; }
    if (check_aligned(fn, a->n_views, "n_views", 4)) return HS_EINVAL;
    if (a->P == 0) return HS_OK;
    // (a workspace that is not even 4-byte aligned is told so first: the texts and their order are part of the contract)
    const Field f[] = {{a->xyz, "xyz", 4}, {a->filter, "filter", 4}, {a->workspace, "workspace", 4}, {a->workspace, "workspace", 256},
                       {a->viewmatrices, "viewmatrices", 4}, {a->intrinsics, "intrinsics", 4}};
    return check_fields(fn, f, a->C > 0 ? 6 : 4);
}

int check_apply_args(const hs_smoothing_apply_args* a, bool backward) {
    const char* fn = backward ? "hs_smoothing_apply_backward" : "hs_smoothing_apply";
    if (check_args(fn, a) || check_rows(fn, "P", a->P)) return HS_EINVAL;
    if (backward) {
        if (a->g_begin < 0 || a->g_begin > a->g_end || a->g_end > a->P) {
            set_error("%s: g_begin=%lld, g_end=%lld outside 0 <= g_begin <= g_end <= P=%lld", fn, (long long)a->g_begin,
                      (long long)a->g_end, (long long)a->P);
            return HS_EINVAL;
        }
        if (a->g_begin == a->g_end) return HS_OK;
        const Field f[] = {{a->opacity_raw, "opacity_raw", 4}, {a->scales_raw, "scales_raw", 4}, {a->filter, "filter", 4},
                           {a->dL_dopacities, "dL_dopacities", 4}, {a->dL_dscales, "dL_dscales", 4}};
        return check_fields(fn, f, 5);
    }
    if (a->P == 0) return HS_OK;
    const Field f[] = {{a->opacity_raw, "opacity_raw", 4}, {a->scales_raw, "scales_raw", 4}, {a->filter, "filter", 4},
                       {a->opacities, "opacities", 4}, {a->scales, "scales", 4}};
    return check_fields(fn, f, 5);
}

int launch_apply(const hs_smoothing_apply_args& a, bool backward, hipStream_t s) {
    SmApply k;
    memset(&k, 0, sizeof(k));
    k.x = a.opacity_raw; k.l = a.scales_raw; k.f = a.filter;
    k.o = a.opacities; k.s = a.scales;
    k.g_o = a.dL_dopacities; k.g_s = a.dL_dscales;
    k.lo = backward ? a.g_begin : 0;
    k.hi = backward ? a.g_end : a.P;
    if (k.lo >= k.hi) return HS_OK;
    k.first = k.lo / 4;
    const int64_t groups = (k.hi + 3) / 4 - k.first;
    k.vec = aligned_to(k.x, 16) && aligned_to(k.l, 16) && aligned_to(k.f, 16) &&
            (backward ? aligned_to(k.g_o, 16) && aligned_to(k.g_s, 16) : aligned_to(k.o, 16) && aligned_to(k.s, 16)) ? 1 : 0;
    const unsigned grid = (unsigned)((groups + kSmThreads - 1) / kSmThreads);      // P < 2^30: at most 2^20 workgroups
    if (backward) smoothing_apply_kernel<true><<<grid, kSmThreads, 0, s>>>(k);
    else smoothing_apply_kernel<false><<<grid, kSmThreads, 0, s>>>(k);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_smoothing_filter_workspace_bytes(int64_t P) {
    if (hs::check_rows("hs_smoothing_filter_workspace_bytes", "P", P)) return HS_EINVAL;
    return hs::align_up(8 * hs::sm_blocks(P), 256);
}

HS_API int hs_smoothing_filter(const hs_smoothing_filter_args* a, void* hip_stream) {
    const int rc = hs::check_filter_args(a);
    if (rc != HS_OK || a->P == 0) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const unsigned grid = (unsigned)hs::sm_blocks(a->P);
    hs::smoothing_depth_kernel<<<grid, hs::kSmThreads, 0, s>>>(a->P, (int32_t)a->C, a->xyz, a->viewmatrices, a->intrinsics, a->filter,
                                                               a->n_views, (float*)a->workspace);
    HS_LAUNCH_CHECK();
    hs::smoothing_radius_kernel<<<grid, hs::kSmThreads, 0, s>>>(a->P, (int32_t)grid, (const float*)a->workspace, a->filter);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

HS_API int hs_smoothing_apply(const hs_smoothing_apply_args* a, void* hip_stream) {
    const int rc = hs::check_apply_args(a, false);
    if (rc != HS_OK) return rc;
    return hs::launch_apply(*a, false, (hipStream_t)hip_stream);
}

HS_API int hs_smoothing_apply_backward(const hs_smoothing_apply_args* a, void* hip_stream) {
    const int rc = hs::check_apply_args(a, true);
    if (rc != HS_OK) return rc;
    return hs::launch_apply(*a, true, (hipStream_t)hip_stream);
}

}  // extern "C"
