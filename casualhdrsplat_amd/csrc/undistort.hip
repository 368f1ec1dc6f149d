// Lens undistortion of captured frames, fused with the area-filtered downscale to the training resolution: the step between a
// COLMAP camera with distortion and the pinhole rasterizer (hs_undistort_map, hs_undistort_remap; include/hdrsplat.h).
//
// Compiled with -ffp-contract=off: both kernels are a STATED ORDER of IEEE fp32 operations, which tests/undistort_reference.py
// restates in numpy float32 and the GPU tests compare bit for bit.  Do not reassociate them.  `/` and sqrtf are the correctly
// rounded ones (hipcc's default); atanf (OPENCV_FISHEYE only) is the library's and is compared in pixels instead.
//
// MAP.  fx, fy, cx, cy, k[0..7]: the source camera, rounded to fp32 by the host.  For pixel (x, y) of the Wf x Hf grid:
//       u = (((float)x + 0.5) - 0.5 (float)Wf) / fx        v = (((float)y + 0.5) - 0.5 (float)Hf) / fy
//   uu = u u, vv = v v, r2 = uu + vv, r4 = r2 r2, r6 = r4 r2, uv = u v, and per model (every product and sum rounded once, sums
//   left to right unless bracketed):
//   SIMPLE_PINHOLE, PINHOLE   ud = u                                            vd = v
//   SIMPLE_RADIAL             rad = k0 r2;             ud = u + u rad            vd = v + v rad
//   RADIAL                    rad = k0 r2 + k1 r4;     ud = u + u rad            vd = v + v rad
//   OPENCV  (k0 k1 = k1 k2, k2 k3 = p1 p2)   rad = k0 r2 + k1 r4,
//                             tu = (k2 + k2) uv + k3 (r2 + (uu + uu))           tv = (k3 + k3) uv + k2 (r2 + (vv + vv))
//                             ud = u + (u rad + tu)                             vd = v + (v rad + tv)
//   FULL_OPENCV (k4 = k3, k5 k6 k7 = k4 k5 k6)   num = ((1 + k0 r2) + k1 r4) + k4 r6, den = ((1 + k5 r2) + k6 r4) + k7 r6,
//                             s = num / den;  tu, tv as above;  ud = u s + tu    vd = v s + tv
//   OPENCV_FISHEYE            r = sqrt(r2);  r > 1e-8:  t = atanf(r), t2 = t t, t4 = t2 t2, t6 = t4 t2, t8 = t4 t4,
//                             td = t ((((1 + k0 t2) + k1 t4) + k2 t6) + k3 t8), s = td / r;  else s = 1
//                             ud = u s                                          vd = v s
//       sx = ud fx + cx      sy = vd fy + cy      map[y, x] = (sx, sy)
//       valid[y, x] = sx >= 0.5 && sx <= (float)W - 0.5 && sy >= 0.5 && sy <= (float)H - 0.5      (a NaN compares false: 0)
// REMAP.  For output pixel (xo, yo) of frame f and channel c, S = factor:
//       acc = 0;  for j = 0 .. S-1, inside it i = 0 .. S-1:  acc = acc + sample_c(map[yo S + j, xo S + i])
//       out = acc / (float)(S S);  uint8 frames:  out = out / 255
//   sample_c(sx, sy):  0 when sx or sy is a NaN, else
//       px = min(max(sx - 0.5, 0), (float)(W - 1)),  x0 = min((int)floor(px), W - 2),  wx = px - (float)x0     (py, y0, wy: H)
//       t_ab = channel c of the source pixel (x0 + b, y0 + a) as a float (a uint8 converts exactly)
//       top = (1 - wx) t00 + wx t01,  bot = (1 - wx) t10 + wx t11,  sample = (1 - wy) top + wy bot
//   (six products, three sums and the two differences 1 - w: exact on a pixel centre, the last one included, where w = 0 or 1)
//
// undistort_map_kernel<MODEL>   64 x 4 threads, one grid pixel each; the model is a template argument (one dispatch per launch).
//                               Writes one float2 and one byte per lane: 9 Hf Wf bytes, once per camera.
// undistort_remap_kernel<S, U8> 64 x 4 threads, one OUTPUT pixel each, 64 consecutive x per wave: the S S map entries of a lane
//                               are float2 loads at a stride of S entries (S = 1: 512 contiguous bytes per wave), the three
//                               planar stores 256 contiguous bytes per wave each.  A workgroup walks a run of up to 8 frames
//                               with the same lanes: the taps (S <= 2: kept in registers; else recomputed from map entries
//                               that the first frame left in L1 / L2) are shared by the frames of the run.  uint8 frames: the
//                               two horizontally adjacent taps of a row are ONE 6-byte span (a dword and a short, at whatever
//                               alignment the pixel has), so a sample is four loads for its three channels; fp32 frames are
//                               planar: twelve dword loads.  Bound by memory: F (3 H W [u8; 12 for fp32] + 12 Ho Wo) + 8 Hf Wf
//                               bytes against a gather whose lines are shared by neighbouring lanes.
// No atomics, no memset, no host wait; every element of map, valid and out is written by its own lane.
#include "hs_cloud.h"

#include <cmath>
#include <math.h>
#include <string.h>

namespace hs {
namespace {

constexpr int kUdMaxSide = 16384;
// A/B switches (make variant TUS=undistort DEFS=...).  Measured on 8 uint8 frames (hs_undistort_remap, ms at 1080p S = 1 / 1080p
// S = 2 / 4K S = 2): 64 x 4 tiles, runs of 8 frames 0.097 / 0.053 / 0.236; runs of 1 0.091 / 0.051 / 0.242; 32 x 8 0.105 / 0.051 /
// 0.248; 64 x 2 0.093 / 0.052 / 0.237; 64 x 8 0.095 / 0.056 / 0.235 -- all inside the spread of two runs of one build.
#ifndef HS_TUNE_UD_TILE_X
#define HS_TUNE_UD_TILE_X 64
#endif
#ifndef HS_TUNE_UD_TILE_Y
#define HS_TUNE_UD_TILE_Y 4
#endif
#ifndef HS_TUNE_UD_RUN
#define HS_TUNE_UD_RUN 8
#endif
constexpr int kUdTileX = HS_TUNE_UD_TILE_X, kUdTileY = HS_TUNE_UD_TILE_Y;
constexpr int kUdFrameRun = HS_TUNE_UD_RUN;          // frames a workgroup walks with the same taps
constexpr int kUdMaxSlices = 65535;     // gridDim.z

struct UdCamera { float fx, fy, cx, cy, k[8]; };

template <int MODEL>
__device__ __forceinline__ void distort(const UdCamera& c, float u, float v, float& ud, float& vd) {
    if constexpr (MODEL == HS_CAMERA_PINHOLE) {
        ud = u; vd = v;
        return;
    }
    const float uu = u * u, vv = v * v, r2 = uu + vv;
    if constexpr (MODEL == HS_CAMERA_SIMPLE_RADIAL) {
        const float rad = c.k[0] * r2;
        ud = u + u * rad; vd = v + v * rad;
    } else if constexpr (MODEL == HS_CAMERA_RADIAL) {
        const float r4 = r2 * r2;
        const float rad = c.k[0] * r2 + c.k[1] * r4;
        ud = u + u * rad; vd = v + v * rad;
    } else if constexpr (MODEL == HS_CAMERA_OPENCV || MODEL == HS_CAMERA_FULL_OPENCV) {
        const float r4 = r2 * r2, uv = u * v;
        const float tu = (c.k[2] + c.k[2]) * uv + c.k[3] * (r2 + (uu + uu));
        const float tv = (c.k[3] + c.k[3]) * uv + c.k[2] * (r2 + (vv + vv));
        if constexpr (MODEL == HS_CAMERA_OPENCV) {
            const float rad = c.k[0] * r2 + c.k[1] * r4;
            ud = u + (u * rad + tu); vd = v + (v * rad + tv);
        } else {
            const float r6 = r4 * r2;
            const float num = ((1.f + c.k[0] * r2) + c.k[1] * r4) + c.k[4] * r6;
            const float den = ((1.f + c.k[5] * r2) + c.k[6] * r4) + c.k[7] * r6;
            const float s = num / den;
            ud = u * s + tu; vd = v * s + tv;
        }
    } else {   // HS_CAMERA_OPENCV_FISHEYE
        const float r = sqrtf(r2);
        float s = 1.f;
        if (r > 1e-8f) {
            const float t = atanf(r);
            const float t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const float td = t * ((((1.f + c.k[0] * t2) + c.k[1] * t4) + c.k[2] * t6) + c.k[3] * t8);
            s = td / r;
        }
        ud = u * s; vd = v * s;
    }
}

template <int MODEL>
__global__ void __launch_bounds__(kUdTileX * kUdTileY) undistort_map_kernel(UdCamera c, int W, int H, int Wf, int Hf,
                                                                             float2* __restrict__ map, uint8_t* __restrict__ valid) {
    const int x = blockIdx.x * kUdTileX + threadIdx.x, y = blockIdx.y * kUdTileY + threadIdx.y;
    if (x >= Wf || y >= Hf) return;
    const float u = (((float)x + 0.5f) - 0.5f * (float)Wf) / c.fx;
    const float v = (((float)y + 0.5f) - 0.5f * (float)Hf) / c.fy;
    float ud, vd;
    distort<MODEL>(c, u, v, ud, vd);
    const float sx = ud * c.fx + c.cx, sy = vd * c.fy + c.cy;
    const int64_t at = (int64_t)y * Wf + x;
    map[at] = make_float2(sx, sy);
    valid[at] = (sx >= 0.5f && sx <= (float)W - 0.5f && sy >= 0.5f && sy <= (float)H - 0.5f) ? 1 : 0;
}

// where a map entry samples: the top-left tap y0 W + x0, the weights w and 1 - w, and whether the coordinate was a number
struct UdTap { int32_t at; float wx, wy, ox, oy; bool ok; };

__device__ __forceinline__ UdTap make_tap(float2 m, int W, int H) {
    UdTap t;
    t.ok = m.x == m.x && m.y == m.y;
    const float px = fminf(fmaxf(m.x - 0.5f, 0.f), (float)(W - 1));   // (fmaxf(NaN, 0) = 0: a NaN addresses tap 0)
    const float py = fminf(fmaxf(m.y - 0.5f, 0.f), (float)(H - 1));
    const int x0 = min((int)floorf(px), W - 2), y0 = min((int)floorf(py), H - 2);
    t.wx = px - (float)x0;
    t.wy = py - (float)y0;
    t.ox = 1.f - t.wx;
    t.oy = 1.f - t.wy;
    t.at = y0 * W + x0;
    return t;
}

__device__ __forceinline__ float blend(const UdTap& t, float t00, float t01, float t10, float t11) {
    const float top = t.ox * t00 + t.wx * t01;
    const float bot = t.ox * t10 + t.wx * t11;
    const float s = t.oy * top + t.wy * bot;
    return t.ok ? s : 0.f;
}

// two horizontally adjacent RGB pixels of a uint8 frame: six bytes at any alignment
struct __attribute__((packed)) UdSpan { uint32_t lo; uint16_t hi; };
__device__ __forceinline__ void span_bytes(const uint8_t* p, float left[3], float right[3]) {
    UdSpan s;
    memcpy(&s, p, sizeof s);
    left[0] = (float)(s.lo & 255u); left[1] = (float)((s.lo >> 8) & 255u); left[2] = (float)((s.lo >> 16) & 255u);
    right[0] = (float)(s.lo >> 24); right[1] = (float)(s.hi & 255u); right[2] = (float)(s.hi >> 8);
}

// `frame`: the first byte / float of one frame
template <bool U8>
__device__ __forceinline__ void sample(const void* frame, const UdTap& t, int W, int H, float acc[3]) {
    if constexpr (U8) {
        const uint8_t* p = (const uint8_t*)frame + 3 * (int64_t)t.at;
        float a0[3], a1[3], b0[3], b1[3];
        span_bytes(p, a0, a1);
        span_bytes(p + 3 * (int64_t)W, b0, b1);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + blend(t, a0[c], a1[c], b0[c], b1[c]);
    } else {
        const float* p = (const float*)frame + t.at;
        const int64_t plane = (int64_t)H * W;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* q = p + c * plane;
            acc[c] = acc[c] + blend(t, q[0], q[1], q[W], q[W + 1]);
        }
    }
}

template <int S, bool U8>
__global__ void __launch_bounds__(kUdTileX * kUdTileY) undistort_remap_kernel(const void* __restrict__ frames,
                                                                               const float2* __restrict__ map, int W, int H, int Wf,
                                                                               int Wo, int Ho, int F, int run,
                                                                               float* __restrict__ out) {
    const int xo = blockIdx.x * kUdTileX + threadIdx.x, yo = blockIdx.y * kUdTileY + threadIdx.y;
    if (xo >= Wo || yo >= Ho) return;
    constexpr bool kKeep = S <= 2;                    // the taps of a lane stay in registers across the frames
    const float2* m = map + ((int64_t)yo * S * Wf + (int64_t)xo * S);
    UdTap taps[kKeep ? S * S : 1];
    if constexpr (kKeep) {
#pragma unroll
        for (int j = 0; j < S; ++j)
#pragma unroll
            for (int i = 0; i < S; ++i) taps[j * S + i] = make_tap(m[(int64_t)j * Wf + i], W, H);
    }
    const int64_t frame_elems = 3 * (int64_t)H * W, plane_out = (int64_t)Ho * Wo;
    const int f_begin = blockIdx.z * run, f_end = min(F, f_begin + run);
    for (int f = f_begin; f < f_end; ++f) {
        const void* frame = U8 ? (const void*)((const uint8_t*)frames + f * frame_elems)
                               : (const void*)((const float*)frames + f * frame_elems);
        float acc[3] = {0.f, 0.f, 0.f};
        if constexpr (kKeep) {
#pragma unroll
            for (int n = 0; n < S * S; ++n) sample<U8>(frame, taps[n], W, H, acc);
        } else {
            for (int j = 0; j < S; ++j)
#pragma unroll
                for (int i = 0; i < S; ++i) sample<U8>(frame, make_tap(m[(int64_t)j * Wf + i], W, H), W, H, acc);
        }
        float* o = out + (3 * (int64_t)f * plane_out + (int64_t)yo * Wo + xo);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float r = acc[c] / (float)(S * S);
            if constexpr (U8) r = r / 255.f;
            o[c * plane_out] = r;
        }
    }
}

int check_sides(const char* fn, const hs_undistort_args& a) {
    if (a.W < 2 || a.W > kUdMaxSide || a.H < 2 || a.H > kUdMaxSide) {
        set_error("%s: W=%d, H=%d outside 2 <= W, H <= %d", fn, a.W, a.H, kUdMaxSide);
        return HS_EINVAL;
    }
    if (a.Wf < 0 || a.Wf > kUdMaxSide || a.Hf < 0 || a.Hf > kUdMaxSide) {
        set_error("%s: Wf=%d, Hf=%d outside 0 <= Wf, Hf <= %d", fn, a.Wf, a.Hf, kUdMaxSide);
        return HS_EINVAL;
    }
    return HS_OK;
}

template <int MODEL>
int launch_map(const hs_undistort_args& a, hipStream_t s) {
    UdCamera c;
    c.fx = a.fx; c.fy = a.fy; c.cx = a.cx; c.cy = a.cy;
    for (int i = 0; i < 8; ++i) c.k[i] = a.k[i];
    const dim3 grid((unsigned)ceil_div(a.Wf, kUdTileX), (unsigned)ceil_div(a.Hf, kUdTileY));
    undistort_map_kernel<MODEL><<<grid, dim3(kUdTileX, kUdTileY), 0, s>>>(c, a.W, a.H, a.Wf, a.Hf, (float2*)a.map, a.valid);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

template <int S, bool U8>
int launch_remap(const hs_undistort_args& a, hipStream_t s) {
    const int Wo = a.Wf / S, Ho = a.Hf / S;
    int slices = ceil_div(a.F, kUdFrameRun);
    if (slices > kUdMaxSlices) slices = kUdMaxSlices;
    const int run = ceil_div(a.F, slices);             // slices * run >= F
    const dim3 grid((unsigned)ceil_div(Wo, kUdTileX), (unsigned)ceil_div(Ho, kUdTileY), (unsigned)ceil_div(a.F, run));
    undistort_remap_kernel<S, U8><<<grid, dim3(kUdTileX, kUdTileY), 0, s>>>(a.frames, (const float2*)a.map, a.W, a.H, a.Wf, Wo, Ho,
                                                                            a.F, run, a.out);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

template <int S>
int launch_remap(const hs_undistort_args& a, hipStream_t s) {
    return a.frames_u8 ? launch_remap<S, true>(a, s) : launch_remap<S, false>(a, s);
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int hs_undistort_map(const hs_undistort_args* a, void* hip_stream) {
    const char* fn = "hs_undistort_map";
    if (hs::check_args(fn, a)) return HS_EINVAL;
    if (a->model < HS_CAMERA_SIMPLE_PINHOLE || a->model > HS_CAMERA_FULL_OPENCV) {
        hs::set_error("%s: model=%d is none of SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, FULL_OPENCV "
                      "(0 .. 6)", fn, a->model);
        return HS_EINVAL;
    }
    if (hs::check_sides(fn, *a)) return HS_EINVAL;
    if (!(std::isfinite(a->fx) && std::isfinite(a->fy) && a->fx > 0.f && a->fy > 0.f)) {
        hs::set_error("%s: fx=%g, fy=%g must be finite and > 0", fn, (double)a->fx, (double)a->fy);
        return HS_EINVAL;
    }
    if (!(std::isfinite(a->cx) && std::isfinite(a->cy))) {
        hs::set_error("%s: cx=%g, cy=%g must be finite", fn, (double)a->cx, (double)a->cy);
        return HS_EINVAL;
    }
    for (int i = 0; i < 8; ++i)
        if (!std::isfinite(a->k[i])) { hs::set_error("%s: k[%d]=%g must be finite", fn, i, (double)a->k[i]); return HS_EINVAL; }
    if (a->Wf == 0 || a->Hf == 0) {
        if (hs::check_aligned(fn, a->map, "map", 8)) return HS_EINVAL;
        return HS_OK;
    }
    const hs::Field f[2] = {{a->map, "map", 8}, {a->valid, "valid", 1}};
    if (hs::check_fields(fn, f, 2)) return HS_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    switch (a->model) {
        case HS_CAMERA_SIMPLE_PINHOLE:
        case HS_CAMERA_PINHOLE: return hs::launch_map<HS_CAMERA_PINHOLE>(*a, s);
        case HS_CAMERA_SIMPLE_RADIAL: return hs::launch_map<HS_CAMERA_SIMPLE_RADIAL>(*a, s);
        case HS_CAMERA_RADIAL: return hs::launch_map<HS_CAMERA_RADIAL>(*a, s);
        case HS_CAMERA_OPENCV: return hs::launch_map<HS_CAMERA_OPENCV>(*a, s);
        case HS_CAMERA_OPENCV_FISHEYE: return hs::launch_map<HS_CAMERA_OPENCV_FISHEYE>(*a, s);
        default: return hs::launch_map<HS_CAMERA_FULL_OPENCV>(*a, s);
    }
}

HS_API int hs_undistort_remap(const hs_undistort_args* a, void* hip_stream) {
    const char* fn = "hs_undistort_remap";
    if (hs::check_args(fn, a) || hs::check_sides(fn, *a)) return HS_EINVAL;
    const int S = a->factor;
    if (!(S == 1 || S == 2 || S == 3 || S == 4 || S == 8)) {
        hs::set_error("%s: factor=%d is none of 1, 2, 3, 4, 8", fn, S);
        return HS_EINVAL;
    }
    if (a->Wf % S || a->Hf % S) {
        hs::set_error("%s: Wf=%d, Hf=%d must be multiples of factor=%d", fn, a->Wf, a->Hf, S);
        return HS_EINVAL;
    }
    const int64_t lim = 1ll << 31, in_px = (int64_t)a->H * a->W, out_px = (int64_t)(a->Hf / S) * (a->Wf / S);
    if (a->F < 0 || 3 * (int64_t)a->F * in_px >= lim || 3 * (int64_t)a->F * out_px >= lim) {
        hs::set_error("%s: F=%d outside F >= 0, 3 F H W < 2^31, 3 F (Hf / factor) (Wf / factor) < 2^31", fn, a->F);
        return HS_EINVAL;
    }
    const uintptr_t frames_align = a->frames_u8 ? 1 : 4;
    if (a->F == 0 || out_px == 0) {
        if (hs::check_aligned(fn, a->map, "map", 8) || hs::check_aligned(fn, a->frames, "frames", frames_align) ||
            hs::check_aligned(fn, a->out, "out", 4))
            return HS_EINVAL;
        return HS_OK;
    }
    const hs::Field f[3] = {{a->map, "map", 8}, {a->frames, "frames", frames_align}, {a->out, "out", 4}};
    if (hs::check_fields(fn, f, 3)) return HS_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    switch (S) {
        case 1: return hs::launch_remap<1>(*a, s);
        case 2: return hs::launch_remap<2>(*a, s);
        case 3: return hs::launch_remap<3>(*a, s);
        case 4: return hs::launch_remap<4>(*a, s);
        default: return hs::launch_remap<8>(*a, s);
    }
}

}  // extern "C"
