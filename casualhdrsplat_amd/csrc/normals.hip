// Depth-normal consistency (2DGS, GOF, RaDe-GS, PGSR, dn-splatter), fused: the normal of the surface the composited depth
// describes, its agreement with a composited normal image, the backward of that term to the normal image, the inverse depth
// and the accumulated opacity, and the per-Gaussian normal that is composited (hs_normal_consistency_workspace_bytes,
// hs_normal_consistency, hs_normal_consistency_backward, hs_gaussian_normals, hs_gaussian_normals_backward;
// include/hdrsplat.h states the definitions).
//
// Compiled with -ffp-contract=off: every line below is a sequence of correctly rounded IEEE fp32 operations, which
// tests/normals_reference.py restates in numpy float32 and bounds term by term.
//
//   sample:  valid when d = invdepth and a = alpha (1 when absent) are finite and > 0;  z = a / d
//   pixel (x, y), interior (it and its four axis neighbours valid, 1 <= x <= W-2, 1 <= y <= H-2), with l, r = the samples at
//   x -+ 1 and u, d = the samples at y -+ 1:
//       sx = zr + zl,  sy = zd + zu,  rx = (zr - zl) / sx,  ry = (zd - zu) / sy
//       xh = (float(x) + 0.5f) - 0.5f * float(W),  yh likewise with H
//       m  = (fx * rx,  fy * ry,  0 - ((ry * yh + rx * xh) + 1))           = fx fy c / (sx sy), c the cross product of the
//       len = sqrt((m0 m0 + m1 m1) + m2 m2),  nd = m / len                    definition: the same direction, no overflow,
//       n_i = (R[i][0] nd0 + R[i][1] nd1) + R[i][2] nd2                        no cancellation in a difference of z * u
//       out = w * (1 - ((N0 n0 + N1 n1) + N2 n2))
//   backward, g = dL_dout:  gw = g * w,  dL_dnormals_k = 0 - gw * n_k,
//       v_j = 0 - gw * ((R[0][j] N0 + R[1][j] N1) + R[2][j] N2),  t = (nd0 v0 + nd1 v1) + nd2 v2,  u_j = (v_j - nd_j * t) / len
//       Gx = u0 * fx - u2 * xh,  hx = Gx / (sx * sx),  to zr: hx * (zl + zl),  to zl: 0 - hx * (zr + zr);  y likewise
//       a sample adds what its four neighbours send it, in the order ((from x-1 + from x+1) + from y-1) + from y+1 = dz;
//       dL_dinvdepth = 0 - (dz * z) / d,  dL_dalpha = dz / d;  an invalid sample: 0
//
// normal_consistency_kernel       one workgroup per 64 x 16 pixel tile of one frame, lane = column, wave = rows wave, wave + 4, ...;
//                                 the stencil's five samples come from memory (the neighbours are cache hits).
// normal_consistency_bwd_kernel   the same tiles.  The backward to the depth is a GATHER: a sample collects what the four pixels
//                                 whose stencil it sits in send it, so a tile needs those pixels' terms on a halo of one and
//                                 their depths on a halo of two.  Phase 1 stages z of the 68 x 20 window in LDS (outside the frame:
//                                 invalid), phase 2 computes the four sends of every pixel of the 66 x 18 window into LDS (and
//                                 writes dL_dnormals for the tile's own pixels), phase 3 adds each sample's four in a fixed order.
//                                 No workspace, no atomics: the same inputs give the same bits.
// gaussian_normals_kernel<kBwd>   one thread per Gaussian.  Bytes per Gaussian: forward 16 + 12 + 12 read, 12 written = 52;
//                                 backward 16 + 12 + 12 + 12 read, 16 written = 68.
#include "hs_cloud.h"

#include <math.h>
#include <string.h>

namespace hs {
namespace {

constexpr int kNcTW = 64, kNcTH = 16, kNcThreads = 256;   // pixel tile; four waves
constexpr int kNcZW = kNcTW + 4, kNcZH = kNcTH + 4;       // depths: halo of two
constexpr int kNcGW = kNcTW + 2, kNcGH = kNcTH + 2;       // sends: halo of one
constexpr int64_t kNcMaxGrid = 1 << 20;
constexpr int kGnThreads = 256;

struct Nc {
    int B, H, W;
    float fx, fy;
    const float* invdepth; const float* alpha; const float* normals; const float* weight; const float* rot;
    float* out; float* depth_normals;
    const float* d_out; float* d_normals; float* d_invdepth; float* d_alpha;
};

// z of a sample, -1 for an invalid one (a valid z is positive)
__device__ __forceinline__ float nc_depth(const Nc& a, int64_t at) {
    const float d = a.invdepth[at];
    const float al = a.alpha ? a.alpha[at] : 1.f;
    const bool ok = d > 0.f && d < INFINITY && al > 0.f && al < INFINITY;
    return ok ? al / d : -1.f;
}

__device__ __forceinline__ float nc_centre(int p, int n) { return ((float)p + 0.5f) - 0.5f * (float)n; }

struct NcPixel { float sx, sy, len, nd[3]; };

__device__ __forceinline__ NcPixel nc_pixel(float zl, float zr, float zu, float zd, float xh, float yh, float fx, float fy) {
    NcPixel p;
    p.sx = zr + zl; p.sy = zd + zu;
    const float rx = (zr - zl) / p.sx, ry = (zd - zu) / p.sy;
    const float m0 = fx * rx, m1 = fy * ry, m2 = 0.f - ((ry * yh + rx * xh) + 1.f);
    p.len = sqrtf((m0 * m0 + m1 * m1) + m2 * m2);
    p.nd[0] = m0 / p.len; p.nd[1] = m1 / p.len; p.nd[2] = m2 / p.len;
    return p;
}

// the frame's rotation (row-major), the identity when there is none
__device__ __forceinline__ void nc_rotation(const Nc& a, int b, float R[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = a.rot ? a.rot[(int64_t)b * 9 + i] : ((i & 3) == 0 ? 1.f : 0.f);
}

__global__ void __launch_bounds__(kNcThreads) normal_consistency_kernel(const Nc a, int tiles_x, int tiles_y, int64_t ntiles) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, W = a.W;
    const int64_t HW = (int64_t)H * W;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int per = tiles_x * tiles_y;
        const int b = (int)(tile / per), rem = (int)(tile - (int64_t)b * per);
        const int oy = (rem / tiles_x) * kNcTH, ox = (rem % tiles_x) * kNcTW;
        const int px = ox + lane;
        if (px >= W) continue;
        float R[9];
        nc_rotation(a, b, R);
        const float xh = nc_centre(px, W);
        for (int py = oy + wave; py < oy + kNcTH && py < H; py += 4) {
            const int64_t at = (int64_t)b * HW + (int64_t)py * W + px;
            const int64_t at3 = (int64_t)b * 3 * HW + (int64_t)py * W + px;
            float o = 0.f, n[3] = {0.f, 0.f, 0.f};
            if (px >= 1 && px <= W - 2 && py >= 1 && py <= H - 2) {
                const float zc = nc_depth(a, at), zl = nc_depth(a, at - 1), zr = nc_depth(a, at + 1);
                const float zu = nc_depth(a, at - W), zd = nc_depth(a, at + W);
                if (zc >= 0.f && zl >= 0.f && zr >= 0.f && zu >= 0.f && zd >= 0.f) {
                    const NcPixel p = nc_pixel(zl, zr, zu, zd, xh, nc_centre(py, H), a.fx, a.fy);
#pragma unroll
                    for (int i = 0; i < 3; ++i) n[i] = (R[3 * i] * p.nd[0] + R[3 * i + 1] * p.nd[1]) + R[3 * i + 2] * p.nd[2];
                    if (a.out) {
                        const float N0 = a.normals[at3], N1 = a.normals[at3 + HW], N2 = a.normals[at3 + 2 * HW];
                        const float w = a.weight ? a.weight[at] : 1.f;
                        o = w * (1.f - ((N0 * n[0] + N1 * n[1]) + N2 * n[2]));
                    }
                }
            }
            if (a.out) a.out[at] = o;
            if (a.depth_normals) {
                a.depth_normals[at3] = n[0]; a.depth_normals[at3 + HW] = n[1]; a.depth_normals[at3 + 2 * HW] = n[2];
            }
        }
    }
}

__global__ void __launch_bounds__(kNcThreads) normal_consistency_bwd_kernel(const Nc a, int tiles_x, int tiles_y, int64_t ntiles) {
    __shared__ float zt[kNcZH][kNcZW];
    __shared__ float send[4][kNcGH][kNcGW];   // to the sample at x + 1, x - 1, y + 1, y - 1 of the pixel
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, W = a.W;
    const int64_t HW = (int64_t)H * W;
    const bool depth = a.d_invdepth || a.d_alpha;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int per = tiles_x * tiles_y;
        const int b = (int)(tile / per), rem = (int)(tile - (int64_t)b * per);
        const int oy = (rem / tiles_x) * kNcTH, ox = (rem % tiles_x) * kNcTW;
        const int64_t base = (int64_t)b * HW, base3 = (int64_t)b * 3 * HW;
        // phase 1: the depths of the window (tile + 2); a sample outside the frame is invalid
        for (int i = tid; i < kNcZH * kNcZW; i += kNcThreads) {
            const int wy = i / kNcZW, wx = i - wy * kNcZW;
            const int py = oy - 2 + wy, px = ox - 2 + wx;
            zt[wy][wx] = (px >= 0 && px < W && py >= 0 && py < H) ? nc_depth(a, base + (int64_t)py * W + px) : -1.f;
        }
        __syncthreads();
        // phase 2: what every pixel of the window (tile + 1) sends to its four neighbours
        float R[9];
        nc_rotation(a, b, R);
        for (int i = tid; i < kNcGH * kNcGW; i += kNcThreads) {
            const int gy = i / kNcGW, gx = i - gy * kNcGW;
            const int py = oy - 1 + gy, px = ox - 1 + gx;
            const bool own = gy >= 1 && gy <= kNcTH && gx >= 1 && gx <= kNcTW && px < W && py < H;   // a pixel of the tile itself
            if (!own && !depth) continue;
            float s[4] = {0.f, 0.f, 0.f, 0.f}, dn[3] = {0.f, 0.f, 0.f};
            if (px >= 1 && px <= W - 2 && py >= 1 && py <= H - 2) {
                const float zc = zt[gy + 1][gx + 1], zl = zt[gy + 1][gx], zr = zt[gy + 1][gx + 2];
                const float zu = zt[gy][gx + 1], zd = zt[gy + 2][gx + 1];
                if (zc >= 0.f && zl >= 0.f && zr >= 0.f && zu >= 0.f && zd >= 0.f) {
                    const float xh = nc_centre(px, W), yh = nc_centre(py, H);
                    const NcPixel p = nc_pixel(zl, zr, zu, zd, xh, yh, a.fx, a.fy);
                    const int64_t at = base + (int64_t)py * W + px, at3 = base3 + (int64_t)py * W + px;
                    const float gw = a.d_out[at] * (a.weight ? a.weight[at] : 1.f);
                    if (own && a.d_normals) {
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            dn[k] = 0.f - gw * ((R[3 * k] * p.nd[0] + R[3 * k + 1] * p.nd[1]) + R[3 * k + 2] * p.nd[2]);
                    }
                    if (depth) {
                        const float N0 = a.normals[at3], N1 = a.normals[at3 + HW], N2 = a.normals[at3 + 2 * HW];
                        float v[3];
#pragma unroll
                        for (int j = 0; j < 3; ++j) v[j] = 0.f - gw * ((R[j] * N0 + R[3 + j] * N1) + R[6 + j] * N2);
                        const float t = (p.nd[0] * v[0] + p.nd[1] * v[1]) + p.nd[2] * v[2];
                        const float u0 = (v[0] - p.nd[0] * t) / p.len, u1 = (v[1] - p.nd[1] * t) / p.len;
                        const float u2 = (v[2] - p.nd[2] * t) / p.len;
                        const float hx = (u0 * a.fx - u2 * xh) / (p.sx * p.sx), hy = (u1 * a.fy - u2 * yh) / (p.sy * p.sy);
                        s[0] = hx * (zl + zl); s[1] = 0.f - hx * (zr + zr);
                        s[2] = hy * (zu + zu); s[3] = 0.f - hy * (zd + zd);
                    }
                }
            }
            if (depth) { send[0][gy][gx] = s[0]; send[1][gy][gx] = s[1]; send[2][gy][gx] = s[2]; send[3][gy][gx] = s[3]; }
            if (own && a.d_normals) {
                const int64_t at3 = base3 + (int64_t)py * W + px;
                a.d_normals[at3] = dn[0]; a.d_normals[at3 + HW] = dn[1]; a.d_normals[at3 + 2 * HW] = dn[2];
            }
        }
        __syncthreads();
        // phase 3: every sample of the tile adds its four
        const int px = ox + lane;
        if (depth && px < W) {
            for (int ty = wave; ty < kNcTH && oy + ty < H; ty += 4) {
                const int gy = ty + 1, gx = lane + 1;
                const float z = zt[ty + 2][lane + 2];
                const int64_t at = base + (int64_t)(oy + ty) * W + px;
                float di = 0.f, da = 0.f;
                if (z >= 0.f) {
                    const float dz = ((send[0][gy][gx - 1] + send[1][gy][gx + 1]) + send[2][gy - 1][gx]) + send[3][gy + 1][gx];
                    const float d = a.invdepth[at];
                    di = 0.f - (dz * z) / d;
                    da = dz / d;
                }
                if (a.d_invdepth) a.d_invdepth[at] = di;
                if (a.d_alpha) a.d_alpha[at] = da;
            }
        }
        __syncthreads();   // (the next tile's staging overwrites the window)
    }
}

// ---- the per-Gaussian normal ----

struct Gn {
    int64_t P;
    const float* rot; const float* scales; const float* means; const float* campos;
    float* normals; const float* d_normals; float* d_rot;
};

template <bool kBwd>
__global__ void __launch_bounds__(kGnThreads) gaussian_normals_kernel(const Gn a) {
    const int64_t i = (int64_t)blockIdx.x * kGnThreads + threadIdx.x;
    if (i >= a.P) return;
    const f4 q = *reinterpret_cast<const f4*>(a.rot + 4 * i);
    const float len = quat_length(q.x, q.y, q.z, q.w);
    if (!(len > 0.f && len < INFINITY)) {   // |q| = 0 (or a NaN / Inf component): no direction, no gradient
        if (kBwd) {
            f4 zero; zero.x = zero.y = zero.z = zero.w = 0.f;
            *reinterpret_cast<f4*>(a.d_rot + 4 * i) = zero;
        } else {
            a.normals[3 * i] = 0.f; a.normals[3 * i + 1] = 0.f; a.normals[3 * i + 2] = 0.f;
        }
        return;
    }
    const float w = q.x / len, x = q.y / len, y = q.z / len, z = q.w / len;
    const float s0 = a.scales[3 * i], s1 = a.scales[3 * i + 1], s2 = a.scales[3 * i + 2];
    int k = 0;
    float best = s0;
    if (s1 < best) { k = 1; best = s1; }
    if (s2 < best) k = 2;
    float c0, c1, c2;   // column k of R
    if (k == 0) { c0 = 1.f - 2.f * (y * y + z * z); c1 = 2.f * (x * y + w * z); c2 = 2.f * (x * z - w * y); }
    else if (k == 1) { c0 = 2.f * (x * y - w * z); c1 = 1.f - 2.f * (x * x + z * z); c2 = 2.f * (y * z + w * x); }
    else { c0 = 2.f * (x * z + w * y); c1 = 2.f * (y * z - w * x); c2 = 1.f - 2.f * (x * x + y * y); }
    const float e0 = a.campos[0] - a.means[3 * i], e1 = a.campos[1] - a.means[3 * i + 1], e2 = a.campos[2] - a.means[3 * i + 2];
    const bool keep = (c0 * e0 + c1 * e1) + c2 * e2 >= 0.f;
    if (!kBwd) {
        a.normals[3 * i] = keep ? c0 : 0.f - c0; a.normals[3 * i + 1] = keep ? c1 : 0.f - c1; a.normals[3 * i + 2] = keep ? c2 : 0.f - c2;
        return;
    }
    float g0 = a.d_normals[3 * i], g1 = a.d_normals[3 * i + 1], g2 = a.d_normals[3 * i + 2];
    if (!keep) { g0 = 0.f - g0; g1 = 0.f - g1; g2 = 0.f - g2; }
    float dw, dx, dy, dz;   // with respect to the unit quaternion
    if (k == 0) {
        dw = 2.f * (z * g1 - y * g2); dx = 2.f * (y * g1 + z * g2);
        dy = 2.f * (x * g1 - w * g2) - 4.f * (y * g0); dz = 2.f * (w * g1 + x * g2) - 4.f * (z * g0);
    } else if (k == 1) {
        dw = 2.f * (x * g2 - z * g0); dx = 2.f * (y * g0 + w * g2) - 4.f * (x * g1);
        dy = 2.f * (x * g0 + z * g2); dz = 2.f * (y * g2 - w * g0) - 4.f * (z * g1);
    } else {
        dw = 2.f * (y * g0 - x * g1); dx = 2.f * (z * g0 - w * g1) - 4.f * (x * g2);
        dy = 2.f * (w * g0 + z * g1) - 4.f * (y * g2); dz = 2.f * (x * g0 + y * g1);
    }
    // through q / |q|: (d - qh (qh . d)) / |q|
    const float t = ((w * dw + x * dx) + y * dy) + z * dz;
    f4 o;
    o.x = (dw - w * t) / len; o.y = (dx - x * t) / len; o.z = (dy - y * t) / len; o.w = (dz - z * t) / len;
    *reinterpret_cast<f4*>(a.d_rot + 4 * i) = o;
}

// ---- host ----

int check_frame(const char* fn, int B, int H, int W) {
    if (B < 1) { set_error("%s: B=%d must be at least 1", fn, B); return HS_EINVAL; }
    if (H < 1) { set_error("%s: H=%d must be at least 1", fn, H); return HS_EINVAL; }
    if (W < 1) { set_error("%s: W=%d must be at least 1", fn, W); return HS_EINVAL; }
    // (in floating point first: three factors below 2^31 overflow an int64 product)
    if (3.0 * B * H * W >= 2147483648.0) {
        set_error("%s: 3*B*H*W=%.0f must be below 2^31", fn, 3.0 * B * H * W);
        return HS_EINVAL;
    }
    return HS_OK;
}

int check_nc_args(const char* fn, const hs_normal_consistency_args* a, bool backward) {
    if (check_args(fn, a) || check_frame(fn, a->B, a->H, a->W)) return HS_EINVAL;
    if (!(a->fx > 0.f && a->fx < INFINITY && a->fy > 0.f && a->fy < INFINITY)) {
        set_error("%s: fx=%g, fy=%g must be finite and positive", fn, (double)a->fx, (double)a->fy);
        return HS_EINVAL;
    }
    if (check_field(fn, a->invdepth, "invdepth", 4)) return HS_EINVAL;
    if (check_aligned(fn, a->alpha, "alpha", 4) || check_aligned(fn, a->weight, "weight", 4) ||
        check_aligned(fn, a->cam_to_world, "cam_to_world", 4))
        return HS_EINVAL;
    if (!backward) {
        if (!a->out && !a->depth_normals) { set_error("%s: null out and null depth_normals: nothing to write", fn); return HS_EINVAL; }
        if (check_aligned(fn, a->out, "out", 4) || check_aligned(fn, a->depth_normals, "depth_normals", 4)) return HS_EINVAL;
        if (a->out && check_field(fn, a->normals, "normals", 4, " (needed with out)")) return HS_EINVAL;
        return check_aligned(fn, a->normals, "normals", 4);
    }
    const Field f[2] = {{a->normals, "normals", 4}, {a->dL_dout, "dL_dout", 4}};
    if (check_fields(fn, f, 2)) return HS_EINVAL;
    if (check_aligned(fn, a->dL_dnormals, "dL_dnormals", 4) || check_aligned(fn, a->dL_dinvdepth, "dL_dinvdepth", 4) ||
        check_aligned(fn, a->dL_dalpha, "dL_dalpha", 4))
        return HS_EINVAL;
    if (a->dL_dalpha && !a->alpha) { set_error("%s: dL_dalpha without alpha: an absent input has no gradient", fn); return HS_EINVAL; }
    return HS_OK;
}

Nc nc_of(const hs_normal_consistency_args& a) {
    Nc n;
    memset(&n, 0, sizeof(n));
    n.B = a.B; n.H = a.H; n.W = a.W; n.fx = a.fx; n.fy = a.fy;
    n.invdepth = a.invdepth; n.alpha = a.alpha; n.normals = a.normals; n.weight = a.weight; n.rot = a.cam_to_world;
    n.out = a.out; n.depth_normals = a.depth_normals;
    n.d_out = a.dL_dout; n.d_normals = a.dL_dnormals; n.d_invdepth = a.dL_dinvdepth; n.d_alpha = a.dL_dalpha;
    return n;
}

int check_gn_args(const char* fn, const hs_gaussian_normals_args* a, bool backward) {
    if (check_args(fn, a) || check_rows(fn, "P", a->P)) return HS_EINVAL;
    if (a->P == 0) return HS_OK;   // no rows: nothing is looked at
    Field f[6] = {{a->rotations, "rotations", 16}, {a->scales, "scales", 4}, {a->means3D, "means3D", 4}, {a->campos, "campos", 4}};
    int n = 4;
    if (backward) { f[n++] = {a->dL_dnormals, "dL_dnormals", 4}; f[n++] = {a->dL_drotations, "dL_drotations", 16}; }
    else f[n++] = {a->normals, "normals", 4};
    return check_fields(fn, f, n);
}

template <bool kBwd>
int launch_gn(const hs_gaussian_normals_args& a, hipStream_t s) {
    if (a.P == 0) return HS_OK;
    Gn g;
    memset(&g, 0, sizeof(g));
    g.P = a.P; g.rot = a.rotations; g.scales = a.scales; g.means = a.means3D; g.campos = a.campos;
    g.normals = a.normals; g.d_normals = a.dL_dnormals; g.d_rot = a.dL_drotations;
    gaussian_normals_kernel<kBwd><<<(unsigned)((a.P + kGnThreads - 1) / kGnThreads), kGnThreads, 0, s>>>(g);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_normal_consistency_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (hs::check_frame("hs_normal_consistency_workspace_bytes", B, H, W)) return HS_EINVAL;
    return 0;   // the backward keeps its halo in LDS
}

HS_API int hs_normal_consistency(const hs_normal_consistency_args* a, void* hip_stream) {
    const int rc = hs::check_nc_args("hs_normal_consistency", a, false);
    if (rc != HS_OK) return rc;
    const int tiles_x = (a->W + hs::kNcTW - 1) / hs::kNcTW, tiles_y = (a->H + hs::kNcTH - 1) / hs::kNcTH;
    const int64_t ntiles = (int64_t)a->B * tiles_x * tiles_y;
    const unsigned grid = (unsigned)(ntiles < hs::kNcMaxGrid ? ntiles : hs::kNcMaxGrid);
    hs::normal_consistency_kernel<<<grid, hs::kNcThreads, 0, (hipStream_t)hip_stream>>>(hs::nc_of(*a), tiles_x, tiles_y, ntiles);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

HS_API int hs_normal_consistency_backward(const hs_normal_consistency_args* a, void* hip_stream) {
    const int rc = hs::check_nc_args("hs_normal_consistency_backward", a, true);
    if (rc != HS_OK) return rc;
    if (!a->dL_dnormals && !a->dL_dinvdepth && !a->dL_dalpha) return HS_OK;
    const int tiles_x = (a->W + hs::kNcTW - 1) / hs::kNcTW, tiles_y = (a->H + hs::kNcTH - 1) / hs::kNcTH;
    const int64_t ntiles = (int64_t)a->B * tiles_x * tiles_y;
    const unsigned grid = (unsigned)(ntiles < hs::kNcMaxGrid ? ntiles : hs::kNcMaxGrid);
    hs::normal_consistency_bwd_kernel<<<grid, hs::kNcThreads, 0, (hipStream_t)hip_stream>>>(hs::nc_of(*a), tiles_x, tiles_y, ntiles);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

HS_API int hs_gaussian_normals(const hs_gaussian_normals_args* a, void* hip_stream) {
    const int rc = hs::check_gn_args("hs_gaussian_normals", a, false);
    if (rc != HS_OK) return rc;
    return hs::launch_gn<false>(*a, (hipStream_t)hip_stream);
}

HS_API int hs_gaussian_normals_backward(const hs_gaussian_normals_args* a, void* hip_stream) {
    const int rc = hs::check_gn_args("hs_gaussian_normals_backward", a, true);
    if (rc != HS_OK) return rc;
    return hs::launch_gn<true>(*a, (hipStream_t)hip_stream);
}

}  // extern "C"
