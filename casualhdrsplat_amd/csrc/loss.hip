// Fused L1 + D-SSIM photometric loss of the published 3DGS train.py, forward and backward (hs_photometric_loss,
// hs_photometric_loss_backward):
//
//   loss = (1 - lambda) * mean|x - y| + lambda * (1 - mean SSIM(x, y))
//
// SSIM as the published ssim(): 11 x 11 Gaussian window, sigma 1.5, zero padding (conv2d(padding=5, groups=C)),
// C1 = 0.01^2, C2 = 0.03^2, averaged over every channel and pixel.  A plane is one channel of one image.  Per plane and
// output pixel q, with w the separable window:
//
//   m1 = Σw·x, m2 = Σw·y, e11 = Σw·x², e22 = Σw·y², e12 = Σw·x·y
//   σ1 = e11 − m1², σ2 = e22 − m2², σ12 = e12 − m1·m2
//   A1 = 2·m1·m2 + C1, A2 = 2·σ12 + C2, B1 = m1² + m2² + C1, B2 = σ1 + σ2 + C2,   S = A1·A2 / (B1·B2)
//
// Sums are accumulated and the per-pixel terms evaluated in fp64 (the staged values and the partial sums between the two
// passes are fp32): on flat regions σ = e − m² cancels almost entirely, and the fp32 formulation's error there is what
// the tests hold this one to.
//
// Forward (loss_fwd_kernel): one workgroup per 64 x 16 output tile of one plane.  The tile and its 5-pixel halo of x and y
// go to LDS (zeros outside the image), a horizontal pass puts the five moments of every halo row into LDS, and a vertical
// pass slides the window down a 4-row column strip per thread in registers.  With gradients wanted it also writes three
// per-pixel partials of S,
//   D_m = dS/dm1 = 2·m2·(A2 − A1)/(B1·B2) − 2·m1·S·(1/B1 − 1/B2),   D_e = dS/de11 = −S/B2,   D_x = dS/de12 = 2·A1/(B1·B2),
// and it writes one fp64 (ΣS, Σ|x−y|) pair per tile.  loss_reduce_kernel adds the pairs up in a fixed order (fp64, no atomics:
// the same inputs give the same bits on every run) into out = {loss, l1_mean, ssim_mean}.
//
// Backward (loss_bwd_kernel): the window is symmetric, so the adjoint of the zero-padded correlation is the same correlation
// summed over the q inside the image:
//   dloss/dx(p) = g · [ (1−λ)·sign(x−y)/N − λ/N · Σ_q w(q−p)·(D_m(q) + 2·x(p)·D_e(q) + y(p)·D_x(q)) ]
// -- the three partial planes are staged with their halo (zeros outside) and run through the same separable pass.  g, the
// upstream gradient of the loss scalar, is read from device memory: the backward needs no host value and can be captured.
#include "hs_common.h"

#include <math.h>

namespace hs {
namespace {

constexpr int kLR = 5;                    // window radius
constexpr int kLTaps = 2 * kLR + 1;       // 11 taps
constexpr int kLTW = 64;                  // output tile: 64 columns (one wave across) ...
constexpr int kLTH = 16;                  // ... by 16 rows
constexpr int kLSW = kLTW + 2 * kLR;      // staged columns (74)
constexpr int kLSH = kLTH + 2 * kLR;      // staged rows (26)
constexpr int kLThreads = 256;            // four waves: wave v owns rows 4v .. 4v+3 of the tile in the vertical pass
constexpr int kLStrip = kLTH / (kLThreads / kLTW);   // 4 output rows per thread
constexpr int kLReduce = 256;
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;
static_assert(kLStrip * (kLThreads / kLTW) == kLTH, "the column strips cover the tile");

struct LossWin {
    float g[kLTaps];   // 1-D weights: exp(-(i-5)^2 / 4.5) in double, stored as fp32, normalised in fp32 (loss_window)
};

struct LossTiles {
    int H, W, tiles_x, tiles_y;
    int64_t ntiles;
};

__device__ __forceinline__ void tile_origin(const LossTiles& t, int64_t tile, int64_t& plane, int& ox, int& oy) {
    const int64_t per_plane = (int64_t)t.tiles_x * t.tiles_y;
    plane = tile / per_plane;
    const int r = (int)(tile - plane * per_plane);
    oy = (r / t.tiles_x) * kLTH;
    ox = (r % t.tiles_x) * kLTW;
}

// stage Q planes (each [H, W], the tile's plane) with the halo, zeros outside the image
template <int Q>
__device__ __forceinline__ void stage(float (*dst)[kLSH][kLSW], const float* const* src, const LossTiles& t, int64_t plane,
                                      int ox, int oy) {
    const int64_t base = plane * (int64_t)t.H * t.W;
    for (int i = threadIdx.x; i < kLSH * kLSW; i += kLThreads) {
        const int r = i / kLSW, c = i - r * kLSW;
        const int64_t gy = (int64_t)oy - kLR + r, gx = (int64_t)ox - kLR + c;   // (64-bit: W may reach 2^31 - 1)
        const bool in = gy >= 0 && gy < t.H && gx >= 0 && gx < t.W;
        const int64_t at = base + (int64_t)gy * t.W + gx;
#pragma unroll
        for (int q = 0; q < Q; ++q) dst[q][r][c] = in ? src[q][at] : 0.0f;
    }
}

template <bool kGrad>
__global__ void __launch_bounds__(kLThreads) loss_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             LossTiles t, LossWin w, double2* __restrict__ pairs,
                                                             float* __restrict__ partials) {
    __shared__ float sxy[2][kLSH][kLSW];
    __shared__ float hm[5][kLSH][kLTW];
    __shared__ double red[2][kLThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t N = (int64_t)t.H * t.W * (t.ntiles / ((int64_t)t.tiles_x * t.tiles_y));
    for (int64_t tile = blockIdx.x; tile < t.ntiles; tile += gridDim.x) {
        int64_t plane; int ox, oy;
        tile_origin(t, tile, plane, ox, oy);
        const float* src[2] = {x, y};
        stage<2>(sxy, src, t, plane, ox, oy);
        __syncthreads();
        // horizontal pass: the five moments of every staged row at the tile's 64 columns
        for (int i = tid; i < kLSH * kLTW; i += kLThreads) {
            const int r = i / kLTW, c = i - r * kLTW;
            double a1 = 0.0, a2 = 0.0, a11 = 0.0, a22 = 0.0, a12 = 0.0;
#pragma unroll
            for (int k = 0; k < kLTaps; ++k) {
                const double u = sxy[0][r][c + k], v = sxy[1][r][c + k], gk = w.g[k];
                const double gu = gk * u, gv = gk * v;   // (exact: fp32 x fp32 products fit an fp64 mantissa)
                a1 += gu; a2 += gv; a11 += gu * u; a22 += gv * v; a12 += gu * v;
            }
            hm[0][r][c] = (float)a1; hm[1][r][c] = (float)a2; hm[2][r][c] = (float)a11; hm[3][r][c] = (float)a22;
            hm[4][r][c] = (float)a12;
        }
        __syncthreads();
        // vertical pass: lane = column, wave = strip of kLStrip output rows; every staged row is read once and added to the
        // (up to) kLStrip outputs it reaches
        double acc[kLStrip][5];
#pragma unroll
        for (int o = 0; o < kLStrip; ++o)
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[o][m] = 0.0;
        const int r0 = wave * kLStrip;
#pragma unroll
        for (int j = 0; j < kLStrip + 2 * kLR; ++j) {
            double v[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] = hm[m][r0 + j][lane];
#pragma unroll
            for (int o = 0; o < kLStrip; ++o) {
                const int k = j - o;
                if (k >= 0 && k < kLTaps) {
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[o][m] += (double)w.g[k] * v[m];
                }
            }
        }
        double sumS = 0.0;
        float sumL = 0.f;
        const int64_t gx = (int64_t)ox + lane;
#pragma unroll
        for (int o = 0; o < kLStrip; ++o) {
            const int64_t gy = (int64_t)oy + r0 + o;
            if (gx < t.W && gy < t.H) {
                // (fp64: sigma = e - m^2 cancels almost entirely on flat image regions)
                const double m1 = acc[o][0], m2 = acc[o][1];
                const double s1 = acc[o][2] - m1 * m1, s2 = acc[o][3] - m2 * m2, s12 = acc[o][4] - m1 * m2;
                const double A1 = 2.0 * m1 * m2 + kC1, A2 = 2.0 * s12 + kC2;
                const double B1 = m1 * m1 + m2 * m2 + kC1, B2 = s1 + s2 + kC2;
                const double inv = 1.0 / (B1 * B2);
                const double S = A1 * A2 * inv;
                sumS += S;
                sumL += fabsf(sxy[0][r0 + o + kLR][lane + kLR] - sxy[1][r0 + o + kLR][lane + kLR]);
                if (kGrad) {
                    const int64_t at = plane * (int64_t)t.H * t.W + (int64_t)gy * t.W + gx;
                    partials[at] = (float)(2.0 * m2 * (A2 - A1) * inv - 2.0 * m1 * S * (1.0 / B1 - 1.0 / B2));
                    partials[N + at] = (float)(-S / B2);
                    partials[2 * N + at] = (float)(2.0 * A1 * inv);
                }
            }
        }
        // the tile's pair: fp64 sums over the wave (fixed butterfly), then over the four waves in order
        double dS = sumS, dL = sumL;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            dS += __shfl_xor(dS, off, 64);
            dL += __shfl_xor(dL, off, 64);
        }
        if (lane == 0) { red[0][wave] = dS; red[1][wave] = dL; }
        __syncthreads();
        if (tid == 0) {
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int v = 0; v < kLThreads / 64; ++v) { a += red[0][v]; b += red[1][v]; }
            pairs[tile] = make_double2(a, b);
        }
        // (the next tile's staging and `red` writes come after this barrier; thread 0 has read `red` before reaching it)
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kLReduce) loss_reduce_kernel(const double2* __restrict__ pairs, int64_t n, double inv_N,
                                                               double lambda, float* __restrict__ out) {
    __shared__ double red[2][kLReduce];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t i = tid; i < n; i += kLReduce) {
        const double2 p = pairs[i];
        a += p.x;
        b += p.y;
    }
    red[0][tid] = a;
    red[1][tid] = b;
    __syncthreads();
    for (int s = kLReduce / 2; s > 0; s >>= 1) {
        if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double ssim = red[0][0] * inv_N, l1 = red[1][0] * inv_N;
        out[0] = (float)((1.0 - lambda) * l1 + lambda * (1.0 - ssim));
        out[1] = (float)l1;
        out[2] = (float)ssim;
    }
}

__global__ void __launch_bounds__(kLThreads) loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ partials, const float* __restrict__ dL_dloss,
                                                             LossTiles t, LossWin w, double c_l1, double c_ssim,
                                                             float* __restrict__ dL_dx) {
    __shared__ float sp[3][kLSH][kLSW];
    __shared__ float hp[3][kLSH][kLTW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t HW = (int64_t)t.H * t.W;
    const int64_t N = HW * (t.ntiles / ((int64_t)t.tiles_x * t.tiles_y));
    const float g = *dL_dloss;
    for (int64_t tile = blockIdx.x; tile < t.ntiles; tile += gridDim.x) {
        int64_t plane; int ox, oy;
        tile_origin(t, tile, plane, ox, oy);
        const float* src[3] = {partials, partials + N, partials + 2 * N};
        stage<3>(sp, src, t, plane, ox, oy);
        __syncthreads();
        for (int i = tid; i < kLSH * kLTW; i += kLThreads) {
            const int r = i / kLTW, c = i - r * kLTW;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
            for (int k = 0; k < kLTaps; ++k) {
                const double gk = w.g[k];
                a0 += gk * sp[0][r][c + k]; a1 += gk * sp[1][r][c + k]; a2 += gk * sp[2][r][c + k];
            }
            hp[0][r][c] = (float)a0; hp[1][r][c] = (float)a1; hp[2][r][c] = (float)a2;
        }
        __syncthreads();
        double acc[kLStrip][3];
#pragma unroll
        for (int o = 0; o < kLStrip; ++o)
#pragma unroll
            for (int m = 0; m < 3; ++m) acc[o][m] = 0.0;
        const int r0 = wave * kLStrip;
#pragma unroll
        for (int j = 0; j < kLStrip + 2 * kLR; ++j) {
            double v[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) v[m] = hp[m][r0 + j][lane];
#pragma unroll
            for (int o = 0; o < kLStrip; ++o) {
                const int k = j - o;
                if (k >= 0 && k < kLTaps) {
#pragma unroll
                    for (int m = 0; m < 3; ++m) acc[o][m] += (double)w.g[k] * v[m];
                }
            }
        }
        const int64_t gx = (int64_t)ox + lane;
#pragma unroll
        for (int o = 0; o < kLStrip; ++o) {
            const int64_t gy = (int64_t)oy + r0 + o;
            if (gx < t.W && gy < t.H) {
                const int64_t at = plane * HW + (int64_t)gy * t.W + gx;
                const float xv = x[at], yv = y[at];
                const float d = xv - yv;
                const double sgn = d > 0.f ? 1.0 : (d < 0.f ? -1.0 : 0.0);
                const double dssim = acc[o][0] + 2.0 * xv * acc[o][1] + (double)yv * acc[o][2];
                // (g multiplies last, in fp32: k * loss gives exactly k times the gradient of loss)
                dL_dx[at] = g * (float)(c_l1 * sgn - c_ssim * dssim);
            }
        }
        __syncthreads();   // (the next tile's staging overwrites sp / hp)
    }
}

LossWin loss_window() {
    // the published gaussian(): fp32 taps divided by their fp32 sum -- the correctly rounded one, as torch's sum of these 11
    // values gives (a sequential fp32 sum is one ulp off, and so would be two of the taps)
    LossWin w;
    double s = 0.0;
    for (int i = 0; i < kLTaps; ++i) {
        w.g[i] = (float)exp(-(double)((i - kLR) * (i - kLR)) / 4.5);
        s += w.g[i];
    }
    const float sf = (float)s;
    for (int i = 0; i < kLTaps; ++i) w.g[i] /= sf;
    return w;
}

LossTiles loss_tiles(int planes, int H, int W) {
    LossTiles t;
    t.H = H; t.W = W;
    t.tiles_x = (int)(((int64_t)W + kLTW - 1) / kLTW);
    t.tiles_y = (int)(((int64_t)H + kLTH - 1) / kLTH);
    t.ntiles = (int64_t)planes * t.tiles_x * t.tiles_y;
    return t;
}

// a grid of at most this many workgroups walks the tiles of larger problems (its blocks stride over them)
constexpr int64_t kLMaxGrid = 1 << 20;

}  // namespace

int64_t loss_pair_count(int planes, int H, int W) { return loss_tiles(planes, H, W).ntiles; }

int launch_loss_fwd(const hs_loss_args& a, hipStream_t s) {
    const LossTiles t = loss_tiles(a.planes, a.H, a.W);
    const LossWin w = loss_window();
    const unsigned grid = (unsigned)(t.ntiles < kLMaxGrid ? t.ntiles : kLMaxGrid);
    double2* pairs = (double2*)a.workspace;
    if (a.partials)
        loss_fwd_kernel<true><<<grid, kLThreads, 0, s>>>(a.image, a.target, t, w, pairs, a.partials);
    else
        loss_fwd_kernel<false><<<grid, kLThreads, 0, s>>>(a.image, a.target, t, w, pairs, nullptr);
    HS_LAUNCH_CHECK();
    const double N = (double)a.planes * a.H * a.W;
    loss_reduce_kernel<<<1, kLReduce, 0, s>>>(pairs, t.ntiles, 1.0 / N, (double)a.lambda_dssim, a.out);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

int launch_loss_bwd(const hs_loss_args& a, hipStream_t s) {
    const LossTiles t = loss_tiles(a.planes, a.H, a.W);
    const LossWin w = loss_window();
    const unsigned grid = (unsigned)(t.ntiles < kLMaxGrid ? t.ntiles : kLMaxGrid);
    const double N = (double)a.planes * a.H * a.W;
    const double c_l1 = (1.0 - (double)a.lambda_dssim) / N, c_ssim = (double)a.lambda_dssim / N;
    loss_bwd_kernel<<<grid, kLThreads, 0, s>>>(a.image, a.target, a.partials, a.dL_dloss, t, w, c_l1, c_ssim, a.dL_dimage);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // namespace hs
