// Bilateral-grid image correction ("Bilateral Guided Radiance Field Processing", SIGGRAPH 2024), fused: the slice of a batch
// of images through per-frame lattices of 3 x 4 affine colour matrices, its backward to the image and to the grids, and the
// total-variation regulariser of the grids with its backward (hs_bilagrid_workspace_bytes, hs_bilagrid_slice,
// hs_bilagrid_slice_backward, hs_bilagrid_tv, hs_bilagrid_tv_backward; include/hdrsplat.h states the definition).
//
// Compiled with -ffp-contract=off: the per-pixel arithmetic below is a STATED ORDER of IEEE fp32 operations, which
// tests/bilagrid_reference.py restates in numpy float32 and the GPU tests compare bit for bit.  Do not reassociate it.
//
//   per axis of n lattice points and a value v (bg_axis):  n == 1: i0 = i1 = 0, f = 0;  else
//       c = v > 0 ? v : 0;  c = c < 1 ? c : 1;  t = c * float(n - 1);  i0 = min(int(floor(t)), n - 2);  i1 = i0 + 1;
//       f = t - float(i0)                                                      (a NaN v counts as 0)
//   pixel (px, py):  x = (float(px) + 0.5f) / float(W),  y = (float(py) + 0.5f) / float(H),
//       z = (0.299f * r + 0.587f * g) + 0.114f * b
//   weights:  wa[0] = 1 - fa, wa[1] = fa for a = x, y, z;  w[dz][dy][dx] = (wz[dz] * wy[dy]) * wx[dx]
//   A[c]   = the eight products w[dz][dy][dx] * grid[c][iz_dz][iy_dy][ix_dx] added in the order dz, dy, dx (dx fastest)
//   out_i  = ((A[4i] * r + A[4i+1] * g) + A[4i+2] * b) + A[4i+3]
//   backward to the image, with d = dL_dout:
//       direct_k = (A[k] * d0 + A[4+k] * d1) + A[8+k] * d2
//       if 0 < z < 1 and L > 1:  u[dy][dx] = wy[dy] * wx[dx];
//           D[c] = the four products u[dy][dx] * (grid[c][iz_1][..] - grid[c][iz_0][..]) added in the order dy, dx
//           s_i = ((D[4i] * r + D[4i+1] * g) + D[4i+2] * b) + D[4i+3];  S = ((d0 * s0 + d1 * s1) + d2 * s2) * float(L - 1)
//           dL_dimage_k = direct_k + luma_k * S        (luma = 0.299f, 0.587f, 0.114f)
//       else dL_dimage_k = direct_k
//   a frame whose grid id is outside [0, G): out = image and dL_dimage = dL_dout, copied bit for bit.
//
// bilagrid_pixel_kernel<kBwd>   one workgroup per 64 x 16 pixel tile of one frame, lane = column, wave = rows wave, wave + 4, ...
//                        The lattice cells the tile can touch -- [i0 of its first column, i1 of its last] x the same in y x every
//                        l x 12 -- are staged in LDS once when they fit kBgStage floats (16 x 16 x 8 on 1080p: at most 3 x 3 x 8
//                        x 12 = 3.4 KB); a tile that sees more (a grid finer than the pixels) reads the grid from memory.
// bilagrid_grid_partial_kernel<LP>   the grid gradient is a GATHER PER DESTINATION: a workgroup owns one lattice column
//                        (frame, yy, xx) and one chunk of kBgChunkRows rows of that column's pixel footprint (bg_footprint: a
//                        superset of the pixels whose axis rule names the column; every pixel recomputes its own i0, i1, f by
//                        the forward's code and takes part only where they name the column).  Thread-private fp32 accumulators
//                        for the column's L x 12 sums in registers (selects over l, LP = L rounded up to 2, 4, 8, 16), a fixed
//                        DPP tree over the wave, the four waves added in order, one record of 12 L floats per workgroup.
// bilagrid_grid_sum_kernel   one thread per element of dL_dgrids: the records of the frames with grid_ids[fr] == g in ascending
//                        fr, chunks ascending.  Every element is written (a grid no frame used: exact zeros); every record it
//                        reads was written by the kernel before it, whatever the workspace held.
// bilagrid_tv_kernel / bilagrid_tv_sum_kernel / bilagrid_tv_bwd_kernel   differences in fp64 (exact), per-block fp64 sums of
//                        the three axes, one workgroup adds the blocks in a fixed order; the backward reads dL_dtv on the device.
// No atomics, no memset, no copy, no synchronisation: the same inputs give the same bits, also inside a captured graph.
#include "hs_cloud.h"

#include <math.h>
#include <string.h>

namespace hs {
namespace {

constexpr int kBgTW = 64, kBgTH = 16, kBgThreads = 256;   // pixel tile; four waves
constexpr int kBgStage = 8192;                            // floats of LDS a tile's lattice cells may take (32 KB)
#ifndef HS_TUNE_BG_CHUNK_ROWS
#define HS_TUNE_BG_CHUNK_ROWS 32
#endif
constexpr int kBgChunkRows = HS_TUNE_BG_CHUNK_ROWS;       // footprint rows per workgroup of the grid gradient
constexpr int kBgMaxL = 16, kBgMaxXY = 64;
constexpr int kTvThreads = 256, kTvMaxBlocks = 1024;
constexpr int64_t kBgMaxGrid = 1 << 20;

struct Bg {
    int F, H, W, G, L, Y, X;
    const float* image; const float* grids; const int32_t* ids;
    float* out; const float* d_out; float* d_image;
};

__device__ __forceinline__ void bg_axis(float v, int n, int& i0, int& i1, float& f) {
    if (n == 1) { i0 = 0; i1 = 0; f = 0.f; return; }
    float c = v > 0.f ? v : 0.f;
    c = c < 1.f ? c : 1.f;
    const float t = c * (float)(n - 1);
    const int fl = (int)floorf(t);
    i0 = fl < n - 2 ? fl : n - 2;
    i1 = i0 + 1;
    f = t - (float)i0;
}

__device__ __forceinline__ float bg_coord(int p, int n) { return ((float)p + 0.5f) / (float)n; }

// Pixels [lo, hi] of an axis of n pixels that CAN name lattice index j of m: those with t = (p + 0.5) / n * (m - 1) in
// [j - 1, j + 1], widened by 2 + n / 2^20 pixels for the rounding of the fp32 t (relative 2^-22: n 2^-22 pixels).
__host__ __device__ inline void bg_footprint(int n, int m, int j, int& lo, int& hi) {
    if (m == 1) { lo = 0; hi = n - 1; return; }
    const int64_t margin = 2 + (n >> 20);
    const int64_t a = j == 0 ? 0 : ((int64_t)(j - 1) * n) / (m - 1) - margin;
    const int64_t b = ((int64_t)(j + 1) * n + (m - 2)) / (m - 1) + margin;
    lo = (int)(a > 0 ? a : 0);
    hi = (int)(b < n - 1 ? b : n - 1);
}

template <bool kBwd>
__global__ void __launch_bounds__(kBgThreads) bilagrid_pixel_kernel(const Bg a, int tiles_x, int tiles_y, int64_t ntiles) {
    __shared__ float cells[kBgStage];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L, X = a.X, Y = a.Y;
    const int64_t HW = (int64_t)a.H * a.W;
    const float* __restrict__ src = kBwd ? a.d_out : a.image;   // what an identity frame copies
    float* __restrict__ dst = kBwd ? a.d_image : a.out;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int per = tiles_x * tiles_y;
        const int fr = (int)(tile / per), rem = (int)(tile - (int64_t)fr * per);
        const int oy = (rem / tiles_x) * kBgTH, ox = (rem % tiles_x) * kBgTW;
        const int g = a.ids[fr];
        const int px = ox + lane;
        const int64_t fbase = (int64_t)fr * 3 * HW;
        if (g < 0 || g >= a.G) {   // (uniform) no grid: the identity, bit for bit
            if (px < a.W)
                for (int py = oy + wave; py < oy + kBgTH && py < a.H; py += 4) {
                    const int64_t at = fbase + (int64_t)py * a.W + px;
                    dst[at] = src[at]; dst[at + HW] = src[at + HW]; dst[at + 2 * HW] = src[at + 2 * HW];
                }
            continue;
        }
        // the lattice cells this tile can touch (the axis rule is monotone: first pixel's i0 .. last pixel's i1)
        int xlo, xhi, ylo, yhi, t0, t1; float tf;
        const int lastx = ox + kBgTW - 1 < a.W - 1 ? ox + kBgTW - 1 : a.W - 1;
        const int lasty = oy + kBgTH - 1 < a.H - 1 ? oy + kBgTH - 1 : a.H - 1;
        bg_axis(bg_coord(ox, a.W), X, xlo, t1, tf);
        bg_axis(bg_coord(lastx, a.W), X, t0, xhi, tf);
        bg_axis(bg_coord(oy, a.H), Y, ylo, t1, tf);
        bg_axis(bg_coord(lasty, a.H), Y, t0, yhi, tf);
        const int nx = xhi - xlo + 1, ny = yhi - ylo + 1;
        const bool staged = nx * ny * L * 12 <= kBgStage;
        const float* __restrict__ gsrc = a.grids + (int64_t)g * 12 * L * Y * X;
        int sx, sy;              // row length and rows of the image of the grid that is read (LDS or memory)
        if (staged) {
            sx = nx; sy = ny;
            const int n = nx * ny * L * 12;
            for (int i = tid; i < n; i += kBgThreads) {
                const int x = i % nx, r1 = i / nx, y = r1 % ny, cl = r1 / ny;   // cl = c * L + l
                cells[i] = gsrc[((int64_t)cl * Y + (ylo + y)) * X + (xlo + x)];
            }
            __syncthreads();
        } else {
            sx = X; sy = Y; xlo = 0; ylo = 0;
        }
        const int sc = L * sy * sx;   // stride of a coefficient
        if (px < a.W) {
            int ix0, ix1; float fx;
            bg_axis(bg_coord(px, a.W), X, ix0, ix1, fx);
            const float wx[2] = {1.f - fx, fx};
            const int cx[2] = {ix0 - xlo, ix1 - xlo};
            for (int py = oy + wave; py < oy + kBgTH && py < a.H; py += 4) {
                int iy0, iy1, iz0, iz1; float fy, fz;
                bg_axis(bg_coord(py, a.H), Y, iy0, iy1, fy);
                const int64_t at = fbase + (int64_t)py * a.W + px;
                const float r = a.image[at], gg = a.image[at + HW], b = a.image[at + 2 * HW];
                const float z = (0.299f * r + 0.587f * gg) + 0.114f * b;
                bg_axis(z, L, iz0, iz1, fz);
                const float wy[2] = {1.f - fy, fy}, wz[2] = {1.f - fz, fz};
                int off[2][2][2];
                const int cy[2] = {iy0 - ylo, iy1 - ylo}, cz[2] = {iz0, iz1};
#pragma unroll
                for (int dz = 0; dz < 2; ++dz)
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 2; ++dx) off[dz][dy][dx] = (cz[dz] * sy + cy[dy]) * sx + cx[dx];
                float A[12];
                const bool luma = kBwd && z > 0.f && z < 1.f && L > 1;
                float D[12];
#pragma unroll
                for (int c = 0; c < 12; ++c) {
                    float v[2][2][2];
#pragma unroll
                    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
                        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 2; ++dx) {
                                const int o = c * sc + off[dz][dy][dx];
                                v[dz][dy][dx] = staged ? cells[o] : gsrc[o];
                            }
                    float acc = 0.f;
#pragma unroll
                    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
                        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 2; ++dx) {
                                const float p = ((wz[dz] * wy[dy]) * wx[dx]) * v[dz][dy][dx];
                                acc = (dz | dy | dx) == 0 ? p : acc + p;
                            }
                    A[c] = acc;
                    if (kBwd) {
                        float dd = 0.f;
#pragma unroll
                        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 2; ++dx) {
                                const float p = (wy[dy] * wx[dx]) * (v[1][dy][dx] - v[0][dy][dx]);
                                dd = (dy | dx) == 0 ? p : dd + p;
                            }
                        D[c] = dd;
                    }
                }
                if (!kBwd) {
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        dst[at + i * HW] = ((A[4 * i] * r + A[4 * i + 1] * gg) + A[4 * i + 2] * b) + A[4 * i + 3];
                } else {
                    const float d0 = a.d_out[at], d1 = a.d_out[at + HW], d2 = a.d_out[at + 2 * HW];
                    float di[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) di[k] = (A[k] * d0 + A[4 + k] * d1) + A[8 + k] * d2;
                    if (luma) {
                        float s[3];
#pragma unroll
                        for (int i = 0; i < 3; ++i) s[i] = ((D[4 * i] * r + D[4 * i + 1] * gg) + D[4 * i + 2] * b) + D[4 * i + 3];
                        const float S = ((d0 * s[0] + d1 * s[1]) + d2 * s[2]) * (float)(L - 1);
                        di[0] = di[0] + 0.299f * S;
                        di[1] = di[1] + 0.587f * S;
                        di[2] = di[2] + 0.114f * S;
                    }
                    dst[at] = di[0]; dst[at + HW] = di[1]; dst[at + 2 * HW] = di[2];
                }
            }
        }
        __syncthreads();   // (the next tile's staging overwrites `cells`)
    }
}

// blockIdx.x = yy * X + xx; blockIdx.y strides over the chunks, blockIdx.z over the frames
template <int LP>
__global__ void __launch_bounds__(kBgThreads) bilagrid_grid_partial_kernel(const Bg a, int nchunks, float* __restrict__ records) {
    __shared__ float red[kBgThreads / 64][LP * 12];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L, X = a.X, Y = a.Y;
    const int col = blockIdx.x;
    const int yy = col / X, xx = col - yy * X;
    const int64_t HW = (int64_t)a.H * a.W;
    int xlo, xhi, ylo, yhi;
    bg_footprint(a.W, X, xx, xlo, xhi);
    bg_footprint(a.H, Y, yy, ylo, yhi);
    for (int chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y)
    for (int fr = blockIdx.z; fr < a.F; fr += gridDim.z) {
        const int64_t r0 = (int64_t)ylo + (int64_t)chunk * kBgChunkRows;   // (past yhi: an empty chunk, a record of zeros)
        const int64_t r1 = r0 + kBgChunkRows - 1 < yhi ? r0 + kBgChunkRows - 1 : yhi;
        const int g = a.ids[fr];
        if (g < 0 || g >= a.G) continue;   // (uniform) an identity frame: no record, and the sum kernel reads none
        float acc[LP][12];
#pragma unroll
        for (int l = 0; l < LP; ++l)
#pragma unroll
            for (int j = 0; j < 12; ++j) acc[l][j] = 0.f;
        const int64_t fbase = (int64_t)fr * 3 * HW;
        for (int64_t row = r0 + wave; row <= r1; row += 4) {
            const int py = (int)row;
            int iy0, iy1; float fy;
            bg_axis(bg_coord(py, a.H), Y, iy0, iy1, fy);
            if (yy != iy0 && yy != iy1) continue;   // (uniform over the wave: a row of the margin)
            const float wy = yy == iy0 ? 1.f - fy : fy;
            for (int px = xlo + lane; px <= xhi; px += 64) {
                int ix0, ix1; float fx;
                bg_axis(bg_coord(px, a.W), X, ix0, ix1, fx);
                if (xx != ix0 && xx != ix1) continue;
                const float wx = xx == ix0 ? 1.f - fx : fx;
                const int64_t at = fbase + (int64_t)py * a.W + px;
                const float r = a.image[at], gg = a.image[at + HW], b = a.image[at + 2 * HW];
                const float d[3] = {a.d_out[at], a.d_out[at + HW], a.d_out[at + 2 * HW]};
                const float z = (0.299f * r + 0.587f * gg) + 0.114f * b;
                int iz0, iz1; float fz;
                bg_axis(z, L, iz0, iz1, fz);
                const float wyx = wy * wx;
                const float w0 = (1.f - fz) * wyx, w1 = fz * wyx;
                float c0[12], c1[12];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float t[4] = {d[i] * r, d[i] * gg, d[i] * b, d[i]};
#pragma unroll
                    for (int k = 0; k < 4; ++k) { c0[4 * i + k] = w0 * t[k]; c1[4 * i + k] = w1 * t[k]; }
                }
                // (L == 1: iz0 == iz1 == 0 and w1 == 0: plane 0 takes c0)
#pragma unroll
                for (int l = 0; l < LP; ++l) {
                    const bool h0 = l == iz0, h1 = l == iz1;
#pragma unroll
                    for (int j = 0; j < 12; ++j) acc[l][j] += h0 ? c0[j] : (h1 ? c1[j] : 0.f);
                }
            }
        }
        // the workgroup's record: a fixed DPP tree over each wave (total in lane 63), then the four waves in order
#pragma unroll
        for (int l = 0; l < LP; ++l)
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const float s = wave_sum_hi_f32(acc[l][j]);
                if (lane == 63) red[wave][l * 12 + j] = s;
            }
        __syncthreads();
        if (tid < L * 12) {
            const int l = tid / 12, c = tid - l * 12;
            const float s = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
            records[(((int64_t)fr * nchunks + chunk) * 12 * L + (int64_t)c * L + l) * (Y * X) + col] = s;
        }
        __syncthreads();   // (`red` is rewritten for the next frame)
    }
}

__global__ void __launch_bounds__(256) bilagrid_grid_sum_kernel(const float* __restrict__ records, const int32_t* __restrict__ ids,
                                                                int F, int nchunks, int64_t slab, int64_t n,
                                                                float* __restrict__ d_grids) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int g = (int)(e / slab);
    const int64_t r = e - (int64_t)g * slab;
    float s = 0.f;
    for (int fr = 0; fr < F; ++fr) {
        if (ids[fr] != g) continue;
        for (int k = 0; k < nchunks; ++k) s += records[((int64_t)fr * nchunks + k) * slab + r];
    }
    d_grids[e] = s;
}

// ---- total variation ----

struct Tv {
    int G, L, Y, X;
    int64_t n;                   // 12 G L Y X
    double kx, ky, kz;           // 1 / (number of differences along the axis), 0 for an axis of size 1
};

__global__ void __launch_bounds__(kTvThreads) bilagrid_tv_kernel(const float* __restrict__ grids, const Tv t, double* __restrict__ blocks) {
    __shared__ double red[3][kTvThreads];
    const int tid = threadIdx.x;
    const int64_t sy = t.X, sz = (int64_t)t.X * t.Y;
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kTvThreads + tid; e < t.n; e += (int64_t)gridDim.x * kTvThreads) {
        const int xx = (int)(e % t.X), yy = (int)((e / sy) % t.Y), l = (int)((e / sz) % t.L);
        const double v = grids[e];
        if (xx + 1 < t.X) { const double d = (double)grids[e + 1] - v; ax += d * d; }
        if (yy + 1 < t.Y) { const double d = (double)grids[e + sy] - v; ay += d * d; }
        if (l + 1 < t.L) { const double d = (double)grids[e + sz] - v; az += d * d; }
    }
    red[0][tid] = ax; red[1][tid] = ay; red[2][tid] = az;
    __syncthreads();
    for (int s = kTvThreads / 2; s > 0; s >>= 1) {
        if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; red[2][tid] += red[2][tid + s]; }
        __syncthreads();
    }
    if (tid < 3) blocks[3 * (int64_t)blockIdx.x + tid] = red[tid][0];
}

__global__ void __launch_bounds__(kTvThreads) bilagrid_tv_sum_kernel(const double* __restrict__ blocks, int nblocks, const Tv t,
                                                                     float* __restrict__ tv) {
    __shared__ double red[3][kTvThreads];
    const int tid = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = tid; b < nblocks; b += kTvThreads) { s[0] += blocks[3 * b]; s[1] += blocks[3 * b + 1]; s[2] += blocks[3 * b + 2]; }
    red[0][tid] = s[0]; red[1][tid] = s[1]; red[2][tid] = s[2];
    __syncthreads();
    for (int h = kTvThreads / 2; h > 0; h >>= 1) {
        if (tid < h) { red[0][tid] += red[0][tid + h]; red[1][tid] += red[1][tid + h]; red[2][tid] += red[2][tid + h]; }
        __syncthreads();
    }
    if (tid == 0) tv[0] = (float)((red[0][0] * t.kx + red[1][0] * t.ky) + red[2][0] * t.kz);
}

__global__ void __launch_bounds__(kTvThreads) bilagrid_tv_bwd_kernel(const float* __restrict__ grids, const Tv t,
                                                                     const float* __restrict__ dL_dtv, float* __restrict__ d_grids) {
    const int64_t e = (int64_t)blockIdx.x * kTvThreads + threadIdx.x;
    if (e >= t.n) return;
    const int64_t sy = t.X, sz = (int64_t)t.X * t.Y;
    const int xx = (int)(e % t.X), yy = (int)((e / sy) % t.Y), l = (int)((e / sz) % t.L);
    const double v = grids[e];
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (xx > 0) gx += v - (double)grids[e - 1];
    if (xx + 1 < t.X) gx -= (double)grids[e + 1] - v;
    if (yy > 0) gy += v - (double)grids[e - sy];
    if (yy + 1 < t.Y) gy -= (double)grids[e + sy] - v;
    if (l > 0) gz += v - (double)grids[e - sz];
    if (l + 1 < t.L) gz -= (double)grids[e + sz] - v;
    // (the upstream gradient multiplies last, in fp32: k * tv gives exactly k times the gradient of tv)
    d_grids[e] = dL_dtv[0] * (float)(2.0 * ((gx * t.kx + gy * t.ky) + gz * t.kz));
}

// ---- host ----

int check_lattice(const char* fn, int G, int L, int Y, int X) {
    if (G < 1) { set_error("%s: G=%d must be at least 1", fn, G); return HS_EINVAL; }
    if (L < 1 || L > kBgMaxL) { set_error("%s: L=%d outside [1, %d]", fn, L, kBgMaxL); return HS_EINVAL; }
    if (Y < 1 || Y > kBgMaxXY) { set_error("%s: Y=%d outside [1, %d]", fn, Y, kBgMaxXY); return HS_EINVAL; }
    if (X < 1 || X > kBgMaxXY) { set_error("%s: X=%d outside [1, %d]", fn, X, kBgMaxXY); return HS_EINVAL; }
    const int64_t n = 12ll * G * L * Y * X;
    if (n >= (1ll << 31)) { set_error("%s: 12*G*L*Y*X=%lld must be below 2^31", fn, (long long)n); return HS_EINVAL; }
    return HS_OK;
}

int check_shape(const char* fn, int F, int H, int W, int G, int L, int Y, int X) {
    if (F < 1) { set_error("%s: F=%d must be at least 1", fn, F); return HS_EINVAL; }
    if (H < 1) { set_error("%s: H=%d must be at least 1", fn, H); return HS_EINVAL; }
    if (W < 1) { set_error("%s: W=%d must be at least 1", fn, W); return HS_EINVAL; }
    // (in floating point first: three factors below 2^31 overflow an int64 product)
    if (3.0 * F * H * W >= 2147483648.0) {
        set_error("%s: 3*F*H*W=%.0f must be below 2^31", fn, 3.0 * F * H * W);
        return HS_EINVAL;
    }
    return check_lattice(fn, G, L, Y, X);
}

// chunks of kBgChunkRows rows that cover the tallest footprint of a lattice row
int grid_chunks(int H, int Y) {
    int tallest = 1;
    for (int yy = 0; yy < Y; ++yy) {
        int lo, hi;
        bg_footprint(H, Y, yy, lo, hi);
        if (hi - lo + 1 > tallest) tallest = hi - lo + 1;
    }
    return (tallest + kBgChunkRows - 1) / kBgChunkRows;
}

Bg bg_of(const hs_bilagrid_args& a) {
    Bg b;
    memset(&b, 0, sizeof(b));
    b.F = a.F; b.H = a.H; b.W = a.W; b.G = a.G; b.L = a.L; b.Y = a.Y; b.X = a.X;
    b.image = a.image; b.grids = a.grids; b.ids = a.grid_ids;
    b.out = a.out; b.d_out = a.dL_dout; b.d_image = a.dL_dimage;
    return b;
}

template <bool kBwd>
int launch_pixels(const hs_bilagrid_args& a, hipStream_t s) {
    const int tiles_x = (a.W + kBgTW - 1) / kBgTW, tiles_y = (a.H + kBgTH - 1) / kBgTH;
    const int64_t ntiles = (int64_t)a.F * tiles_x * tiles_y;
    const unsigned grid = (unsigned)(ntiles < kBgMaxGrid ? ntiles : kBgMaxGrid);
    bilagrid_pixel_kernel<kBwd><<<grid, kBgThreads, 0, s>>>(bg_of(a), tiles_x, tiles_y, ntiles);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

int launch_grid_gradient(const hs_bilagrid_args& a, hipStream_t s) {
    const int nchunks = grid_chunks(a.H, a.Y);
    const dim3 grid((unsigned)(a.X * a.Y), (unsigned)(nchunks < 65535 ? nchunks : 65535), (unsigned)(a.F < 65535 ? a.F : 65535));
    float* records = (float*)a.workspace;
    const Bg b = bg_of(a);
    if (a.L <= 2) bilagrid_grid_partial_kernel<2><<<grid, kBgThreads, 0, s>>>(b, nchunks, records);
    else if (a.L <= 4) bilagrid_grid_partial_kernel<4><<<grid, kBgThreads, 0, s>>>(b, nchunks, records);
    else if (a.L <= 8) bilagrid_grid_partial_kernel<8><<<grid, kBgThreads, 0, s>>>(b, nchunks, records);
    else bilagrid_grid_partial_kernel<16><<<grid, kBgThreads, 0, s>>>(b, nchunks, records);
    HS_LAUNCH_CHECK();
    const int64_t slab = 12ll * a.L * a.Y * a.X, n = slab * a.G;
    bilagrid_grid_sum_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(records, a.grid_ids, a.F, nchunks, slab, n, a.dL_dgrids);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

int check_slice_args(const char* fn, const hs_bilagrid_args* a, bool backward) {
    if (check_args(fn, a) || check_shape(fn, a->F, a->H, a->W, a->G, a->L, a->Y, a->X)) return HS_EINVAL;
    Field f[5] = {{a->image, "image", 4}, {a->grids, "grids", 4}, {a->grid_ids, "grid_ids", 4}};
    int n = 3;
    if (backward) f[n++] = {a->dL_dout, "dL_dout", 4};
    else f[n++] = {a->out, "out", 4};
    if (check_fields(fn, f, n)) return HS_EINVAL;
    if (backward) {
        if (check_aligned(fn, a->dL_dimage, "dL_dimage", 4) || check_aligned(fn, a->dL_dgrids, "dL_dgrids", 4)) return HS_EINVAL;
        if (a->dL_dgrids && check_field(fn, a->workspace, "workspace", 256, " (needed with dL_dgrids)")) return HS_EINVAL;
    }
    return HS_OK;
}

Tv tv_of(const hs_bilagrid_tv_args& a) {
    Tv t;
    memset(&t, 0, sizeof(t));
    t.G = a.G; t.L = a.L; t.Y = a.Y; t.X = a.X;
    t.n = 12ll * a.G * a.L * a.Y * a.X;
    const double rows = 12.0 * a.G;
    t.kx = a.X > 1 ? 1.0 / (rows * a.L * a.Y * (a.X - 1)) : 0.0;
    t.ky = a.Y > 1 ? 1.0 / (rows * a.L * (a.Y - 1) * a.X) : 0.0;
    t.kz = a.L > 1 ? 1.0 / (rows * (a.L - 1) * a.Y * a.X) : 0.0;
    return t;
}

int tv_blocks(int64_t n) {
    const int64_t b = (n + kTvThreads - 1) / kTvThreads;
    return (int)(b < kTvMaxBlocks ? b : kTvMaxBlocks);
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_bilagrid_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t G, int32_t L, int32_t Y, int32_t X) {
    if (hs::check_shape("hs_bilagrid_workspace_bytes", F, H, W, G, L, Y, X)) return HS_EINVAL;
    return hs::align_up(4ll * F * hs::grid_chunks(H, Y) * 12 * L * Y * X, 256);
}

HS_API int hs_bilagrid_slice(const hs_bilagrid_args* a, void* hip_stream) {
    const int rc = hs::check_slice_args("hs_bilagrid_slice", a, false);
    if (rc != HS_OK) return rc;
    return hs::launch_pixels<false>(*a, (hipStream_t)hip_stream);
}

HS_API int hs_bilagrid_slice_backward(const hs_bilagrid_args* a, void* hip_stream) {
    int rc = hs::check_slice_args("hs_bilagrid_slice_backward", a, true);
    if (rc != HS_OK) return rc;
    if (a->dL_dimage) rc = hs::launch_pixels<true>(*a, (hipStream_t)hip_stream);
    if (rc == HS_OK && a->dL_dgrids) rc = hs::launch_grid_gradient(*a, (hipStream_t)hip_stream);
    return rc;
}

HS_API int hs_bilagrid_tv(const hs_bilagrid_tv_args* a, void* hip_stream) {
    const char* fn = "hs_bilagrid_tv";
    if (hs::check_args(fn, a) || hs::check_lattice(fn, a->G, a->L, a->Y, a->X)) return HS_EINVAL;
    const hs::Field f[3] = {{a->grids, "grids", 4}, {a->tv, "tv", 4}, {a->workspace, "workspace", 256}};
    if (hs::check_fields(fn, f, 3)) return HS_EINVAL;
    const hs::Tv t = hs::tv_of(*a);
    const int nb = hs::tv_blocks(t.n);
    hs::bilagrid_tv_kernel<<<nb, hs::kTvThreads, 0, (hipStream_t)hip_stream>>>(a->grids, t, (double*)a->workspace);
    HS_LAUNCH_CHECK();
    hs::bilagrid_tv_sum_kernel<<<1, hs::kTvThreads, 0, (hipStream_t)hip_stream>>>((const double*)a->workspace, nb, t, a->tv);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

HS_API int hs_bilagrid_tv_backward(const hs_bilagrid_tv_args* a, void* hip_stream) {
    const char* fn = "hs_bilagrid_tv_backward";
    if (hs::check_args(fn, a) || hs::check_lattice(fn, a->G, a->L, a->Y, a->X)) return HS_EINVAL;
    const hs::Field f[3] = {{a->grids, "grids", 4}, {a->dL_dtv, "dL_dtv", 4}, {a->dL_dgrids, "dL_dgrids", 4}};
    if (hs::check_fields(fn, f, 3)) return HS_EINVAL;
    const hs::Tv t = hs::tv_of(*a);
    hs::bilagrid_tv_bwd_kernel<<<(unsigned)((t.n + hs::kTvThreads - 1) / hs::kTvThreads), hs::kTvThreads, 0,
                                 (hipStream_t)hip_stream>>>(a->grids, t, a->dL_dtv, a->dL_dgrids);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
