// TSDF fusion of rendered depth maps and mesh extraction by marching tetrahedra on the lattice: from "a cloud whose depth describes
// a surface" to the surface (hs_tsdf_integrate, hs_tsdf_mesh_plan, hs_tsdf_mesh_emit; include/hdrsplat.h).
//
// Compiled with -ffp-contract=off: every float below is a STATED ORDER of IEEE fp32 operations, which tests/tsdf_reference.py
// restates in numpy float32 and the GPU tests compare bit for bit.  Do not reassociate them.  `/` is the correctly rounded one.
//
// The lattice.  Sample (i, j, k) of an nx x ny x nz volume sits at p = (ox + h (float)i, oy + h (float)j, oz + h (float)k) (one
// product, one sum each) and has the linear index q = (k ny + j) nx + i.
//
// INTEGRATE.  For every sample, frames f = 0 .. F-1 in order, V = viewmatrices[f] (row-major [4][4], the rasterizer's transposed
// convention), halfW = 0.5 (float)W, halfH = 0.5 (float)H:
//       xc = ((p.x V[0][0] + p.y V[1][0]) + p.z V[2][0]) + V[3][0]      yc, zc: columns 1, 2
//       zc > 0 is false: skip.     u = fx (xc / zc) + halfW     v = fy (yc / zc) + halfH
//       u >= 0 && u < (float)W && v >= 0 && v < (float)H is false: skip.     ix = (int)u, iy = (int)v
//       d = invdepth[f, iy, ix], a = alpha[f, iy, ix] (no alpha: 1);  d, a finite and > 0 and a >= min_alpha is false: skip
//       depth = a / d;  depth <= max_depth is false: skip.     sdf = depth - zc;  sdf < -trunc: skip
//       t = sdf / trunc;  t > 1: t = 1
//       w1 = w + 1;  tsdf = (tsdf w + t) / w1;  colour_c = (colour_c w + frame_colour[f, c, iy, ix]) / w1;  w = w1
// tsdf_integrate_kernel<COLOR>  32 x 8 threads, a brick of 32 x 8 x 4 samples per workgroup: a thread keeps its four samples
//       (consecutive k) in registers across all frames and reads and writes them once: 16 B per sample, 40 B with colour,
//       whatever F.  The matrix of a frame is wave-uniform (scalar loads); the partial sums p.x V[0][c] + p.y V[1][c] are
//       shared by the four samples of a thread -- the stated order, computed once.
//   The cull.  Before the walk, lane l of every wave decides for frame 64 n + l whether the WHOLE brick fails zc > 0 or the
//       bounds test in that frame, from the eight corner samples of the brick; the ballot of the survivors is the list of frames
//       the workgroup walks.  It cannot change a bit: every operation of the chain i -> p -> (xc, yc, zc) -> u, v is a correctly
//       rounded monotone function of each of its arguments (rounding preserves order, fx, fy, h > 0), so the COMPUTED xc, yc,
//       zc of every sample of the brick lie between the computed extremes of the corners, and with zc > 0 throughout the
//       computed u lies between the extremes of fx (x / z) + halfW over x in {xmin, xmax}, z in {zmin, zmax}.  A frame is
//       dropped only when those bounds, computed with the same operations, fail the same comparisons the samples would; a
//       corner value that is not finite drops nothing.
//
// MESH.  Marching tetrahedra on the Kuhn decomposition: cell (i, j, k) -> six tetrahedra 000 -> e_a -> e_a + e_b -> 111, one
// per permutation (a, b, c) of the axes in lexicographic order; tetrahedra 0, 3, 4 (even permutations) are positively oriented,
// 1, 2, 5 negatively.  A sample is OBSERVED when weight >= min_weight and INSIDE when tsdf < 0 (a NaN is neither).  The
// lattice edges are the translates of the directions 100, 010, 001, 110, 101, 011, 111 (edge numbers 0 .. 6, x the first digit),
// owned by their lower end.  An owned edge carries a vertex when both ends are observed and exactly one is inside: with a, pa
// the value and position at the owner and b, pb at the other end,
//       s = a / (a - b)       vertex_c = pa_c + s (pb_c - pa_c)       colour_c = ca_c + s (cb_c - ca_c)
// A tetrahedron whose four corners are observed emits the triangles of kTetTri[case] (case: bit m = corner m inside), each
// triangle three tetrahedron edges 01 02 03 12 13 23 (numbers 0 .. 5), wound so that the normal points to the outside (positive)
// corners in a positively oriented tetrahedron; a negatively oriented one swaps the last two vertices.
// Order: vertices by (q, edge number), triangles by (q, tetrahedron, position in the case).
//   tsdf_count_kernel    256 consecutive q per workgroup: the 7-bit edge mask of each (one byte of the workspace) and the
//                        workgroup's sums of vertices and triangles (two u64).
//   tsdf_scan_kernel     one workgroup of 1024 threads: exclusive scan of the sums in place, totals {V, T} as int64.  (Not
//                        hs_rowplan.h's densify_scan_kernel: that one carries four u32 counts and the densify totals; the
//                        sums here pass 2^32 before the caller can refuse them, so they are two u64.)
//   tsdf_vbase_kernel    vbase[q] = the workgroup's prefix + the exclusive scan of popcount(mask) inside it (int32).
//   tsdf_emit_kernel     256 consecutive q: writes the vertices of its owned edges and, from the same eight corner samples,
//                        its triangles at the workgroup's triangle prefix + an exclusive scan inside it; the index of the
//                        vertex on an edge owned by q' is vbase[q'] + popcount(mask[q'] & ((1 << e) - 1)).
// No atomics, no memset, no host wait; every element of every output and of the workspace is written before it is read.
#include "hs_cloud.h"

#include <cfloat>
#include <cmath>
#include <math.h>

namespace hs {
namespace {

constexpr int64_t kTsdfMaxSamples = 1ll << 30;
constexpr int kTsdfMaxSide = 65536;       // of a frame: (float)W and (float)H are exact, so u < (float)W means (int)u < W
// the brick of the integration: kTsdfBx x kTsdfBy threads, kTsdfBz samples each (rows of 128 contiguous bytes, a compact brick
// for the cull; not A/B-timed against other shapes: DESIGN.md 4.31)
constexpr int kTsdfBx = 32, kTsdfBy = 8, kTsdfBz = 4;
static_assert(kTsdfBx * kTsdfBy == 256, "the integration's workgroup is four waves");
constexpr int kMeshRows = 256;            // samples per workgroup of the mesh kernels (= threads)
constexpr int kMeshScanThreads = 1024;

struct TsdfGrid { int nx, ny, nz; float ox, oy, oz, h; };

__device__ __forceinline__ float lattice(float o, float h, int i) { return o + h * (float)i; }

// one camera-space coordinate of p through column c of V, in the stated order
__device__ __forceinline__ float cam(const float* V, int c, float px, float py, float pz) {
    return ((px * V[c] + py * V[4 + c]) + pz * V[8 + c]) + V[12 + c];
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= FLT_MAX; }

// true: no sample of the brick [x] x [y] x [z] (corner positions) passes zc > 0 and the bounds test in this frame
__device__ bool brick_misses_frame(const float* V, const float px[2], const float py[2], const float pz[2], float fx, float fy,
                                   float halfW, float halfH, float Wf, float Hf) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool finite = true;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = cam(V, c, px[n & 1], py[(n >> 1) & 1], pz[n >> 2]);
            finite = finite && finite_f(v);
            lo[c] = fminf(lo[c], v);
            hi[c] = fmaxf(hi[c], v);
        }
    }
    if (!finite) return false;
    if (hi[2] <= 0.f) return true;                    // zc > 0 fails everywhere
    if (!(lo[2] > 0.f)) return false;                 // the brick straddles the camera plane: no bound on x / z
    float ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const float z = (n & 1) ? hi[2] : lo[2];
        const float u = fx * (((n & 2) ? hi[0] : lo[0]) / z) + halfW;
        const float v = fy * (((n & 2) ? hi[1] : lo[1]) / z) + halfH;
        ulo = fminf(ulo, u); uhi = fmaxf(uhi, u);
        vlo = fminf(vlo, v); vhi = fmaxf(vhi, v);
    }
    return uhi < 0.f || ulo >= Wf || vhi < 0.f || vlo >= Hf;
}

template <bool COLOR>
__global__ void __launch_bounds__(kTsdfBx * kTsdfBy) tsdf_integrate_kernel(
        TsdfGrid g, float trunc, float fx, float fy, float min_alpha, float max_depth, int F, int H, int W,
        const float* __restrict__ views, const float* __restrict__ invdepth, const float* __restrict__ alpha,
        const float* __restrict__ frame_color, float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color) {
    const int x0 = blockIdx.x * kTsdfBx, y0 = blockIdx.y * kTsdfBy, z0 = blockIdx.z * kTsdfBz;
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    const bool mine = x < g.nx && y < g.ny;
    const int nz_here = min(kTsdfBz, g.nz - z0);
    const int lane = (threadIdx.y * kTsdfBx + threadIdx.x) & 63;
    const float halfW = 0.5f * (float)W, halfH = 0.5f * (float)H, Wf = (float)W, Hf = (float)H;
    const int64_t n_samples = (int64_t)g.nx * g.ny * g.nz, plane = (int64_t)H * W;

    // the brick's corner samples (uniform)
    const float bx[2] = {lattice(g.ox, g.h, x0), lattice(g.ox, g.h, min(x0 + kTsdfBx, g.nx) - 1)};
    const float by[2] = {lattice(g.oy, g.h, y0), lattice(g.oy, g.h, min(y0 + kTsdfBy, g.ny) - 1)};
    const float bz[2] = {lattice(g.oz, g.h, z0), lattice(g.oz, g.h, z0 + nz_here - 1)};

    const float px = lattice(g.ox, g.h, x), py = lattice(g.oy, g.h, y);
    const int64_t q0 = ((int64_t)z0 * g.ny + y) * g.nx + x, slab = (int64_t)g.nx * g.ny;
    float ts[kTsdfBz], wt[kTsdfBz], col[COLOR ? 3 * kTsdfBz : 1], pz[kTsdfBz];
#pragma unroll
    for (int k = 0; k < kTsdfBz; ++k) {
        pz[k] = lattice(g.oz, g.h, z0 + k);
        const bool have = mine && k < nz_here;
        ts[k] = have ? tsdf[q0 + k * slab] : 0.f;
        wt[k] = have ? weight[q0 + k * slab] : 0.f;
        if constexpr (COLOR) {
#pragma unroll
            for (int c = 0; c < 3; ++c) col[3 * k + c] = have ? color[c * n_samples + q0 + k * slab] : 0.f;
        }
    }

    for (int f_base = 0; f_base < F; f_base += 64) {
        const int f_lane = f_base + lane;
        const bool walk = f_lane < F && !brick_misses_frame(views + 16 * (int64_t)f_lane, bx, by, bz, fx, fy, halfW, halfH, Wf, Hf);
        unsigned long long todo = __ballot(walk);
        while (todo) {
            const int f = f_base + __builtin_ctzll(todo);
            todo &= todo - 1;
            if (!mine) continue;
            const float* V = views + 16 * (int64_t)f;
            const float ax = px * V[0] + py * V[4], ay = px * V[1] + py * V[5], az = px * V[2] + py * V[6];
            const float* df = invdepth + f * plane;
#pragma unroll
            for (int k = 0; k < kTsdfBz; ++k) {
                if (k >= nz_here) continue;
                const float zc = (az + pz[k] * V[10]) + V[14];
                if (!(zc > 0.f)) continue;
                const float xc = (ax + pz[k] * V[8]) + V[12];
                const float yc = (ay + pz[k] * V[9]) + V[13];
                const float u = fx * (xc / zc) + halfW;
                const float v = fy * (yc / zc) + halfH;
                if (!(u >= 0.f && u < Wf && v >= 0.f && v < Hf)) continue;
                const int64_t at = (int64_t)(int)v * W + (int)u;
                const float d = df[at];
                const float a = alpha ? alpha[f * plane + at] : 1.f;
                if (!(finite_f(d) && d > 0.f && finite_f(a) && a > 0.f && a >= min_alpha)) continue;
                const float depth = a / d;
                if (!(depth <= max_depth)) continue;
                const float sdf = depth - zc;
                if (sdf < -trunc) continue;
                float t = sdf / trunc;
                t = t > 1.f ? 1.f : t;
                const float w = wt[k], w1 = w + 1.f;
                ts[k] = (ts[k] * w + t) / w1;
                if constexpr (COLOR) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        col[3 * k + c] = (col[3 * k + c] * w + frame_color[(3 * (int64_t)f + c) * plane + at]) / w1;
                }
                wt[k] = w1;
            }
        }
    }
    if (!mine) return;
#pragma unroll
    for (int k = 0; k < kTsdfBz; ++k) {
        if (k >= nz_here) continue;
        tsdf[q0 + k * slab] = ts[k];
        weight[q0 + k * slab] = wt[k];
        if constexpr (COLOR) {
#pragma unroll
            for (int c = 0; c < 3; ++c) color[c * n_samples + q0 + k * slab] = col[3 * k + c];
        }
    }
}

// ---- marching tetrahedra ----

// lattice direction (bit 0 = x, 1 = y, 2 = z) of edge number e, and back
__constant__ const uint8_t kEdgeDir[7] = {1, 2, 4, 3, 5, 6, 7};
__constant__ const uint8_t kDirEdge[8] = {0, 0, 1, 3, 2, 4, 5, 6};
// the cell corners (bit 0 = x, ...) of tetrahedron t's corners 0 .. 3, permutations of the axes in lexicographic order
__constant__ const uint8_t kTetCorner[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
// the tetrahedron edges 01 02 03 12 13 23 as corner pairs
__constant__ const uint8_t kTetEdge[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// case (bit m: corner m inside) -> {triangles, their tetrahedron edges}, wound for a positively oriented tetrahedron so that
// the normal points from the inside corners to the outside ones
__constant__ const uint8_t kTetTri[16][7] = {
    {0, 0, 0, 0, 0, 0, 0}, {1, 0, 1, 2, 0, 0, 0}, {1, 0, 4, 3, 0, 0, 0}, {2, 1, 2, 4, 1, 4, 3},
    {1, 1, 3, 5, 0, 0, 0}, {2, 0, 5, 2, 0, 3, 5}, {2, 0, 4, 5, 0, 5, 1}, {1, 2, 4, 5, 0, 0, 0},
    {1, 2, 5, 4, 0, 0, 0}, {2, 0, 1, 5, 0, 5, 4}, {2, 0, 5, 3, 0, 2, 5}, {1, 1, 5, 3, 0, 0, 0},
    {2, 1, 3, 4, 1, 4, 2}, {1, 0, 3, 4, 0, 0, 0}, {1, 0, 2, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0}};

struct MeshGrid { int nx, ny, nz; int64_t n; float ox, oy, oz, h, min_weight; };

struct Cell { uint32_t obs, ins; int i, j, k; };   // bit c (0 .. 7): the state of corner c; a corner off the lattice is not observed

__device__ __forceinline__ int64_t corner_offset(const MeshGrid& g, int c) {
    return (int64_t)(c & 1) + (int64_t)((c >> 1) & 1) * g.nx + (int64_t)(c >> 2) * g.nx * g.ny;
}

__device__ __forceinline__ Cell load_cell(const MeshGrid& g, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                          int64_t q) {
    Cell cell;
    const uint32_t row = (uint32_t)q / (uint32_t)g.nx;
    cell.i = (int)((uint32_t)q - row * (uint32_t)g.nx);
    cell.k = (int)(row / (uint32_t)g.ny);
    cell.j = (int)(row - (uint32_t)cell.k * (uint32_t)g.ny);
    cell.obs = cell.ins = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool in = cell.i + (c & 1) < g.nx && cell.j + ((c >> 1) & 1) < g.ny && cell.k + (c >> 2) < g.nz;
        if (in) {
            const int64_t at = q + corner_offset(g, c);
            cell.obs |= (weight[at] >= g.min_weight ? 1u : 0u) << c;
            cell.ins |= (tsdf[at] < 0.f ? 1u : 0u) << c;
        }
    }
    return cell;
}

__device__ __forceinline__ uint32_t edge_mask(const Cell& cell) {
    uint32_t mask = 0u;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        const int d = kEdgeDir[e];
        const bool vertex = (cell.obs & 1u) && ((cell.obs >> d) & 1u) && (((cell.ins ^ (cell.ins >> d)) & 1u) != 0u);
        mask |= (vertex ? 1u : 0u) << e;
    }
    return mask;
}

// the case of tetrahedron t, or 0 (no triangle) when one of its corners is not observed
__device__ __forceinline__ int tet_case(const Cell& cell, int t) {
    int code = 0;
    bool all = true;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = kTetCorner[t][m];
        all = all && ((cell.obs >> c) & 1u);
        code |= (int)((cell.ins >> c) & 1u) << m;
    }
    return all ? code : 0;
}

__device__ __forceinline__ uint32_t cell_triangles(const Cell& cell) {
    uint32_t n = 0u;
#pragma unroll
    for (int t = 0; t < 6; ++t) n += kTetTri[tet_case(cell, t)][0];
    return n;
}

// exclusive scan of `v` over the 256 threads of a workgroup; `total`: the workgroup's sum
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t& total) {
    __shared__ uint32_t s_wave[kMeshRows / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    __syncthreads();                                  // (a second call in one kernel: the table is free again)
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
#pragma unroll
    for (int w = 0; w < kMeshRows / 64; ++w) {
        before += w < wave ? s_wave[w] : 0u;
        total += s_wave[w];
    }
    return before + incl - v;
}

__global__ void __launch_bounds__(kMeshRows) tsdf_count_kernel(MeshGrid g, const float* __restrict__ tsdf,
                                                               const float* __restrict__ weight, uint8_t* __restrict__ mask,
                                                               unsigned long long* __restrict__ blocks) {
    const int64_t q = (int64_t)blockIdx.x * kMeshRows + threadIdx.x;
    uint32_t nv = 0u, nt = 0u;
    if (q < g.n) {
        const Cell cell = load_cell(g, tsdf, weight, q);
        const uint32_t m = edge_mask(cell);
        mask[q] = (uint8_t)m;
        nv = (uint32_t)__popc(m);
        nt = cell_triangles(cell);
    }
    uint32_t total;
    block_scan((nv << 16) | nt, total);               // both sums in one scan: at most 256 * 7 and 256 * 12
    if (threadIdx.x == 0) {
        blocks[2 * (int64_t)blockIdx.x] = total >> 16;
        blocks[2 * (int64_t)blockIdx.x + 1] = total & 0xFFFFu;
    }
}

__global__ void __launch_bounds__(kMeshScanThreads) tsdf_scan_kernel(unsigned long long* __restrict__ blocks, int64_t nblk,
                                                                     int64_t* __restrict__ totals) {
    __shared__ unsigned long long s_v[kMeshScanThreads], s_t[kMeshScanThreads];
    const int t = threadIdx.x;
    const int64_t per = (nblk + kMeshScanThreads - 1) / kMeshScanThreads;
    const int64_t b0 = t * per < nblk ? t * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
    unsigned long long av = 0ull, at = 0ull;
    for (int64_t b = b0; b < b1; ++b) { av += blocks[2 * b]; at += blocks[2 * b + 1]; }
    s_v[t] = av;
    s_t[t] = at;
    __syncthreads();
    for (int off = 1; off < kMeshScanThreads; off <<= 1) {
        const unsigned long long uv = t >= off ? s_v[t - off] : 0ull, ut = t >= off ? s_t[t - off] : 0ull;
        __syncthreads();
        s_v[t] += uv;
        s_t[t] += ut;
        __syncthreads();
    }
    unsigned long long rv = t ? s_v[t - 1] : 0ull, rt = t ? s_t[t - 1] : 0ull;
    for (int64_t b = b0; b < b1; ++b) {
        const unsigned long long cv = blocks[2 * b], ct = blocks[2 * b + 1];
        blocks[2 * b] = rv;
        blocks[2 * b + 1] = rt;
        rv += cv;
        rt += ct;
    }
    if (t == kMeshScanThreads - 1) {
        totals[0] = (int64_t)s_v[t];
        totals[1] = (int64_t)s_t[t];
    }
}

__global__ void __launch_bounds__(kMeshRows) tsdf_vbase_kernel(int64_t n, const uint8_t* __restrict__ mask,
                                                               const unsigned long long* __restrict__ blocks,
                                                               int32_t* __restrict__ vbase) {
    const int64_t q = (int64_t)blockIdx.x * kMeshRows + threadIdx.x;
    uint32_t total;
    const uint32_t before = block_scan(q < n ? (uint32_t)__popc((uint32_t)mask[q]) : 0u, total);
    if (q < n) vbase[q] = (int32_t)(uint32_t)(blocks[2 * (int64_t)blockIdx.x] + before);
}

template <bool COLOR>
__global__ void __launch_bounds__(kMeshRows) tsdf_emit_kernel(MeshGrid g, const float* __restrict__ tsdf,
                                                              const float* __restrict__ weight, const float* __restrict__ color,
                                                              const uint8_t* __restrict__ mask, const int32_t* __restrict__ vbase,
                                                              const unsigned long long* __restrict__ blocks, int64_t n_vertices,
                                                              int64_t n_faces, float* __restrict__ vertices,
                                                              int32_t* __restrict__ faces, float* __restrict__ colors) {
    const int64_t q = (int64_t)blockIdx.x * kMeshRows + threadIdx.x;
    const bool live = q < g.n;
    Cell cell;
    cell.obs = cell.ins = 0u;
    cell.i = cell.j = cell.k = 0;
    if (live) cell = load_cell(g, tsdf, weight, q);
    uint32_t total;
    const uint32_t t_before = block_scan(live ? cell_triangles(cell) : 0u, total);
    if (!live) return;

    const uint32_t m = edge_mask(cell);               // (= mask[q]; recomputed: what is read below depends on the volume alone)
    if (m) {
        const float a = tsdf[q];
        const float pa[3] = {lattice(g.ox, g.h, cell.i), lattice(g.oy, g.h, cell.j), lattice(g.oz, g.h, cell.k)};
        int64_t at = vbase[q];
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            if (!((m >> e) & 1u)) continue;
            const int d = kEdgeDir[e];
            const int64_t other = q + corner_offset(g, d);
            const float b = tsdf[other];
            const float s = a / (a - b);
            const float pb[3] = {lattice(g.ox, g.h, cell.i + (d & 1)), lattice(g.oy, g.h, cell.j + ((d >> 1) & 1)),
                                 lattice(g.oz, g.h, cell.k + (d >> 2))};
            if (at >= 0 && at < n_vertices) {         // (always: the plan counted these; a stale plan must not write outside)
#pragma unroll
                for (int c = 0; c < 3; ++c) vertices[3 * at + c] = pa[c] + s * (pb[c] - pa[c]);
                if constexpr (COLOR) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float ca = color[c * g.n + q], cb = color[c * g.n + other];
                        colors[3 * at + c] = ca + s * (cb - ca);
                    }
                }
            }
            ++at;
        }
    }

    int64_t face = (int64_t)blocks[2 * (int64_t)blockIdx.x + 1] + t_before;
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {
        const int code = tet_case(cell, t);
        const int n_tri = kTetTri[code][0];
        const bool odd = t == 1 || t == 2 || t == 5;
        for (int r = 0; r < n_tri; ++r) {
            int32_t idx[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int te = kTetTri[code][1 + 3 * r + c];
                const int ca = kTetCorner[t][kTetEdge[te][0]], cb = kTetCorner[t][kTetEdge[te][1]];
                const int64_t owner = q + corner_offset(g, ca);
                const uint32_t below = (1u << kDirEdge[cb ^ ca]) - 1u;
                idx[c] = vbase[owner] + (int32_t)__popc((uint32_t)mask[owner] & below);
            }
            if (face >= 0 && face < n_faces) {
                faces[3 * face] = idx[0];
                faces[3 * face + 1] = odd ? idx[2] : idx[1];
                faces[3 * face + 2] = odd ? idx[1] : idx[2];
            }
            ++face;
        }
    }
}

// ---- host ----

struct MeshLayout { int64_t blocks, mask, bytes, nblk; };   // vbase at 0

MeshLayout mesh_layout(int64_t n) {
    MeshLayout l;
    l.nblk = (n + kMeshRows - 1) / kMeshRows;
    l.blocks = (4 * n + 15) / 16 * 16;
    l.mask = l.blocks + 16 * l.nblk;
    l.bytes = (l.mask + n + 15) / 16 * 16;
    return l;
}

int check_dims(const char* fn, int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) {
        set_error("%s: nx=%d, ny=%d, nz=%d must be at least 2 each", fn, nx, ny, nz);
        return HS_EINVAL;
    }
    if ((int64_t)nx * ny > kTsdfMaxSamples || (int64_t)nx * ny * nz > kTsdfMaxSamples) {
        set_error("%s: nx=%d, ny=%d, nz=%d hold more than 2^30 samples", fn, nx, ny, nz);
        return HS_EINVAL;
    }
    return HS_OK;
}

int check_positive(const char* fn, const char* name, float v) {
    if (!(std::isfinite(v) && v > 0.f)) { set_error("%s: %s=%g must be finite and > 0", fn, name, (double)v); return HS_EINVAL; }
    return HS_OK;
}

int check_grid(const char* fn, const hs_tsdf_args& a) {
    if (check_dims(fn, a.nx, a.ny, a.nz)) return HS_EINVAL;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(a.origin[c])) { set_error("%s: origin[%d]=%g must be finite", fn, c, (double)a.origin[c]); return HS_EINVAL; }
    return check_positive(fn, "voxel_size", a.voxel_size);
}

int check_mesh(const char* fn, const hs_tsdf_args& a) {
    if (check_grid(fn, a)) return HS_EINVAL;
    if (std::isnan(a.min_weight)) { set_error("%s: min_weight is a NaN", fn); return HS_EINVAL; }
    const Field f[3] = {{a.tsdf, "tsdf", 4}, {a.weight, "weight", 4}, {a.workspace, "workspace", 16}};
    return check_fields(fn, f, 3);
}

MeshGrid mesh_grid(const hs_tsdf_args& a) {
    MeshGrid g;
    g.nx = a.nx; g.ny = a.ny; g.nz = a.nz;
    g.n = (int64_t)a.nx * a.ny * a.nz;
    g.ox = a.origin[0]; g.oy = a.origin[1]; g.oz = a.origin[2];
    g.h = a.voxel_size;
    g.min_weight = a.min_weight;
    return g;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int hs_tsdf_integrate(const hs_tsdf_args* a, void* hip_stream) {
    const char* fn = "hs_tsdf_integrate";
    if (hs::check_args(fn, a) || hs::check_grid(fn, *a)) return HS_EINVAL;
    const int64_t lim = 1ll << 31, px = (int64_t)a->H * a->W;       // (no product here passes 2^63)
    if (a->F < 1 || a->H < 1 || a->W < 1 || a->H > hs::kTsdfMaxSide || a->W > hs::kTsdfMaxSide ||
        (int64_t)a->F > (lim - 1) / (3 * px)) {
        hs::set_error("%s: F=%d, H=%d, W=%d outside F >= 1, 1 <= H, W <= %d, 3 F H W < 2^31", fn, a->F, a->H, a->W, hs::kTsdfMaxSide);
        return HS_EINVAL;
    }
    if (hs::check_positive(fn, "fx", a->fx) || hs::check_positive(fn, "fy", a->fy) || hs::check_positive(fn, "trunc", a->trunc))
        return HS_EINVAL;
    if (std::isnan(a->min_alpha)) { hs::set_error("%s: min_alpha is a NaN", fn); return HS_EINVAL; }
    if (!(a->max_depth > 0.f)) { hs::set_error("%s: max_depth=%g must be > 0 (infinity: no limit)", fn, (double)a->max_depth); return HS_EINVAL; }
    const hs::Field f[4] = {{a->tsdf, "tsdf", 4}, {a->weight, "weight", 4}, {a->invdepth, "invdepth", 4},
                            {a->viewmatrices, "viewmatrices", 4}};
    if (hs::check_fields(fn, f, 4)) return HS_EINVAL;
    if (hs::check_aligned(fn, a->alpha, "alpha", 4) || hs::check_aligned(fn, a->color, "color", 4) ||
        hs::check_aligned(fn, a->frame_color, "frame_color", 4))
        return HS_EINVAL;
    if ((a->color != nullptr) != (a->frame_color != nullptr)) {
        hs::set_error("%s: %s", fn, a->color ? "the volume has colour (color), the frames have none (null frame_color)"
                                             : "frame_color given for a volume without colour (null color)");
        return HS_EINVAL;
    }
    hs::TsdfGrid g;
    g.nx = a->nx; g.ny = a->ny; g.nz = a->nz;
    g.ox = a->origin[0]; g.oy = a->origin[1]; g.oz = a->origin[2];
    g.h = a->voxel_size;
    const dim3 grid((unsigned)hs::ceil_div(a->nx, hs::kTsdfBx), (unsigned)hs::ceil_div(a->ny, hs::kTsdfBy),
                    (unsigned)hs::ceil_div(a->nz, hs::kTsdfBz));
    if (grid.y > 65535u || grid.z > 65535u) {
        hs::set_error("%s: ny=%d, nz=%d pass the grid of one launch (%d and %d)", fn, a->ny, a->nz, 65535 * hs::kTsdfBy, 65535 * hs::kTsdfBz);
        return HS_EINVAL;
    }
    const dim3 block(hs::kTsdfBx, hs::kTsdfBy);
    hipStream_t s = (hipStream_t)hip_stream;
    if (a->color)
        hs::tsdf_integrate_kernel<true><<<grid, block, 0, s>>>(g, a->trunc, a->fx, a->fy, a->min_alpha, a->max_depth, a->F, a->H,
                                                               a->W, a->viewmatrices, a->invdepth, a->alpha, a->frame_color,
                                                               a->tsdf, a->weight, a->color);
    else
        hs::tsdf_integrate_kernel<false><<<grid, block, 0, s>>>(g, a->trunc, a->fx, a->fy, a->min_alpha, a->max_depth, a->F, a->H,
                                                                a->W, a->viewmatrices, a->invdepth, a->alpha, nullptr, a->tsdf,
                                                                a->weight, nullptr);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

HS_API int64_t hs_tsdf_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (hs::check_dims("hs_tsdf_mesh_workspace_bytes", nx, ny, nz)) return HS_EINVAL;
    return hs::mesh_layout((int64_t)nx * ny * nz).bytes;
}

HS_API int hs_tsdf_mesh_plan(const hs_tsdf_args* a, void* hip_stream) {
    const char* fn = "hs_tsdf_mesh_plan";
    if (hs::check_args(fn, a) || hs::check_mesh(fn, *a)) return HS_EINVAL;
    if (hs::check_field(fn, a->totals, "totals", 8)) return HS_EINVAL;
    const hs::MeshGrid g = hs::mesh_grid(*a);
    const hs::MeshLayout l = hs::mesh_layout(g.n);
    char* ws = (char*)a->workspace;
    int32_t* vbase = (int32_t*)ws;
    unsigned long long* blocks = (unsigned long long*)(ws + l.blocks);
    uint8_t* mask = (uint8_t*)(ws + l.mask);
    hipStream_t s = (hipStream_t)hip_stream;
    hs::tsdf_count_kernel<<<(unsigned)l.nblk, hs::kMeshRows, 0, s>>>(g, a->tsdf, a->weight, mask, blocks);
    HS_LAUNCH_CHECK();
    hs::tsdf_scan_kernel<<<1, hs::kMeshScanThreads, 0, s>>>(blocks, l.nblk, a->totals);
    HS_LAUNCH_CHECK();
    hs::tsdf_vbase_kernel<<<(unsigned)l.nblk, hs::kMeshRows, 0, s>>>(g.n, mask, blocks, vbase);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

HS_API int hs_tsdf_mesh_emit(const hs_tsdf_args* a, void* hip_stream) {
    const char* fn = "hs_tsdf_mesh_emit";
    if (hs::check_args(fn, a) || hs::check_mesh(fn, *a)) return HS_EINVAL;
    const int64_t lim = 1ll << 31;
    if (a->n_vertices < 0 || a->n_vertices >= lim || a->n_faces < 0 || a->n_faces >= lim) {
        hs::set_error("%s: n_vertices=%lld, n_faces=%lld outside [0, 2^31)", fn, (long long)a->n_vertices, (long long)a->n_faces);
        return HS_EINVAL;
    }
    if (hs::check_aligned(fn, a->color, "color", 4) || hs::check_aligned(fn, a->colors, "colors", 4)) return HS_EINVAL;
    if ((a->color != nullptr) != (a->colors != nullptr)) {
        hs::set_error("%s: %s", fn, a->color ? "the volume has colour (color), the mesh has none (null colors)"
                                             : "colors given for a volume without colour (null color)");
        return HS_EINVAL;
    }
    if (a->n_vertices > 0 && hs::check_field(fn, a->vertices, "vertices", 4)) return HS_EINVAL;
    if (a->n_faces > 0 && hs::check_field(fn, a->faces, "faces", 4)) return HS_EINVAL;
    if (a->n_vertices == 0 && a->n_faces == 0) return HS_OK;
    const hs::MeshGrid g = hs::mesh_grid(*a);
    const hs::MeshLayout l = hs::mesh_layout(g.n);
    const char* ws = (const char*)a->workspace;
    const int32_t* vbase = (const int32_t*)ws;
    const unsigned long long* blocks = (const unsigned long long*)(ws + l.blocks);
    const uint8_t* mask = (const uint8_t*)(ws + l.mask);
    hipStream_t s = (hipStream_t)hip_stream;
    if (a->color)
        hs::tsdf_emit_kernel<true><<<(unsigned)l.nblk, hs::kMeshRows, 0, s>>>(g, a->tsdf, a->weight, a->color, mask, vbase, blocks,
                                                                            a->n_vertices, a->n_faces, a->vertices, a->faces, a->colors);
    else
        hs::tsdf_emit_kernel<false><<<(unsigned)l.nblk, hs::kMeshRows, 0, s>>>(g, a->tsdf, a->weight, nullptr, mask, vbase, blocks,
                                                                             a->n_vertices, a->n_faces, a->vertices, a->faces, nullptr);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
