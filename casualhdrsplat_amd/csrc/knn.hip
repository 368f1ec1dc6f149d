// Mean squared distance to the three nearest neighbours of every point (hs_knn_workspace_bytes, hs_knn_mean_dist_sq;
// include/hdrsplat.h states the contract): the scale of the published SfM initialisation, upstream's simple_knn.distCUDA2.
//
// The result is a function of VALUES only -- the k = min(3, P - 1) smallest of the multiset {d2(i, j), j != i} -- so it is
// the same whatever order candidates are met in, and an exact search may prune by any lower bound that never exceeds a
// computed distance.  Six of our own kernels around the library's radix passes (launch_radix_sort, binning.hip):
//   knn_setup_kernel    bounding box per workgroup (<= 256 partial boxes), the sort's scratch cleared, the header written
//   knn_morton_kernel   every workgroup folds the partial boxes, then 30-bit Morton codes (10 bits per axis; an axis of zero
//                       extent gets code 0, nothing is divided by zero) as the keys, the point numbers as the values
//   (four radix passes of 8 + 8 + 7 + 7 bits over (code, index))
//   knn_gather_kernel   the points in Morton order as float4 {x, y, z, index} -- the index clamped below P, so that a damaged
//                       permutation cannot lead outside the arrays --, the AABB of every BOX of 64 consecutive points (one
//                       wave, a shuffle tree), and the sort's verdict copied to the caller's status word
//   knn_super_kernel    the AABB of every SUPER-BOX of 64 consecutive boxes
//   knn_search_kernel   one wave per box, one lane per point:
//       seeds      the +-3 neighbours in Morton order give `reject`, the k-th smallest seed distance; the best-list is then
//                  CLEARED (the seeds are met again when their boxes are scanned: a seed kept would be counted twice)
//       own box    the wave's own 64 points, from LDS, excluded by index
//       the rest   per super-box, then per box of an accepted super-box: lb = ((ex ex) + (ey ey)) + (ez ez) with
//                  e = max(0, bmin - p, p - bmax) per axis -- the operation order of d2, and rounding is monotonic, so lb never
//                  exceeds the computed distance to any point inside.  A lane skips when lb > reject, or when its list holds
//                  k distances and lb >= best[k - 1] (an equal value cannot change the k smallest VALUES; this is what keeps
//                  a cloud of coincident points from scanning every box).  The wave decides by ballot; an accepted box is
//                  staged once in LDS and every lane reads the same address (a broadcast: no bank conflict), every lane
//                  inserting every point -- more candidates never change the k smallest.
// Cost: P / 4096 + 64 x (accepted super-boxes) bound tests per point; a cloud whose boxes prune nothing for many points (one
// far outlier that stretches the bounding box until the 10-bit grid no longer resolves the rest) degenerates to
// O(P^2 / 64), still exact.
// Kernels only, on the caller's stream: no memset, no copy, no allocation, no synchronisation, no floating-point atomics;
// compiled with -ffp-contract=off; the same inputs give the same bits.
#include "hs_cloud.h"

#include <math.h>
#include <stddef.h>

namespace hs {
namespace {

constexpr int kKnnBox = 64;                   // points per box = lanes of the wave that owns it
constexpr int kKnnSuper = 64;                 // boxes per super-box
constexpr int kKnnThreads = 256;
constexpr int kKnnPartials = 256;             // most workgroups of the bounding-box reduction (one partial per thread later)
constexpr int kKnnBits = 30;                  // Morton code: 10 bits per axis
constexpr int kKnnHdrWords = 64;              // [0] element count of the sort, [1] its fail word (+ the words it counts in)

struct KnnWs {
    int64_t nbox, nsuper;
    int64_t hdr, partials, ka, va, kb, vb, sorted, bmin, bmax, smin, smax, sort_tmp, bytes;
    explicit KnnWs(int64_t P) {
        nbox = (P + kKnnBox - 1) / kKnnBox;
        nsuper = (nbox + kKnnSuper - 1) / kKnnSuper;
        int64_t o = 0;
        auto carve = [&](int64_t b) { const int64_t at = o; o += align_up(b, 256); return at; };
        hdr = carve(kKnnHdrWords * 4);
        partials = carve(kKnnPartials * 8 * 4);
        ka = carve(P * 8); va = carve(P * 4); kb = carve(P * 8); vb = carve(P * 4);
        sorted = carve(P * 16);
        bmin = carve(nbox * 16); bmax = carve(nbox * 16);
        smin = carve(nsuper * 16); smax = carve(nsuper * 16);
        sort_tmp = carve(sort_tmp_bytes(P));
        bytes = o;
    }
};

__device__ __forceinline__ float sel_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float sel_max(float a, float b) { return b > a ? b : a; }

// min / max over the 64 lanes of a wave, valid in every lane (order-independent: exact)
__device__ __forceinline__ void wave_minmax3(float mn[3], float mx[3]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mn[c] = sel_min(mn[c], __shfl_xor(mn[c], m));
            mx[c] = sel_max(mx[c], __shfl_xor(mx[c], m));
        }
    }
}

// the same over a 256-thread workgroup, valid in every thread
__device__ __forceinline__ void block_minmax3(float mn[3], float mx[3], float (*s_red)[6]) {
    wave_minmax3(mn, mx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s_red[wave][c] = mn[c]; s_red[wave][3 + c] = mx[c]; }
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kKnnThreads / 64; ++w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { mn[c] = sel_min(mn[c], s_red[w][c]); mx[c] = sel_max(mx[c], s_red[w][3 + c]); }
    }
}

__global__ void __launch_bounds__(kKnnThreads) knn_setup_kernel(const float* __restrict__ xyz, int64_t P, uint32_t* __restrict__ hdr,
                                                                float* __restrict__ partials, uint32_t* __restrict__ scratch,
                                                                int64_t scratch_words) {
    __shared__ float s_red[kKnnThreads / 64][6];
    const int64_t tid = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x, nthr = (int64_t)gridDim.x * kKnnThreads;
    for (int64_t i = tid; i < scratch_words; i += nthr) scratch[i] = 0u;
    if (tid < kKnnHdrWords) hdr[tid] = tid == 0 ? (uint32_t)P : 0u;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = tid; i < P; i += nthr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = xyz[3 * i + c];
            mn[c] = sel_min(mn[c], v);
            mx[c] = sel_max(mx[c], v);
        }
    }
    block_minmax3(mn, mx, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { partials[8 * blockIdx.x + c] = mn[c]; partials[8 * blockIdx.x + 3 + c] = mx[c]; }
    }
}

__device__ __forceinline__ uint32_t spread3(uint32_t v) {   // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// cell of coordinate p on an axis [mn, mx]: 0 for an axis without extent; a quotient that is not a number (an extent that
// overflowed) fails both comparisons and gives 0 as well
__device__ __forceinline__ uint32_t knn_cell(float p, float mn, float mx) {
    const float ext = mx - mn;
    if (!(ext > 0.f)) return 0u;
    const float u = ((p - mn) / ext) * 1024.f;
    return u >= 0.f ? (u < 1023.f ? (uint32_t)u : 1023u) : 0u;
}

__global__ void __launch_bounds__(kKnnThreads) knn_morton_kernel(const float* __restrict__ xyz, int64_t P,
                                                                 const float* __restrict__ partials, int n_partials,
                                                                 uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    __shared__ float s_red[kKnnThreads / 64][6];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if ((int)threadIdx.x < n_partials) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { mn[c] = partials[8 * threadIdx.x + c]; mx[c] = partials[8 * threadIdx.x + 3 + c]; }
    }
    block_minmax3(mn, mx, s_red);
    const int64_t i = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x;
    if (i >= P) return;
    const uint32_t cx = knn_cell(xyz[3 * i], mn[0], mx[0]), cy = knn_cell(xyz[3 * i + 1], mn[1], mx[1]),
                   cz = knn_cell(xyz[3 * i + 2], mn[2], mx[2]);
    keys[i] = (uint64_t)(spread3(cx) | (spread3(cy) << 1) | (spread3(cz) << 2));
    vals[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(kKnnThreads) knn_gather_kernel(const float* __restrict__ xyz, int64_t P,
                                                                 const uint32_t* __restrict__ order, float4* __restrict__ sorted,
                                                                 float4* __restrict__ bmin, float4* __restrict__ bmax,
                                                                 const uint32_t* __restrict__ fail_word, uint32_t* __restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = *fail_word >= 2u ? 2u : 0u;
    const int64_t s = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (s < P) {
        int64_t idx = order[s];
        idx = idx < P ? idx : P - 1;          // (a sort that gave up leaves anything here)
#pragma unroll
        for (int c = 0; c < 3; ++c) mn[c] = mx[c] = xyz[3 * idx + c];
        sorted[s] = make_float4(mn[0], mn[1], mn[2], __uint_as_float((uint32_t)idx));
    }
    wave_minmax3(mn, mx);
    const int64_t box = s / kKnnBox;
    if ((threadIdx.x & 63) == 0 && box * kKnnBox < P) {
        bmin[box] = make_float4(mn[0], mn[1], mn[2], 0.f);
        bmax[box] = make_float4(mx[0], mx[1], mx[2], 0.f);
    }
}

__global__ void __launch_bounds__(kKnnThreads) knn_super_kernel(const float4* __restrict__ bmin, const float4* __restrict__ bmax,
                                                                int64_t nbox, float4* __restrict__ smin, float4* __restrict__ smax) {
    const int64_t b = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x;     // (kKnnSuper = 64 boxes = the lanes of one wave)
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (b < nbox) {
        const float4 lo = bmin[b], hi = bmax[b];
        mn[0] = lo.x; mn[1] = lo.y; mn[2] = lo.z; mx[0] = hi.x; mx[1] = hi.y; mx[2] = hi.z;
    }
    wave_minmax3(mn, mx);
    const int64_t sb = b / kKnnSuper;
    if ((threadIdx.x & 63) == 0 && sb * kKnnSuper < nbox) {
        smin[sb] = make_float4(mn[0], mn[1], mn[2], 0.f);
        smax[sb] = make_float4(mx[0], mx[1], mx[2], 0.f);
    }
}

struct Best {
    float b0, b1, b2;
    int cnt;
    __device__ __forceinline__ void clear() { b0 = b1 = b2 = INFINITY; cnt = 0; }
    __device__ __forceinline__ void insert(float d) {
        const bool l0 = d < b0, l1 = d < b1, l2 = d < b2;
        b2 = l1 ? b1 : (l2 ? d : b2);
        b1 = l0 ? b0 : (l1 ? d : b1);
        b0 = l0 ? d : b0;
        ++cnt;
    }
    __device__ __forceinline__ float kth(int k) const { return k == 3 ? b2 : (k == 2 ? b1 : b0); }
};

__device__ __forceinline__ float knn_d2(const float4& p, const float4& q) {
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

__device__ __forceinline__ float knn_lb(const float4& p, const float4& lo, const float4& hi) {
    const float ex = sel_max(0.f, sel_max(lo.x - p.x, p.x - hi.x));
    const float ey = sel_max(0.f, sel_max(lo.y - p.y, p.y - hi.y));
    const float ez = sel_max(0.f, sel_max(lo.z - p.z, p.z - hi.z));
    return ((ex * ex) + (ey * ey)) + (ez * ez);
}

__global__ void __launch_bounds__(kKnnBox) knn_search_kernel(const float4* __restrict__ sorted, const float4* __restrict__ bmin,
                                                             const float4* __restrict__ bmax, const float4* __restrict__ smin,
                                                             const float4* __restrict__ smax, int64_t P, int64_t nbox, int64_t nsuper,
                                                             float* __restrict__ mean_d2) {
    __shared__ float4 s_pts[kKnnBox];
    const int lane = threadIdx.x;
    const int64_t own = blockIdx.x;
    const int64_t s = own * kKnnBox + lane;
    const bool active = s < P;
    const int k = P - 1 < 3 ? (int)(P - 1) : 3;
    const float4 me = active ? sorted[s] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (k == 0) {                                   // a single point has no neighbour
        if (active) mean_d2[0] = 0.f;
        return;
    }
    Best best;
    best.clear();
    // seeds: with P >= 4 at least three of the six exist; with fewer points they are all the others, k of them
#pragma unroll
    for (int o = -3; o <= 3; ++o) {
        const int64_t j = s + o;
        if (o != 0 && active && j >= 0 && j < P) best.insert(knn_d2(me, sorted[j]));
    }
    const float reject = active ? best.kth(k) : -1.f;     // (a bound is never negative: a lane without a point accepts nothing)
    best.clear();

    s_pts[lane] = me;
    __syncthreads();
    const int n_own = (int)(P - own * kKnnBox < kKnnBox ? P - own * kKnnBox : kKnnBox);
    for (int j = 0; j < n_own; ++j) {
        const float d = knn_d2(me, s_pts[j]);
        if (j != lane) best.insert(d);
    }

    for (int64_t sb = 0; sb < nsuper; ++sb) {
        const float lbs = knn_lb(me, smin[sb], smax[sb]);
        const bool skip_s = lbs > reject || (best.cnt >= k && lbs >= best.kth(k));
        if (__ballot(!skip_s) == 0ull) continue;
        const int64_t b_end = (sb + 1) * kKnnSuper < nbox ? (sb + 1) * kKnnSuper : nbox;
        for (int64_t b = sb * kKnnSuper; b < b_end; ++b) {
            if (b == own) continue;
            const float lb = knn_lb(me, bmin[b], bmax[b]);
            const bool skip = lb > reject || (best.cnt >= k && lb >= best.kth(k));
            if (__ballot(!skip) == 0ull) continue;
            const int64_t first = b * kKnnBox;
            const int nb = (int)(P - first < kKnnBox ? P - first : kKnnBox);
            __syncthreads();                         // (every lane is done with the box staged before)
            if (lane < nb) s_pts[lane] = sorted[first + lane];
            __syncthreads();
            for (int j = 0; j < nb; ++j) best.insert(knn_d2(me, s_pts[j]));
        }
    }
    if (active) {
        const float sum = k == 1 ? best.b0 : (k == 2 ? best.b0 + best.b1 : (best.b0 + best.b1) + best.b2);
        mean_d2[__float_as_uint(me.w)] = sum / (float)k;
    }
}

int check_knn_args(const hs_knn_args* a) {
    const char* fn = "hs_knn_mean_dist_sq";
    if (check_args(fn, a) || check_rows(fn, "P", a->P)) return HS_EINVAL;
    const Field in[] = {{a->xyz, "xyz", 4}, {a->mean_d2, "mean_d2", 4}, {a->workspace, "workspace", 256}, {a->status, "status", 4}};
    return check_fields(fn, in, 4);
}

int launch_knn(const hs_knn_args& a, hipStream_t s) {
    const int64_t P = a.P;
    const KnnWs w(P);
    char* base = (char*)a.workspace;
    uint32_t* hdr = (uint32_t*)(base + w.hdr);
    float* partials = (float*)(base + w.partials);
    uint64_t* ka = (uint64_t*)(base + w.ka); uint32_t* va = (uint32_t*)(base + w.va);
    uint64_t* kb = (uint64_t*)(base + w.kb); uint32_t* vb = (uint32_t*)(base + w.vb);
    float4* sorted = (float4*)(base + w.sorted);
    float4* bmin = (float4*)(base + w.bmin); float4* bmax = (float4*)(base + w.bmax);
    float4* smin = (float4*)(base + w.smin); float4* smax = (float4*)(base + w.smax);
    void* sort_tmp = base + w.sort_tmp;
    const int passes = sort_passes(kKnnBits);
    static_assert(kKnnBits == 30, "four passes: the sorted pairs land in the first buffer");
    const int64_t scratch_words = sort_scratch_words(P, passes, kU64Tile);

    const int64_t pblocks = (P + kKnnThreads - 1) / kKnnThreads;
    const int n_partials = (int)(pblocks < kKnnPartials ? pblocks : kKnnPartials);
    knn_setup_kernel<<<n_partials, kKnnThreads, 0, s>>>(a.xyz, P, hdr, partials, (uint32_t*)sort_tmp, scratch_words);
    HS_LAUNCH_CHECK();
    knn_morton_kernel<<<(unsigned)pblocks, kKnnThreads, 0, s>>>(a.xyz, P, partials, n_partials, ka, va);
    HS_LAUNCH_CHECK();
    const int rc = launch_radix_sort(ka, va, kb, vb, hdr, P, kKnnBits, sort_tmp, hdr + 1, s, /*zeroed=*/true);
    if (rc != HS_OK) return rc;
    knn_gather_kernel<<<(unsigned)pblocks, kKnnThreads, 0, s>>>(a.xyz, P, va, sorted, bmin, bmax, hdr + 1, a.status);
    HS_LAUNCH_CHECK();
    knn_super_kernel<<<(unsigned)((w.nbox + kKnnThreads - 1) / kKnnThreads), kKnnThreads, 0, s>>>(bmin, bmax, w.nbox, smin, smax);
    HS_LAUNCH_CHECK();
    knn_search_kernel<<<(unsigned)w.nbox, kKnnBox, 0, s>>>(sorted, bmin, bmax, smin, smax, P, w.nbox, w.nsuper, a.mean_d2);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_knn_workspace_bytes(int64_t P) {
    if (hs::check_rows("hs_knn_workspace_bytes", "P", P)) return HS_EINVAL;
    return hs::KnnWs(P).bytes;
}

HS_API int hs_knn_mean_dist_sq(const hs_knn_args* a, void* hip_stream) {
    const int rc = hs::check_knn_args(a);
    if (rc != HS_OK) return rc;
    if (a->P == 0) return HS_OK;
    return hs::launch_knn(*a, (hipStream_t)hip_stream);
}

}  // extern "C"
