// k-means vector quantisation of the rows of a matrix -- the SH codebook compression of a finished cloud (LightGaussian's
// "VecTree", gsplat's PngCompression on shN, Compact3D): Lloyd's assignment and its importance-weighted centroid update
// (hs_vq_workspace_bytes, hs_vq_assign, hs_vq_update; include/hdrsplat.h).
//
// Compiled with -ffp-contract=off: the assignment is an INTEGER DECISION from a STATED ORDER of IEEE fp32 operations, which
// tests/vq_reference.py restates in numpy float32 and the GPU tests compare bit for bit.  Do not reassociate it.
//
// ASSIGN.  x [N, D] fp32 row-major, codebook [K, D] fp32.  For every row i and centroid k
//       acc = 0;  for d = 0 .. D-1 ascending:  t = x[i,d] - c[k,d];  acc = acc + t * t        (three roundings per term)
//   d2(i, k) = acc.  best = +inf, code = 0;  for k = 0 .. K-1 ascending:  if d2(i, k) < best: best = d2(i, k), code = k.
//   Strict <: ties go to the lower k, a NaN distance never wins, a row whose distances are all NaN keeps code 0 and +inf.
//   codes[i] = code (int32), dist2[i] = best (when asked for).
// UPDATE.  weights [N] fp32 >= 0 (null: all 1), codes [N] int32, the previous codebook.  For each cluster k with members
//   {i : codes[i] == k}:  S_w = sum (double)w_i,  S_d = sum (double)w_i * (double)x[i,d]  (the product is exact in fp64),
//   out[k,d] = (float)(S_d / S_w) when S_w > 0, else the previous codebook's row bit for bit (an empty cluster, or one whose
//   weights are all zero).  counts[k] = members of k, whatever their weights.  A code outside [0, K) belongs to no cluster.
//   ORDER OF THE fp64 SUMS, a function of (N, K, codes) alone.  The members of cluster k, in ascending row index (a stable
//   counting sort), are numbered j = 0 .. n_k - 1.  With S = vq_slices(N, K) = min(64, max(1, ceil(N / (1024 K)))), slice s of
//   the cluster holds j in [floor(n_k s / S), floor(n_k (s+1) / S)).  Inside a slice that starts at j0, chain q = 0 .. 3 adds
//   the members j0 + q, j0 + q + 4, ... in ascending order, from +0; the slice's sum is ((chain0 + chain1) + chain2) + chain3;
//   the cluster's sum adds the slices s = 0 .. S-1 in ascending order, from +0.  S_w is summed the same way.
//
// vq_assign_kernel<DP>  256 threads, one row per thread with its D values (zero-padded to DP, a multiple of 4: the padding adds
//                        exact zeros to acc) in registers.  The codebook goes through LDS in chunks of 64 centroids; every lane
//                        reads the same 16 bytes -- a broadcast, no bank conflict -- and a thread runs the add chains of four
//                        centroids side by side.  Plain fp32 sub / mul / add (the unit is compiled without SLP vectorisation:
//                        packed fp32 measured slower, see HS_TUNE_VQ_GROUP).  Bound by the vector ALU: 3 N K DP lane operations.
// vq_rank_kernel<false>  one wave per block of consecutive rows (at most 1024 blocks), walking them 64 at a time IN ORDER:
//                        per-block histogram of the codes in LDS (plain stores by one lane per distinct code of the step:
//                        no atomics), K in ranges of 8192 bins.  Writes every word of hist [blocks, K].
// vq_column_scan_kernel  per k: exclusive prefix down the blocks in place (four runs of blocks, a thread each), counts[k] = the total.
// vq_start_kernel        one workgroup: exclusive prefix of counts -> start [K].
// vq_rank_kernel<true>   the same walk, now placing row i at start[c] + hist[block, c] + (members of c seen earlier in the
//                        block): perm [N], rows sorted by code, ascending row index inside a code.
// vq_segsum_kernel       one workgroup per (cluster, slice): wave q is chain q, lane d owns dimension d; writes the record
//                        of D + 1 doubles of EVERY (cluster, slice), empty ones as zeros.  Bound by the gather of x (N D 4 bytes).
// vq_finish_kernel       one thread per (k, d): the slices added in order, the divide, or the previous row.
// No atomics on memory, no memset, no copy, no host wait: every word of the workspace that is read was written by an earlier
// kernel of the same call, and the same inputs give the same bits, also inside a captured graph.
#include "hs_cloud.h"

#include <math.h>

namespace hs {
namespace {

constexpr int kVqMaxD = 48, kVqMaxK = 65536;
constexpr int64_t kVqMaxN = 1ll << 30;
// Centroids a thread evaluates side by side (independent add chains).  Measured at N = 2^20, D = 45, K = 4096 (hs_vq_assign, ms):
// 4 -> 10.62, 8 -> 10.58; two rows per thread with 2 / 4 -> 10.67 / 10.40; two centroids per packed-fp32 instruction (two rows
// / one row per thread) 12.07 / 11.85 (as if a packed instruction took the issue slots of both its halves).
#ifndef HS_TUNE_VQ_GROUP
#define HS_TUNE_VQ_GROUP 4
#endif
constexpr int kVqThreads = 256, kVqGroup = HS_TUNE_VQ_GROUP;
constexpr int kVqChunk = 64;                          // centroids per LDS chunk
static_assert(kVqChunk % kVqGroup == 0, "a group of centroids stays inside the chunk");
constexpr int kVqMaxBlocks = 1024, kVqMinBlockRows = 256, kVqBins = 8192;
constexpr int kVqSliceRows = 1024, kVqMaxSlices = 64;
constexpr int kVqStartThreads = 1024;

// rows per block of the counting sort: a multiple of 64, at least 256, and so that at most 1024 blocks cover N
inline int64_t vq_block_rows(int64_t N) {
    const int64_t per = (N + kVqMaxBlocks - 1) / kVqMaxBlocks;
    return align_up(per > kVqMinBlockRows ? per : kVqMinBlockRows, 64);
}
inline int64_t vq_blocks(int64_t N) { return (N + vq_block_rows(N) - 1) / vq_block_rows(N); }
inline int vq_slices(int64_t N, int K) {
    const int64_t s = (N + (int64_t)kVqSliceRows * K - 1) / ((int64_t)kVqSliceRows * K);
    return (int)(s < 1 ? 1 : s > kVqMaxSlices ? kVqMaxSlices : s);
}

struct VqWs {
    int64_t hist, start, perm, records, bytes;
    VqWs(int64_t N, int D, int K) {
        int64_t o = 0;
        const int64_t most = (N + kVqMinBlockRows - 1) / kVqMinBlockRows;   // >= vq_blocks(N), and never shrinks as N grows
        hist = o; o += align_up(4 * (most < kVqMaxBlocks ? most : kVqMaxBlocks) * K, 256);
        start = o; o += align_up(4ll * K, 256);
        perm = o; o += align_up(4 * N, 256);
        records = o; o += align_up(8ll * K * vq_slices(N, K) * (D + 1), 256);
        bytes = o;
    }
};

template <int DP>
__global__ void __launch_bounds__(kVqThreads) vq_assign_kernel(const float* __restrict__ x, const float* __restrict__ cb, int64_t N,
                                                               int D, int K, int32_t* __restrict__ codes, float* __restrict__ dist2) {
    __shared__ __attribute__((aligned(16))) float s_cb[kVqChunk * DP];   // [centroid of the chunk][d], zero-padded
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kVqThreads + tid;
    float xr[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) xr[d] = (i < N && d < D) ? x[i * D + d] : 0.f;
    float best = INFINITY;
    int code = 0;
    for (int k0 = 0; k0 < K; k0 += kVqChunk) {
        __syncthreads();   // the chunk before this one has been read
        for (int e = tid; e < kVqChunk * DP; e += kVqThreads) {
            const int kk = e / DP, d = e - kk * DP;
            s_cb[e] = (k0 + kk < K && d < D) ? cb[(int64_t)(k0 + kk) * D + d] : 0.f;
        }
        __syncthreads();
        const int nk = K - k0 < kVqChunk ? K - k0 : kVqChunk;
        for (int kk = 0; kk < nk; kk += kVqGroup) {   // (a group may reach past nk: zero rows, computed and not compared)
            float acc[kVqGroup];
#pragma unroll
            for (int j = 0; j < kVqGroup; ++j) acc[j] = 0.f;
#pragma unroll
            for (int d = 0; d < DP; d += 4) {
                f4 c[kVqGroup];
#pragma unroll
                for (int j = 0; j < kVqGroup; ++j) c[j] = *reinterpret_cast<const f4*>(s_cb + (kk + j) * DP + d);
#pragma unroll
                for (int j = 0; j < kVqGroup; ++j) {
                    float t = xr[d] - c[j].x; acc[j] = acc[j] + t * t;
                    t = xr[d + 1] - c[j].y; acc[j] = acc[j] + t * t;
                    t = xr[d + 2] - c[j].z; acc[j] = acc[j] + t * t;
                    t = xr[d + 3] - c[j].w; acc[j] = acc[j] + t * t;
                }
            }
#pragma unroll
            for (int j = 0; j < kVqGroup; ++j)
                if (kk + j < nk && acc[j] < best) { best = acc[j]; code = k0 + kk + j; }
        }
    }
    if (i < N) {
        codes[i] = code;
        if (dist2) dist2[i] = best;
    }
}

// One wave per block of `block_rows` consecutive rows.  kScatter = false: hist[block, k] = rows of the block with code k.
// kScatter = true: perm[start[c] + hist[block, c] + earlier members of c in the block] = i (hist then holds the exclusive
// prefixes down the blocks).
template <bool kScatter>
__global__ void __launch_bounds__(64) vq_rank_kernel(const int32_t* __restrict__ codes, int64_t N, int K, int64_t block_rows,
                                                     uint32_t* __restrict__ hist, const uint32_t* __restrict__ start,
                                                     uint32_t* __restrict__ perm) {
    __shared__ uint32_t s_cnt[kVqBins];
    const int lane = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * block_rows, hi = lo + block_rows < N ? lo + block_rows : N;
    uint32_t* __restrict__ my_hist = hist + (int64_t)blockIdx.x * K;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int kbase = 0; kbase < K; kbase += kVqBins) {
        const int nb = K - kbase < kVqBins ? K - kbase : kVqBins;
        for (int j = lane; j < nb; j += 64) s_cnt[j] = 0u;
        __syncthreads();
        for (int64_t i0 = lo; i0 < hi; i0 += 64) {
            const int64_t i = i0 + lane;
            const int c = i < hi ? codes[i] : -1;
            const bool valid = c >= kbase && c < kbase + nb;
            const uint32_t local = valid ? (uint32_t)(c - kbase) : 0u;
            unsigned long long same = __ballot(valid);   // the lanes of this step with my code
#pragma unroll
            for (int b = 0; b < 13; ++b) {
                const bool bit = (local >> b) & 1u;
                const unsigned long long bal = __ballot(bit);
                same &= bit ? bal : ~bal;
            }
            const uint32_t rank = (uint32_t)__popcll(same & below), total = (uint32_t)__popcll(same);
            const uint32_t seen = valid ? s_cnt[local] : 0u;
            if (kScatter && valid) perm[start[c] + my_hist[c] + seen + rank] = (uint32_t)i;
            __syncthreads();
            if (valid && rank + 1u == total) s_cnt[local] = seen + total;   // one lane per distinct code
            __syncthreads();
        }
        if (!kScatter)
            for (int j = lane; j < nb; j += 64) my_hist[kbase + j] = s_cnt[j];
        __syncthreads();
    }
}

// lane = one of 64 consecutive k, wave = one of four runs of consecutive blocks: sums of the runs, then the prefixes
__global__ void __launch_bounds__(256) vq_column_scan_kernel(uint32_t* __restrict__ hist, int nblk, int K, int32_t* __restrict__ counts) {
    __shared__ uint32_t s_run[4][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane;
    const int per = (nblk + 3) / 4;
    const int b0 = q * per < nblk ? q * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
    uint32_t sum = 0u;
    if (k < K) {
        int b = b0;
        for (; b + 8 <= b1; b += 8) {   // eight loads in flight
            uint32_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = hist[(int64_t)(b + u) * K + k];
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += v[u];
        }
        for (; b < b1; ++b) sum += hist[(int64_t)b * K + k];
    }
    s_run[q][lane] = sum;
    __syncthreads();
    if (k >= K) return;
    uint32_t run = 0u;
    for (int w = 0; w < q; ++w) run += s_run[w][lane];
    if (q == 3) counts[k] = (int32_t)(run + sum);
    int b = b0;
    for (; b + 8 <= b1; b += 8) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = hist[(int64_t)(b + u) * K + k];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            hist[(int64_t)(b + u) * K + k] = run;
            run += v[u];
        }
    }
    for (; b < b1; ++b) {
        const uint32_t c = hist[(int64_t)b * K + k];
        hist[(int64_t)b * K + k] = run;
        run += c;
    }
}

__global__ void __launch_bounds__(kVqStartThreads) vq_start_kernel(const int32_t* __restrict__ counts, int K, uint32_t* __restrict__ start) {
    __shared__ uint32_t s_part[kVqStartThreads];
    const int t = threadIdx.x;
    const int per = (K + kVqStartThreads - 1) / kVqStartThreads;
    const int b0 = t * per < K ? t * per : K, b1 = b0 + per < K ? b0 + per : K;
    uint32_t acc = 0u;
    for (int k = b0; k < b1; ++k) acc += (uint32_t)counts[k];
    s_part[t] = acc;
    __syncthreads();
    for (int off = 1; off < kVqStartThreads; off <<= 1) {
        const uint32_t v = t >= off ? s_part[t - off] : 0u;
        __syncthreads();
        s_part[t] += v;
        __syncthreads();
    }
    uint32_t run = t ? s_part[t - 1] : 0u;
    for (int k = b0; k < b1; ++k) {
        start[k] = run;
        run += (uint32_t)counts[k];
    }
}

__global__ void __launch_bounds__(256) vq_segsum_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const uint32_t* __restrict__ perm, const uint32_t* __restrict__ start,
                                                        const int32_t* __restrict__ counts, int D, int S, double* __restrict__ records) {
    __shared__ double s_acc[4][64];
    __shared__ double s_sw[4];
    const int k = blockIdx.x, s = blockIdx.y;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t n = counts[k];
    const int64_t j0 = n * s / S, j1 = n * (s + 1) / S;
    const uint32_t* __restrict__ mem = perm + start[k];
    const bool on = lane < D;
    double acc = 0.0, sw = 0.0;
    int64_t j = j0 + q;
    for (; j + 12 < j1; j += 16) {   // four members of the chain in flight; added in order
        const int64_t i0 = mem[j], i1 = mem[j + 4], i2 = mem[j + 8], i3 = mem[j + 12];
        const float w0 = w ? w[i0] : 1.f, w1 = w ? w[i1] : 1.f, w2 = w ? w[i2] : 1.f, w3 = w ? w[i3] : 1.f;
        const float x0 = on ? x[i0 * D + lane] : 0.f, x1 = on ? x[i1 * D + lane] : 0.f;
        const float x2 = on ? x[i2 * D + lane] : 0.f, x3 = on ? x[i3 * D + lane] : 0.f;
        acc += (double)w0 * (double)x0; sw += (double)w0;
        acc += (double)w1 * (double)x1; sw += (double)w1;
        acc += (double)w2 * (double)x2; sw += (double)w2;
        acc += (double)w3 * (double)x3; sw += (double)w3;
    }
    for (; j < j1; j += 4) {
        const int64_t i = mem[j];
        const float wi = w ? w[i] : 1.f;
        const float xi = on ? x[i * D + lane] : 0.f;
        acc += (double)wi * (double)xi; sw += (double)wi;
    }
    s_acc[q][lane] = acc;
    if (lane == 0) s_sw[q] = sw;
    __syncthreads();
    if (q == 0) {
        double* __restrict__ rec = records + ((int64_t)k * S + s) * (D + 1);
        if (on) rec[lane] = ((s_acc[0][lane] + s_acc[1][lane]) + s_acc[2][lane]) + s_acc[3][lane];
        if (lane == 0) rec[D] = ((s_sw[0] + s_sw[1]) + s_sw[2]) + s_sw[3];
    }
}

// S = 0: no rows at all (N = 0): every row is the previous one and the counts are zero
__global__ void __launch_bounds__(256) vq_finish_kernel(const double* __restrict__ records, const float* __restrict__ prev, int D, int K,
                                                        int S, float* __restrict__ out, int32_t* __restrict__ counts) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= K * D) return;
    const int k = e / D, d = e - k * D;
    double sd = 0.0, sw = 0.0;
    for (int s = 0; s < S; ++s) {
        const double* __restrict__ rec = records + ((int64_t)k * S + s) * (D + 1);
        sd += rec[d];
        sw += rec[D];
    }
    out[e] = sw > 0.0 ? (float)(sd / sw) : prev[e];
    if (S == 0 && d == 0) counts[k] = 0;
}

int check_shape(const char* fn, int64_t N, int D, int K) {
    if (N < 0 || N > kVqMaxN || D < 1 || D > kVqMaxD || K < 1 || K > kVqMaxK) {
        set_error("%s: N=%lld, D=%d, K=%d outside 0 <= N <= 2^30, 1 <= D <= %d, 1 <= K <= %d", fn, (long long)N, D, K, kVqMaxD,
                  kVqMaxK);
        return HS_EINVAL;
    }
    return HS_OK;
}

template <int DP>
int launch_assign(const hs_vq_args& a, hipStream_t s) {
    const unsigned grid = (unsigned)((a.N + kVqThreads - 1) / kVqThreads);
    vq_assign_kernel<DP><<<grid, kVqThreads, 0, s>>>(a.x, a.codebook_in, a.N, a.D, a.K, a.codes, a.dist2);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_vq_workspace_bytes(int32_t N, int32_t D, int32_t K) {
    if (hs::check_shape("hs_vq_workspace_bytes", N, D, K)) return HS_EINVAL;
    const int64_t b = hs::VqWs(N, D, K).bytes;
    return b > 0 ? b : 256;
}

HS_API int hs_vq_assign(const hs_vq_args* a, void* hip_stream) {
    const char* fn = "hs_vq_assign";
    if (hs::check_args(fn, a) || hs::check_shape(fn, a->N, a->D, a->K)) return HS_EINVAL;
    if (hs::check_field(fn, a->codebook_in, "codebook_in", 4) || hs::check_aligned(fn, a->dist2, "dist2", 4)) return HS_EINVAL;
    if (a->N == 0) {
        if (hs::check_aligned(fn, a->x, "x", 4) || hs::check_aligned(fn, a->codes, "codes", 4)) return HS_EINVAL;
        return HS_OK;
    }
    const hs::Field f[2] = {{a->x, "x", 4}, {a->codes, "codes", 4}};
    if (hs::check_fields(fn, f, 2)) return HS_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    const int D = a->D;
    if (D <= 4) return hs::launch_assign<4>(*a, s);
    if (D <= 8) return hs::launch_assign<8>(*a, s);
    if (D <= 12) return hs::launch_assign<12>(*a, s);
    if (D <= 16) return hs::launch_assign<16>(*a, s);
    if (D <= 24) return hs::launch_assign<24>(*a, s);
    if (D <= 32) return hs::launch_assign<32>(*a, s);
    return hs::launch_assign<48>(*a, s);
}

HS_API int hs_vq_update(const hs_vq_args* a, void* hip_stream) {
    const char* fn = "hs_vq_update";
    if (hs::check_args(fn, a) || hs::check_shape(fn, a->N, a->D, a->K)) return HS_EINVAL;
    const hs::Field f[3] = {{a->codebook_in, "codebook_in", 4}, {a->codebook_out, "codebook_out", 4}, {a->counts, "counts", 4}};
    if (hs::check_fields(fn, f, 3) || hs::check_aligned(fn, a->weights, "weights", 4)) return HS_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    const int D = a->D, K = a->K;
    const unsigned finish_grid = (unsigned)((K * D + 255) / 256);
    if (a->N == 0) {
        if (hs::check_aligned(fn, a->x, "x", 4) || hs::check_aligned(fn, a->codes, "codes", 4) ||
            hs::check_aligned(fn, a->workspace, "workspace", 256))
            return HS_EINVAL;
        hs::vq_finish_kernel<<<finish_grid, 256, 0, s>>>(nullptr, a->codebook_in, D, K, 0, a->codebook_out, a->counts);
        HS_LAUNCH_CHECK();
        return HS_OK;
    }
    const hs::Field g[3] = {{a->x, "x", 4}, {a->codes, "codes", 4}, {a->workspace, "workspace", 256}};
    if (hs::check_fields(fn, g, 3)) return HS_EINVAL;
    const int64_t N = a->N;
    const hs::VqWs ws(N, D, K);
    char* base = (char*)a->workspace;
    uint32_t* hist = (uint32_t*)(base + ws.hist);
    uint32_t* start = (uint32_t*)(base + ws.start);
    uint32_t* perm = (uint32_t*)(base + ws.perm);
    double* records = (double*)(base + ws.records);
    const int64_t block_rows = hs::vq_block_rows(N);
    const int nblk = (int)hs::vq_blocks(N), S = hs::vq_slices(N, K);
    hs::vq_rank_kernel<false><<<nblk, 64, 0, s>>>(a->codes, N, K, block_rows, hist, nullptr, nullptr);
    HS_LAUNCH_CHECK();
    hs::vq_column_scan_kernel<<<(K + 63) / 64, 256, 0, s>>>(hist, nblk, K, a->counts);
    HS_LAUNCH_CHECK();
    hs::vq_start_kernel<<<1, hs::kVqStartThreads, 0, s>>>(a->counts, K, start);
    HS_LAUNCH_CHECK();
    hs::vq_rank_kernel<true><<<nblk, 64, 0, s>>>(a->codes, N, K, block_rows, hist, start, perm);
    HS_LAUNCH_CHECK();
    hs::vq_segsum_kernel<<<dim3((unsigned)K, (unsigned)S), 256, 0, s>>>(a->x, a->weights, perm, start, a->counts, D, S, records);
    HS_LAUNCH_CHECK();
    hs::vq_finish_kernel<<<finish_grid, 256, 0, s>>>(records, a->codebook_in, D, K, S, a->codebook_out, a->counts);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
