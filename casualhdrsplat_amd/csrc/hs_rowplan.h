// The tail of a row plan, shared by densify.hip (hs_densify_plan) and rows.hip (hs_rows_plan): a classify kernel of the
// including unit leaves a 2-bit code per row
//     0 leaves nothing   1 survives   2 survives + one clone   3 goes, two children
// as a byte of the workspace and per block of 256 rows four counts {survivors, clones, kept splits, split sources}; the two
// kernels here turn them into `counts` and row_map (include/hdrsplat.h, hs_densify_plan, states both formats).  Kernels
// in a header: each unit compiles its own copy inside its unnamed namespace, from this one text.
#pragma once
#include "hs_cloud.h"

namespace hs {
namespace {

constexpr int kDenRows = 256;                 // rows per workgroup of the plan (= threads)
constexpr int kDenScanThreads = 1024;

inline int64_t den_blocks(int64_t P) { return (P + kDenRows - 1) / kDenRows; }

__device__ __forceinline__ uint4 add4(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

__global__ void __launch_bounds__(kDenScanThreads) densify_scan_kernel(uint4* __restrict__ blocks, int64_t nblk, uint32_t P,
                                                                        uint32_t* __restrict__ counts) {
    __shared__ uint4 s_part[kDenScanThreads];
    const int t = threadIdx.x;
    const int64_t per = (nblk + kDenScanThreads - 1) / kDenScanThreads;
    const int64_t b0 = t * per < nblk ? t * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
    uint4 acc = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t b = b0; b < b1; ++b) acc = add4(acc, blocks[b]);
    s_part[t] = acc;
    __syncthreads();
    for (int off = 1; off < kDenScanThreads; off <<= 1) {
        const uint4 v = t >= off ? s_part[t - off] : make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        s_part[t] = add4(s_part[t], v);
        __syncthreads();
    }
    uint4 run = t ? s_part[t - 1] : make_uint4(0u, 0u, 0u, 0u);
    for (int64_t b = b0; b < b1; ++b) {
        const uint4 c = blocks[b];
        blocks[b] = run;
        run = add4(run, c);
    }
    if (t == kDenScanThreads - 1) {
        const uint4 tot = s_part[t];      // {survivors, clones, kept splits, split sources}
        counts[0] = tot.x + tot.y + 2u * tot.z;
        counts[1] = tot.x;
        counts[2] = tot.y;
        counts[3] = 2u * tot.z;
        counts[4] = P - tot.x - tot.z;
        counts[5] = tot.w;
        counts[6] = P;
        counts[7] = 0u;
    }
}

__global__ void __launch_bounds__(kDenRows) densify_map_kernel(const uint8_t* __restrict__ codes, const uint4* __restrict__ prefix,
                                                               int64_t P, const uint32_t* __restrict__ counts,
                                                               uint32_t* __restrict__ row_map, uint32_t* counts_host) {
    __shared__ uint32_t s_cnt[kDenRows / 64][3];
    if (counts_host && blockIdx.x == 0 && threadIdx.x < HS_DENSIFY_COUNTS)   // (the stage's last kernel, as tile_ranges_kernel is)
        __hip_atomic_store(counts_host + threadIdx.x, counts[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (P == 0) return;
    const int64_t i = (int64_t)blockIdx.x * kDenRows + threadIdx.x;
    const uint32_t code = i < P ? codes[i] : 0u;
    const bool surv = code == 1u || code == 2u, clone = code == 2u, kept = code == 3u;
    const unsigned long long b_surv = __ballot(surv), b_clone = __ballot(clone), b_kept = __ballot(kept);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_cnt[wave][0] = (uint32_t)__popcll(b_surv);
        s_cnt[wave][1] = (uint32_t)__popcll(b_clone);
        s_cnt[wave][2] = (uint32_t)__popcll(b_kept);
    }
    __syncthreads();
    const uint4 pre = prefix[blockIdx.x];
    uint32_t js = pre.x, jc = pre.y, jk = pre.z;
    for (int w = 0; w < wave; ++w) { js += s_cnt[w][0]; jc += s_cnt[w][1]; jk += s_cnt[w][2]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    js += (uint32_t)__popcll(b_surv & below);
    jc += (uint32_t)__popcll(b_clone & below);
    jk += (uint32_t)__popcll(b_kept & below);
    const uint32_t n_surv = counts[1], n_clone = counts[2], n_kept = counts[3] >> 1;
    const uint32_t src = (uint32_t)i;
    // (every index is below P_out = n_surv + n_clone + 2 n_kept <= 2 P: the prefixes and totals count the same codes)
    if (surv) row_map[js] = ((uint32_t)HS_DENSIFY_KIND_SURVIVOR << 30) | src;
    if (clone) row_map[n_surv + jc] = ((uint32_t)HS_DENSIFY_KIND_CLONE << 30) | src;
    if (kept) {
        row_map[n_surv + n_clone + jk] = ((uint32_t)HS_DENSIFY_KIND_CHILD0 << 30) | src;
        row_map[n_surv + n_clone + n_kept + jk] = ((uint32_t)HS_DENSIFY_KIND_CHILD1 << 30) | src;
    }
}

}  // namespace
}  // namespace hs
