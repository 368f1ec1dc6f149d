// Score-driven row plans of the cloud (hs_rows_workspace_bytes, hs_rows_plan; include/hdrsplat.h states the contract, the
// order on scores and the three modes).  The plan's output is hs_densify_plan's: hs_densify_apply gathers from it.
//
// SELECT (KEEP and DENSIFY with k > 0), an exact radix select over the order-preserving 32-bit key of the score, most
// significant byte first, four passes of two kernels:
//   rows_hist_kernel   each workgroup owns a CONTIGUOUS chunk of rows (a multiple of 256, at most kSelBlocks workgroups) and
//                      counts, in LDS (integer atomics), the byte of the pass over the rows whose higher bytes equal the
//                      prefix found so far; it writes its 256 counts to the workspace: no global atomics, nothing to zero
//   rows_pick_kernel   ONE workgroup sums the histograms, walks them from the largest byte down and picks the byte that holds
//                      the k-th best key; it leaves {prefix, rows still to take, rows in the picked bin} in the workspace.
//                      After the last pass the prefix is the k-th best key, "rows still to take" is the number of rows AT the
//                      threshold that are selected (k minus the rows strictly above) and the bin is the tie class T -- and
//                      since chunks are contiguous, the last pass's histograms hold every chunk's number of threshold rows:
//                      their exclusive prefix over the chunks is written too
// CLASSIFY, one kernel (all three modes), the same chunks: a workgroup walks its chunk 256 rows at a time and carries the rank
// among the threshold rows (chunk prefix + rows of earlier tiles + wave counts + ballot rank: source order).  A row is
// selected when its key is above the threshold, or at it with rank < rows to take.  It writes densify's 2-bit code per row
// and densify's four counts per 256 rows.
// TAIL: densify's own scan and map kernels (hs_rowplan.h); with k > 0 one more single-wave kernel puts T into counts[7] and
// leaves the host copy.
// No float arithmetic, no float atomics, no global atomics, no look-back; every workspace word is written before it is read.
#include "hs_cloud.h"
#include "hs_rowplan.h"

#include <math.h>
#include <string.h>

namespace hs {
namespace {

constexpr int kSelBlocks = 256;               // most chunks of the select and the classify (<= the pick's 256 scan threads)
constexpr int kSelBins = 256;                 // 8-bit digits
constexpr int kPickThreads = 1024;
static_assert(kSelBlocks <= kSelBins, "the pick scans the chunks' threshold rows with one thread per bin");

struct RowsPlan {
    int64_t P, k, chunk;                      // chunk: rows per workgroup, a multiple of kDenRows
    const float* score; const uint8_t* mask; const float* scales;
    float tau_split;
    int32_t mode;
};

// The order on scores as an unsigned key: NaN -> 0 (below -inf, whose key is 0x007fffff), -0 -> the key of +0, everything
// else the usual sign flip.  Bits only.
__device__ __forceinline__ uint32_t score_key(float x) {
    uint32_t b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0u;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// state words the pick leaves in the workspace
enum { kSelPrefix = 0, kSelTake = 1, kSelTies = 2 };

__global__ void __launch_bounds__(kDenRows) rows_hist_kernel(const float* __restrict__ score, int64_t P, int64_t chunk, int pass,
                                                             const uint32_t* __restrict__ sel, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[kSelBins];
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t prefix = pass ? sel[kSelPrefix] : 0u;
    const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = r0 + chunk < P ? r0 + chunk : P;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kDenRows) {
        const uint32_t key = score_key(score[i]);
        // (pass 0: every row is a candidate; later: the bytes above this pass's equal the prefix's)
        if (pass == 0 || ((key ^ prefix) >> (shift + 8)) == 0u) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(int64_t)blockIdx.x * kSelBins + threadIdx.x] = s_hist[threadIdx.x];
}

// inclusive scan of s[0 .. 256) by the first 256 threads of the workgroup (all threads reach the barriers); `down`: suffix sums
__device__ __forceinline__ void pick_scan(uint32_t* s, int t, bool down) {
    for (int off = 1; off < kSelBins; off <<= 1) {
        uint32_t v = 0u;
        if (t < kSelBins) v = down ? (t + off < kSelBins ? s[t + off] : 0u) : (t >= off ? s[t - off] : 0u);
        __syncthreads();
        if (t < kSelBins) s[t] += v;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kPickThreads) rows_pick_kernel(const uint32_t* __restrict__ hist, int nchunks, int pass, uint32_t k,
                                                                 uint32_t* __restrict__ sel, uint32_t* __restrict__ tie_prefix) {
    __shared__ uint32_t s_part[kPickThreads];
    __shared__ uint32_t s_suf[kSelBins];
    __shared__ uint32_t s_digit;
    const int t = threadIdx.x;
    const uint32_t take = pass ? sel[kSelTake] : k, prefix = pass ? sel[kSelPrefix] : 0u;
    uint32_t part = 0u;                       // bin (t & 255) over every fourth chunk; the four partial sums meet in LDS
#pragma unroll 8
    for (int b = t >> 8; b < nchunks; b += kPickThreads / kSelBins) part += hist[b * kSelBins + (t & 255)];
    s_part[t] = part;
    __syncthreads();                          // (also: every thread has read `sel` before the winner writes it)
    uint32_t total = 0u;
    if (t < kSelBins) {
        total = ((s_part[t] + s_part[t + 256]) + s_part[t + 512]) + s_part[t + 768];
        s_suf[t] = total;
    }
    __syncthreads();
    pick_scan(s_suf, t, true);                // rows in bins >= t
    if (t < kSelBins) {
        const uint32_t above = s_suf[t] - total;      // candidates in larger bins
        // 1 <= take <= candidates, and the bins partition the candidates: exactly one thread finds its bin
        if (above < take && take <= above + total) {
            sel[kSelPrefix] = prefix | ((uint32_t)t << (24 - 8 * pass));
            sel[kSelTake] = take - above;
            sel[kSelTies] = total;
            s_digit = (uint32_t)t;
        }
    }
    if (pass != 3) return;                    // (uniform)
    __syncthreads();
    // chunk t's rows AT the threshold, and their exclusive prefix over the chunks
    const uint32_t mine = t < nchunks ? hist[t * kSelBins + s_digit] : 0u;      // (nchunks <= kSelBlocks = 256)
    if (t < kSelBins) s_suf[t] = mine;
    __syncthreads();
    pick_scan(s_suf, t, false);
    if (t < nchunks) tie_prefix[t] = s_suf[t] - mine;
}

__global__ void __launch_bounds__(kDenRows) rows_classify_kernel(const RowsPlan a, const uint32_t* __restrict__ sel,
                                                                 const uint32_t* __restrict__ tie_prefix, uint8_t* __restrict__ codes,
                                                                 uint4* __restrict__ blocks) {
    __shared__ uint32_t s_tie[kDenRows / 64];
    __shared__ uint32_t s_cnt[kDenRows / 64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool scored = a.mode != HS_ROWS_MASK && a.k > 0;      // (k == 0: nothing is selected and the state was never written)
    const uint32_t thr = scored ? sel[kSelPrefix] : 0u, take = scored ? sel[kSelTake] : 0u;
    uint32_t rank0 = scored ? tie_prefix[blockIdx.x] : 0u;      // threshold rows before this tile
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk, r1 = r0 + a.chunk < a.P ? r0 + a.chunk : a.P;
    for (int64_t base = r0; base < r1; base += kDenRows) {      // (uniform: chunk is a multiple of kDenRows)
        const int64_t i = base + threadIdx.x;
        const bool live = i < r1;
        bool selected = false;
        if (scored) {
            const uint32_t key = live ? score_key(a.score[i]) : 0u;
            const bool tie = live && key == thr;
            const unsigned long long b_tie = __ballot(tie);
            if (lane == 0) s_tie[wave] = (uint32_t)__popcll(b_tie);
            __syncthreads();
            uint32_t rank = rank0 + (uint32_t)__popcll(b_tie & below);
            for (int w = 0; w < wave; ++w) rank += s_tie[w];
            for (int w = 0; w < kDenRows / 64; ++w) rank0 += s_tie[w];
            selected = live && (key > thr || (tie && rank < take));
        }
        uint32_t code = 0u;
        if (live) {
            if (a.mode == HS_ROWS_MASK) {
                code = a.mask[i] ? 0u : 1u;
            } else if (a.mode == HS_ROWS_KEEP) {
                code = selected ? 1u : 0u;
            } else {
                code = 1u;
                if (selected) {
                    float s = a.scales[3 * i];
                    const float s1 = a.scales[3 * i + 1], s2 = a.scales[3 * i + 2];
                    if (s1 > s) s = s1;
                    if (s2 > s) s = s2;
                    code = s > a.tau_split ? 3u : 2u;
                }
            }
            codes[i] = (uint8_t)code;
        }
        const unsigned long long b_surv = __ballot(code == 1u || code == 2u), b_clone = __ballot(code == 2u);
        const unsigned long long b_kept = __ballot(code == 3u);
        if (lane == 0) {
            s_cnt[wave][0] = (uint32_t)__popcll(b_surv);
            s_cnt[wave][1] = (uint32_t)__popcll(b_clone);
            s_cnt[wave][2] = (uint32_t)__popcll(b_kept);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint4 c = make_uint4(0u, 0u, 0u, 0u);
            for (int w = 0; w < kDenRows / 64; ++w) { c.x += s_cnt[w][0]; c.y += s_cnt[w][1]; c.z += s_cnt[w][2]; }
            c.w = c.z;                        // split sources: nothing is pruned, every split keeps its children
            blocks[base / kDenRows] = c;
        }
        __syncthreads();                      // (s_tie and s_cnt are rewritten by the next tile)
    }
}

// k > 0: counts[7] = T after densify's scan wrote 0 there, and the host copy the map kernel was not asked for
__global__ void __launch_bounds__(64) rows_ties_kernel(uint32_t* __restrict__ counts, const uint32_t* __restrict__ sel,
                                                       uint32_t* counts_host) {
    const int t = threadIdx.x;
    if (t >= HS_DENSIFY_COUNTS) return;
    const uint32_t v = t == HS_DENSIFY_COUNTS - 1 ? sel[kSelTies] : counts[t];
    if (t == HS_DENSIFY_COUNTS - 1) counts[t] = v;
    if (counts_host) __hip_atomic_store(counts_host + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- host ----

int check_plan_args(const hs_rows_args* a) {
    const char* fn = "hs_rows_plan";
    int rc = check_args(fn, a);
    if (rc == HS_OK) rc = check_rows(fn, "P", a->P);
    if (rc != HS_OK) return rc;
    if (a->mode != HS_ROWS_MASK && a->mode != HS_ROWS_KEEP && a->mode != HS_ROWS_DENSIFY) {
        set_error("%s: mode=%d is none of HS_ROWS_MASK / _KEEP / _DENSIFY", fn, a->mode);
        return HS_EINVAL;
    }
    if (a->k < 0 || a->k > a->P) { set_error("%s: k=%lld outside [0, P = %lld]", fn, (long long)a->k, (long long)a->P); return HS_EINVAL; }
    if (a->flags & ~HS_DENSIFY_RAW_SCALES) {
        set_error("%s: flags=%d has bits other than HS_DENSIFY_RAW_SCALES", fn, a->flags);
        return HS_EINVAL;
    }
    if (a->mode == HS_ROWS_DENSIFY && a->tau_split != a->tau_split) { set_error("%s: tau_split is NaN", fn); return HS_EINVAL; }
    if (check_field(fn, a->counts, "counts", 4) || check_aligned(fn, a->counts_host, "counts_host", 4)) return HS_EINVAL;
    if (a->P == 0) return HS_OK;
    const Field common[] = {{a->row_map, "row_map", 4}, {a->workspace, "workspace", 16}};
    if (check_fields(fn, common, 2)) return HS_EINVAL;
    if (a->mode == HS_ROWS_MASK) return check_field(fn, a->mask, "mask", 1, " (read by HS_ROWS_MASK)");
    if (check_field(fn, a->score, "score", 4, " (read by HS_ROWS_KEEP / HS_ROWS_DENSIFY)")) return HS_EINVAL;
    if (a->mode == HS_ROWS_DENSIFY) return check_field(fn, a->scales, "scales", 4, " (read by HS_ROWS_DENSIFY)");
    return HS_OK;
}

// the workspace: codes [P] u8 | uint4 per 256 rows | histograms [kSelBlocks][256] u32 | chunk prefixes [kSelBlocks] u32 | state
struct RowsWs { int64_t codes, blocks, hist, tie_prefix, sel, bytes; };

RowsWs rows_workspace(int64_t P) {
    RowsWs w;
    w.codes = 0;
    w.blocks = align_up(P, 256);
    w.hist = w.blocks + align_up(16 * den_blocks(P), 256);
    w.tie_prefix = w.hist + (int64_t)kSelBlocks * kSelBins * 4;
    w.sel = w.tie_prefix + (int64_t)kSelBlocks * 4;
    w.bytes = w.sel + 256;
    return w;
}

int launch_plan(const hs_rows_args& a, hipStream_t s) {
    const RowsWs w = rows_workspace(a.P);
    char* ws = (char*)a.workspace;
    uint8_t* codes = (uint8_t*)(ws + w.codes);
    uint4* blocks = (uint4*)(ws + w.blocks);
    uint32_t* hist = (uint32_t*)(ws + w.hist);
    uint32_t* tie_prefix = (uint32_t*)(ws + w.tie_prefix);
    uint32_t* sel = (uint32_t*)(ws + w.sel);
    const int64_t nblk = den_blocks(a.P);
    RowsPlan p;
    memset(&p, 0, sizeof(p));
    p.P = a.P; p.k = a.k; p.mode = a.mode;
    p.score = a.score; p.mask = a.mask; p.scales = a.scales; p.tau_split = a.tau_split;
    p.chunk = (nblk + kSelBlocks - 1) / kSelBlocks * kDenRows;
    const int nchunks = p.chunk ? (int)((a.P + p.chunk - 1) / p.chunk) : 0;      // <= kSelBlocks
    const bool scored = a.mode != HS_ROWS_MASK && a.k > 0;                        // (then P > 0)
    if (scored) {
        for (int pass = 0; pass < 4; ++pass) {
            rows_hist_kernel<<<(unsigned)nchunks, kDenRows, 0, s>>>(a.score, a.P, p.chunk, pass, sel, hist);
            HS_LAUNCH_CHECK();
            rows_pick_kernel<<<1, kPickThreads, 0, s>>>(hist, nchunks, pass, (uint32_t)a.k, sel, tie_prefix);
            HS_LAUNCH_CHECK();
        }
    }
    if (nchunks > 0) {
        rows_classify_kernel<<<(unsigned)nchunks, kDenRows, 0, s>>>(p, sel, tie_prefix, codes, blocks);
        HS_LAUNCH_CHECK();
    }
    densify_scan_kernel<<<1, kDenScanThreads, 0, s>>>(blocks, nblk, (uint32_t)a.P, a.counts);
    HS_LAUNCH_CHECK();
    uint32_t* map_host = scored ? nullptr : a.counts_host;
    if (nblk > 0 || map_host) {
        densify_map_kernel<<<(unsigned)(nblk > 0 ? nblk : 1), kDenRows, 0, s>>>(codes, blocks, a.P, a.counts, a.row_map, map_host);
        HS_LAUNCH_CHECK();
    }
    if (scored) {
        rows_ties_kernel<<<1, 64, 0, s>>>(a.counts, sel, a.counts_host);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_rows_workspace_bytes(int64_t P) {
    if (hs::check_rows("hs_rows_workspace_bytes", "P", P)) return HS_EINVAL;
    return hs::rows_workspace(P).bytes;
}

HS_API int hs_rows_plan(const hs_rows_args* a, void* hip_stream) {
    const int rc = hs::check_plan_args(a);
    if (rc != HS_OK) return rc;
    return hs::launch_plan(*a, (hipStream_t)hip_stream);
}

}  // extern "C"
