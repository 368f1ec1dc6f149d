// Densify / prune of the cloud (hs_densify_workspace_bytes, hs_densify_plan, hs_densify_apply; include/hdrsplat.h states the
// contract and the policy, rule by rule).
//
// PLAN, three kernels (the scan and the map live in hs_rowplan.h, which rows.hip includes too):
//   densify_classify_kernel  one row per thread, 256 rows per workgroup: the row's 2-bit code
//                                0 leaves nothing   1 survives   2 survives + one clone   3 goes, two children
//                            as a byte of the workspace, and per workgroup four counts {survivors, clones, kept splits,
//                            split sources} from wave ballots (no atomics)
//   densify_scan_kernel      ONE workgroup turns the block counts into exclusive prefixes in place (each thread a contiguous
//                            run of blocks, a scan of the 1024 run totals in LDS) and writes `counts`.  Block sums -> one small
//                            scan -> apply, as everywhere in this library: 3907 blocks at 1 M rows, no look-back chain
//   densify_map_kernel       one row per thread again: block prefix + rank inside the block (ballots) = the row's place in
//                            its segment; writes row_map[j] = kind << 30 | source for j < P_out, segments in the order
//                            survivors | clones | children k = 0 | children k = 1, each in source order.  Its first thread
//                            leaves a copy of `counts` at the caller's page-locked address
// APPLY, one kernel over every matrix (descriptors by value in the kernel arguments, a prefix table of virtual blocks, grid
// capped at 2048 workgroups, as adam.hip does with its segments).  Output row j gathers source row row_map[j] & (2^30 - 1).
// A matrix runs in one of three shapes:
//   rows4   row_stride a multiple of 4 floats, src and dst 16-byte aligned: a work item is (row, quad): one 16-byte load, one
//           16-byte store (SH coefficients and their moments, rotations: 3/4 of the bytes at SH degree 3)
//   quad    dst 16-byte aligned: a work item is four consecutive floats of dst -- they span up to four source rows (row
//           strides 1 and 3), read with 4-byte loads of exactly those elements, stored with one 16-byte store (the last,
//           partial quad: 4-byte stores)
//   scalar  anything else: one element per work item
// The survivor segment is an increasing map: its reads walk the source arrays monotonically.  Nothing at or beyond row P_out
// of a destination is written.  No atomics, no LDS in the apply; this file is compiled with -ffp-contract=off, and the order
// of operations of a child's mean is the header's.
#include "hs_cloud.h"
#include "hs_rowplan.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

namespace hs {
namespace {

constexpr int kDenThreads = 256;              // apply
constexpr int kDenMaxGrid = 2048;             // 256 CUs x 8 workgroups; larger problems stride
constexpr int kDenMaxMat = HS_DENSIFY_MAX_MATRICES;
constexpr uint32_t kSrcMask = (1u << 30) - 1u;

struct DenPlan {
    int64_t P;
    const float* grad_accum; const float* denom; const int32_t* max_radii; const float* opacities; const float* scales;
    float tau_grad, tau_split, o_min, sigma_max;
    int32_t r_max, sigma_on, raw_scales, pad;
};

__device__ __forceinline__ float child_scale(float x, bool raw) { return raw ? x - HS_DENSIFY_LOG_1_6 : x / 1.6f; }

__global__ void __launch_bounds__(kDenRows) densify_classify_kernel(const DenPlan a, uint8_t* __restrict__ codes,
                                                                    uint4* __restrict__ blocks) {
    __shared__ uint32_t s_cnt[kDenRows / 64][4];
    const int64_t i = (int64_t)blockIdx.x * kDenRows + threadIdx.x;
    uint32_t code = 0;
    bool split = false;
    if (i < a.P) {
        const float dn = a.denom[i];
        float g = a.grad_accum[i] / dn;
        if (dn == 0.f || g != g) g = 0.f;
        const bool sel = g >= a.tau_grad;
        float s = a.scales[3 * i];
        const float s1 = a.scales[3 * i + 1], s2 = a.scales[3 * i + 2];
        if (s1 > s) s = s1;
        if (s2 > s) s = s2;
        split = sel && s > a.tau_split;
        const float st = split ? child_scale(s, a.raw_scales != 0) : s;
        const bool prune = a.opacities[i] < a.o_min || (a.r_max > 0 && a.max_radii[i] > a.r_max) || (a.sigma_on && st > a.sigma_max);
        code = prune ? 0u : (split ? 3u : (sel ? 2u : 1u));
        codes[i] = (uint8_t)code;
    }
    const unsigned long long b_surv = __ballot(code == 1u || code == 2u), b_clone = __ballot(code == 2u);
    const unsigned long long b_kept = __ballot(code == 3u), b_split = __ballot(split);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_cnt[wave][0] = (uint32_t)__popcll(b_surv);
        s_cnt[wave][1] = (uint32_t)__popcll(b_clone);
        s_cnt[wave][2] = (uint32_t)__popcll(b_kept);
        s_cnt[wave][3] = (uint32_t)__popcll(b_split);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint4 c = make_uint4(0u, 0u, 0u, 0u);
        for (int w = 0; w < kDenRows / 64; ++w) { c.x += s_cnt[w][0]; c.y += s_cnt[w][1]; c.z += s_cnt[w][2]; c.w += s_cnt[w][3]; }
        blocks[blockIdx.x] = c;
    }
}

// ---- apply ----

enum { kMatRows4 = 0, kMatQuad = 1, kMatScalar = 2 };

struct DenMat {
    const float* src; float* dst;
    int64_t S;           // floats per row
    int64_t n_floats;    // P_out * S
    int64_t n_items;     // work items: (row, quad) pairs, quads of dst, or elements
    int32_t per_row;     // rows4: quads per row
    int32_t role, mode, small;
};

struct DenLaunch {
    DenMat m[kDenMaxMat];
    uint32_t first_block[kDenMaxMat + 1];   // prefix table of virtual blocks
    int32_t n_mat;
    int32_t raw_scales;
    int64_t P;                              // source rows: a map entry is clamped below it (a P_out that is not the plan's
                                            // would otherwise turn stale map entries into reads outside the sources)
    const uint32_t* row_map;
    const float* scales; const float* rotations; const float* noise;
};

__device__ __forceinline__ int64_t source_row(const DenLaunch& L, uint32_t rm) {
    const int64_t r = (int64_t)(rm & kSrcMask);
    return r < L.P ? r : L.P - 1;
}

// component c of the mean of child k of source row `srow` (the header states this order of operations)
__device__ __forceinline__ float child_mean(const DenLaunch& L, int64_t srow, int k, int c, float mu) {
    const float* q = L.rotations + 4 * srow;
    float w = q[0], x = q[1], y = q[2], z = q[3];
    quat_normalize(w, x, y, z);
    const float* sp = L.scales + 3 * srow;
    const float* xi = L.noise + 6 * srow + 3 * k;
    float s0 = sp[0], s1 = sp[1], s2 = sp[2];
    if (L.raw_scales) { s0 = expf(s0); s1 = expf(s1); s2 = expf(s2); }
    const float v0 = s0 * xi[0], v1 = s1 * xi[1], v2 = s2 * xi[2];
    float r0, r1, r2;
    quat_rot_row(c, w, x, y, z, r0, r1, r2);
    return ((r0 * v0 + r1 * v1) + r2 * v2) + mu;
}

// element (output row with map entry `rm`, column c) of matrix M
__device__ __forceinline__ float den_elem(const DenMat& M, const DenLaunch& L, uint32_t rm, int64_t c) {
    const uint32_t kind = rm >> 30;
    if (M.role == HS_DENSIFY_ZERO_NEW && kind != HS_DENSIFY_KIND_SURVIVOR) return 0.f;
    const int64_t srow = source_row(L, rm);
    const float x = M.src[srow * M.S + c];
    if (kind < HS_DENSIFY_KIND_CHILD0) return x;
    if (M.role == HS_DENSIFY_SCALES) return child_scale(x, L.raw_scales != 0);
    if (M.role == HS_DENSIFY_MEANS) return child_mean(L, srow, (int)(kind - HS_DENSIFY_KIND_CHILD0), (int)c, x);
    return x;
}

__global__ void __launch_bounds__(kDenThreads) densify_apply_kernel(const DenLaunch L) {
    const uint32_t n_blocks = L.first_block[L.n_mat];
    for (uint32_t vb = blockIdx.x; vb < n_blocks; vb += gridDim.x) {
        HS_BLOCK_OWNER(mi, vb, L.first_block, L.n_mat);
        const DenMat& M = L.m[mi];
        const int64_t w = (int64_t)(vb - L.first_block[mi]) * kDenThreads + threadIdx.x;
        if (w >= M.n_items) continue;
        const bool small = M.small != 0;

        if (M.mode == kMatRows4) {          // (COPY / ZERO_NEW only: MEANS and SCALES have rows of 3)
            int64_t j, q;
            divmod(w, M.per_row, small, j, q);
            const uint32_t rm = L.row_map[j];
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (!(M.role == HS_DENSIFY_ZERO_NEW && (rm >> 30) != HS_DENSIFY_KIND_SURVIVOR))
                v = *reinterpret_cast<const f4*>(M.src + source_row(L, rm) * M.S + 4 * q);
            *reinterpret_cast<f4*>(M.dst + j * M.S + 4 * q) = v;
            continue;
        }
        if (M.mode == kMatScalar) {
            int64_t j, c;
            divmod(w, M.S, small, j, c);
            M.dst[w] = den_elem(M, L, L.row_map[j], c);
            continue;
        }
        // four consecutive floats e0 .. e0 + 3 of dst, of up to four output rows
        const int64_t e0 = 4 * w;
        int64_t j, c;
        divmod(e0, M.S, small, j, c);
        uint32_t rm = L.row_map[j];          // (e0 < n_floats: row j exists)
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (e0 + i >= M.n_floats) break;
            v[i] = den_elem(M, L, rm, c);
            if (++c == M.S) {
                c = 0;
                ++j;
                if (e0 + i + 1 < M.n_floats) rm = L.row_map[j];
            }
        }
        if (e0 + 4 <= M.n_floats) {
            const f4 o = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f4*>(M.dst + e0) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e0 + i < M.n_floats) M.dst[e0 + i] = v[i];
        }
    }
}

// ---- host ----

int check_common(const hs_densify_args* a, const char* fn) {
    int rc = check_args(fn, a);
    if (rc == HS_OK) rc = check_rows(fn, "P", a->P);
    if (rc == HS_OK) rc = check_raw_flags(fn, a->flags);
    return rc;
}

int check_plan_args(const hs_densify_args* a) {
    const char* fn = "hs_densify_plan";
    const int rc = check_common(a, fn);
    if (rc != HS_OK) return rc;
    if (a->r_max < 0) { set_error("%s: r_max=%d is negative (0 = off)", fn, a->r_max); return HS_EINVAL; }
    if (a->tau_grad != a->tau_grad) { set_error("%s: tau_grad is NaN", fn); return HS_EINVAL; }
    if (a->tau_split != a->tau_split) { set_error("%s: tau_split is NaN", fn); return HS_EINVAL; }
    if (a->o_min != a->o_min) { set_error("%s: o_min is NaN", fn); return HS_EINVAL; }
    if (a->sigma_max != a->sigma_max) { set_error("%s: sigma_max is NaN (+INFINITY = off)", fn); return HS_EINVAL; }
    if (check_field(fn, a->counts, "counts", 4) || check_aligned(fn, a->counts_host, "counts_host", 4)) return HS_EINVAL;
    if (a->P == 0) return HS_OK;
    const Field in[] = {{a->grad_accum, "grad_accum", 4}, {a->denom, "denom", 4}, {a->max_radii, "max_radii", 4},
                        {a->opacities, "opacities", 4}, {a->scales, "scales", 4}, {a->row_map, "row_map", 4},
                        {a->workspace, "workspace", 16}};
    return check_fields(fn, in, 7);
}

int check_apply_args(const hs_densify_args* a) {
    const char* fn = "hs_densify_apply";
    const int rc = check_common(a, fn);
    if (rc != HS_OK) return rc;
    if (a->P_out < 0 || a->P_out > 2 * a->P) {
        set_error("%s: P_out=%lld outside [0, 2 P = %lld]", fn, (long long)a->P_out, (long long)(2 * a->P));
        return HS_EINVAL;
    }
    if (a->n_matrices < 1 || a->n_matrices > HS_DENSIFY_MAX_MATRICES) {
        set_error("%s: n_matrices=%d outside [1, %d]", fn, a->n_matrices, HS_DENSIFY_MAX_MATRICES);
        return HS_EINVAL;
    }
    if (!a->matrices) { set_error("%s: null matrices", fn); return HS_EINVAL; }
    bool means = false;
    for (int i = 0; i < a->n_matrices; ++i) {
        const hs_densify_matrix& M = a->matrices[i];
        if (M.role < HS_DENSIFY_COPY || M.role > HS_DENSIFY_SCALES) {
            set_error("%s: matrices[%d].role=%d is none of HS_DENSIFY_COPY / _ZERO_NEW / _MEANS / _SCALES", fn, i, M.role);
            return HS_EINVAL;
        }
        if (M.row_stride < 1) { set_error("%s: matrices[%d].row_stride=%lld (need >= 1)", fn, i, (long long)M.row_stride); return HS_EINVAL; }
        if ((M.role == HS_DENSIFY_MEANS || M.role == HS_DENSIFY_SCALES) && M.row_stride != 3) {
            set_error("%s: matrices[%d].row_stride=%lld: the MEANS and SCALES roles take rows of 3", fn, i, (long long)M.row_stride);
            return HS_EINVAL;
        }
        if (a->P_out > 0 && M.row_stride >= kMaxFloats / a->P_out) {
            set_error("%s: matrices[%d]: P_out * row_stride = %lld * %lld reaches 2^40", fn, i, (long long)a->P_out, (long long)M.row_stride);
            return HS_EINVAL;
        }
        means = means || M.role == HS_DENSIFY_MEANS;
        if (a->P_out == 0) continue;
        if (!M.src || !M.dst) { set_error("%s: matrices[%d]: null src/dst", fn, i); return HS_EINVAL; }
        if (!aligned_to(M.src, 4) || !aligned_to(M.dst, 4)) { set_error("%s: matrices[%d]: src/dst must be 4-byte aligned", fn, i); return HS_EINVAL; }
        if (M.src == M.dst) { set_error("%s: matrices[%d]: dst must not be src (the gather is not in place)", fn, i); return HS_EINVAL; }
    }
    if (a->P_out == 0) return HS_OK;
    if (check_field(fn, a->row_map, "row_map", 4)) return HS_EINVAL;
    if (!means) return HS_OK;
    const Field in[] = {{a->scales, "scales", 4}, {a->rotations, "rotations", 4}, {a->noise, "noise", 4}};
    return check_fields(fn, in, 3, " (read by the HS_DENSIFY_MEANS role)");
}

int launch_plan(const hs_densify_args& a, hipStream_t s) {
    DenPlan p;
    memset(&p, 0, sizeof(p));
    p.P = a.P;
    p.grad_accum = a.grad_accum; p.denom = a.denom; p.max_radii = a.max_radii; p.opacities = a.opacities; p.scales = a.scales;
    p.tau_grad = a.tau_grad; p.tau_split = a.tau_split; p.o_min = a.o_min; p.sigma_max = a.sigma_max;
    p.r_max = a.r_max;
    p.raw_scales = (a.flags & HS_DENSIFY_RAW_SCALES) ? 1 : 0;
    p.sigma_on = (a.sigma_max == INFINITY || (!p.raw_scales && a.sigma_max == 0.f)) ? 0 : 1;
    const int64_t nblk = den_blocks(a.P);
    uint8_t* codes = (uint8_t*)a.workspace;
    uint4* blocks = (uint4*)((char*)a.workspace + align_up(a.P, 256));
    if (nblk > 0) {
        densify_classify_kernel<<<(unsigned)nblk, kDenRows, 0, s>>>(p, codes, blocks);
        HS_LAUNCH_CHECK();
    }
    densify_scan_kernel<<<1, kDenScanThreads, 0, s>>>(blocks, nblk, (uint32_t)a.P, a.counts);
    HS_LAUNCH_CHECK();
    if (nblk > 0 || a.counts_host) {
        densify_map_kernel<<<(unsigned)(nblk > 0 ? nblk : 1), kDenRows, 0, s>>>(codes, blocks, a.P, a.counts, a.row_map, a.counts_host);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

int launch_apply(const hs_densify_args& a, hipStream_t s) {
    if (a.P_out == 0) return HS_OK;
    DenLaunch L;
    memset(&L, 0, sizeof(L));
    L.row_map = a.row_map;
    L.P = a.P;
    L.scales = a.scales; L.rotations = a.rotations; L.noise = a.noise;
    L.raw_scales = (a.flags & HS_DENSIFY_RAW_SCALES) ? 1 : 0;
    L.n_mat = a.n_matrices;
    uint64_t blocks = 0;
    for (int i = 0; i < a.n_matrices; ++i) {
        const hs_densify_matrix& G = a.matrices[i];
        DenMat& M = L.m[i];
        M.src = G.src; M.dst = G.dst; M.S = G.row_stride; M.role = G.role;
        M.n_floats = a.P_out * G.row_stride;
        M.small = (M.n_floats < (1ll << 32) && a.P * G.row_stride < (1ll << 32)) ? 1 : 0;
        const bool plain = G.role == HS_DENSIFY_COPY || G.role == HS_DENSIFY_ZERO_NEW;
        if (plain && G.row_stride % 4 == 0 && G.row_stride / 4 <= INT32_MAX && aligned_to(G.src, 16) && aligned_to(G.dst, 16)) {
            M.mode = kMatRows4;
            M.per_row = (int32_t)(G.row_stride / 4);
            M.n_items = a.P_out * M.per_row;
        } else if (aligned_to(G.dst, 16)) {
            M.mode = kMatQuad;
            M.n_items = (M.n_floats + 3) / 4;
        } else {
            M.mode = kMatScalar;
            M.n_items = M.n_floats;
        }
        L.first_block[i] = (uint32_t)blocks;
        blocks += (uint64_t)((M.n_items + kDenThreads - 1) / kDenThreads);
        if (blocks >= (1ull << 31)) { set_error("hs_densify_apply: more than 2^31 blocks of work"); return HS_EINVAL; }
    }
    for (int i = a.n_matrices; i <= kDenMaxMat; ++i) L.first_block[i] = (uint32_t)blocks;
    const unsigned grid = (unsigned)(blocks < (uint64_t)kDenMaxGrid ? blocks : (uint64_t)kDenMaxGrid);
    densify_apply_kernel<<<grid, kDenThreads, 0, s>>>(L);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_densify_workspace_bytes(int64_t P) {
    if (hs::check_rows("hs_densify_workspace_bytes", "P", P)) return HS_EINVAL;
    return hs::align_up(P, 256) + 16 * hs::den_blocks(P);
}

HS_API int hs_densify_plan(const hs_densify_args* a, void* hip_stream) {
    const int rc = hs::check_plan_args(a);
    if (rc != HS_OK) return rc;
    return hs::launch_plan(*a, (hipStream_t)hip_stream);
}

HS_API int hs_densify_apply(const hs_densify_args* a, void* hip_stream) {
    const int rc = hs::check_apply_args(a);
    if (rc != HS_OK) return rc;
    return hs::launch_apply(*a, (hipStream_t)hip_stream);
}

}  // extern "C"
