// Fused, optionally visibility-masked Adam step (hs_adam_state_bytes, hs_adam_step; include/hdrsplat.h states the contract).
//
// Two kernels per call, nothing else:
//
//   adam_tick_kernel    one workgroup: advances the device-resident state -- the step count t, per group the running
//                       products B1 = beta1^t, B2 = beta2^t in fp64 -- and derives per group, from the hyper-parameter
//                       table {lr, beta1, beta2, eps} the caller keeps on the device,
//                           step_size = (float)(lr / (1 - B1)),  bc2 = (float)sqrt(1 - B2),
//                       b1 = (float)beta1, b2 = (float)beta2, c1 = (float)(1 - beta1), c2 = (float)(1 - beta2), e = (float)eps
//                       (1 - beta is formed in fp64 and rounded ONCE: 1.0f - (float)0.999 is 4.7e-5 off 0.001 in relative
//                       terms, an error that goes straight into v and tripled the RMS distance to fp64 Adam).
//   adam_update_kernel  one launch over every group.  Per element, fp32, IEEE + - x / sqrt, no contraction (this file is
//                       compiled with -ffp-contract=off), denormals kept, in exactly this order:
//                           m' = b1 * m + c1 * g
//                           v' = b2 * v + (c2 * g) * g
//                           d  = sqrtf(v') / bc2 + e
//                           p' = p - step_size * (m' / d)
//
// The update is a stream: 28 bytes per element (read p, g, m, v; write p, m, v), each touched once.  A work item is a QUAD,
// four consecutive floats at a 16-byte aligned address of param / exp_avg / exp_avg_sq: one 16-byte load per array, one
// 16-byte store (the moments leave non-temporally: nothing reads them again before the next step).  The gradient is often a
// view into a flat buffer and only 4-byte aligned: its quad is then four 4-byte loads (neighbouring lanes still cover one
// contiguous span).  A quad that is only partly inside its group's column range, or partly visible, falls back to 4-byte
// accesses of exactly the elements it owns -- no byte outside a group's elements is ever read or written.
//
// A group becomes a SEGMENT of the grid, in one of three shapes:
//   flat    full rows (col_begin = 0, col_count = row_stride): the matrix is one run of rows * row_stride floats
//   rows    row_stride a multiple of 4: quads never straddle a row; a work item is (row, quad of the column range).  Two
//           groups over the same arrays with adjacent column ranges -- SH coefficients split into DC and the rest, each with
//           its learning rate -- are MERGED into one segment whose elements choose their hyper-parameters by column: the
//           rows stream through once, fully coalesced, instead of once per group at a 3-of-48 stride
//   scalar  anything else (unaligned param / moments, a column range of rows that are no multiple of 4 floats): one
//           element per work item
// Segment descriptors travel by value in the kernel arguments; a workgroup takes virtual blocks of 256 work items, finds the
// segment of each from a prefix table, and strides over them (the grid is capped at 2048 workgroups).
//
// Visibility: in a masked segment the row's mask entry is read FIRST; rows that are not visible are not loaded, not stored.
#include "hs_cloud.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

#ifndef HS_TUNE_ADAM_NT
#define HS_TUNE_ADAM_NT 1     // A/B switch: non-temporal stores of the moments
#endif

namespace hs {
namespace {

constexpr int kAdamThreads = 256;
constexpr int kAdamMaxGrid = 2048;           // 256 CUs x 8 workgroups; larger problems stride
constexpr int kAdamMaxSeg = HS_ADAM_MAX_GROUPS;

struct AdamHyp {            // what the tick derives for one group (the tail of its 64-byte state slot)
    float step_size, bc2, b1, b2, omb1, omb2, eps, pad;
};
struct AdamGroupState {
    double B1, B2;
    AdamHyp h;
    double pad[2];
};
struct AdamState {
    unsigned long long t;
    unsigned long long pad[7];
    AdamGroupState grp[kAdamMaxSeg];
};
static_assert(sizeof(AdamGroupState) == 64 && offsetof(AdamState, grp) == 64, "the state layout is part of the C ABI");

enum { kSegFlat = 0, kSegRows = 1, kSegScalar = 2 };

struct AdamSeg {
    float* p; const float* g; float* m; float* v;
    int64_t n_items;     // work items: quads (flat, rows) or elements (scalar)
    int64_t row_len;     // floats from one row to the next (rows, scalar); flat: the run's length
    int64_t lo, hi;      // the elements a quad may touch: columns [lo, hi) of its row (flat: [0, n) of the run)
    int64_t split;       // columns >= split take hyp_b (merged column groups); else == hi
    int32_t per_row;     // rows: quads per row;  scalar: columns per row
    int32_t first;       // rows: first quad of the column range;  scalar: first column
    int32_t mask_div;    // flat, masked: floats per mask row
    int32_t mode, masked, g_vec, small, hyp_a, hyp_b, pad;
};

struct AdamLaunch {
    AdamSeg seg[kAdamMaxSeg];
    uint32_t first_block[kAdamMaxSeg + 1];   // prefix table of virtual blocks
    int32_t n_seg;
    int32_t mask_kind;
    const void* mask;
};

__global__ void __launch_bounds__(64) adam_tick_kernel(AdamState* __restrict__ st, const double* __restrict__ hyper, int n) {
    const int g = threadIdx.x;
    const unsigned long long t = st->t;
    __syncthreads();                      // (every thread has read t before it moves)
    if (g == 0) st->t = t + 1;
    if (g < n) {
        const double lr = hyper[4 * g + 0], beta1 = hyper[4 * g + 1], beta2 = hyper[4 * g + 2], eps = hyper[4 * g + 3];
        AdamGroupState& s = st->grp[g];
        // running products, not pow: a CPU restatement reproduces them bit for bit.  All-zero bytes are t = 0: product 1.
        const double B1 = (t == 0 ? 1.0 : s.B1) * beta1;
        const double B2 = (t == 0 ? 1.0 : s.B2) * beta2;
        s.B1 = B1;
        s.B2 = B2;
        AdamHyp h;
        h.step_size = (float)(lr / (1.0 - B1));
        h.bc2 = (float)sqrt(1.0 - B2);
        h.b1 = (float)beta1;
        h.b2 = (float)beta2;
        h.omb1 = (float)(1.0 - beta1);
        h.omb2 = (float)(1.0 - beta2);
        h.eps = (float)eps;
        h.pad = 0.f;
        s.h = h;
    }
}

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamHyp& h) {
    m = h.b1 * m + h.omb1 * g;
    v = h.b2 * v + (h.omb2 * g) * g;
    const float d = sqrtf(v) / h.bc2 + h.eps;
    p = p - h.step_size * (m / d);
}

__device__ __forceinline__ AdamHyp pick(const AdamHyp& a, const AdamHyp& b, bool second) {
    AdamHyp h;
    h.step_size = second ? b.step_size : a.step_size;
    h.bc2 = second ? b.bc2 : a.bc2;
    h.b1 = second ? b.b1 : a.b1;
    h.b2 = second ? b.b2 : a.b2;
    h.omb1 = second ? b.omb1 : a.omb1;
    h.omb2 = second ? b.omb2 : a.omb2;
    h.eps = second ? b.eps : a.eps;
    h.pad = 0.f;
    return h;
}

__device__ __forceinline__ bool row_visible(const void* mask, int kind, int64_t row) {
    if (kind == HS_ADAM_MASK_RADII) return reinterpret_cast<const int32_t*>(mask)[row] > 0;
    return reinterpret_cast<const uint8_t*>(mask)[row] != 0;
}

__device__ __forceinline__ void store_moment(f4* dst, f4 val) {
#if HS_TUNE_ADAM_NT
    __builtin_nontemporal_store(val, dst);
#else
    *dst = val;
#endif
}

__global__ void __launch_bounds__(kAdamThreads) adam_update_kernel(const AdamLaunch L, const AdamState* __restrict__ st) {
    const uint32_t n_blocks = L.first_block[L.n_seg];
    for (uint32_t vb = blockIdx.x; vb < n_blocks; vb += gridDim.x) {
        HS_BLOCK_OWNER(si, vb, L.first_block, L.n_seg);
        const AdamSeg& S = L.seg[si];
        const int64_t w = (int64_t)(vb - L.first_block[si]) * kAdamThreads + threadIdx.x;
        if (w >= S.n_items) continue;
        const AdamHyp ha = st->grp[S.hyp_a].h, hb = st->grp[S.hyp_b].h;
        const bool masked = S.masked != 0;

        if (S.mode == kSegScalar) {
            int64_t row, c;
            divmod(w, S.per_row, S.small != 0, row, c);
            c += S.first;
            if (masked && !row_visible(L.mask, L.mask_kind, row)) continue;
            const int64_t e = row * S.row_len + c;
            float p = S.p[e], m = S.m[e], v = S.v[e];
            adam_elem(p, S.g[e], m, v, pick(ha, hb, c >= S.split));
            S.p[e] = p; S.m[e] = m; S.v[e] = v;
            continue;
        }

        // a quad: floats e0 .. e0 + 3 of the arrays, columns c0 .. c0 + 3 of the row (flat: of the run)
        int64_t row = 0, q = w;
        if (S.mode == kSegRows) divmod(w, S.per_row, S.small != 0, row, q);
        const int64_t c0 = 4 * (S.first + q);
        const int64_t e0 = row * S.row_len + c0;
        bool ok[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) ok[i] = c0 + i >= S.lo && c0 + i < S.hi;
        if (masked) {
            if (S.mode == kSegRows) {
                const bool vis = row_visible(L.mask, L.mask_kind, row);
#pragma unroll
                for (int i = 0; i < 4; ++i) ok[i] = ok[i] && vis;
            } else {
                int64_t mrow, rem;
                divmod(e0, S.mask_div, S.small != 0, mrow, rem);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (ok[i]) ok[i] = row_visible(L.mask, L.mask_kind, mrow);     // (ok[i]: the row exists)
                    if (++rem == S.mask_div) { rem = 0; ++mrow; }
                }
            }
        }
        const bool all = ok[0] && ok[1] && ok[2] && ok[3];
        if (all) {
            f4 p = *reinterpret_cast<const f4*>(S.p + e0);
            f4 m = *reinterpret_cast<const f4*>(S.m + e0);
            f4 v = *reinterpret_cast<const f4*>(S.v + e0);
            f4 g;
            if (S.g_vec) {
                g = *reinterpret_cast<const f4*>(S.g + e0);
            } else {
                g.x = S.g[e0]; g.y = S.g[e0 + 1]; g.z = S.g[e0 + 2]; g.w = S.g[e0 + 3];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float pi = p[i], mi = m[i], vi = v[i];
                adam_elem(pi, g[i], mi, vi, pick(ha, hb, c0 + i >= S.split));
                p[i] = pi; m[i] = mi; v[i] = vi;
            }
            *reinterpret_cast<f4*>(S.p + e0) = p;
            store_moment(reinterpret_cast<f4*>(S.m + e0), m);
            store_moment(reinterpret_cast<f4*>(S.v + e0), v);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!ok[i]) continue;
                const int64_t e = e0 + i;
                float p = S.p[e], m = S.m[e], v = S.v[e];
                adam_elem(p, S.g[e], m, v, pick(ha, hb, c0 + i >= S.split));
                S.p[e] = p; S.m[e] = m; S.v[e] = v;
            }
        }
    }
}

// the segment of one group (`masked`: the mask applies)
AdamSeg make_segment(const hs_adam_group& G, int hyp, bool masked) {
    AdamSeg s;
    memset(&s, 0, sizeof(s));
    s.p = G.param; s.g = G.grad; s.m = G.exp_avg; s.v = G.exp_avg_sq;
    s.hyp_a = s.hyp_b = hyp;
    s.masked = masked ? 1 : 0;
    const int64_t S = G.row_stride, n = G.rows * S;
    const bool vec = aligned_to(G.param, 16) && aligned_to(G.exp_avg, 16) && aligned_to(G.exp_avg_sq, 16);
    const bool full = G.col_begin == 0 && G.col_count == S;
    s.small = n < (1ll << 32) ? 1 : 0;
    s.g_vec = aligned_to(G.grad, 16) ? 1 : 0;
    if (vec && full && (!masked || S % 4 != 0)) {
        s.mode = kSegFlat;
        s.row_len = n;
        s.lo = 0; s.hi = n; s.split = n;
        s.n_items = (n + 3) / 4;
        s.mask_div = (int32_t)(masked ? S : 1);
    } else if (vec && S % 4 == 0 && S / 4 <= INT32_MAX) {
        s.mode = kSegRows;
        s.row_len = S;
        s.lo = G.col_begin; s.hi = G.col_begin + G.col_count; s.split = s.hi;
        s.first = (int32_t)(G.col_begin / 4);
        s.per_row = (int32_t)((s.hi + 3) / 4 - s.first);
        s.n_items = G.rows * s.per_row;
    } else {
        s.mode = kSegScalar;
        s.row_len = S;
        s.lo = G.col_begin; s.hi = G.col_begin + G.col_count; s.split = s.hi;
        s.first = (int32_t)G.col_begin;
        s.per_row = (int32_t)G.col_count;
        s.n_items = G.rows * G.col_count;
        s.g_vec = 0;
    }
    return s;
}

// two segments over the same arrays and rows whose column ranges touch: one segment, hyper-parameters chosen by column
bool merge_columns(AdamSeg& a, const AdamSeg& b) {
    if (a.mode != kSegRows || b.mode != kSegRows || a.hyp_a != a.hyp_b || b.hyp_a != b.hyp_b) return false;
    if (a.p != b.p || a.g != b.g || a.m != b.m || a.v != b.v || a.row_len != b.row_len || a.masked != b.masked) return false;
    const int64_t rows_a = a.n_items / a.per_row, rows_b = b.n_items / b.per_row;
    if (rows_a != rows_b) return false;
    const AdamSeg& left = a.lo <= b.lo ? a : b;
    const AdamSeg& right = a.lo <= b.lo ? b : a;
    if (left.hi != right.lo) return false;
    AdamSeg s = left;
    s.hi = right.hi;
    s.split = right.lo;
    s.hyp_b = right.hyp_a;
    s.per_row = (int32_t)((s.hi + 3) / 4 - s.first);
    s.n_items = rows_a * s.per_row;
    a = s;
    return true;
}

int check_adam_args(const hs_adam_args* a) {
    if (check_args("hs_adam_step", a)) return HS_EINVAL;
    if (a->n_groups < 1 || a->n_groups > HS_ADAM_MAX_GROUPS) {
        set_error("hs_adam_step: n_groups=%d outside [1, %d]", a->n_groups, HS_ADAM_MAX_GROUPS);
        return HS_EINVAL;
    }
    if (!a->groups) { set_error("hs_adam_step: null groups"); return HS_EINVAL; }
    if (!a->state) { set_error("hs_adam_step: null state"); return HS_EINVAL; }
    if (!a->hyper) { set_error("hs_adam_step: null hyper"); return HS_EINVAL; }
    if (!aligned_to(a->state, 16)) { set_error("hs_adam_step: state must be 16-byte aligned"); return HS_EINVAL; }
    if (!aligned_to(a->hyper, 8)) { set_error("hs_adam_step: hyper must be 8-byte aligned"); return HS_EINVAL; }
    if (a->mask_kind != HS_ADAM_MASK_NONE && a->mask_kind != HS_ADAM_MASK_RADII && a->mask_kind != HS_ADAM_MASK_BYTES) {
        set_error("hs_adam_step: mask_kind=%d is none of HS_ADAM_MASK_NONE / _RADII / _BYTES", a->mask_kind);
        return HS_EINVAL;
    }
    if (a->mask_len < 0) { set_error("hs_adam_step: mask_len=%lld is negative", (long long)a->mask_len); return HS_EINVAL; }
    if (a->mask_kind != HS_ADAM_MASK_NONE && !a->mask && a->mask_len > 0) { set_error("hs_adam_step: null mask"); return HS_EINVAL; }
    if (a->mask_kind == HS_ADAM_MASK_RADII && !aligned_to(a->mask, 4)) {
        set_error("hs_adam_step: mask (int32 radii) must be 4-byte aligned");
        return HS_EINVAL;
    }
    for (int i = 0; i < a->n_groups; ++i) {
        const hs_adam_group& G = a->groups[i];
        if (G.rows < 0) { set_error("hs_adam_step: groups[%d].rows=%lld is negative", i, (long long)G.rows); return HS_EINVAL; }
        if (G.row_stride < 1 || G.col_begin < 0 || G.col_count < 1) {
            set_error("hs_adam_step: groups[%d]: row_stride=%lld col_begin=%lld col_count=%lld (need row_stride >= 1, col_begin >= 0, "
                      "col_count >= 1)", i, (long long)G.row_stride, (long long)G.col_begin, (long long)G.col_count);
            return HS_EINVAL;
        }
        if (G.col_begin > G.row_stride || G.col_count > G.row_stride - G.col_begin) {
            set_error("hs_adam_step: groups[%d]: col_begin + col_count > row_stride (%lld + %lld > %lld)", i, (long long)G.col_begin,
                      (long long)G.col_count, (long long)G.row_stride);
            return HS_EINVAL;
        }
        if (G.rows > 0 && G.row_stride > kMaxFloats / G.rows) {
            set_error("hs_adam_step: groups[%d]: rows * row_stride = %lld * %lld exceeds 2^40", i, (long long)G.rows, (long long)G.row_stride);
            return HS_EINVAL;
        }
        if (G.rows == 0) continue;
        if (G.masked && a->mask_kind != HS_ADAM_MASK_NONE && G.rows != a->mask_len) {
            set_error("hs_adam_step: groups[%d].rows=%lld differs from mask_len=%lld (a masked group has one mask entry per row)", i,
                      (long long)G.rows, (long long)a->mask_len);
            return HS_EINVAL;
        }
        if (!G.param || !G.grad || !G.exp_avg || !G.exp_avg_sq) {
            set_error("hs_adam_step: groups[%d]: null param/grad/exp_avg/exp_avg_sq", i);
            return HS_EINVAL;
        }
        if (!aligned_to(G.param, 4) || !aligned_to(G.grad, 4) || !aligned_to(G.exp_avg, 4) || !aligned_to(G.exp_avg_sq, 4)) {
            set_error("hs_adam_step: groups[%d]: param/grad/exp_avg/exp_avg_sq must be 4-byte aligned", i);
            return HS_EINVAL;
        }
    }
    return HS_OK;
}

int launch_adam(const hs_adam_args& a, hipStream_t s) {
    AdamLaunch L;
    memset(&L, 0, sizeof(L));
    L.mask = a.mask;
    L.mask_kind = a.mask_kind;
    int n = 0;
    for (int i = 0; i < a.n_groups; ++i) {
        const hs_adam_group& G = a.groups[i];
        if (G.rows == 0) continue;
        AdamSeg seg = make_segment(G, i, G.masked && a.mask_kind != HS_ADAM_MASK_NONE);
        bool merged = false;
        for (int k = 0; k < n && !merged; ++k) merged = merge_columns(L.seg[k], seg);
        if (!merged) L.seg[n++] = seg;
    }
    L.n_seg = n;
    uint64_t blocks = 0;
    for (int k = 0; k < n; ++k) {
        L.first_block[k] = (uint32_t)blocks;
        blocks += (uint64_t)((L.seg[k].n_items + kAdamThreads - 1) / kAdamThreads);
        if (blocks >= (1ull << 31)) { set_error("hs_adam_step: more than 2^31 blocks of work"); return HS_EINVAL; }
    }
    for (int k = n; k <= kAdamMaxSeg; ++k) L.first_block[k] = (uint32_t)blocks;
    adam_tick_kernel<<<1, 64, 0, s>>>((AdamState*)a.state, a.hyper, a.n_groups);
    HS_LAUNCH_CHECK();
    if (blocks == 0) return HS_OK;
    const unsigned grid = (unsigned)(blocks < (uint64_t)kAdamMaxGrid ? blocks : (uint64_t)kAdamMaxGrid);
    adam_update_kernel<<<grid, kAdamThreads, 0, s>>>(L, (const AdamState*)a.state);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_adam_state_bytes(int32_t n_groups) {
    if (n_groups < 1 || n_groups > HS_ADAM_MAX_GROUPS) {
        hs::set_error("hs_adam_state_bytes: n_groups=%d outside [1, %d]", n_groups, HS_ADAM_MAX_GROUPS);
        return HS_EINVAL;
    }
    return 64 + 64 * (int64_t)n_groups;
}

HS_API int hs_adam_step(const hs_adam_args* a, void* hip_stream) {
    const int rc = hs::check_adam_args(a);
    if (rc != HS_OK) return rc;
    return hs::launch_adam(*a, (hipStream_t)hip_stream);
}

}  // extern "C"
