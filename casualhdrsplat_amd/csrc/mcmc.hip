// MCMC refinement of the cloud (hs_mcmc_workspace_bytes, hs_mcmc_sample, hs_mcmc_update, hs_mcmc_noise; include/hdrsplat.h
// states the contract rule by rule): relocation of dead rows onto live ones, growth by clones of drawn rows, and the
// per-step position noise.  The kernels hold no random-number generator: every random input is a caller-drawn tensor.
//
// SAMPLE, three kernels (four with a host copy of the counts):
//   mcmc_weight_kernel   one row per thread, 256 rows per workgroup: the dead flag, the integer weight (fp64 exp, rint), the
//                        inclusive prefix of the weights INSIDE the block (u64, a scan in LDS), cnt[i] = 0, and per block
//                        {sum of weights, dead rows}
//   mcmc_scan_kernel     ONE workgroup turns the block records into exclusive prefixes in place (densify_scan_kernel's
//                        shape: block sums -> one small scan -> apply, no look-back chain), leaves {S, dead rows} in the
//                        record behind the last block and writes `counts`
//   mcmc_draw_kernel     one draw per thread: t = mulhi64(u, S); the block is the last whose exclusive prefix is <= t, the
//                        row the first of that block whose inner prefix exceeds t minus it (two binary searches: the
//                        global prefix C_i = block prefix + inner prefix is never materialised).  cnt[src] += 1 is an integer
//                        atomic (order-free), and the first draw of a source counts it in counts[3].  Growth also writes
//                        row_map: survivors, then one HS_DENSIFY_KIND_CLONE entry per draw
//   mcmc_counts_kernel   the copy of `counts` at the caller's page-locked address
// UPDATE, two kernels:
//   mcmc_source_kernel   one row per thread: rows with cnt >= 1 get the corrected opacity and scales (fp64, rounded once)
//   mcmc_rows_kernel     relocation only, one row per thread and the WAVE working together on every affected row of its 64
//                        (ballot, then the lanes stride over the row's floats): a dead row becomes a copy of its source in
//                        the parameter matrices, the moments of a source row become zeros.  Sources are never dead, and
//                        their parameters were written by the launch before: the copies read what no thread here writes
// NOISE, one kernel: one row per thread, a 16-byte load of the quaternion where the address allows, no atomics, no LDS.
// This file is compiled with -ffp-contract=off; the order of operations of the noise is the header's.
#include "hs_cloud.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

namespace hs {
namespace {

constexpr int kMcRows = 256;                  // rows per workgroup (= threads)
constexpr int kMcScanThreads = 1024;
constexpr int kMcMaxMat = HS_DENSIFY_MAX_MATRICES;
constexpr int kMcMaxRatio = 51;

struct McBlock { unsigned long long sum; uint32_t dead; uint32_t pad; };   // 16 bytes per block of 256 rows
static_assert(sizeof(McBlock) == 16, "the workspace formula counts 16 bytes per block record");

struct McWs { int64_t prefix, blocks, cnt, sources, bytes; };
inline int64_t mc_blocks(int64_t P) { return (P + kMcRows - 1) / kMcRows; }
inline McWs mc_carve(int64_t P, int64_t n_draws) {
    McWs w;
    int64_t o = 0;
    w.prefix = o;  o += align_up(8 * P, 256);
    w.blocks = o;  o += align_up(16 * (mc_blocks(P) + 1), 256);
    w.cnt = o;     o += align_up(4 * P, 256);
    w.sources = o; o += align_up(4 * n_draws, 256);
    w.bytes = o;
    return w;
}

// ---- sample ----

__global__ void __launch_bounds__(kMcRows) mcmc_weight_kernel(const float* __restrict__ opacities, int64_t P, float o_min, int raw,
                                                              int relocate, unsigned long long* __restrict__ prefix,
                                                              uint32_t* __restrict__ cnt, McBlock* __restrict__ blocks) {
    __shared__ unsigned long long s_w[kMcRows];
    __shared__ uint32_t s_dead[kMcRows / 64];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kMcRows + t;
    unsigned long long w = 0;
    bool dead = false;
    if (i < P) {
        const float o = opacities[i];
        dead = !(o > o_min);
        if (o == o && !(relocate && dead)) {
            const double x = (double)o;
            const double s = raw ? 1.0 / (1.0 + exp(-x)) : fmin(fmax(x, 0.0), 1.0);
            w = (unsigned long long)rint(16777216.0 * s);
        }
        cnt[i] = 0u;
    }
    const unsigned long long b_dead = __ballot(dead);
    if ((t & 63) == 0) s_dead[t >> 6] = (uint32_t)__popcll(b_dead);
    s_w[t] = w;
    __syncthreads();
    for (int off = 1; off < kMcRows; off <<= 1) {
        const unsigned long long v = t >= off ? s_w[t - off] : 0ull;
        __syncthreads();
        s_w[t] += v;
        __syncthreads();
    }
    if (i < P) prefix[i] = s_w[t];
    if (t == kMcRows - 1) {
        McBlock b;
        b.sum = s_w[t];
        b.dead = 0u;
        for (int k = 0; k < kMcRows / 64; ++k) b.dead += s_dead[k];
        b.pad = 0u;
        blocks[blockIdx.x] = b;
    }
}

__global__ void __launch_bounds__(kMcScanThreads) mcmc_scan_kernel(McBlock* __restrict__ blocks, int64_t nblk, uint32_t P,
                                                                    uint32_t n_draws, int relocate, uint32_t* __restrict__ counts) {
    __shared__ unsigned long long s_sum[kMcScanThreads];
    __shared__ uint32_t s_dead[kMcScanThreads];
    const int t = threadIdx.x;
    const int64_t per = (nblk + kMcScanThreads - 1) / kMcScanThreads;
    const int64_t b0 = t * per < nblk ? t * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
    unsigned long long acc = 0;
    uint32_t dead = 0;
    for (int64_t b = b0; b < b1; ++b) { acc += blocks[b].sum; dead += blocks[b].dead; }
    s_sum[t] = acc;
    s_dead[t] = dead;
    __syncthreads();
    for (int off = 1; off < kMcScanThreads; off <<= 1) {
        const unsigned long long v = t >= off ? s_sum[t - off] : 0ull;
        const uint32_t d = t >= off ? s_dead[t - off] : 0u;
        __syncthreads();
        s_sum[t] += v;
        s_dead[t] += d;
        __syncthreads();
    }
    unsigned long long run = t ? s_sum[t - 1] : 0ull;
    for (int64_t b = b0; b < b1; ++b) {
        const unsigned long long c = blocks[b].sum;
        blocks[b].sum = run;
        run += c;
    }
    if (t == kMcScanThreads - 1) {
        const unsigned long long S = s_sum[t];
        const uint32_t n_dead = s_dead[t];
        McBlock tot;
        tot.sum = S; tot.dead = n_dead; tot.pad = 0u;
        blocks[nblk] = tot;
        counts[0] = P;
        counts[1] = n_dead;
        counts[2] = S == 0ull ? 0u : (relocate ? n_dead : n_draws);
        counts[3] = 0u;                       // sources: counted by the draws
        counts[4] = S == 0ull ? 1u : 0u;
        counts[5] = 0u; counts[6] = 0u; counts[7] = 0u;
    }
}

struct McDraw {
    int64_t P, n_draws, nblk;
    const float* opacities; const unsigned long long* u;
    const unsigned long long* prefix; const McBlock* blocks;
    uint32_t* cnt; int32_t* sources; uint32_t* row_map; uint32_t* counts;
    float o_min; int32_t relocate;
};

// first row whose global inclusive prefix exceeds t (t < S: it exists, and its weight is not zero)
__device__ __forceinline__ int64_t mc_find(const McDraw& a, unsigned long long t) {
    int64_t lo = 0, hi = a.nblk - 1;          // last block whose exclusive prefix is <= t (block 0's is 0)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.blocks[mid].sum <= t) lo = mid; else hi = mid - 1;
    }
    const unsigned long long tt = t - a.blocks[lo].sum;
    const int64_t base = lo * kMcRows;
    const int64_t n = a.P - base < kMcRows ? a.P - base : kMcRows;
    int64_t l = 0, h = n - 1;                 // first row of the block whose inner prefix exceeds tt
    while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if (a.prefix[base + mid] > tt) h = mid; else l = mid + 1;
    }
    return base + l;
}

__global__ void __launch_bounds__(kMcRows) mcmc_draw_kernel(const McDraw a) {
    const int64_t j = (int64_t)blockIdx.x * kMcRows + threadIdx.x;
    const unsigned long long S = a.blocks[a.nblk].sum;
    int64_t k = -1;                           // this thread's draw
    if (a.relocate) {
        if (j >= a.P) return;
        if (!(a.opacities[j] > a.o_min)) k = j;
        else a.sources[j] = -1;
    } else {
        if (j >= a.P + a.n_draws) return;
        if (j < a.P) a.row_map[j] = ((uint32_t)HS_DENSIFY_KIND_SURVIVOR << 30) | (uint32_t)j;
        else k = j - a.P;
    }
    if (k < 0) return;
    if (S == 0ull) {                          // no draw is made; growth's new rows still name a source inside the cloud
        a.sources[k] = -1;
        if (!a.relocate) a.row_map[j] = ((uint32_t)HS_DENSIFY_KIND_CLONE << 30) | (uint32_t)(k % a.P);
        return;
    }
    const int64_t src = mc_find(a, __umul64hi(a.u[k], S));
    a.sources[k] = (int32_t)src;
    if (!a.relocate) a.row_map[j] = ((uint32_t)HS_DENSIFY_KIND_CLONE << 30) | (uint32_t)src;
    if (atomicAdd(a.cnt + src, 1u) == 0u) atomicAdd(a.counts + 3, 1u);
}

__global__ void mcmc_counts_kernel(const uint32_t* __restrict__ counts, uint32_t* counts_host) {
    if (threadIdx.x < HS_MCMC_COUNTS)
        __hip_atomic_store(counts_host + threadIdx.x, counts[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- update ----

__global__ void __launch_bounds__(kMcRows) mcmc_source_kernel(int64_t P, const uint32_t* __restrict__ cnt, float* __restrict__ opacities,
                                                              float* __restrict__ scales, double min_opacity, int raw_o, int raw_s) {
    const int64_t i = (int64_t)blockIdx.x * kMcRows + threadIdx.x;
    if (i >= P) return;
    const uint32_t c = cnt[i];
    if (c == 0u) return;
    const int r = c + 1u < (uint32_t)kMcMaxRatio ? (int)(c + 1u) : kMcMaxRatio;
    const double ov = (double)opacities[i];
    const double o = raw_o ? 1.0 / (1.0 + exp(-ov)) : ov;
    const double x = 1.0 - pow(1.0 - o, 1.0 / (double)r);
    double D = 0.0;
    for (int n = 1; n <= r; ++n) {
        double b = 1.0, xp = x, sg = 1.0;     // C(n - 1, k), x^(k + 1), (-1)^k
        for (int k = 0; k < n; ++k) {
            D += ((b * sg) * xp) / sqrt((double)(k + 1));
            b = (b * (double)(n - 1 - k)) / (double)(k + 1);    // exact: every binomial here is below 2^53
            xp *= x;
            sg = -sg;
        }
    }
    const double xc = fmin(fmax(x, min_opacity), 1.0 - 1.1920928955078125e-07);
    opacities[i] = (float)(raw_o ? log(xc / (1.0 - xc)) : xc);
    const double f = o / D;
    const double lf = raw_s ? log(f) : f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double s = (double)scales[3 * i + j];
        scales[3 * i + j] = (float)(raw_s ? s + lf : s * lf);
    }
}

struct McMat { float* p; int64_t S; int32_t role; int32_t pad; };
struct McRows {
    McMat m[kMcMaxMat];
    int32_t n_mat, pad;
    int64_t P;
    const uint32_t* cnt; const int32_t* sources;
};

__global__ void __launch_bounds__(kMcRows) mcmc_rows_kernel(const McRows a) {
    const int64_t i = (int64_t)blockIdx.x * kMcRows + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int64_t base = i - lane;
    int32_t src = -1;
    bool is_src = false;
    if (i < a.P) {
        src = a.sources[i];
        is_src = a.cnt[i] != 0u;
    }
    if (src >= a.P) src = -1;                 // (a stale workspace cannot turn into an access outside the matrices)
    unsigned long long m_dead = __ballot(src >= 0), m_src = __ballot(is_src);
    while (m_dead) {
        const int b = __ffsll((long long)m_dead) - 1;
        m_dead &= m_dead - 1ull;
        const int64_t row = base + b, srow = (int64_t)__shfl(src, b);
#pragma unroll 1
        for (int mi = 0; mi < a.n_mat; ++mi) {
            const McMat& M = a.m[mi];
            if (M.role != HS_DENSIFY_COPY) continue;
            for (int64_t c = lane; c < M.S; c += 64) M.p[row * M.S + c] = M.p[srow * M.S + c];
        }
    }
    while (m_src) {
        const int b = __ffsll((long long)m_src) - 1;
        m_src &= m_src - 1ull;
        const int64_t row = base + b;
#pragma unroll 1
        for (int mi = 0; mi < a.n_mat; ++mi) {
            const McMat& M = a.m[mi];
            if (M.role != HS_DENSIFY_ZERO_NEW) continue;
            for (int64_t c = lane; c < M.S; c += 64) M.p[row * M.S + c] = 0.f;
        }
    }
}

// ---- noise ----

struct McNoise {
    int64_t P;
    float* means; const float* opacities; const float* scales; const float* rotations; const float* xi;
    float scaler; int32_t raw_o, raw_s, rot16;
};

__global__ void __launch_bounds__(kMcRows) mcmc_noise_kernel(const McNoise a) {
    const int64_t i = (int64_t)blockIdx.x * kMcRows + threadIdx.x;
    if (i >= a.P) return;
    float o = a.opacities[i];
    if (a.raw_o) o = sigmoid_of(o);
    const float t = (1.f - o) - 0.995f;
    const float g = 1.f / (1.f + expf(-100.f * t));
    const float gs = g * a.scaler;
    if (gs == 0.f) return;                    // the row keeps its bits (and nothing else of it is read)
    const f4 q = load_quad(a.rotations + 4 * i, a.rot16 != 0);
    float w = q.x, x = q.y, y = q.z, z = q.w;
    quat_normalize(w, x, y, z);
    const float* sp = a.scales + 3 * i;
    float s0 = sp[0], s1 = sp[1], s2 = sp[2];
    if (a.raw_s) { s0 = expf(s0); s1 = expf(s1); s2 = expf(s2); }
    const float* xp = a.xi + 3 * i;
    const float v0 = xp[0] * gs, v1 = xp[1] * gs, v2 = xp[2] * gs;
    float r00, r01, r02, r10, r11, r12, r20, r21, r22;
    quat_rot_row(0, w, x, y, z, r00, r01, r02);
    quat_rot_row(1, w, x, y, z, r10, r11, r12);
    quat_rot_row(2, w, x, y, z, r20, r21, r22);
    const float b0 = (s0 * s0) * ((r00 * v0 + r10 * v1) + r20 * v2);      // sigma^2 (R^T v)
    const float b1 = (s1 * s1) * ((r01 * v0 + r11 * v1) + r21 * v2);
    const float b2 = (s2 * s2) * ((r02 * v0 + r12 * v1) + r22 * v2);
    float* mu = a.means + 3 * i;
    const float m0 = mu[0], m1 = mu[1], m2 = mu[2];
    mu[0] = ((r00 * b0 + r01 * b1) + r02 * b2) + m0;
    mu[1] = ((r10 * b0 + r11 * b1) + r12 * b2) + m1;
    mu[2] = ((r20 * b0 + r21 * b1) + r22 * b2) + m2;
}

// ---- host ----

int check_mcmc_common(const hs_mcmc_args* a, const char* fn) {
    if (check_args(fn, a) || check_rows(fn, "P", a->P)) return HS_EINVAL;
    if (a->mode != HS_MCMC_RELOCATE && a->mode != HS_MCMC_GROW) {
        set_error("%s: mode=%d is neither HS_MCMC_RELOCATE nor HS_MCMC_GROW", fn, a->mode);
        return HS_EINVAL;
    }
    if (check_raw_flags(fn, a->flags)) return HS_EINVAL;
    if (a->mode == HS_MCMC_RELOCATE && a->n_draws != a->P) {
        set_error("%s: n_draws=%lld: a relocation has one draw slot per row (n_draws == P = %lld)", fn, (long long)a->n_draws, (long long)a->P);
        return HS_EINVAL;
    }
    if (a->mode == HS_MCMC_GROW && (a->n_draws < 0 || a->n_draws > a->P)) {
        set_error("%s: n_draws=%lld outside [0, P = %lld]", fn, (long long)a->n_draws, (long long)a->P);
        return HS_EINVAL;
    }
    return HS_OK;
}

int check_sample_args(const hs_mcmc_args* a) {
    const char* fn = "hs_mcmc_sample";
    const int rc = check_mcmc_common(a, fn);
    if (rc != HS_OK) return rc;
    if (a->o_min != a->o_min) { set_error("%s: o_min is NaN", fn); return HS_EINVAL; }
    if (check_field(fn, a->counts, "counts", 4) || check_aligned(fn, a->counts_host, "counts_host", 4) ||
        check_field(fn, a->workspace, "workspace", 16))
        return HS_EINVAL;
    if (a->P == 0) return HS_OK;
    if (check_field(fn, a->opacities, "opacities", 4)) return HS_EINVAL;
    if (a->n_draws > 0 && check_field(fn, a->u, "u", 8)) return HS_EINVAL;
    if (a->mode == HS_MCMC_GROW && check_field(fn, a->row_map, "row_map", 4)) return HS_EINVAL;
    return HS_OK;
}

int check_update_args(const hs_mcmc_args* a) {
    const char* fn = "hs_mcmc_update";
    const int rc = check_mcmc_common(a, fn);
    if (rc != HS_OK) return rc;
    if (!(a->min_opacity >= 0.0 && a->min_opacity <= 1.0)) {
        set_error("%s: min_opacity=%g outside [0, 1]", fn, a->min_opacity);
        return HS_EINVAL;
    }
    if (a->n_matrices < 0 || a->n_matrices > HS_DENSIFY_MAX_MATRICES) {
        set_error("%s: n_matrices=%d outside [0, %d]", fn, a->n_matrices, HS_DENSIFY_MAX_MATRICES);
        return HS_EINVAL;
    }
    if (a->n_matrices > 0 && !a->matrices) { set_error("%s: null matrices", fn); return HS_EINVAL; }
    for (int i = 0; i < a->n_matrices; ++i) {
        const hs_densify_matrix& M = a->matrices[i];
        if (M.role != HS_DENSIFY_COPY && M.role != HS_DENSIFY_ZERO_NEW) {
            set_error("%s: matrices[%d].role=%d is neither HS_DENSIFY_COPY nor HS_DENSIFY_ZERO_NEW", fn, i, M.role);
            return HS_EINVAL;
        }
        if (M.row_stride < 1) { set_error("%s: matrices[%d].row_stride=%lld (need >= 1)", fn, i, (long long)M.row_stride); return HS_EINVAL; }
        if (a->P > 0 && M.row_stride >= kMaxFloats / a->P) {
            set_error("%s: matrices[%d]: P * row_stride = %lld * %lld reaches 2^40", fn, i, (long long)a->P, (long long)M.row_stride);
            return HS_EINVAL;
        }
        if (a->P == 0) continue;
        if (!M.dst) { set_error("%s: matrices[%d]: null dst", fn, i); return HS_EINVAL; }
        if (!aligned_to(M.dst, 4)) { set_error("%s: matrices[%d]: dst must be 4-byte aligned", fn, i); return HS_EINVAL; }
        if (M.src && M.src != M.dst) { set_error("%s: matrices[%d]: src must be NULL or dst (the update is in place)", fn, i); return HS_EINVAL; }
    }
    if (a->P == 0) return HS_OK;
    const Field in[] = {{a->workspace, "workspace", 16}, {a->opacities, "opacities", 4}, {a->scales, "scales", 4}};
    return check_fields(fn, in, 3);
}

int check_noise_args(const hs_mcmc_noise_args* a) {
    const char* fn = "hs_mcmc_noise";
    if (check_args(fn, a) || check_rows(fn, "P", a->P) || check_raw_flags(fn, a->flags)) return HS_EINVAL;
    if (!(a->scaler - a->scaler == 0.f)) { set_error("%s: scaler=%g is not finite", fn, (double)a->scaler); return HS_EINVAL; }
    if (a->P == 0) return HS_OK;
    const Field in[] = {{a->means3D, "means3D", 4}, {a->opacities, "opacities", 4}, {a->scales, "scales", 4},
                        {a->rotations, "rotations", 4}, {a->xi, "xi", 4}};
    return check_fields(fn, in, 5);
}

int launch_sample(const hs_mcmc_args& a, hipStream_t s) {
    const McWs w = mc_carve(a.P, a.n_draws);
    char* ws = (char*)a.workspace;
    const int64_t nblk = mc_blocks(a.P);
    const int relocate = a.mode == HS_MCMC_RELOCATE ? 1 : 0;
    McBlock* blocks = (McBlock*)(ws + w.blocks);
    if (nblk > 0) {
        mcmc_weight_kernel<<<(unsigned)nblk, kMcRows, 0, s>>>(a.opacities, a.P, a.o_min, (a.flags & HS_DENSIFY_RAW_OPACITY) ? 1 : 0, relocate,
                                                             (unsigned long long*)(ws + w.prefix), (uint32_t*)(ws + w.cnt), blocks);
        HS_LAUNCH_CHECK();
    }
    mcmc_scan_kernel<<<1, kMcScanThreads, 0, s>>>(blocks, nblk, (uint32_t)a.P, (uint32_t)a.n_draws, relocate, a.counts);
    HS_LAUNCH_CHECK();
    const int64_t items = relocate ? a.P : a.P + a.n_draws;
    if (nblk > 0 && items > 0) {
        McDraw d;
        memset(&d, 0, sizeof(d));
        d.P = a.P; d.n_draws = a.n_draws; d.nblk = nblk;
        d.opacities = a.opacities; d.u = (const unsigned long long*)a.u;
        d.prefix = (const unsigned long long*)(ws + w.prefix); d.blocks = blocks;
        d.cnt = (uint32_t*)(ws + w.cnt); d.sources = (int32_t*)(ws + w.sources); d.row_map = a.row_map; d.counts = a.counts;
        d.o_min = a.o_min; d.relocate = relocate;
        mcmc_draw_kernel<<<(unsigned)mc_blocks(items), kMcRows, 0, s>>>(d);
        HS_LAUNCH_CHECK();
    }
    if (a.counts_host) {
        mcmc_counts_kernel<<<1, 64, 0, s>>>(a.counts, a.counts_host);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

int launch_update(const hs_mcmc_args& a, hipStream_t s) {
    if (a.P == 0) return HS_OK;
    const McWs w = mc_carve(a.P, a.n_draws);
    char* ws = (char*)a.workspace;
    const unsigned nblk = (unsigned)mc_blocks(a.P);
    mcmc_source_kernel<<<nblk, kMcRows, 0, s>>>(a.P, (const uint32_t*)(ws + w.cnt), a.opacities, a.scales, a.min_opacity,
                                               (a.flags & HS_DENSIFY_RAW_OPACITY) ? 1 : 0, (a.flags & HS_DENSIFY_RAW_SCALES) ? 1 : 0);
    HS_LAUNCH_CHECK();
    if (a.mode != HS_MCMC_RELOCATE || a.n_matrices == 0) return HS_OK;
    McRows r;
    memset(&r, 0, sizeof(r));
    r.P = a.P;
    r.cnt = (const uint32_t*)(ws + w.cnt);
    r.sources = (const int32_t*)(ws + w.sources);
    r.n_mat = a.n_matrices;
    for (int i = 0; i < a.n_matrices; ++i) {
        r.m[i].p = a.matrices[i].dst;
        r.m[i].S = a.matrices[i].row_stride;
        r.m[i].role = a.matrices[i].role;
    }
    mcmc_rows_kernel<<<nblk, kMcRows, 0, s>>>(r);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

int launch_noise(const hs_mcmc_noise_args& a, hipStream_t s) {
    if (a.P == 0) return HS_OK;
    McNoise n;
    memset(&n, 0, sizeof(n));
    n.P = a.P;
    n.means = a.means3D; n.opacities = a.opacities; n.scales = a.scales; n.rotations = a.rotations; n.xi = a.xi;
    n.scaler = a.scaler;
    n.raw_o = (a.flags & HS_DENSIFY_RAW_OPACITY) ? 1 : 0;
    n.raw_s = (a.flags & HS_DENSIFY_RAW_SCALES) ? 1 : 0;
    n.rot16 = aligned_to(a.rotations, 16) ? 1 : 0;
    mcmc_noise_kernel<<<(unsigned)mc_blocks(a.P), kMcRows, 0, s>>>(n);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_mcmc_workspace_bytes(int64_t P, int64_t n_draws) {
    const char* fn = "hs_mcmc_workspace_bytes";
    if (hs::check_rows(fn, "P", P) || hs::check_rows(fn, "n_draws", n_draws)) return HS_EINVAL;
    return hs::mc_carve(P, n_draws).bytes;
}

HS_API int hs_mcmc_sample(const hs_mcmc_args* a, void* hip_stream) {
    const int rc = hs::check_sample_args(a);
    if (rc != HS_OK) return rc;
    return hs::launch_sample(*a, (hipStream_t)hip_stream);
}

HS_API int hs_mcmc_update(const hs_mcmc_args* a, void* hip_stream) {
    const int rc = hs::check_update_args(a);
    if (rc != HS_OK) return rc;
    return hs::launch_update(*a, (hipStream_t)hip_stream);
}

HS_API int hs_mcmc_noise(const hs_mcmc_noise_args* a, void* hip_stream) {
    const int rc = hs::check_noise_args(a);
    if (rc != HS_OK) return rc;
    return hs::launch_noise(*a, (hipStream_t)hip_stream);
}

}  // extern "C"
