// The regularisers of the MCMC policy (hs_mcmc_reg_workspace_bytes, hs_mcmc_regularize; include/hdrsplat.h states the
// arithmetic): lambda_o mean|opacity| + lambda_s mean|scale|, as the gradient they add to the rows hs_backward wrote and,
// optionally, as two numbers on the device.  A translation unit of its own beside mcmc.hip (whose kernel list, resources and
// atomics tests/test_mcmc.py pins); it shares nothing with it but the flags.
//
//   mcmc_reg_kernel      256 Gaussians per workgroup, one opacity and three scale ELEMENTS per thread: thread t of block b takes
//                        opacity 256 b + t and the scale floats 768 b + t, + 256, + 512 -- the map is elementwise, so every load
//                        and store of a wave is 256 contiguous bytes, whatever the row a float belongs to.  g += k * term in
//                        place, read and written by the same thread; an array whose lambda is 0 is not touched.  With `loss`:
//                        each thread's terms as doubles, added over the block by a fixed tree in LDS, one {S_o, S_s} per block
//   mcmc_reg_sum_kernel  with `loss` only, ONE workgroup: thread t adds the block records [t c, (t + 1) c) in ascending order
//                        (c = ceil(blocks / 256)), thread 0 adds the 256 thread sums in ascending order and writes loss[0..1].
//                        The order is a function of P alone and every record is written before it is read: the same bits on
//                        every run, whatever the workspace held.
// No atomics, no memset, no copy, no synchronisation.  Compiled with -ffp-contract=off; denormals kept.
#include "hs_cloud.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

namespace hs {
namespace {

constexpr int kRegRows = 256;                 // Gaussians per workgroup (= threads)
constexpr int kRegSumThreads = 256;

struct RegBlock { double o, s; };             // 16 bytes per block of 256 Gaussians
static_assert(sizeof(RegBlock) == 16, "the workspace formula counts 16 bytes per block record");

inline int64_t reg_blocks(int64_t P) { return (P + kRegRows - 1) / kRegRows; }

struct McReg {
    int64_t P;
    const float* opacities; const float* scales;
    float* g_o; float* g_s;
    RegBlock* blocks;                         // NULL: no loss is asked for
    float ko, ks;
    int32_t raw_o, raw_s, do_o, do_s;         // do_*: the gradient array is updated (its lambda is not 0)
};

__device__ __forceinline__ float reg_sign(float x) { return x != x ? x : (float)((x > 0.f) - (x < 0.f)); }

__global__ void __launch_bounds__(kRegRows) mcmc_reg_kernel(const McReg a) {
    __shared__ double s_o[kRegRows], s_s[kRegRows];
    const int t = threadIdx.x;
    const bool sum = a.blocks != nullptr;
    double acc_o = 0.0, acc_s = 0.0;
    const int64_t i = (int64_t)blockIdx.x * kRegRows + t;
    if (i < a.P && (a.do_o || sum)) {
        const float x = a.opacities[i];
        float term, mag;
        if (a.raw_o) {
            const float o = sigmoid_of(x);
            term = (1.f - o) * o;
            mag = o;
        } else {
            term = reg_sign(x);
            mag = fabsf(x);
        }
        if (a.do_o) a.g_o[i] = a.g_o[i] + a.ko * term;
        acc_o = (double)mag;
    }
    if (a.do_s || sum) {
        const int64_t n = 3 * a.P;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int64_t e = (int64_t)blockIdx.x * (3 * kRegRows) + j * kRegRows + t;
            if (e >= n) break;
            const float x = a.scales[e];
            float term, mag;
            if (a.raw_s) {
                term = expf(x);
                mag = term;
            } else {
                term = reg_sign(x);
                mag = fabsf(x);
            }
            if (a.do_s) a.g_s[e] = a.g_s[e] + a.ks * term;
            acc_s += (double)mag;
        }
    }
    if (!sum) return;
    s_o[t] = acc_o;
    s_s[t] = acc_s;
    __syncthreads();
    for (int off = kRegRows / 2; off > 0; off >>= 1) {
        if (t < off) {
            s_o[t] += s_o[t + off];
            s_s[t] += s_s[t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        RegBlock b;
        b.o = s_o[0];
        b.s = s_s[0];
        a.blocks[blockIdx.x] = b;
    }
}

__global__ void __launch_bounds__(kRegSumThreads) mcmc_reg_sum_kernel(const RegBlock* __restrict__ blocks, int64_t nblk, double P,
                                                                       double lambda_o, double lambda_s, float* __restrict__ loss) {
    __shared__ double s_o[kRegSumThreads], s_s[kRegSumThreads];
    const int t = threadIdx.x;
    const int64_t per = (nblk + kRegSumThreads - 1) / kRegSumThreads;
    const int64_t b0 = t * per < nblk ? t * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
    double o = 0.0, s = 0.0;
    for (int64_t b = b0; b < b1; ++b) { o += blocks[b].o; s += blocks[b].s; }
    s_o[t] = o;
    s_s[t] = s;
    __syncthreads();
    if (t != 0) return;
    if (nblk == 0) {                          // an empty cloud: both terms are zero, not 0 / 0
        loss[0] = 0.f;
        loss[1] = 0.f;
        return;
    }
    o = 0.0; s = 0.0;
    for (int k = 0; k < kRegSumThreads; ++k) { o += s_o[k]; s += s_s[k]; }
    loss[0] = (float)(lambda_o * (o / P));
    loss[1] = (float)(lambda_s * (s / (3.0 * P)));
}

int check_reg_args(const hs_mcmc_reg_args* a) {
    const char* fn = "hs_mcmc_regularize";
    if (check_args(fn, a) || check_rows(fn, "P", a->P) || check_raw_flags(fn, a->flags)) return HS_EINVAL;
    if (!(a->lambda_opacity >= 0.0 && a->lambda_opacity - a->lambda_opacity == 0.0)) {
        set_error("%s: lambda_opacity=%g must be finite and not negative", fn, a->lambda_opacity);
        return HS_EINVAL;
    }
    if (!(a->lambda_scale >= 0.0 && a->lambda_scale - a->lambda_scale == 0.0)) {
        set_error("%s: lambda_scale=%g must be finite and not negative", fn, a->lambda_scale);
        return HS_EINVAL;
    }
    if (check_aligned(fn, a->loss, "loss", 4)) return HS_EINVAL;
    if (a->P == 0) return HS_OK;
    if (a->loss && check_field(fn, a->workspace, "workspace", 16, " (needed with loss)")) return HS_EINVAL;
    const bool do_o = a->lambda_opacity != 0.0, do_s = a->lambda_scale != 0.0;
    Field f[4];
    int n = 0;
    if (do_o || a->loss) f[n++] = {a->opacities, "opacities", 4};
    if (do_s || a->loss) f[n++] = {a->scales, "scales", 4};
    if (do_o) f[n++] = {a->dL_dopacities, "dL_dopacities", 4};
    if (do_s) f[n++] = {a->dL_dscales, "dL_dscales", 4};
    return check_fields(fn, f, n);
}

int launch_reg(const hs_mcmc_reg_args& a, hipStream_t s) {
    const bool do_o = a.lambda_opacity != 0.0, do_s = a.lambda_scale != 0.0;
    if (!do_o && !do_s && !a.loss) return HS_OK;
    const int64_t nblk = reg_blocks(a.P);
    if (nblk > 0) {
        McReg r;
        memset(&r, 0, sizeof(r));
        r.P = a.P;
        r.opacities = a.opacities; r.scales = a.scales;
        r.g_o = a.dL_dopacities; r.g_s = a.dL_dscales;
        r.blocks = a.loss ? (RegBlock*)a.workspace : nullptr;
        r.ko = (float)(a.lambda_opacity / (double)a.P);
        r.ks = (float)(a.lambda_scale / (3.0 * (double)a.P));
        r.raw_o = (a.flags & HS_DENSIFY_RAW_OPACITY) ? 1 : 0;
        r.raw_s = (a.flags & HS_DENSIFY_RAW_SCALES) ? 1 : 0;
        r.do_o = do_o ? 1 : 0;
        r.do_s = do_s ? 1 : 0;
        mcmc_reg_kernel<<<(unsigned)nblk, kRegRows, 0, s>>>(r);
        HS_LAUNCH_CHECK();
    }
    if (a.loss) {
        mcmc_reg_sum_kernel<<<1, kRegSumThreads, 0, s>>>((const RegBlock*)a.workspace, nblk, (double)a.P, a.lambda_opacity,
                                                         a.lambda_scale, a.loss);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_mcmc_reg_workspace_bytes(int64_t P) {
    if (hs::check_rows("hs_mcmc_reg_workspace_bytes", "P", P)) return HS_EINVAL;
    return hs::align_up(16 * hs::reg_blocks(P), 256);
}

HS_API int hs_mcmc_regularize(const hs_mcmc_reg_args* a, void* hip_stream) {
    const int rc = hs::check_reg_args(a);
    if (rc != HS_OK) return rc;
    return hs::launch_reg(*a, (hipStream_t)hip_stream);
}

}  // extern "C"
