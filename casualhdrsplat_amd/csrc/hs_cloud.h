// Shared by the translation units that work on the cloud rather than on a frame: adam, densify, activate, knn, mcmc, mcmc_reg,
// smoothing, and api (which checks the arguments of hs_activate).  The rasterizer's units do not include it; the replay units
// (hs_replay.h: contrib, absgrad) take the host-side argument checks only.
//
// Every unit that uses the float helpers below is compiled with -ffp-contract=off (Makefile, FAST_TUS), and they
// STATE an order of operations: each line is a sequence of correctly rounded IEEE operations around the library expf / sqrtf,
// which the tests compare bit for bit with restatements.  Do not reassociate them.
#pragma once
#include "hs_common.h"

#include <math.h>

namespace hs {

// ---- host: argument checks (each sets the error text and returns HS_EINVAL, or returns HS_OK) ----

constexpr int64_t kMaxRows = 1ll << 30;       // rows of a cloud, draws: counts and row maps keep two bits beside a 30-bit index
constexpr int64_t kMaxFloats = 1ll << 40;     // floats of one matrix (rows * row_stride)

static inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static inline int check_args(const char* fn, const void* a) {
    if (!a) { set_error("%s: null args", fn); return HS_EINVAL; }
    return HS_OK;
}

// a row count (`name` = "P", "n_draws")
static inline int check_rows(const char* fn, const char* name, int64_t n) {
    if (n < 0 || n >= kMaxRows) { set_error("%s: %s=%lld outside [0, 2^30)", fn, name, (long long)n); return HS_EINVAL; }
    return HS_OK;
}

static inline int check_raw_flags(const char* fn, int flags) {
    if (flags & ~(HS_DENSIFY_RAW_OPACITY | HS_DENSIFY_RAW_SCALES)) {
        set_error("%s: flags=%d has bits other than HS_DENSIFY_RAW_OPACITY | HS_DENSIFY_RAW_SCALES", fn, flags);
        return HS_EINVAL;
    }
    return HS_OK;
}

// a pointer that may be null but must be aligned when given (counts_host, n_views, loss)
static inline int check_aligned(const char* fn, const void* p, const char* name, uintptr_t align) {
    if (!aligned_to(p, align)) { set_error("%s: %s must be %d-byte aligned", fn, name, (int)align); return HS_EINVAL; }
    return HS_OK;
}

// required pointers: the first that is null or misaligned is reported (`why`: appended to the "null <name>" text)
struct Field { const void* p; const char* name; uintptr_t align; };

static inline int check_fields(const char* fn, const Field* f, int n, const char* why = "") {
    for (int i = 0; i < n; ++i) {
        if (!f[i].p) { set_error("%s: null %s%s", fn, f[i].name, why); return HS_EINVAL; }
        const int rc = check_aligned(fn, f[i].p, f[i].name, f[i].align);
        if (rc != HS_OK) return rc;
    }
    return HS_OK;
}
static inline int check_field(const char* fn, const void* p, const char* name, uintptr_t align, const char* why = "") {
    const Field f = {p, name, align};
    return check_fields(fn, &f, 1, why);
}

// ---- device ----

typedef float f4 __attribute__((ext_vector_type(4)));

// a / b and a % b of non-negative values; `small`: both below 2^32 (a uniform flag: 32-bit division is a fifth of the 64-bit one)
__device__ __forceinline__ void divmod(int64_t a, int64_t b, bool small, int64_t& q, int64_t& r) {
    if (small) {
        const uint32_t qq = (uint32_t)a / (uint32_t)b;
        q = qq;
        r = (uint32_t)a - qq * (uint32_t)b;
    } else {
        q = a / b;
        r = a - q * b;
    }
}

// HS_BLOCK_OWNER(k, vb, first_block, n) declares `int k`, the owner of virtual block `vb` in the prefix table
// first_block[0 .. n) (uniform: scalar loads of the kernel arguments).  A macro, not a function: as an inlined function the
// compiler lays the streaming kernels around it out differently, and adam_update_kernel's dense path measured 2 % slower.
#define HS_BLOCK_OWNER(k, vb, first_block, n) \
    int k = 0;                                 \
    _Pragma("unroll 1")                        \
    for (int i_ = 1; i_ < (n); ++i_) k += (vb) >= (first_block)[i_] ? 1 : 0

__device__ __forceinline__ f4 load_quad(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const f4*>(p);
    f4 v;
    v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3];
    return v;
}

__device__ __forceinline__ void store_quad(float* p, const f4 v, bool vec) {
    if (vec) {
        *reinterpret_cast<f4*>(p) = v;
    } else {
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}

__device__ __forceinline__ float sigmoid_of(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float quat_length(float q0, float q1, float q2, float q3) {
    return sqrtf(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
}

// q / |q|: four divides, no clamp (hdrsplat.h, the child mean and the position noise)
__device__ __forceinline__ void quat_normalize(float& w, float& x, float& y, float& z) {
    const float n = quat_length(w, x, y, z);
    w = w / n; x = x / n; y = y / n; z = z / n;
}

// row `i` of the rotation matrix of the unit quaternion (w, x, y, z), in the operation order hdrsplat.h states
__device__ __forceinline__ void quat_rot_row(int i, float w, float x, float y, float z, float& r0, float& r1, float& r2) {
    if (i == 0) {
        r0 = 1.f - 2.f * (y * y + z * z); r1 = 2.f * (x * y - w * z); r2 = 2.f * (x * z + w * y);
    } else if (i == 1) {
        r0 = 2.f * (x * y + w * z); r1 = 1.f - 2.f * (x * x + z * z); r2 = 2.f * (y * z - w * x);
    } else {
        r0 = 2.f * (x * z - w * y); r1 = 2.f * (y * z + w * x); r2 = 1.f - 2.f * (x * x + y * y);
    }
}

}  // namespace hs
