// Host-side sanitizer driver of the depth-distortion loss (hs_distortion_workspace_bytes, hs_distortion,
// hs_distortion_backward): their argument validation and the workspace arithmetic, with AddressSanitizer + UBSan on the host
// objects of libhdrsplat (built and run by `make -C casualhdrsplat_amd/csrc asan`, beside asan_host.cpp, features_host.cpp and
// the others).  No GPU is needed or touched: every call here returns before its first HIP call.  Exit code 0 = clean.
#include <cstdio>
#include <cstring>
#include <thread>

#include "hdrsplat.h"

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) { std::fprintf(stderr, "FAILED: %s (line %d): %s\n", #cond, __LINE__, hs_last_error()); return 1; } \
    } while (0)
#define REJECTS(call, text) CHECK((call) == HS_EINVAL && std::strstr(hs_last_error(), text))

static int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

static hs_dims dims_of(int P, int n_poses, int64_t capacity) {
    hs_dims d;
    std::memset(&d, 0, sizeof d);
    d.P = P; d.M = 16; d.sh_degree = 3; d.W = 128; d.H = 72; d.n_poses = n_poses; d.capacity = capacity;
    return d;
}

static int run() {
    CHECK(hs_version() == HS_VERSION);
    // the workspace: 64-byte pair records, 64-byte rows per instance, one flag byte per pair
    const int64_t caps[] = {0, 1, 15, 16, 17, 1000, 100000, 10000000, (1ll << 30) - 1};
    int64_t last = 0;
    for (int64_t cap : caps) {
        const hs_dims d = dims_of(1000, 3, cap);
        const int64_t b = hs_distortion_workspace_bytes(&d);
        CHECK(b == align256(64 * cap) + align256(64 * 1000 * 3) + align256(cap) && b % 256 == 0 && b >= last);
        last = b;
    }
    {
        const hs_dims big = dims_of(1000000, 4, 1000);
        CHECK(hs_distortion_workspace_bytes(&big) == align256(64 * 1000) + 64ll * 1000000 * 4 + align256(1000));
        const hs_dims d = dims_of(0, 1, 0);
        CHECK(hs_distortion_workspace_bytes(&d) == 256);
        hs_dims bad = dims_of(1000, 1, 1ll << 30);
        REJECTS(hs_distortion_workspace_bytes(&bad), "hs_plan:");
        bad = dims_of(-1, 1, 100);
        REJECTS(hs_distortion_workspace_bytes(&bad), "hs_plan:");
        bad = dims_of(1000, 3, 100); bad.n_frames = 2;
        REJECTS(hs_distortion_workspace_bytes(&bad), "hs_plan:");
        REJECTS(hs_distortion_workspace_bytes(nullptr), "hs_distortion_workspace_bytes: null args");
    }

    char* fake = reinterpret_cast<char*>(4096);  // never dereferenced on the host
    hs_distortion_args good;
    std::memset(&good, 0, sizeof good);
    good.dims = dims_of(1000, 2, 10000);
    good.geom = fake; good.binning = fake; good.image = fake;
    good.out_distortion = (float*)fake; good.out_moment = (float*)fake;
    REJECTS(hs_distortion(nullptr, nullptr), "hs_distortion: null args");
    hs_distortion_args a = good;
    a.dims.W = 0; REJECTS(hs_distortion(&a, nullptr), "hs_plan:");
    a = good; a.dims.capacity = -1; REJECTS(hs_distortion(&a, nullptr), "hs_plan:");
    a = good; a.out_distortion = nullptr; REJECTS(hs_distortion(&a, nullptr), "null out_distortion");
    a = good; a.out_distortion = (float*)(fake + 2); REJECTS(hs_distortion(&a, nullptr), "out_distortion must be 4-byte aligned");
    a = good; a.out_moment = nullptr; REJECTS(hs_distortion(&a, nullptr), "null out_moment");
    a = good; a.out_moment = (float*)(fake + 1); REJECTS(hs_distortion(&a, nullptr), "out_moment must be 4-byte aligned");
    a = good; a.geom = nullptr; REJECTS(hs_distortion(&a, nullptr), "null geom");
    a = good; a.geom = fake + 64; REJECTS(hs_distortion(&a, nullptr), "geom must be 256-byte aligned");
    a = good; a.binning = nullptr; REJECTS(hs_distortion(&a, nullptr), "null binning");
    a = good; a.binning = fake + 128; REJECTS(hs_distortion(&a, nullptr), "binning must be 256-byte aligned");
    a = good; a.image = nullptr; REJECTS(hs_distortion(&a, nullptr), "null image");
    a = good; a.image = fake + 16; REJECTS(hs_distortion(&a, nullptr), "image must be 256-byte aligned");
    // an empty cloud still has two planes to write: they must be there
    std::memset(&a, 0, sizeof a);
    a.dims = dims_of(0, 1, 0);
    REJECTS(hs_distortion(&a, nullptr), "null out_distortion");

    hs_distortion_bwd_args bgood;
    std::memset(&bgood, 0, sizeof bgood);
    bgood.dims = dims_of(1000, 2, 10000);
    bgood.tanfovx = bgood.tanfovy = 0.5f; bgood.scale_modifier = 1.f;
    bgood.viewmatrices = bgood.projmatrices = bgood.camposes = (const float*)fake;
    bgood.means3D = bgood.opacities = bgood.scales = bgood.rotations = (const float*)fake;
    bgood.geom = fake; bgood.binning = fake; bgood.image = fake; bgood.ws = fake;
    bgood.moment = bgood.dL_ddistortion = (const float*)fake;
    bgood.dL_dmeans3D = bgood.dL_dopacities = bgood.dL_dscales = bgood.dL_drotations = (float*)fake;
    REJECTS(hs_distortion_backward(nullptr, nullptr), "hs_distortion_backward: null args");
    hs_distortion_bwd_args b = bgood;
    b.dims.n_poses = 0; REJECTS(hs_distortion_backward(&b, nullptr), "hs_plan:");
    b = bgood; b.dims.n_frames = 3; REJECTS(hs_distortion_backward(&b, nullptr), "hs_plan:");
    b = bgood; b.scales = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null scales (the forward's scales and rotations: a cov3D_precomp");
    b = bgood; b.rotations = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "cov3D_precomp");
    b = bgood; b.rotations = (const float*)(fake + 4); REJECTS(hs_distortion_backward(&b, nullptr), "rotations must be 16-byte aligned");
    b = bgood; b.geom = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null geom");
    b = bgood; b.binning = fake + 128; REJECTS(hs_distortion_backward(&b, nullptr), "binning must be 256-byte aligned");
    b = bgood; b.image = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null image");
    b = bgood; b.ws = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null ws");
    b = bgood; b.ws = fake + 64; REJECTS(hs_distortion_backward(&b, nullptr), "ws must be 256-byte aligned");
    b = bgood; b.viewmatrices = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null viewmatrices");
    b = bgood; b.projmatrices = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null projmatrices");
    b = bgood; b.camposes = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null camposes");
    b = bgood; b.means3D = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null means3D");
    b = bgood; b.opacities = (const float*)(fake + 2); REJECTS(hs_distortion_backward(&b, nullptr), "opacities must be 4-byte aligned");
    b = bgood; b.moment = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null moment");
    b = bgood; b.moment = (const float*)(fake + 2); REJECTS(hs_distortion_backward(&b, nullptr), "moment must be 4-byte aligned");
    b = bgood; b.dL_ddistortion = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null dL_ddistortion");
    b = bgood; b.dL_dmeans3D = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null dL_dmeans3D");
    b = bgood; b.dL_dopacities = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null dL_dopacities");
    b = bgood; b.dL_dscales = (float*)(fake + 1); REJECTS(hs_distortion_backward(&b, nullptr), "dL_dscales must be 4-byte aligned");
    b = bgood; b.dL_drotations = nullptr; REJECTS(hs_distortion_backward(&b, nullptr), "null dL_drotations");
    b = bgood; b.dL_drotations = (float*)(fake + 8); REJECTS(hs_distortion_backward(&b, nullptr), "dL_drotations must be 16-byte aligned");
    // an empty cloud: the gradients have no elements -- a no-op that looks at no pointer
    std::memset(&b, 0, sizeof b);
    b.dims = dims_of(0, 1, 0);
    CHECK(hs_distortion_backward(&b, nullptr) == HS_OK);
    return 0;
}

int main() {
    // the error text is thread-local: two threads validating at once must not trample each other's message
    int rc[2] = {1, 1};
    std::thread t0([&] { rc[0] = run(); }), t1([&] { rc[1] = run(); });
    t0.join();
    t1.join();
    if (rc[0] || rc[1]) return 1;
    std::puts("distortion_host: clean");
    return 0;
}
