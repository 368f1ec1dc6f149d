// Host-side sanitizer driver of the per-Gaussian feature compositing (hs_composite_features_workspace_bytes,
// hs_composite_features, hs_composite_features_backward): their argument validation and the workspace arithmetic, with
// AddressSanitizer + UBSan on the host objects of libhdrsplat (built and run by `make -C casualhdrsplat_amd/csrc asan`, beside
// asan_host.cpp, rows_host.cpp and the others).  No GPU is needed or touched: every call here returns before its first HIP
// call.  Exit code 0 = clean.
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
    // the workspace: 32-byte records (eight channels per pass), whatever the number of channels
    const int64_t caps[] = {0, 1, 15, 16, 17, 1000, 100000, 10000000, (1ll << 30) - 1};
    int64_t last = 0;
    for (int64_t cap : caps) {
        const hs_dims d = dims_of(1000, 3, cap);
        const int64_t b = hs_composite_features_workspace_bytes(&d);
        CHECK(b == align256(32 * cap) + align256(32 * 1000 * 3) && b % 256 == 0 && b >= last);
        last = b;
    }
    {
        const hs_dims d = dims_of(0, 1, 0);
        CHECK(hs_composite_features_workspace_bytes(&d) == 256);
        hs_dims bad = dims_of(1000, 1, 1ll << 30);
        REJECTS(hs_composite_features_workspace_bytes(&bad), "hs_plan:");
        bad = dims_of(-1, 1, 100);
        REJECTS(hs_composite_features_workspace_bytes(&bad), "hs_plan:");
        bad = dims_of(1000, 3, 100); bad.n_frames = 2;
        REJECTS(hs_composite_features_workspace_bytes(&bad), "hs_plan:");
        REJECTS(hs_composite_features_workspace_bytes(nullptr), "hs_composite_features_workspace_bytes: null args");
    }

    char* fake = reinterpret_cast<char*>(4096);  // never dereferenced on the host
    hs_composite_features_args good;
    std::memset(&good, 0, sizeof good);
    good.dims = dims_of(1000, 2, 10000);
    good.geom = fake; good.binning = fake; good.image = fake; good.n_channels = 7;
    good.features = (const float*)fake; good.out = (float*)fake;
    REJECTS(hs_composite_features(nullptr, nullptr), "hs_composite_features: null args");
    hs_composite_features_args a = good;
    a.dims.W = 0; REJECTS(hs_composite_features(&a, nullptr), "hs_plan:");
    a = good; a.dims.capacity = -1; REJECTS(hs_composite_features(&a, nullptr), "hs_plan:");
    a = good; a.n_channels = 0; REJECTS(hs_composite_features(&a, nullptr), "n_channels=0 outside [1, 512]");
    a = good; a.n_channels = 513; REJECTS(hs_composite_features(&a, nullptr), "n_channels=513 outside [1, 512]");
    a = good; a.n_channels = -5; REJECTS(hs_composite_features(&a, nullptr), "n_channels=-5");
    a = good; a.out = nullptr; REJECTS(hs_composite_features(&a, nullptr), "null out");
    a = good; a.out = (float*)(fake + 2); REJECTS(hs_composite_features(&a, nullptr), "out must be 4-byte aligned");
    a = good; a.geom = nullptr; REJECTS(hs_composite_features(&a, nullptr), "null geom");
    a = good; a.geom = fake + 64; REJECTS(hs_composite_features(&a, nullptr), "geom must be 256-byte aligned");
    a = good; a.binning = nullptr; REJECTS(hs_composite_features(&a, nullptr), "null binning");
    a = good; a.binning = fake + 128; REJECTS(hs_composite_features(&a, nullptr), "binning must be 256-byte aligned");
    a = good; a.image = nullptr; REJECTS(hs_composite_features(&a, nullptr), "null image");
    a = good; a.image = fake + 16; REJECTS(hs_composite_features(&a, nullptr), "image must be 256-byte aligned");
    a = good; a.features = nullptr; REJECTS(hs_composite_features(&a, nullptr), "null features");
    a = good; a.features = (const float*)(fake + 1); REJECTS(hs_composite_features(&a, nullptr), "features must be 4-byte aligned");
    // an empty cloud still has `out` to write: it must be there
    std::memset(&a, 0, sizeof a);
    a.dims = dims_of(0, 1, 0); a.n_channels = 3;
    REJECTS(hs_composite_features(&a, nullptr), "null out");

    hs_composite_features_bwd_args bgood;
    std::memset(&bgood, 0, sizeof bgood);
    bgood.dims = dims_of(1000, 2, 10000);
    bgood.geom = fake; bgood.binning = fake; bgood.image = fake; bgood.ws = fake; bgood.n_channels = 19;
    bgood.dL_dout = (const float*)fake; bgood.dL_dfeatures = (float*)fake;
    REJECTS(hs_composite_features_backward(nullptr, nullptr), "hs_composite_features_backward: null args");
    hs_composite_features_bwd_args b = bgood;
    b.dims.n_poses = 0; REJECTS(hs_composite_features_backward(&b, nullptr), "hs_plan:");
    b = bgood; b.n_channels = 0; REJECTS(hs_composite_features_backward(&b, nullptr), "n_channels=0 outside [1, 512]");
    b = bgood; b.n_channels = 1024; REJECTS(hs_composite_features_backward(&b, nullptr), "n_channels=1024 outside [1, 512]");
    b = bgood; b.geom = nullptr; REJECTS(hs_composite_features_backward(&b, nullptr), "null geom");
    b = bgood; b.binning = nullptr; REJECTS(hs_composite_features_backward(&b, nullptr), "null binning");
    b = bgood; b.image = nullptr; REJECTS(hs_composite_features_backward(&b, nullptr), "null image");
    b = bgood; b.image = fake + 32; REJECTS(hs_composite_features_backward(&b, nullptr), "image must be 256-byte aligned");
    b = bgood; b.ws = nullptr; REJECTS(hs_composite_features_backward(&b, nullptr), "null ws");
    b = bgood; b.ws = fake + 128; REJECTS(hs_composite_features_backward(&b, nullptr), "ws must be 256-byte aligned");
    b = bgood; b.dL_dout = nullptr; REJECTS(hs_composite_features_backward(&b, nullptr), "null dL_dout");
    b = bgood; b.dL_dout = (const float*)(fake + 2); REJECTS(hs_composite_features_backward(&b, nullptr), "dL_dout must be 4-byte aligned");
    b = bgood; b.dL_dfeatures = nullptr; REJECTS(hs_composite_features_backward(&b, nullptr), "null dL_dfeatures");
    b = bgood; b.dL_dfeatures = (float*)(fake + 3); REJECTS(hs_composite_features_backward(&b, nullptr), "dL_dfeatures must be 4-byte aligned");
    // an empty cloud: dL_dfeatures has no elements -- a no-op that looks at no pointer, but C is still checked
    std::memset(&b, 0, sizeof b);
    b.dims = dims_of(0, 1, 0); b.n_channels = 600;
    REJECTS(hs_composite_features_backward(&b, nullptr), "n_channels=600");
    b.n_channels = 4;
    CHECK(hs_composite_features_backward(&b, nullptr) == HS_OK);
    return 0;
}

int main() {
    // the error text is thread-local: two threads validating at once must not trample each other's message
    int rc[2] = {1, 1};
    std::thread t0([&] { rc[0] = run(); }), t1([&] { rc[1] = run(); });
    t0.join();
    t1.join();
    if (rc[0] || rc[1]) return 1;
    std::puts("features_host: clean");
    return 0;
}
