// Host-side sanitizer driver of the depth-normal consistency term and of the per-Gaussian normal
// (hs_normal_consistency_workspace_bytes, hs_normal_consistency, hs_normal_consistency_backward, hs_gaussian_normals,
// hs_gaussian_normals_backward): their argument validation and the workspace arithmetic, with AddressSanitizer + UBSan on the
// host objects of libhdrsplat (built and run by `make -C casualhdrsplat_amd/csrc asan`, beside asan_host.cpp,
// distortion_host.cpp and the others).  No GPU is needed or touched: every call here returns before its first HIP call.
// Exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>

#include "hdrsplat.h"

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) { std::fprintf(stderr, "FAILED: %s (line %d): %s\n", #cond, __LINE__, hs_last_error()); return 1; } \
    } while (0)
#define REJECTS(call, text) CHECK((call) == HS_EINVAL && std::strstr(hs_last_error(), text))

static int run() {
    CHECK(hs_version() == HS_VERSION);
    // the workspace: none (the backward keeps its halo in LDS), for every frame the calls accept
    const int sizes[][3] = {{1, 1, 1}, {1, 3, 3}, {2, 37, 70}, {1, 1080, 1920}, {8, 2160, 3840}, {1, 1, 715827882}, {715827882, 1, 1}};
    for (const auto& s : sizes) CHECK(hs_normal_consistency_workspace_bytes(s[0], s[1], s[2]) == 0);
    REJECTS(hs_normal_consistency_workspace_bytes(0, 8, 8), "B=0 must be at least 1");
    REJECTS(hs_normal_consistency_workspace_bytes(1, -1, 8), "H=-1 must be at least 1");
    REJECTS(hs_normal_consistency_workspace_bytes(1, 8, 0), "W=0 must be at least 1");
    REJECTS(hs_normal_consistency_workspace_bytes(1, 1, 715827883), "must be below 2^31");
    REJECTS(hs_normal_consistency_workspace_bytes(2147483647, 2147483647, 2147483647), "must be below 2^31");

    char* fake = reinterpret_cast<char*>(4096);  // never dereferenced on the host
    hs_normal_consistency_args good;
    std::memset(&good, 0, sizeof good);
    good.B = 2; good.H = 37; good.W = 70; good.fx = 77.f; good.fy = 63.f;
    good.invdepth = good.alpha = good.normals = good.weight = good.cam_to_world = (const float*)fake;
    good.out = good.depth_normals = (float*)fake;
    good.dL_dout = (const float*)fake;
    good.dL_dnormals = good.dL_dinvdepth = good.dL_dalpha = (float*)fake;

    REJECTS(hs_normal_consistency(nullptr, nullptr), "hs_normal_consistency: null args");
    hs_normal_consistency_args a = good;
    a.B = 0; REJECTS(hs_normal_consistency(&a, nullptr), "B=0");
    a = good; a.H = 0; REJECTS(hs_normal_consistency(&a, nullptr), "H=0");
    a = good; a.W = -5; REJECTS(hs_normal_consistency(&a, nullptr), "W=-5");
    a = good; a.B = 1 << 12; a.H = 1 << 10; a.W = 1 << 10; REJECTS(hs_normal_consistency(&a, nullptr), "must be below 2^31");
    a = good; a.fx = 0.f; REJECTS(hs_normal_consistency(&a, nullptr), "must be finite and positive");
    a = good; a.fy = -1.f; REJECTS(hs_normal_consistency(&a, nullptr), "must be finite and positive");
    a = good; a.fx = std::numeric_limits<float>::quiet_NaN(); REJECTS(hs_normal_consistency(&a, nullptr), "must be finite and positive");
    a = good; a.fy = std::numeric_limits<float>::infinity(); REJECTS(hs_normal_consistency(&a, nullptr), "must be finite and positive");
    a = good; a.invdepth = nullptr; REJECTS(hs_normal_consistency(&a, nullptr), "null invdepth");
    a = good; a.invdepth = (const float*)(fake + 2); REJECTS(hs_normal_consistency(&a, nullptr), "invdepth must be 4-byte aligned");
    a = good; a.alpha = (const float*)(fake + 1); REJECTS(hs_normal_consistency(&a, nullptr), "alpha must be 4-byte aligned");
    a = good; a.weight = (const float*)(fake + 3); REJECTS(hs_normal_consistency(&a, nullptr), "weight must be 4-byte aligned");
    a = good; a.cam_to_world = (const float*)(fake + 2); REJECTS(hs_normal_consistency(&a, nullptr), "cam_to_world must be 4-byte aligned");
    a = good; a.normals = nullptr; REJECTS(hs_normal_consistency(&a, nullptr), "null normals (needed with out)");
    a = good; a.normals = (const float*)(fake + 2); REJECTS(hs_normal_consistency(&a, nullptr), "normals must be 4-byte aligned");
    a = good; a.out = (float*)(fake + 2); REJECTS(hs_normal_consistency(&a, nullptr), "out must be 4-byte aligned");
    a = good; a.depth_normals = (float*)(fake + 2); REJECTS(hs_normal_consistency(&a, nullptr), "depth_normals must be 4-byte aligned");
    a = good; a.out = nullptr; a.depth_normals = nullptr; REJECTS(hs_normal_consistency(&a, nullptr), "nothing to write");
    // the normals are not needed for the depth normals alone, but must be aligned when given
    a = good; a.out = nullptr; a.normals = (const float*)(fake + 1); REJECTS(hs_normal_consistency(&a, nullptr), "normals must be 4-byte aligned");

    REJECTS(hs_normal_consistency_backward(nullptr, nullptr), "hs_normal_consistency_backward: null args");
    a = good; a.W = 0; REJECTS(hs_normal_consistency_backward(&a, nullptr), "W=0");
    a = good; a.fx = 0.f; REJECTS(hs_normal_consistency_backward(&a, nullptr), "must be finite and positive");
    a = good; a.invdepth = nullptr; REJECTS(hs_normal_consistency_backward(&a, nullptr), "null invdepth");
    a = good; a.normals = nullptr; REJECTS(hs_normal_consistency_backward(&a, nullptr), "null normals");
    a = good; a.dL_dout = nullptr; REJECTS(hs_normal_consistency_backward(&a, nullptr), "null dL_dout");
    a = good; a.dL_dout = (const float*)(fake + 2); REJECTS(hs_normal_consistency_backward(&a, nullptr), "dL_dout must be 4-byte aligned");
    a = good; a.dL_dnormals = (float*)(fake + 2); REJECTS(hs_normal_consistency_backward(&a, nullptr), "dL_dnormals must be 4-byte aligned");
    a = good; a.dL_dinvdepth = (float*)(fake + 1); REJECTS(hs_normal_consistency_backward(&a, nullptr), "dL_dinvdepth must be 4-byte aligned");
    a = good; a.dL_dalpha = (float*)(fake + 3); REJECTS(hs_normal_consistency_backward(&a, nullptr), "dL_dalpha must be 4-byte aligned");
    a = good; a.alpha = nullptr; REJECTS(hs_normal_consistency_backward(&a, nullptr), "dL_dalpha without alpha");
    // no gradient asked for: a no-op
    a = good; a.dL_dnormals = a.dL_dinvdepth = a.dL_dalpha = nullptr; CHECK(hs_normal_consistency_backward(&a, nullptr) == HS_OK);

    hs_gaussian_normals_args ggood;
    std::memset(&ggood, 0, sizeof ggood);
    ggood.P = 1000;
    ggood.rotations = ggood.scales = ggood.means3D = ggood.campos = ggood.dL_dnormals = (const float*)fake;
    ggood.normals = ggood.dL_drotations = (float*)fake;
    REJECTS(hs_gaussian_normals(nullptr, nullptr), "hs_gaussian_normals: null args");
    REJECTS(hs_gaussian_normals_backward(nullptr, nullptr), "hs_gaussian_normals_backward: null args");
    hs_gaussian_normals_args g = ggood;
    g.P = -1; REJECTS(hs_gaussian_normals(&g, nullptr), "P=-1 outside [0, 2^30)");
    g = ggood; g.P = 1ll << 30; REJECTS(hs_gaussian_normals_backward(&g, nullptr), "outside [0, 2^30)");
    g = ggood; g.rotations = nullptr; REJECTS(hs_gaussian_normals(&g, nullptr), "null rotations");
    g = ggood; g.rotations = (const float*)(fake + 4); REJECTS(hs_gaussian_normals(&g, nullptr), "rotations must be 16-byte aligned");
    g = ggood; g.scales = nullptr; REJECTS(hs_gaussian_normals(&g, nullptr), "null scales");
    g = ggood; g.means3D = (const float*)(fake + 2); REJECTS(hs_gaussian_normals(&g, nullptr), "means3D must be 4-byte aligned");
    g = ggood; g.campos = nullptr; REJECTS(hs_gaussian_normals(&g, nullptr), "null campos");
    g = ggood; g.normals = nullptr; REJECTS(hs_gaussian_normals(&g, nullptr), "null normals");
    g = ggood; g.normals = (float*)(fake + 2); REJECTS(hs_gaussian_normals(&g, nullptr), "normals must be 4-byte aligned");
    g = ggood; g.dL_dnormals = nullptr; REJECTS(hs_gaussian_normals_backward(&g, nullptr), "null dL_dnormals");
    g = ggood; g.dL_drotations = nullptr; REJECTS(hs_gaussian_normals_backward(&g, nullptr), "null dL_drotations");
    g = ggood; g.dL_drotations = (float*)(fake + 8); REJECTS(hs_gaussian_normals_backward(&g, nullptr), "dL_drotations must be 16-byte aligned");
    g = ggood; g.scales = (const float*)(fake + 1); REJECTS(hs_gaussian_normals_backward(&g, nullptr), "scales must be 4-byte aligned");
    // an empty cloud: a no-op that looks at no pointer
    std::memset(&g, 0, sizeof g);
    CHECK(hs_gaussian_normals(&g, nullptr) == HS_OK && hs_gaussian_normals_backward(&g, nullptr) == HS_OK);
    return 0;
}

int main() {
    // the error text is thread-local: two threads validating at once must not trample each other's message
    int rc[2] = {1, 1};
    std::thread t0([&] { rc[0] = run(); }), t1([&] { rc[1] = run(); });
    t0.join();
    t1.join();
    if (rc[0] || rc[1]) return 1;
    std::puts("normals_host: clean");
    return 0;
}
