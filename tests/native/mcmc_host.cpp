// Host-side sanitizer driver of the MCMC entry points (hs_mcmc_workspace_bytes, hs_mcmc_sample, hs_mcmc_update,
// hs_mcmc_noise): their argument validation and the workspace arithmetic, with AddressSanitizer + UBSan on the host objects
// of libhdrsplat (built and run by `make -C casualhdrsplat_amd/csrc asan`, beside asan_host.cpp).  No GPU is needed or
// touched: every call here returns before its first HIP call.  Exit code 0 = clean.
#include <cmath>
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

static int run() {
    CHECK(hs_version() == HS_VERSION);
    const int64_t Ps[] = {0, 1, 255, 256, 257, 10007, 1000000, (1ll << 30) - 1};
    for (int64_t P : Ps)
        for (int64_t n : {(int64_t)0, (int64_t)1, P / 20, P})
            CHECK(hs_mcmc_workspace_bytes(P, n) == align256(8 * P) + align256(16 * ((P + 255) / 256 + 1)) + align256(4 * P) + align256(4 * n));
    REJECTS(hs_mcmc_workspace_bytes(-1, 0), "P=-1");
    REJECTS(hs_mcmc_workspace_bytes(1ll << 30, 0), "P=1073741824");
    REJECTS(hs_mcmc_workspace_bytes(10, -1), "n_draws=-1");
    REJECTS(hs_mcmc_workspace_bytes(10, 1ll << 30), "n_draws=1073741824");

    char* fake = reinterpret_cast<char*>(4096);  // never dereferenced on the host
    hs_densify_matrix mats[HS_DENSIFY_MAX_MATRICES + 1];
    for (auto& m : mats) { m.src = nullptr; m.dst = (float*)fake; m.row_stride = 3; m.role = HS_DENSIFY_COPY; m.reserved = 0; }
    hs_mcmc_args good;
    std::memset(&good, 0, sizeof good);
    good.P = 100; good.n_draws = 100; good.mode = HS_MCMC_RELOCATE; good.flags = 3;
    good.o_min = -5.3f; good.min_opacity = 0.005;
    good.opacities = (float*)fake; good.scales = (float*)fake; good.u = (const int64_t*)fake; good.workspace = fake;
    good.row_map = (uint32_t*)fake; good.counts = (uint32_t*)fake; good.counts_host = nullptr;
    good.matrices = mats; good.n_matrices = 15;

    REJECTS(hs_mcmc_sample(nullptr, nullptr), "null args");
    REJECTS(hs_mcmc_update(nullptr, nullptr), "null args");
    REJECTS(hs_mcmc_noise(nullptr, nullptr), "null args");
    for (int which = 0; which < 2; ++which) {
        auto call = [&](const hs_mcmc_args& a) { return which ? hs_mcmc_update(&a, nullptr) : hs_mcmc_sample(&a, nullptr); };
        hs_mcmc_args a = good;
        a.P = -1; REJECTS(call(a), "P=-1");
        a = good; a.P = 1ll << 30; REJECTS(call(a), "P=1073741824");
        a = good; a.mode = 2; REJECTS(call(a), "mode=2");
        a = good; a.flags = 4; REJECTS(call(a), "flags=4");
        a = good; a.n_draws = 99; REJECTS(call(a), "n_draws=99");
        a = good; a.mode = HS_MCMC_GROW; a.n_draws = 101; REJECTS(call(a), "n_draws=101");
        a = good; a.mode = HS_MCMC_GROW; a.n_draws = -1; REJECTS(call(a), "n_draws=-1");
        a = good; a.workspace = nullptr; REJECTS(call(a), "null workspace");
        a = good; a.workspace = fake + 8; REJECTS(call(a), "workspace must be 16-byte aligned");
        a = good; a.opacities = nullptr; REJECTS(call(a), "null opacities");
        a = good; a.opacities = (float*)(fake + 2); REJECTS(call(a), "opacities must be 4-byte aligned");
    }
    {
        hs_mcmc_args a = good;
        a.o_min = NAN; REJECTS(hs_mcmc_sample(&a, nullptr), "o_min is NaN");
        a = good; a.counts = nullptr; REJECTS(hs_mcmc_sample(&a, nullptr), "null counts");
        a = good; a.counts = (uint32_t*)(fake + 2); REJECTS(hs_mcmc_sample(&a, nullptr), "counts must be 4-byte aligned");
        a = good; a.counts_host = (uint32_t*)(fake + 1); REJECTS(hs_mcmc_sample(&a, nullptr), "counts_host must be 4-byte aligned");
        a = good; a.u = nullptr; REJECTS(hs_mcmc_sample(&a, nullptr), "null u");
        a = good; a.u = (const int64_t*)(fake + 4); REJECTS(hs_mcmc_sample(&a, nullptr), "u must be 8-byte aligned");
        a = good; a.mode = HS_MCMC_GROW; a.n_draws = 5; a.row_map = nullptr; REJECTS(hs_mcmc_sample(&a, nullptr), "null row_map");
        a = good; a.min_opacity = -0.1; REJECTS(hs_mcmc_update(&a, nullptr), "min_opacity=-0.1");
        a = good; a.min_opacity = NAN; REJECTS(hs_mcmc_update(&a, nullptr), "min_opacity=");
        a = good; a.scales = nullptr; REJECTS(hs_mcmc_update(&a, nullptr), "null scales");
        a = good; a.n_matrices = -1; REJECTS(hs_mcmc_update(&a, nullptr), "n_matrices=-1");
        a = good; a.n_matrices = 17; REJECTS(hs_mcmc_update(&a, nullptr), "n_matrices=17");
        a = good; a.matrices = nullptr; REJECTS(hs_mcmc_update(&a, nullptr), "null matrices");
        mats[3].role = HS_DENSIFY_MEANS; REJECTS(hs_mcmc_update(&good, nullptr), "matrices[3].role=2");
        mats[3].role = HS_DENSIFY_ZERO_NEW; mats[3].row_stride = 0; REJECTS(hs_mcmc_update(&good, nullptr), "matrices[3].row_stride=0");
        mats[3].row_stride = 1ll << 36; REJECTS(hs_mcmc_update(&good, nullptr), "reaches 2^40");
        mats[3].row_stride = 3; mats[3].dst = nullptr; REJECTS(hs_mcmc_update(&good, nullptr), "matrices[3]: null dst");
        mats[3].dst = (float*)(fake + 2); REJECTS(hs_mcmc_update(&good, nullptr), "matrices[3]: dst must be 4-byte aligned");
        mats[3].dst = (float*)fake; mats[3].src = (const float*)(fake + 64); REJECTS(hs_mcmc_update(&good, nullptr), "matrices[3]: src must be NULL or dst");
        mats[3].src = nullptr;
        // an empty cloud: the update has nothing to do and looks at no pointer
        a = good; a.P = 0; a.n_draws = 0; a.opacities = nullptr; a.scales = nullptr; a.workspace = nullptr;
        CHECK(hs_mcmc_update(&a, nullptr) == HS_OK);
    }
    {
        hs_mcmc_noise_args n;
        std::memset(&n, 0, sizeof n);
        n.P = 100; n.flags = 3; n.scaler = 80.f;
        n.means3D = (float*)fake; n.opacities = n.scales = n.rotations = n.xi = (const float*)fake;
        hs_mcmc_noise_args b = n;
        b.P = -1; REJECTS(hs_mcmc_noise(&b, nullptr), "P=-1");
        b = n; b.P = 1ll << 30; REJECTS(hs_mcmc_noise(&b, nullptr), "P=1073741824");
        b = n; b.flags = 8; REJECTS(hs_mcmc_noise(&b, nullptr), "flags=8");
        b = n; b.scaler = INFINITY; REJECTS(hs_mcmc_noise(&b, nullptr), "scaler=inf");
        b = n; b.scaler = NAN; REJECTS(hs_mcmc_noise(&b, nullptr), "scaler=");
        b = n; b.means3D = nullptr; REJECTS(hs_mcmc_noise(&b, nullptr), "null means3D");
        b = n; b.opacities = nullptr; REJECTS(hs_mcmc_noise(&b, nullptr), "null opacities");
        b = n; b.scales = nullptr; REJECTS(hs_mcmc_noise(&b, nullptr), "null scales");
        b = n; b.rotations = nullptr; REJECTS(hs_mcmc_noise(&b, nullptr), "null rotations");
        b = n; b.xi = (const float*)(fake + 2); REJECTS(hs_mcmc_noise(&b, nullptr), "xi must be 4-byte aligned");
        b = n; b.P = 0; b.means3D = nullptr; CHECK(hs_mcmc_noise(&b, nullptr) == HS_OK);
    }
    return 0;
}

int main() {
    // the error text is thread-local: two threads validating at once must not trample each other's message
    int rc[2] = {1, 1};
    std::thread t0([&] { rc[0] = run(); }), t1([&] { rc[1] = run(); });
    t0.join();
    t1.join();
    if (rc[0] || rc[1]) return 1;
    std::puts("mcmc_host: clean");
    return 0;
}
