// Host-side sanitizer driver of the MCMC regularisers (hs_mcmc_reg_workspace_bytes, hs_mcmc_regularize): their argument
// validation and the workspace arithmetic, with AddressSanitizer + UBSan on the host objects of libhdrsplat (built and run by
// `make -C casualhdrsplat_amd/csrc asan`, beside asan_host.cpp and mcmc_host.cpp).  No GPU is needed or touched: every call
// here returns before its first HIP call.  Exit code 0 = clean.
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
    const int64_t Ps[] = {0, 1, 255, 256, 257, 4096, 4097, 10007, 1000000, (1ll << 30) - 1};
    for (int64_t P : Ps) CHECK(hs_mcmc_reg_workspace_bytes(P) == align256(16 * ((P + 255) / 256)));
    REJECTS(hs_mcmc_reg_workspace_bytes(-1), "P=-1");
    REJECTS(hs_mcmc_reg_workspace_bytes(1ll << 30), "P=1073741824");

    char* fake = reinterpret_cast<char*>(4096);  // never dereferenced on the host
    hs_mcmc_reg_args good;
    std::memset(&good, 0, sizeof good);
    good.P = 100; good.flags = 3; good.lambda_opacity = 0.01; good.lambda_scale = 0.01;
    good.opacities = (const float*)fake; good.scales = (const float*)fake;
    good.dL_dopacities = (float*)fake; good.dL_dscales = (float*)fake; good.loss = (float*)fake; good.workspace = fake;

    REJECTS(hs_mcmc_regularize(nullptr, nullptr), "null args");
    hs_mcmc_reg_args a = good;
    a.P = -1; REJECTS(hs_mcmc_regularize(&a, nullptr), "P=-1");
    a = good; a.P = 1ll << 30; REJECTS(hs_mcmc_regularize(&a, nullptr), "P=1073741824");
    a = good; a.flags = 4; REJECTS(hs_mcmc_regularize(&a, nullptr), "flags=4");
    a = good; a.flags = -1; REJECTS(hs_mcmc_regularize(&a, nullptr), "flags=-1");
    a = good; a.lambda_opacity = -0.01; REJECTS(hs_mcmc_regularize(&a, nullptr), "lambda_opacity=-0.01");
    a = good; a.lambda_opacity = NAN; REJECTS(hs_mcmc_regularize(&a, nullptr), "lambda_opacity=");
    a = good; a.lambda_opacity = INFINITY; REJECTS(hs_mcmc_regularize(&a, nullptr), "lambda_opacity=inf");
    a = good; a.lambda_scale = -1.0; REJECTS(hs_mcmc_regularize(&a, nullptr), "lambda_scale=-1");
    a = good; a.lambda_scale = NAN; REJECTS(hs_mcmc_regularize(&a, nullptr), "lambda_scale=");
    a = good; a.lambda_scale = INFINITY; REJECTS(hs_mcmc_regularize(&a, nullptr), "lambda_scale=inf");
    a = good; a.opacities = nullptr; REJECTS(hs_mcmc_regularize(&a, nullptr), "null opacities");
    a = good; a.scales = nullptr; REJECTS(hs_mcmc_regularize(&a, nullptr), "null scales");
    a = good; a.dL_dopacities = nullptr; REJECTS(hs_mcmc_regularize(&a, nullptr), "null dL_dopacities");
    a = good; a.dL_dscales = nullptr; REJECTS(hs_mcmc_regularize(&a, nullptr), "null dL_dscales");
    a = good; a.opacities = (const float*)(fake + 2); REJECTS(hs_mcmc_regularize(&a, nullptr), "opacities must be 4-byte aligned");
    a = good; a.scales = (const float*)(fake + 1); REJECTS(hs_mcmc_regularize(&a, nullptr), "scales must be 4-byte aligned");
    a = good; a.dL_dopacities = (float*)(fake + 2); REJECTS(hs_mcmc_regularize(&a, nullptr), "dL_dopacities must be 4-byte aligned");
    a = good; a.dL_dscales = (float*)(fake + 3); REJECTS(hs_mcmc_regularize(&a, nullptr), "dL_dscales must be 4-byte aligned");
    a = good; a.loss = (float*)(fake + 2); REJECTS(hs_mcmc_regularize(&a, nullptr), "loss must be 4-byte aligned");
    a = good; a.workspace = nullptr; REJECTS(hs_mcmc_regularize(&a, nullptr), "null workspace");
    a = good; a.workspace = fake + 8; REJECTS(hs_mcmc_regularize(&a, nullptr), "workspace must be 16-byte aligned");
    // a lambda of 0 frees its gradient array, not the values the loss is made of
    a = good; a.lambda_opacity = 0.0; a.dL_dopacities = nullptr; a.opacities = nullptr; REJECTS(hs_mcmc_regularize(&a, nullptr), "null opacities");
    a = good; a.lambda_scale = 0.0; a.dL_dscales = nullptr; a.scales = nullptr; REJECTS(hs_mcmc_regularize(&a, nullptr), "null scales");
    // nothing to do: no pointer is looked at and nothing is launched
    std::memset(&a, 0, sizeof a);
    CHECK(hs_mcmc_regularize(&a, nullptr) == HS_OK);                      // P == 0, no loss
    a = good; a.lambda_opacity = 0.0; a.lambda_scale = 0.0; a.loss = nullptr; a.workspace = nullptr;
    a.opacities = a.scales = nullptr; a.dL_dopacities = a.dL_dscales = nullptr;
    CHECK(hs_mcmc_regularize(&a, nullptr) == HS_OK);                      // both lambdas 0, no loss
    return 0;
}

int main() {
    // the error text is thread-local: two threads validating at once must not trample each other's message
    int rc[2] = {1, 1};
    std::thread t0([&] { rc[0] = run(); }), t1([&] { rc[1] = run(); });
    t0.join();
    t1.join();
    if (rc[0] || rc[1]) return 1;
    std::puts("mcmc_reg_host: clean");
    return 0;
}
