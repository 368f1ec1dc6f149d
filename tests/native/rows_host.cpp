// Host-side sanitizer driver of the score-driven row plans (hs_rows_workspace_bytes, hs_rows_plan): their argument validation
// and the workspace arithmetic, with AddressSanitizer + UBSan on the host objects of libhdrsplat (built and run by
// `make -C casualhdrsplat_amd/csrc asan`, beside asan_host.cpp, mcmc_host.cpp, mcmc_reg_host.cpp and smoothing_host.cpp).  No
// GPU is needed or touched: every call here returns before its first HIP call.  Exit code 0 = clean.
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
    const int64_t Ps[] = {0, 1, 255, 256, 257, 4096, 4097, 10007, 65536, 65537, 1000000, (1ll << 30) - 1};
    int64_t last = 0;
    for (int64_t P : Ps) {
        const int64_t b = hs_rows_workspace_bytes(P);
        CHECK(b == align256(P) + align256(16 * ((P + 255) / 256)) + 263424 && b % 16 == 0 && b > 0 && b >= last);
        last = b;
    }
    REJECTS(hs_rows_workspace_bytes(-1), "P=-1");
    REJECTS(hs_rows_workspace_bytes(1ll << 30), "P=1073741824");

    char* fake = reinterpret_cast<char*>(4096);  // never dereferenced on the host
    hs_rows_args good;
    std::memset(&good, 0, sizeof good);
    good.P = 100; good.k = 10; good.mode = HS_ROWS_KEEP;
    good.score = (const float*)fake; good.mask = (const uint8_t*)fake; good.scales = (const float*)fake;
    good.workspace = fake; good.row_map = (uint32_t*)fake; good.counts = (uint32_t*)fake; good.counts_host = (uint32_t*)fake;
    REJECTS(hs_rows_plan(nullptr, nullptr), "hs_rows_plan: null args");
    hs_rows_args a = good;
    a.P = -1; REJECTS(hs_rows_plan(&a, nullptr), "P=-1");
    a = good; a.P = 1ll << 30; REJECTS(hs_rows_plan(&a, nullptr), "P=1073741824");
    a = good; a.k = -1; REJECTS(hs_rows_plan(&a, nullptr), "k=-1");
    a = good; a.k = 101; REJECTS(hs_rows_plan(&a, nullptr), "k=101");
    a = good; a.mode = 3; REJECTS(hs_rows_plan(&a, nullptr), "mode=3");
    a = good; a.mode = -1; REJECTS(hs_rows_plan(&a, nullptr), "mode=-1");
    a = good; a.flags = HS_DENSIFY_RAW_OPACITY; REJECTS(hs_rows_plan(&a, nullptr), "flags=1");
    a = good; a.flags = 8; REJECTS(hs_rows_plan(&a, nullptr), "flags=8");
    a = good; a.mode = HS_ROWS_DENSIFY; a.tau_split = NAN; REJECTS(hs_rows_plan(&a, nullptr), "tau_split is NaN");
    a = good; a.counts = nullptr; REJECTS(hs_rows_plan(&a, nullptr), "null counts");
    a = good; a.counts = (uint32_t*)(fake + 2); REJECTS(hs_rows_plan(&a, nullptr), "counts must be 4-byte aligned");
    a = good; a.counts_host = (uint32_t*)(fake + 1); REJECTS(hs_rows_plan(&a, nullptr), "counts_host must be 4-byte aligned");
    a = good; a.row_map = nullptr; REJECTS(hs_rows_plan(&a, nullptr), "null row_map");
    a = good; a.row_map = (uint32_t*)(fake + 3); REJECTS(hs_rows_plan(&a, nullptr), "row_map must be 4-byte aligned");
    a = good; a.workspace = nullptr; REJECTS(hs_rows_plan(&a, nullptr), "null workspace");
    a = good; a.workspace = fake + 4; REJECTS(hs_rows_plan(&a, nullptr), "workspace must be 16-byte aligned");
    a = good; a.score = nullptr; REJECTS(hs_rows_plan(&a, nullptr), "null score");
    a = good; a.score = (const float*)(fake + 2); REJECTS(hs_rows_plan(&a, nullptr), "score must be 4-byte aligned");
    a = good; a.mode = HS_ROWS_DENSIFY; a.scales = nullptr; REJECTS(hs_rows_plan(&a, nullptr), "null scales");
    a = good; a.mode = HS_ROWS_DENSIFY; a.scales = (const float*)(fake + 1); REJECTS(hs_rows_plan(&a, nullptr), "scales must be 4-byte aligned");
    a = good; a.mode = HS_ROWS_DENSIFY; a.score = nullptr; REJECTS(hs_rows_plan(&a, nullptr), "null score");
    a = good; a.mode = HS_ROWS_MASK; a.k = 0; a.mask = nullptr; REJECTS(hs_rows_plan(&a, nullptr), "null mask");
    // an empty cloud: no data pointer is looked at; k must still lie in [0, P], and counts is written, so it must be there
    std::memset(&a, 0, sizeof a);
    a.k = 1; REJECTS(hs_rows_plan(&a, nullptr), "k=1");
    a.k = 0; REJECTS(hs_rows_plan(&a, nullptr), "null counts");
    return 0;
}

int main() {
    // the error text is thread-local: two threads validating at once must not trample each other's message
    int rc[2] = {1, 1};
    std::thread t0([&] { rc[0] = run(); }), t1([&] { rc[1] = run(); });
    t0.join();
    t1.join();
    if (rc[0] || rc[1]) return 1;
    std::puts("rows_host: clean");
    return 0;
}
