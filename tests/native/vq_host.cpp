// Host-side sanitizer driver of the k-means vector quantisation (hs_vq_workspace_bytes, hs_vq_assign, hs_vq_update): their
// argument validation and the workspace arithmetic, with AddressSanitizer + UBSan on the host objects of libhdrsplat (built
// and run by `make -C casualhdrsplat_amd/csrc asan`, beside asan_host.cpp).  No GPU is needed or touched: every call here
// returns before its first HIP call.  Exit code 0 = clean.
#include <cstdio>
#include <cstring>

#include "hdrsplat.h"

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) { std::fprintf(stderr, "FAILED: %s (line %d): %s\n", #cond, __LINE__, hs_last_error()); return 1; } \
    } while (0)
#define REJECTS(call, text) CHECK((call) == HS_EINVAL && std::strstr(hs_last_error(), text))

static int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// the workspace as DESIGN.md 4.26 states it
static int64_t workspace(int64_t N, int64_t D, int64_t K) {
    int64_t blocks = (N + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    int64_t S = (N + 1024 * K - 1) / (1024 * K);
    S = S < 1 ? 1 : S > 64 ? 64 : S;
    return align256(4 * blocks * K) + align256(4 * K) + align256(4 * N) + align256(8 * K * S * (D + 1));
}

static int run() {
    CHECK(hs_version() == HS_VERSION);
    const int32_t shapes[][3] = {{1 << 20, 45, 4096}, {100000, 9, 256}, {3001, 24, 65}, {1, 1, 1}, {70000, 45, 1},
                                 {1 << 30, 48, 65536}, {262145, 48, 65536}, {0, 45, 4096}, {255, 3, 9000}};
    for (const auto& s : shapes) CHECK(hs_vq_workspace_bytes(s[0], s[1], s[2]) == workspace(s[0], s[1], s[2]));
    int64_t last = 0;
    for (int32_t n = 0; n < 600000; n += 997) {   // never shrinks, also where the number of blocks steps
        const int64_t b = hs_vq_workspace_bytes(n, 48, 65536);
        CHECK(b >= last && b % 256 == 0 && b > 0);
        last = b;
    }
    REJECTS(hs_vq_workspace_bytes(-1, 8, 8), "N=-1");
    REJECTS(hs_vq_workspace_bytes((1 << 30) + 1, 8, 8), "N=1073741825");
    REJECTS(hs_vq_workspace_bytes(100, 0, 8), "D=0");
    REJECTS(hs_vq_workspace_bytes(100, 49, 8), "D=49");
    REJECTS(hs_vq_workspace_bytes(100, 8, 0), "K=0");
    REJECTS(hs_vq_workspace_bytes(100, 8, 65537), "K=65537");
    REJECTS(hs_vq_workspace_bytes(2147483647, 2147483647, 2147483647), "hs_vq_workspace_bytes");

    char* fake = reinterpret_cast<char*>(4096);  // never dereferenced on the host
    hs_vq_args good;
    std::memset(&good, 0, sizeof good);
    good.N = 1000; good.D = 45; good.K = 64;
    good.x = reinterpret_cast<const float*>(fake);
    good.weights = reinterpret_cast<const float*>(fake);
    good.codebook_in = reinterpret_cast<const float*>(fake);
    good.codes = reinterpret_cast<int32_t*>(fake);
    good.dist2 = reinterpret_cast<float*>(fake);
    good.codebook_out = reinterpret_cast<float*>(fake);
    good.counts = reinterpret_cast<int32_t*>(fake);
    good.workspace = fake;

    REJECTS(hs_vq_assign(nullptr, nullptr), "null args");
    REJECTS(hs_vq_update(nullptr, nullptr), "null args");
    int (*const fns[2])(const hs_vq_args*, void*) = {hs_vq_assign, hs_vq_update};
    for (int f = 0; f < 2; ++f) {
        hs_vq_args a = good;
        a.D = 49; REJECTS(fns[f](&a, nullptr), "D=49");
        a = good; a.K = 65537; REJECTS(fns[f](&a, nullptr), "K=65537");
        a = good; a.N = -3; REJECTS(fns[f](&a, nullptr), "N=-3");
        a = good; a.x = nullptr; REJECTS(fns[f](&a, nullptr), "null x");
        a = good; a.codes = nullptr; REJECTS(fns[f](&a, nullptr), "null codes");
        a = good; a.codebook_in = nullptr; REJECTS(fns[f](&a, nullptr), "null codebook_in");
        a = good; a.x = reinterpret_cast<const float*>(fake + 2); REJECTS(fns[f](&a, nullptr), "x must be 4-byte aligned");
    }
    hs_vq_args a = good;
    a.dist2 = reinterpret_cast<float*>(fake + 1); REJECTS(hs_vq_assign(&a, nullptr), "dist2 must be 4-byte aligned");
    a = good; a.codebook_out = nullptr; REJECTS(hs_vq_update(&a, nullptr), "null codebook_out");
    a = good; a.counts = nullptr; REJECTS(hs_vq_update(&a, nullptr), "null counts");
    a = good; a.workspace = nullptr; REJECTS(hs_vq_update(&a, nullptr), "null workspace");
    a = good; a.workspace = fake + 128; REJECTS(hs_vq_update(&a, nullptr), "workspace must be 256-byte aligned");
    a = good; a.weights = reinterpret_cast<const float*>(fake + 2); REJECTS(hs_vq_update(&a, nullptr), "weights must be 4-byte aligned");
    // no rows: the assignment has nothing to do and launches nothing
    a = good; a.N = 0; a.x = nullptr; a.codes = nullptr; a.dist2 = nullptr;
    CHECK(hs_vq_assign(&a, nullptr) == HS_OK);
    return 0;
}

int main() {
    const int rc = run();
    std::printf(rc == 0 ? "vq_host: ok\n" : "vq_host: FAILED\n");
    return rc;
}
