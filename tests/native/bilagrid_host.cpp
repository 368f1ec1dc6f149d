// Host-side sanitizer driver of the bilateral-grid correction (hs_bilagrid_workspace_bytes, hs_bilagrid_slice,
// hs_bilagrid_slice_backward, hs_bilagrid_tv, hs_bilagrid_tv_backward): their argument validation and the workspace
// arithmetic, with AddressSanitizer + UBSan on the host objects of libhdrsplat (built and run by
// `make -C casualhdrsplat_amd/csrc asan`, beside asan_host.cpp).  No GPU is needed or touched: every call here returns before
// its first HIP call.  Exit code 0 = clean.
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

// the chunk count as hdrsplat.h states it
static int64_t chunks(int64_t H, int64_t Y) {
    int64_t tallest = 1;
    for (int64_t yy = 0; yy < Y; ++yy) {
        int64_t lo = 0, hi = H - 1;
        if (Y > 1) {
            const int64_t m = 2 + (H >> 20);
            const int64_t a = yy == 0 ? 0 : ((yy - 1) * H) / (Y - 1) - m, b = ((yy + 1) * H + Y - 2) / (Y - 1) + m;
            lo = a > 0 ? a : 0;
            hi = b < H - 1 ? b : H - 1;
        }
        if (hi - lo + 1 > tallest) tallest = hi - lo + 1;
    }
    return (tallest + 31) / 32;
}

static int run() {
    CHECK(hs_version() == HS_VERSION);
    const int32_t shapes[][7] = {{1, 1080, 1920, 1, 8, 16, 16}, {4, 208, 320, 4, 8, 16, 16}, {1, 37, 70, 1, 5, 3, 4},
                                 {2, 33, 65, 2, 1, 1, 1},       {3, 1, 1, 2, 16, 64, 64},    {1, 100000, 7, 1, 1, 64, 1},
                                 {1, 32768, 21845, 1, 1, 1, 1}, {1, 4, 4, 2730, 16, 64, 64}, {1, 715827882, 1, 1, 2, 64, 2}};
    for (const auto& s : shapes)
        CHECK(hs_bilagrid_workspace_bytes(s[0], s[1], s[2], s[3], s[4], s[5], s[6]) ==
              align256(4ll * s[0] * chunks(s[1], s[5]) * 12 * s[4] * s[5] * s[6]));
    REJECTS(hs_bilagrid_workspace_bytes(0, 40, 72, 3, 4, 3, 4), "F=0");
    REJECTS(hs_bilagrid_workspace_bytes(2, -5, 72, 3, 4, 3, 4), "H=-5");
    REJECTS(hs_bilagrid_workspace_bytes(2, 40, 0, 3, 4, 3, 4), "W=0");
    REJECTS(hs_bilagrid_workspace_bytes(2, 40, 72, 0, 4, 3, 4), "G=0");
    REJECTS(hs_bilagrid_workspace_bytes(2, 40, 72, 3, 0, 3, 4), "L=0");
    REJECTS(hs_bilagrid_workspace_bytes(2, 40, 72, 3, 17, 3, 4), "L=17");
    REJECTS(hs_bilagrid_workspace_bytes(2, 40, 72, 3, 4, 65, 4), "Y=65");
    REJECTS(hs_bilagrid_workspace_bytes(2, 40, 72, 3, 4, 3, 0), "X=0");
    REJECTS(hs_bilagrid_workspace_bytes(1, 32768, 21846, 3, 4, 3, 4), "3*F*H*W=");
    REJECTS(hs_bilagrid_workspace_bytes(2147483647, 2147483647, 2147483647, 3, 4, 3, 4), "3*F*H*W=");
    REJECTS(hs_bilagrid_workspace_bytes(2, 40, 72, 2731, 16, 64, 64), "12*G*L*Y*X=");
    REJECTS(hs_bilagrid_workspace_bytes(2, 40, 72, 2147483647, 16, 64, 64), "12*G*L*Y*X=");

    char* fake = reinterpret_cast<char*>(4096);  // never dereferenced on the host
    hs_bilagrid_args good;
    std::memset(&good, 0, sizeof good);
    good.F = 2; good.H = 40; good.W = 72; good.G = 3; good.L = 4; good.Y = 3; good.X = 4;
    good.image = (const float*)fake; good.grids = (const float*)fake; good.grid_ids = (const int32_t*)fake;
    good.out = (float*)fake; good.dL_dout = (const float*)fake; good.dL_dimage = (float*)fake; good.dL_dgrids = (float*)fake;
    good.workspace = fake;

    int (*const fns[2])(const hs_bilagrid_args*, void*) = {hs_bilagrid_slice, hs_bilagrid_slice_backward};
    for (int k = 0; k < 2; ++k) {
        REJECTS(fns[k](nullptr, nullptr), "null args");
        hs_bilagrid_args a = good;
        a.F = 0; REJECTS(fns[k](&a, nullptr), "F=0");
        a = good; a.H = 0; REJECTS(fns[k](&a, nullptr), "H=0");
        a = good; a.W = -1; REJECTS(fns[k](&a, nullptr), "W=-1");
        a = good; a.G = 0; REJECTS(fns[k](&a, nullptr), "G=0");
        a = good; a.L = 17; REJECTS(fns[k](&a, nullptr), "L=17");
        a = good; a.Y = 0; REJECTS(fns[k](&a, nullptr), "Y=0");
        a = good; a.X = 65; REJECTS(fns[k](&a, nullptr), "X=65");
        a = good; a.H = 32768; a.W = 21846; a.F = 1; REJECTS(fns[k](&a, nullptr), "3*F*H*W=");
        a = good; a.G = 2731; a.L = 16; a.Y = 64; a.X = 64; REJECTS(fns[k](&a, nullptr), "12*G*L*Y*X=");
        a = good; a.image = nullptr; REJECTS(fns[k](&a, nullptr), "null image");
        a = good; a.grids = nullptr; REJECTS(fns[k](&a, nullptr), "null grids");
        a = good; a.grid_ids = nullptr; REJECTS(fns[k](&a, nullptr), "null grid_ids");
        a = good; a.image = (const float*)(fake + 2); REJECTS(fns[k](&a, nullptr), "image must be 4-byte aligned");
        a = good; a.grids = (const float*)(fake + 1); REJECTS(fns[k](&a, nullptr), "grids must be 4-byte aligned");
        a = good; a.grid_ids = (const int32_t*)(fake + 2); REJECTS(fns[k](&a, nullptr), "grid_ids must be 4-byte aligned");
    }
    hs_bilagrid_args a = good;
    a.out = nullptr; REJECTS(hs_bilagrid_slice(&a, nullptr), "null out");
    a = good; a.out = (float*)(fake + 2); REJECTS(hs_bilagrid_slice(&a, nullptr), "out must be 4-byte aligned");
    a = good; a.dL_dout = nullptr; REJECTS(hs_bilagrid_slice_backward(&a, nullptr), "null dL_dout");
    a = good; a.dL_dout = (const float*)(fake + 3); REJECTS(hs_bilagrid_slice_backward(&a, nullptr), "dL_dout must be 4-byte aligned");
    a = good; a.dL_dimage = (float*)(fake + 2); REJECTS(hs_bilagrid_slice_backward(&a, nullptr), "dL_dimage must be 4-byte aligned");
    a = good; a.dL_dgrids = (float*)(fake + 2); REJECTS(hs_bilagrid_slice_backward(&a, nullptr), "dL_dgrids must be 4-byte aligned");
    a = good; a.workspace = nullptr; REJECTS(hs_bilagrid_slice_backward(&a, nullptr), "null workspace");
    a = good; a.workspace = fake + 128; REJECTS(hs_bilagrid_slice_backward(&a, nullptr), "workspace must be 256-byte aligned");
    // neither gradient asked for: nothing to do, nothing is launched
    a = good; a.dL_dimage = nullptr; a.dL_dgrids = nullptr; a.workspace = nullptr;
    CHECK(hs_bilagrid_slice_backward(&a, nullptr) == HS_OK);

    hs_bilagrid_tv_args tgood;
    std::memset(&tgood, 0, sizeof tgood);
    tgood.G = 3; tgood.L = 4; tgood.Y = 3; tgood.X = 4;
    tgood.grids = (const float*)fake; tgood.tv = (float*)fake; tgood.dL_dtv = (const float*)fake; tgood.dL_dgrids = (float*)fake;
    tgood.workspace = fake;
    int (*const tfns[2])(const hs_bilagrid_tv_args*, void*) = {hs_bilagrid_tv, hs_bilagrid_tv_backward};
    for (int k = 0; k < 2; ++k) {
        REJECTS(tfns[k](nullptr, nullptr), "null args");
        hs_bilagrid_tv_args t = tgood;
        t.G = 0; REJECTS(tfns[k](&t, nullptr), "G=0");
        t = tgood; t.L = 0; REJECTS(tfns[k](&t, nullptr), "L=0");
        t = tgood; t.L = 17; REJECTS(tfns[k](&t, nullptr), "L=17");
        t = tgood; t.Y = 65; REJECTS(tfns[k](&t, nullptr), "Y=65");
        t = tgood; t.X = 0; REJECTS(tfns[k](&t, nullptr), "X=0");
        t = tgood; t.G = 2731; t.L = 16; t.Y = 64; t.X = 64; REJECTS(tfns[k](&t, nullptr), "12*G*L*Y*X=");
        t = tgood; t.grids = nullptr; REJECTS(tfns[k](&t, nullptr), "null grids");
        t = tgood; t.grids = (const float*)(fake + 2); REJECTS(tfns[k](&t, nullptr), "grids must be 4-byte aligned");
    }
    hs_bilagrid_tv_args t = tgood;
    t.tv = nullptr; REJECTS(hs_bilagrid_tv(&t, nullptr), "null tv");
    t = tgood; t.workspace = nullptr; REJECTS(hs_bilagrid_tv(&t, nullptr), "null workspace");
    t = tgood; t.workspace = fake + 16; REJECTS(hs_bilagrid_tv(&t, nullptr), "workspace must be 256-byte aligned");
    t = tgood; t.dL_dtv = nullptr; REJECTS(hs_bilagrid_tv_backward(&t, nullptr), "null dL_dtv");
    t = tgood; t.dL_dgrids = nullptr; REJECTS(hs_bilagrid_tv_backward(&t, nullptr), "null dL_dgrids");
    t = tgood; t.dL_dgrids = (float*)(fake + 1); REJECTS(hs_bilagrid_tv_backward(&t, nullptr), "dL_dgrids must be 4-byte aligned");
    return 0;
}

int main() {
    // the error text is thread-local: two threads validating at once must not trample each other's message
    int rc[2] = {1, 1};
    std::thread t0([&] { rc[0] = run(); }), t1([&] { rc[1] = run(); });
    t0.join();
    t1.join();
    if (rc[0] || rc[1]) return 1;
    std::puts("bilagrid_host: clean");
    return 0;
}
