// Host-side sanitizer driver of the lens undistortion (hs_undistort_map, hs_undistort_remap): every argument check of both entry
// points, with AddressSanitizer + UBSan on the host objects of libhdrsplat (built and run by
// `make -C casualhdrsplat_amd/csrc asan`, beside asan_host.cpp).  No GPU is needed or touched: every call here returns before
// its first HIP call.  Exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "hdrsplat.h"

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) { std::fprintf(stderr, "FAILED: %s (line %d): %s\n", #cond, __LINE__, hs_last_error()); return 1; } \
    } while (0)
#define REJECTS(call, text) CHECK((call) == HS_EINVAL && std::strstr(hs_last_error(), text))

static int run() {
    CHECK(hs_version() == HS_VERSION);
    char* fake = reinterpret_cast<char*>(4096);  // never dereferenced on the host
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    hs_undistort_args good;
    std::memset(&good, 0, sizeof good);
    good.model = HS_CAMERA_OPENCV;
    good.W = 97; good.H = 61; good.Wf = 96; good.Hf = 56; good.F = 3; good.factor = 2; good.frames_u8 = 1;
    good.fx = 80.f; good.fy = 78.f; good.cx = 50.3f; good.cy = 29.1f;
    good.k[0] = -0.1f; good.k[1] = 0.03f; good.k[2] = 0.004f; good.k[3] = -0.003f;
    good.map = reinterpret_cast<float*>(fake);
    good.valid = reinterpret_cast<uint8_t*>(fake);
    good.frames = fake;
    good.out = reinterpret_cast<float*>(fake);

    REJECTS(hs_undistort_map(nullptr, nullptr), "null args");
    REJECTS(hs_undistort_remap(nullptr, nullptr), "null args");
    int (*const fns[2])(const hs_undistort_args*, void*) = {hs_undistort_map, hs_undistort_remap};
    for (int f = 0; f < 2; ++f) {
        hs_undistort_args a = good;
        a.W = 1; REJECTS(fns[f](&a, nullptr), "W=1");
        a = good; a.H = 0; REJECTS(fns[f](&a, nullptr), "H=0");
        a = good; a.W = 16385; REJECTS(fns[f](&a, nullptr), "W=16385");
        a = good; a.H = 16385; REJECTS(fns[f](&a, nullptr), "H=16385");
        a = good; a.Wf = -2; REJECTS(fns[f](&a, nullptr), "Wf=-2");
        a = good; a.Hf = 16386; REJECTS(fns[f](&a, nullptr), "Hf=16386");
        a = good; a.map = nullptr; REJECTS(fns[f](&a, nullptr), "null map");
        a = good; a.map = reinterpret_cast<float*>(fake + 4); REJECTS(fns[f](&a, nullptr), "map must be 8-byte aligned");
        // an empty grid: nothing to do, with or without pointers
        a = good; a.Wf = 0; CHECK(fns[f](&a, nullptr) == HS_OK);
        a = good; a.Hf = 0; a.map = nullptr; a.valid = nullptr; a.frames = nullptr; a.out = nullptr; CHECK(fns[f](&a, nullptr) == HS_OK);
    }
    hs_undistort_args a = good;
    a.model = -1; REJECTS(hs_undistort_map(&a, nullptr), "model=-1");
    a = good; a.model = 7; REJECTS(hs_undistort_map(&a, nullptr), "model=7");
    a = good; a.fx = 0.f; REJECTS(hs_undistort_map(&a, nullptr), "fx=0");
    a = good; a.fy = -1.f; REJECTS(hs_undistort_map(&a, nullptr), "fy=-1");
    a = good; a.fx = nan; REJECTS(hs_undistort_map(&a, nullptr), "fx=nan");
    a = good; a.fy = inf; REJECTS(hs_undistort_map(&a, nullptr), "fy=inf");
    a = good; a.cx = nan; REJECTS(hs_undistort_map(&a, nullptr), "cx=nan");
    a = good; a.cy = -inf; REJECTS(hs_undistort_map(&a, nullptr), "cy=-inf");
    for (int i = 0; i < 8; ++i) {
        char text[16];
        std::snprintf(text, sizeof text, "k[%d]=nan", i);
        a = good; a.k[i] = nan; REJECTS(hs_undistort_map(&a, nullptr), text);
    }
    a = good; a.valid = nullptr; REJECTS(hs_undistort_map(&a, nullptr), "null valid");
    for (int m = HS_CAMERA_SIMPLE_PINHOLE; m <= HS_CAMERA_FULL_OPENCV; ++m) {   // every model passes the checks up to the pointers
        a = good; a.model = m; a.map = nullptr; REJECTS(hs_undistort_map(&a, nullptr), "null map");
    }

    const int bad_factors[] = {0, -1, 5, 6, 7, 9, 16};
    for (int s : bad_factors) { a = good; a.factor = s; REJECTS(hs_undistort_remap(&a, nullptr), "factor="); }
    const int factors[] = {1, 2, 3, 4, 8};
    for (int s : factors) {                                                    // every factor passes, up to the pointers
        a = good; a.factor = s; a.Wf = 24 * 4; a.Hf = 24 * 2; a.out = nullptr; REJECTS(hs_undistort_remap(&a, nullptr), "null out");
    }
    a = good; a.Wf = 97; REJECTS(hs_undistort_remap(&a, nullptr), "multiples of factor=2");
    a = good; a.factor = 3; REJECTS(hs_undistort_remap(&a, nullptr), "multiples of factor=3");
    a = good; a.F = -1; REJECTS(hs_undistort_remap(&a, nullptr), "F=-1");
    a = good; a.F = 2147483647; REJECTS(hs_undistort_remap(&a, nullptr), "2^31");             // (no overflow on the way)
    a = good; a.F = 120979; REJECTS(hs_undistort_remap(&a, nullptr), "2^31");                 // 3 F 61 97 >= 2^31 ...
    a = good; a.F = 120978; a.out = nullptr; REJECTS(hs_undistort_remap(&a, nullptr), "null out");   // ... and just below
    a = good; a.W = 2; a.H = 2; a.factor = 1; a.Wf = 4096; a.Hf = 4096; a.F = 43; REJECTS(hs_undistort_remap(&a, nullptr), "2^31");
    a = good; a.W = 16384; a.H = 16384; a.Wf = 16384; a.Hf = 16384; a.factor = 8; a.F = 2; a.frames = nullptr;
    REJECTS(hs_undistort_remap(&a, nullptr), "null frames");
    a = good; a.out = reinterpret_cast<float*>(fake + 2); REJECTS(hs_undistort_remap(&a, nullptr), "out must be 4-byte aligned");
    a = good; a.frames = fake + 1; a.out = nullptr; REJECTS(hs_undistort_remap(&a, nullptr), "null out");   // uint8 frames: any byte
    a = good; a.frames_u8 = 0; a.frames = fake + 1; REJECTS(hs_undistort_remap(&a, nullptr), "frames must be 4-byte aligned");
    // no frames: nothing to do
    a = good; a.F = 0; CHECK(hs_undistort_remap(&a, nullptr) == HS_OK);
    a = good; a.F = 0; a.frames = nullptr; a.out = nullptr; a.map = nullptr; CHECK(hs_undistort_remap(&a, nullptr) == HS_OK);
    a = good; a.F = 0; a.out = reinterpret_cast<float*>(fake + 2); REJECTS(hs_undistort_remap(&a, nullptr), "out must be 4-byte aligned");
    return 0;
}

int main() {
    const int rc = run();
    std::printf(rc == 0 ? "undistort_host: ok\n" : "undistort_host: FAILED\n");
    return rc;
}
