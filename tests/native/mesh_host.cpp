// Host-side sanitizer driver of the mesh clean-up by connected components (hs_mesh_workspace_bytes, hs_mesh_components,
// hs_mesh_clean_plan, hs_mesh_clean_emit): every argument check of the four entry points, with AddressSanitizer + UBSan on the host
// objects of libhdrsplat (built and run by `make -C casualhdrsplat_amd/csrc asan`, beside asan_host.cpp).  No GPU is needed or
// touched: every call here returns before its first HIP call.  Exit code 0 = clean.
#include <cstdio>
#include <cstring>

#include "hdrsplat.h"

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) { std::fprintf(stderr, "FAILED: %s (line %d): %s\n", #cond, __LINE__, hs_last_error()); return 1; } \
    } while (0)
#define REJECTS(call, text) CHECK((call) == HS_EINVAL && std::strstr(hs_last_error(), text))

static int run() {
    CHECK(hs_version() == HS_VERSION);
    char* fake = reinterpret_cast<char*>(4096);  // never dereferenced on the host
    float* ff = reinterpret_cast<float*>(fake);
    int32_t* fi = reinterpret_cast<int32_t*>(fake);
    hs_mesh_args good;
    std::memset(&good, 0, sizeof good);
    good.n_vertices = 100; good.n_faces = 200; good.min_faces = 3; good.keep_largest = 2; good.remove_degenerate = 1;
    good.vertices = ff; good.faces = fi; good.colors = ff; good.workspace = fake; good.label = fi; good.size = fi;
    good.totals = reinterpret_cast<int64_t*>(fake);
    good.n_vertices_out = 10; good.n_faces_out = 20;
    good.vertices_out = ff; good.faces_out = fi; good.colors_out = ff; good.vertex_index = fi; good.face_index = fi;

    // the workspace's size: 3 r(4 V) + r(4 T) + r(8 ceil(V / 256)) + r(8 ceil(T / 256)) + 8256
    CHECK(hs_mesh_workspace_bytes(0, 0) == 8256);
    CHECK(hs_mesh_workspace_bytes(3, 7) == 3 * 16 + 32 + 16 + 16 + 8256);
    CHECK(hs_mesh_workspace_bytes(257, 513) == 3 * 1040 + 2064 + 16 + 32 + 8256);
    const int64_t top = (1ll << 31) - 1;
    CHECK(hs_mesh_workspace_bytes(top, top) == 4 * (1ll << 33) + 2 * (1ll << 26) + 8256);
    REJECTS(hs_mesh_workspace_bytes(-1, 5), "n_vertices=-1");
    REJECTS(hs_mesh_workspace_bytes(5, -1), "n_faces=-1");
    REJECTS(hs_mesh_workspace_bytes(1ll << 31, 5), "2^31");
    REJECTS(hs_mesh_workspace_bytes(5, 1ll << 31), "2^31");
    REJECTS(hs_mesh_workspace_bytes(1ll << 62, 1ll << 62), "2^31");   // (no overflow on the way)
    CHECK(std::strstr(hs_last_error(), "hs_mesh_workspace_bytes:") == hs_last_error());

    int (*const fns[3])(const hs_mesh_args*, void*) = {hs_mesh_components, hs_mesh_clean_plan, hs_mesh_clean_emit};
    const char* names[3] = {"hs_mesh_components:", "hs_mesh_clean_plan:", "hs_mesh_clean_emit:"};
    for (int f = 0; f < 3; ++f) {
        REJECTS(fns[f](nullptr, nullptr), "null args");
        hs_mesh_args a = good;
        a.n_vertices = -1; REJECTS(fns[f](&a, nullptr), "n_vertices=-1");
        CHECK(std::strstr(hs_last_error(), names[f]) == hs_last_error());
        a = good; a.n_faces = -2; REJECTS(fns[f](&a, nullptr), "n_faces=-2");
        a = good; a.n_vertices = 1ll << 31; REJECTS(fns[f](&a, nullptr), "n_vertices=2147483648");
        a = good; a.n_faces = 1ll << 31; REJECTS(fns[f](&a, nullptr), "n_faces=2147483648");
        a = good; a.n_vertices = top; a.n_faces = top; a.workspace = nullptr; REJECTS(fns[f](&a, nullptr), "null workspace");   // the top passes
        a = good; a.faces = nullptr; REJECTS(fns[f](&a, nullptr), "null faces");
        a = good; a.faces = reinterpret_cast<int32_t*>(fake + 2); REJECTS(fns[f](&a, nullptr), "faces must be 4-byte aligned");
        a = good; a.n_faces = 0; a.faces = reinterpret_cast<int32_t*>(fake + 2); REJECTS(fns[f](&a, nullptr), "faces must be 4-byte aligned");
        a = good; a.workspace = nullptr; REJECTS(fns[f](&a, nullptr), "null workspace");
        a = good; a.workspace = fake + 8; REJECTS(fns[f](&a, nullptr), "workspace must be 16-byte aligned");
    }

    hs_mesh_args a = good;
    a.label = nullptr; REJECTS(hs_mesh_components(&a, nullptr), "null label");
    a = good; a.size = nullptr; REJECTS(hs_mesh_components(&a, nullptr), "null size");
    a = good; a.label = reinterpret_cast<int32_t*>(fake + 2); REJECTS(hs_mesh_components(&a, nullptr), "label must be 4-byte aligned");
    a = good; a.size = reinterpret_cast<int32_t*>(fake + 1); REJECTS(hs_mesh_components(&a, nullptr), "size must be 4-byte aligned");
    // no faces: nothing to do, with or without outputs; what components does not use is not looked at
    a = good; a.n_faces = 0; a.faces = nullptr; a.label = nullptr; a.size = nullptr; a.vertices = nullptr; a.totals = nullptr;
    a.min_faces = -1; a.remove_degenerate = 7; CHECK(hs_mesh_components(&a, nullptr) == HS_OK);

    a = good; a.min_faces = -1; REJECTS(hs_mesh_clean_plan(&a, nullptr), "min_faces=-1");
    a = good; a.keep_largest = -5; REJECTS(hs_mesh_clean_plan(&a, nullptr), "keep_largest=-5");
    a = good; a.remove_degenerate = 2; REJECTS(hs_mesh_clean_plan(&a, nullptr), "remove_degenerate=2");
    a = good; a.remove_degenerate = -1; REJECTS(hs_mesh_clean_plan(&a, nullptr), "remove_degenerate=-1");
    a = good; a.vertices = nullptr; REJECTS(hs_mesh_clean_plan(&a, nullptr), "null vertices");
    a = good; a.vertices = reinterpret_cast<float*>(fake + 2); REJECTS(hs_mesh_clean_plan(&a, nullptr), "vertices must be 4-byte aligned");
    a = good; a.totals = nullptr; REJECTS(hs_mesh_clean_plan(&a, nullptr), "null totals");
    a = good; a.totals = reinterpret_cast<int64_t*>(fake + 4); REJECTS(hs_mesh_clean_plan(&a, nullptr), "totals must be 8-byte aligned");
    // vertices are not needed without the degenerate test (the launch itself needs a GPU: the last check before it fails)
    a = good; a.remove_degenerate = 0; a.vertices = nullptr; a.totals = nullptr; REJECTS(hs_mesh_clean_plan(&a, nullptr), "null totals");

    a = good; a.n_vertices_out = -1; REJECTS(hs_mesh_clean_emit(&a, nullptr), "n_vertices_out=-1");
    a = good; a.n_vertices_out = 101; REJECTS(hs_mesh_clean_emit(&a, nullptr), "n_vertices_out=101");
    a = good; a.n_faces_out = -1; REJECTS(hs_mesh_clean_emit(&a, nullptr), "n_faces_out=-1");
    a = good; a.n_faces_out = 201; REJECTS(hs_mesh_clean_emit(&a, nullptr), "n_faces_out=201");
    a = good; a.vertices = nullptr; REJECTS(hs_mesh_clean_emit(&a, nullptr), "null vertices");
    a = good; a.vertices_out = nullptr; REJECTS(hs_mesh_clean_emit(&a, nullptr), "null vertices_out");
    a = good; a.faces_out = nullptr; REJECTS(hs_mesh_clean_emit(&a, nullptr), "null faces_out");
    a = good; a.colors = nullptr; REJECTS(hs_mesh_clean_emit(&a, nullptr), "colors_out given for a mesh without colours");
    a = good; a.colors_out = nullptr; REJECTS(hs_mesh_clean_emit(&a, nullptr), "the mesh has colours");
    a = good; a.vertices = reinterpret_cast<float*>(fake + 2); REJECTS(hs_mesh_clean_emit(&a, nullptr), "vertices must be 4-byte aligned");
    a = good; a.colors = reinterpret_cast<float*>(fake + 2); REJECTS(hs_mesh_clean_emit(&a, nullptr), "colors must be 4-byte aligned");
    a = good; a.vertices_out = reinterpret_cast<float*>(fake + 2); REJECTS(hs_mesh_clean_emit(&a, nullptr), "vertices_out must be 4-byte aligned");
    a = good; a.faces_out = reinterpret_cast<int32_t*>(fake + 2); REJECTS(hs_mesh_clean_emit(&a, nullptr), "faces_out must be 4-byte aligned");
    a = good; a.colors_out = reinterpret_cast<float*>(fake + 2); REJECTS(hs_mesh_clean_emit(&a, nullptr), "colors_out must be 4-byte aligned");
    a = good; a.vertex_index = reinterpret_cast<int32_t*>(fake + 2); REJECTS(hs_mesh_clean_emit(&a, nullptr), "vertex_index must be 4-byte aligned");
    a = good; a.face_index = reinterpret_cast<int32_t*>(fake + 1); REJECTS(hs_mesh_clean_emit(&a, nullptr), "face_index must be 4-byte aligned");
    // an empty result: nothing to do, with or without outputs
    a = good; a.n_vertices_out = 0; a.n_faces_out = 0; CHECK(hs_mesh_clean_emit(&a, nullptr) == HS_OK);
    a = good; a.n_vertices_out = 0; a.n_faces_out = 0; a.vertices = nullptr; a.vertices_out = nullptr; a.faces_out = nullptr;
    a.colors = nullptr; a.colors_out = nullptr; a.vertex_index = nullptr; a.face_index = nullptr; a.totals = nullptr;
    CHECK(hs_mesh_clean_emit(&a, nullptr) == HS_OK);
    a = good; a.n_vertices_out = 0; a.n_faces_out = 0; a.workspace = nullptr; REJECTS(hs_mesh_clean_emit(&a, nullptr), "null workspace");
    return 0;
}

int main() {
    const int rc = run();
    std::printf(rc == 0 ? "mesh_host: ok\n" : "mesh_host: FAILED\n");
    return rc;
}
