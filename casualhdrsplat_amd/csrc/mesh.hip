// Mesh clean-up by connected components: cluster the triangles of a mesh, keep the large clusters, drop degenerate faces and
// the vertices nothing references (hs_mesh_components, hs_mesh_clean_plan, hs_mesh_clean_emit; include/hdrsplat.h).  What
// tsdf.hip's extraction leaves raw: every floater of the cloud is a closed blob of its own next to the surface.
//
// No float arithmetic: integers, fp32 `==` on stored coordinates, and copies of 32-bit words.  Every result is exact and
// tests/mesh_reference.py restates the definitions (hdrsplat.h) sequentially.  On the exact side of the Makefile all the same.
//
// Atomics.  This unit uses INTEGER atomics at agent scope (compare-and-swap on `parent`, add on `size`): integer min and sum do
// not depend on the order of arrival, so the outputs are the same bits on every run.  Float atomics would not be, and are not
// acceptable here or anywhere else in the library's exact units.
//
// UNION-FIND over vertices.  parent[v] = v at the start; parent[x] <= x ALWAYS, and parent[x] < x once x is not a root: an index
// only ever hangs under a smaller one, so chains strictly descend -- no cycle can form and every walk ends after at most V steps.
//   find(x)       walks to the root; on the way x's link is moved to its grandparent (path halving, a plain store of an ancestor).
//   hook(a, b)    ra = find(a), rb = find(b); while they differ: compare-and-swap parent[hi] from hi to lo (hi, lo = the larger
//                 and the smaller root).  Only a ROOT has parent[hi] == hi, so only roots are ever hooked, and a halving store
//                 (which targets a non-root: once under another index, never a root again) cannot collide with a swap.  The
//                 swap fails only because another swap on the same word succeeded -- hi hangs under `seen` < hi now -- and the
//                 loop goes on from find(seen) and find(lo): max(ra, rb) falls strictly with every failure, so the loop ends
//                 whatever the other waves do (at most V - 1 swaps succeed in the whole launch).  Lock-free: no thread
//                 ever waits for another wave or workgroup -- no look-back, no ticket, no grid barrier, no cooperative launch.
//   The larger root always goes under the smaller, so when the launch is over the root of a tree is the MINIMUM index of its
//   component, whatever the arrival order: the labels are the same bits on every run.
//   Stale reads.  The per-XCD L2s are not coherent; `parent` is read and written with agent-scope relaxed atomics (loads and
//   stores that bypass the non-coherent levels), but nothing below needs that for correctness: every value parent[x] ever held is
//   an ancestor-or-self of x in x's tree and stays one (links only move to smaller indices inside the same tree), so a stale
//   value costs steps of the walk, never a wrong tree; a stale "root" loses its swap, which returns the true word.  The flatten
//   runs in a LATER launch, when no hook is in flight: parent[v] = root for every v, in place (a walker that meets an already
//   flattened link reads the root: the same argument).
//   An index is compared with [0, V) before anything is addressed through it; a face with an index outside is INVALID: it hooks
//   nothing, has label -1 and size 0, and is counted.
//
// The kernels (256 threads each unless stated; V vertices, T faces):
//   mesh_init_kernel      parent[v] = v, size[v] = 0, vflag[v] = 0; the select's histograms and state = 0.
//   mesh_hook_kernel      one face per thread: hook(a, b), hook(b, c).
//   mesh_flatten_kernel   one vertex per thread: parent[v] = find's root (= the component's label).
//   mesh_size_kernel      one face per thread, 1024 per workgroup: size[label] += 1 with ONE atomic per distinct label per wave
//                         (faces arrive in emission order: neighbours in a wave mostly share a label; the largest component
//                         would otherwise take millions of adds on one address), and the waves of a workgroup whose faces all
//                         carry one label share one add.  Measured at T = 4.2 M, 2.65 M of them in one component: 526 us
//                         with one add per wave (41 000 adds on one address), 157 us with this form.
//   mesh_face_out_kernel  (components only) label[t], size[t] of every face.
//   mesh_hist_kernel, mesh_pick_kernel   (keep_largest only) exact select of the n-th largest key (size << 32) | ~label over the
//                         roots with size > 0, eight bits per pass from the top, eight passes: a fixed number of launches, no
//                         host read.  The keys are distinct (the labels are), so "key >= the n-th" keeps exactly
//                         min(n, components) components, ties in size going to the lower label.
//   mesh_keep_kernel      one face per thread: fflag[t] = 1 kept, 2 invalid, 0 dropped; vflag[v] = 1 for the corners of a kept face
//                         (plain stores of the same value).
//   mesh_sums_kernel      per 256 flags: {sum of bit 0, second count}: kept faces and invalid faces; referenced vertices and
//                         components (roots with size > 0).
//   mesh_scan_kernel      one workgroup of 1024 threads: exclusive scan of both tables of sums in place (tsdf.hip's scan, restated
//                         for two u32 columns: V, T < 2^31), totals = {V', T', components, invalid faces} as int64.
//   mesh_base_kernel      flag -> new index (the workgroup's prefix + an exclusive scan inside it), or -1.
//   mesh_emit_faces_kernel, mesh_emit_vertices_kernel   the gathers: faces with the remap (and face_index), vertices as 32-bit
//                         words (and colours, vertex_index).  Every output element is written: the new indices are a bijection
//                         onto [0, T') and [0, V').
// Nothing depends on what the workspace held on entry: every word is written by an earlier kernel of the same call before it is read.
#include "hs_cloud.h"

namespace hs {
namespace {

constexpr int64_t kMeshMax = 1ll << 31;          // V, T < 2^31: indices and counts are int32
constexpr int kMeshBlock = 256;
constexpr int kSizeBlock = 1024;               // mesh_size_kernel: sixteen waves share one add where they share a label
constexpr int kMeshScanThreads = 1024;
constexpr int kSelPasses = 8, kSelBins = 256;

#define HS_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ int32_t ld_parent(const int32_t* p) { return __hip_atomic_load(p, HS_RLX_AGENT); }
__device__ __forceinline__ void st_parent(int32_t* p, int32_t v) { __hip_atomic_store(p, v, HS_RLX_AGENT); }

// the root of x's tree; x's link and those of the nodes it passes are moved to their grandparents (ancestors: see the top)
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
    int32_t p = ld_parent(parent + x);
    while (p != x) {
        const int32_t g = ld_parent(parent + p);
        if (g != p) st_parent(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void hook(int32_t* parent, int32_t a, int32_t b) {
    int32_t ra = find_root(parent, a), rb = find_root(parent, b);
    while (ra != rb) {
        const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            break;
        // lost: another hook put hi under `seen` < hi.  Both walks restart below hi: max(ra, rb) falls with every failure.
        ra = find_root(parent, seen);
        rb = find_root(parent, lo);
    }
}

struct SelState { unsigned long long prefix; unsigned long long k; };      // the key's bits found so far; the rank left among them

__device__ __forceinline__ unsigned long long comp_key(uint32_t size, int32_t label) {
    return ((unsigned long long)size << 32) | (uint32_t)~(uint32_t)label;
}

__device__ __forceinline__ bool valid_face(int32_t a, int32_t b, int32_t c, int64_t V) {
    return a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
}

__global__ void __launch_bounds__(kMeshBlock) mesh_init_kernel(int64_t V, int32_t* __restrict__ parent, uint32_t* __restrict__ size,
                                                                int32_t* __restrict__ vflag, uint32_t* __restrict__ hist,
                                                                SelState* __restrict__ sel) {
    const int64_t v = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (v < V) {
        parent[v] = (int32_t)v;
        size[v] = 0u;
        vflag[v] = 0;
    }
    if (v < kSelPasses * kSelBins) hist[v] = 0u;
    if (v == 0) { sel->prefix = 0ull; sel->k = 0ull; }
}

__global__ void __launch_bounds__(kMeshBlock) mesh_hook_kernel(int64_t V, int64_t T, const int32_t* __restrict__ faces,
                                                                int32_t* parent) {
    const int64_t t = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (t >= T) return;
    const int32_t a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
    if (!valid_face(a, b, c, V)) return;
    if (a != b) hook(parent, a, b);
    if (b != c) hook(parent, b, c);
}

__global__ void __launch_bounds__(kMeshBlock) mesh_flatten_kernel(int64_t V, int32_t* parent) {
    const int64_t v = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (v >= V) return;
    int32_t r = (int32_t)v, p = ld_parent(parent + r);
    while (p != r) { r = p; p = ld_parent(parent + r); }
    st_parent(parent + v, r);
}

__global__ void __launch_bounds__(kSizeBlock) mesh_size_kernel(int64_t V, int64_t T, const int32_t* __restrict__ faces,
                                                                const int32_t* __restrict__ label, uint32_t* size) {
    __shared__ int32_t s_label[kSizeBlock / 64];
    __shared__ uint32_t s_count[kSizeBlock / 64];
    const int64_t t = (int64_t)blockIdx.x * kSizeBlock + threadIdx.x;
    int32_t l = -1;
    if (t < T) {
        const int32_t a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
        if (valid_face(a, b, c, V)) l = label[a];
    }
    // one add per distinct label of the wave: the first lane still waiting names the label, the lanes that share it leave.
    // A wave whose faces all share ONE label (the rule inside a large component) hands its count to the workgroup instead,
    // which adds the counts of its waves that agree in one atomic: the largest component takes T / 1024 adds, not T / 64.
    unsigned long long todo = __ballot(l >= 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t mine = -1;
    uint32_t n_mine = 0u;
    if (todo) {
        const int32_t lead = __shfl(l, __builtin_ctzll(todo), 64);
        const unsigned long long same = __ballot(l == lead) & todo;
        if (same == todo) { mine = lead; n_mine = (uint32_t)__popcll(same); todo = 0ull; }
    }
    while (todo) {
        const int first = __builtin_ctzll(todo);
        const int32_t lead = __shfl(l, first, 64);
        const unsigned long long same = __ballot(l == lead) & todo;
        if (lane == first) atomicAdd(size + lead, (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if (lane == 0) { s_label[wave] = mine; s_count[wave] = n_mine; }
    __syncthreads();
    if (threadIdx.x < kSizeBlock / 64) {             // wave w's count goes with the first wave of its label
        const int32_t lw = s_label[threadIdx.x];
        bool first = lw >= 0;
        uint32_t n = 0u;
        for (int w = 0; w < kSizeBlock / 64; ++w) {
            if (s_label[w] != lw) continue;
            if (w < (int)threadIdx.x) first = false;
            n += s_count[w];
        }
        if (first) atomicAdd(size + lw, n);
    }
}

__global__ void __launch_bounds__(kMeshBlock) mesh_face_out_kernel(int64_t V, int64_t T, const int32_t* __restrict__ faces,
                                                                    const int32_t* __restrict__ label, const uint32_t* __restrict__ size,
                                                                    int32_t* __restrict__ out_label, int32_t* __restrict__ out_size) {
    const int64_t t = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (t >= T) return;
    const int32_t a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
    const bool ok = valid_face(a, b, c, V);
    const int32_t l = ok ? label[a] : -1;
    out_label[t] = l;
    out_size[t] = ok ? (int32_t)size[l] : 0;
}

// ---- the select of keep_largest ----

// pass `pass` (0 = the top eight bits): the roots whose key agrees with the prefix on the bits above count in the bin of their
// next eight bits.  LDS histogram per workgroup, one integer add per non-empty bin.
__global__ void __launch_bounds__(kMeshBlock) mesh_hist_kernel(int64_t V, int pass, const int32_t* __restrict__ label,
                                                                const uint32_t* __restrict__ size, const SelState* __restrict__ sel,
                                                                uint32_t* hist) {
    __shared__ uint32_t s_bin[kSelBins];
    s_bin[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t v = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    const int shift = 56 - 8 * pass;
    if (v < V && label[v] == (int32_t)v && size[v] > 0u) {
        const unsigned long long key = comp_key(size[v], (int32_t)v);
        const bool in = pass == 0 || (key >> (shift + 8)) == (sel->prefix >> (shift + 8));
        if (in) atomicAdd(&s_bin[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (s_bin[threadIdx.x]) atomicAdd(hist + pass * kSelBins + threadIdx.x, s_bin[threadIdx.x]);
}

// one thread: the bin that holds the k-th largest of the keys counted, from the top.  Pass 0 clamps k to the number of
// components (keep_largest >= components keeps them all: the k-th largest is then the smallest key).
__global__ void mesh_pick_kernel(int pass, unsigned long long keep_largest, const uint32_t* __restrict__ hist, SelState* sel) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t* h = hist + pass * kSelBins;
    unsigned long long k = sel->k;
    if (pass == 0) {
        unsigned long long total = 0ull;
        for (int d = 0; d < kSelBins; ++d) total += h[d];
        k = keep_largest < total ? keep_largest : total;
    }
    unsigned long long above = 0ull;
    int d = kSelBins - 1;
    for (; d > 0; --d) {
        if (above + h[d] >= k) break;
        above += h[d];
    }
    sel->prefix |= (unsigned long long)d << (56 - 8 * pass);
    sel->k = k - above;
}

// ---- flags, sums, scan, bases ----

__device__ __forceinline__ bool same_corner(const float* __restrict__ x, int32_t a, int32_t b) {
    return x[3 * (int64_t)a] == x[3 * (int64_t)b] && x[3 * (int64_t)a + 1] == x[3 * (int64_t)b + 1] &&
           x[3 * (int64_t)a + 2] == x[3 * (int64_t)b + 2];
}

__global__ void __launch_bounds__(kMeshBlock) mesh_keep_kernel(int64_t V, int64_t T, const int32_t* __restrict__ faces,
                                                                const float* __restrict__ vertices, const int32_t* __restrict__ label,
                                                                const uint32_t* __restrict__ size, const SelState* __restrict__ sel,
                                                                int64_t min_faces, bool select, bool remove_degenerate,
                                                                int32_t* __restrict__ fflag, int32_t* vflag) {
    const int64_t t = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (t >= T) return;
    const int32_t a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
    if (!valid_face(a, b, c, V)) { fflag[t] = 2; return; }
    const int32_t l = label[a];
    const uint32_t n = size[l];
    bool keep = (int64_t)n >= min_faces;
    if (select) keep = keep && comp_key(n, l) >= sel->prefix;
    if (keep && remove_degenerate) {
        const bool degenerate = a == b || b == c || a == c || same_corner(vertices, a, b) || same_corner(vertices, b, c) ||
                                same_corner(vertices, a, c);
        keep = !degenerate;
    }
    fflag[t] = keep ? 1 : 0;
    if (keep) { vflag[a] = 1; vflag[b] = 1; vflag[c] = 1; }
}

// exclusive scan of `v` over the 256 threads of a workgroup; `total`: the workgroup's sum (tsdf.hip's block_scan)
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t& total) {
    __shared__ uint32_t s_wave[kMeshBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    __syncthreads();                                  // (a second call in one kernel: the table is free again)
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
#pragma unroll
    for (int w = 0; w < kMeshBlock / 64; ++w) {
        before += w < wave ? s_wave[w] : 0u;
        total += s_wave[w];
    }
    return before + incl - v;
}

// blocks[2 b] = the flags with bit 0 set among the workgroup's 256; blocks[2 b + 1] = VERTEX: the components among its vertices
// (roots with size > 0), else the flags with bit 1 set (invalid faces).  Both in one scan: at most 256 each.
template <bool VERTEX>
__global__ void __launch_bounds__(kMeshBlock) mesh_sums_kernel(int64_t n, const int32_t* __restrict__ flag,
                                                                const int32_t* __restrict__ label, const uint32_t* __restrict__ size,
                                                                uint32_t* __restrict__ blocks) {
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    uint32_t one = 0u, two = 0u;
    if (i < n) {
        const int32_t f = flag[i];
        one = (uint32_t)f & 1u;
        two = VERTEX ? (label[i] == (int32_t)i && size[i] > 0u ? 1u : 0u) : ((uint32_t)f >> 1) & 1u;
    }
    uint32_t total;
    block_scan((one << 16) | two, total);
    if (threadIdx.x == 0) {
        blocks[2 * (int64_t)blockIdx.x] = total >> 16;
        blocks[2 * (int64_t)blockIdx.x + 1] = total & 0xFFFFu;
    }
}

// exclusive scan of column 0 of both tables in place, the sums of all four columns to totals.  One workgroup: thread t takes
// ceil(nblk / 1024) workgroups' sums in a row, of the vertices' table and of the faces' table.
__global__ void __launch_bounds__(kMeshScanThreads) mesh_scan_kernel(uint32_t* __restrict__ vblocks, int64_t nvblk,
                                                                     uint32_t* __restrict__ fblocks, int64_t nfblk,
                                                                     int64_t* __restrict__ totals) {
    __shared__ uint32_t s_a[kMeshScanThreads], s_b[kMeshScanThreads];
    const int t = threadIdx.x;
    for (int table = 0; table < 2; ++table) {
        uint32_t* blocks = table ? fblocks : vblocks;
        const int64_t nblk = table ? nfblk : nvblk;
        const int64_t per = (nblk + kMeshScanThreads - 1) / kMeshScanThreads;
        const int64_t b0 = t * per < nblk ? t * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
        uint32_t a = 0u, b = 0u;
        for (int64_t i = b0; i < b1; ++i) { a += blocks[2 * i]; b += blocks[2 * i + 1]; }
        __syncthreads();                              // (the second table: the first one's reads of s_a, s_b are over)
        s_a[t] = a;
        s_b[t] = b;
        __syncthreads();
        for (int off = 1; off < kMeshScanThreads; off <<= 1) {
            const uint32_t ua = t >= off ? s_a[t - off] : 0u, ub = t >= off ? s_b[t - off] : 0u;
            __syncthreads();
            s_a[t] += ua;
            s_b[t] += ub;
            __syncthreads();
        }
        uint32_t run = t ? s_a[t - 1] : 0u;
        for (int64_t i = b0; i < b1; ++i) {
            const uint32_t c = blocks[2 * i];
            blocks[2 * i] = run;
            run += c;
        }
        if (t == kMeshScanThreads - 1) {
            totals[table ? 1 : 0] = (int64_t)s_a[t];      // V' | T'
            totals[table ? 3 : 2] = (int64_t)s_b[t];      // components | invalid faces
        }
    }
}

// flag (bit 0) -> the element's new index, or -1: in place
__global__ void __launch_bounds__(kMeshBlock) mesh_base_kernel(int64_t n, const uint32_t* __restrict__ blocks, int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    const uint32_t mine = i < n ? (uint32_t)flag[i] & 1u : 0u;
    uint32_t total;
    const uint32_t before = block_scan(mine, total);
    if (i < n) flag[i] = mine ? (int32_t)(blocks[2 * (int64_t)blockIdx.x] + before) : -1;
}

// ---- emit ----

__global__ void __launch_bounds__(kMeshBlock) mesh_emit_faces_kernel(int64_t V, int64_t T, int64_t T_out,
                                                                      const int32_t* __restrict__ faces, const int32_t* __restrict__ fnew,
                                                                      const int32_t* __restrict__ vnew, int32_t* __restrict__ faces_out,
                                                                      int32_t* __restrict__ face_index) {
    const int64_t t = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (t >= T) return;
    const int64_t at = fnew[t];
    if (at < 0 || at >= T_out) return;                // (>= T_out: never; a stale plan must not write outside)
    const int32_t a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
    if (!valid_face(a, b, c, V)) return;              // (never: the plan kept valid faces only)
    faces_out[3 * at] = vnew[a];
    faces_out[3 * at + 1] = vnew[b];
    faces_out[3 * at + 2] = vnew[c];
    if (face_index) face_index[at] = (int32_t)t;
}

__global__ void __launch_bounds__(kMeshBlock) mesh_emit_vertices_kernel(int64_t V, int64_t V_out, const uint32_t* __restrict__ vertices,
                                                                         const uint32_t* __restrict__ colors,
                                                                         const int32_t* __restrict__ vnew, uint32_t* __restrict__ vertices_out,
                                                                         uint32_t* __restrict__ colors_out, int32_t* __restrict__ vertex_index) {
    const int64_t v = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (v >= V) return;
    const int64_t at = vnew[v];
    if (at < 0 || at >= V_out) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) vertices_out[3 * at + c] = vertices[3 * v + c];      // 32-bit words: the floats' bits
    if (colors) {
#pragma unroll
        for (int c = 0; c < 3; ++c) colors_out[3 * at + c] = colors[3 * v + c];
    }
    if (vertex_index) vertex_index[at] = (int32_t)v;
}

// ---- host ----

// parent (the labels once flattened) at 0
struct MeshWs { int64_t size, vflag, fflag, vblocks, fblocks, hist, sel, bytes, nvblk, nfblk; };

MeshWs mesh_ws(int64_t V, int64_t T) {
    MeshWs w;
    w.nvblk = (V + kMeshBlock - 1) / kMeshBlock;
    w.nfblk = (T + kMeshBlock - 1) / kMeshBlock;
    const int64_t per_v = align_up(4 * V, 16);
    w.size = per_v;
    w.vflag = 2 * per_v;
    w.fflag = 3 * per_v;
    w.vblocks = w.fflag + align_up(4 * T, 16);
    w.fblocks = w.vblocks + align_up(8 * w.nvblk, 16);
    w.hist = w.fblocks + align_up(8 * w.nfblk, 16);
    w.sel = w.hist + 4 * kSelPasses * kSelBins;
    w.bytes = w.sel + 64;
    return w;
}

int check_counts(const char* fn, int64_t V, int64_t T) {
    if (V < 0 || V >= kMeshMax || T < 0 || T >= kMeshMax) {
        set_error("%s: n_vertices=%lld, n_faces=%lld outside [0, 2^31)", fn, (long long)V, (long long)T);
        return HS_EINVAL;
    }
    return HS_OK;
}

// what the three calls share: the counts, faces (when there are any) and the workspace
int check_mesh_input(const char* fn, const hs_mesh_args& a) {
    if (check_counts(fn, a.n_vertices, a.n_faces)) return HS_EINVAL;
    if (a.n_faces > 0 && check_field(fn, a.faces, "faces", 4)) return HS_EINVAL;
    if (check_aligned(fn, a.faces, "faces", 4)) return HS_EINVAL;
    return check_field(fn, a.workspace, "workspace", 16);
}

inline unsigned grid_of(int64_t n) { return (unsigned)((n + kMeshBlock - 1) / kMeshBlock); }

// init, hook, flatten, size: afterwards parent[v] = label of v, size[label] = faces of the component
int launch_components(const hs_mesh_args& a, const MeshWs& w, hipStream_t s) {
    char* ws = (char*)a.workspace;
    int32_t* parent = (int32_t*)ws;
    uint32_t* size = (uint32_t*)(ws + w.size);
    const int64_t V = a.n_vertices, T = a.n_faces;
    const int64_t n_init = V > kSelPasses * kSelBins ? V : kSelPasses * kSelBins;
    mesh_init_kernel<<<grid_of(n_init), kMeshBlock, 0, s>>>(V, parent, size, (int32_t*)(ws + w.vflag), (uint32_t*)(ws + w.hist),
                                                            (SelState*)(ws + w.sel));
    HS_LAUNCH_CHECK();
    if (T > 0) {
        mesh_hook_kernel<<<grid_of(T), kMeshBlock, 0, s>>>(V, T, a.faces, parent);
        HS_LAUNCH_CHECK();
    }
    if (V > 0) {
        mesh_flatten_kernel<<<grid_of(V), kMeshBlock, 0, s>>>(V, parent);
        HS_LAUNCH_CHECK();
    }
    if (T > 0) {
        mesh_size_kernel<<<(unsigned)((T + kSizeBlock - 1) / kSizeBlock), kSizeBlock, 0, s>>>(V, T, a.faces, parent, size);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

}  // namespace
}  // namespace hs

extern "C" {

HS_API int64_t hs_mesh_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (hs::check_counts("hs_mesh_workspace_bytes", n_vertices, n_faces)) return HS_EINVAL;
    return hs::mesh_ws(n_vertices, n_faces).bytes;
}

HS_API int hs_mesh_components(const hs_mesh_args* a, void* hip_stream) {
    const char* fn = "hs_mesh_components";
    if (hs::check_args(fn, a) || hs::check_mesh_input(fn, *a)) return HS_EINVAL;
    if (hs::check_aligned(fn, a->label, "label", 4) || hs::check_aligned(fn, a->size, "size", 4)) return HS_EINVAL;
    if (a->n_faces > 0) {
        const hs::Field f[2] = {{a->label, "label", 4}, {a->size, "size", 4}};
        if (hs::check_fields(fn, f, 2)) return HS_EINVAL;
    }
    if (a->n_faces == 0) return HS_OK;
    const hs::MeshWs w = hs::mesh_ws(a->n_vertices, a->n_faces);
    hipStream_t s = (hipStream_t)hip_stream;
    const int rc = hs::launch_components(*a, w, s);
    if (rc != HS_OK) return rc;
    const char* ws = (const char*)a->workspace;
    hs::mesh_face_out_kernel<<<hs::grid_of(a->n_faces), hs::kMeshBlock, 0, s>>>(a->n_vertices, a->n_faces, a->faces, (const int32_t*)ws,
                                                                               (const uint32_t*)(ws + w.size), a->label, a->size);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

HS_API int hs_mesh_clean_plan(const hs_mesh_args* a, void* hip_stream) {
    const char* fn = "hs_mesh_clean_plan";
    if (hs::check_args(fn, a) || hs::check_mesh_input(fn, *a)) return HS_EINVAL;
    if (a->min_faces < 0 || a->keep_largest < 0) {
        hs::set_error("%s: min_faces=%lld, keep_largest=%lld must be >= 0 (0: no limit)", fn, (long long)a->min_faces,
                      (long long)a->keep_largest);
        return HS_EINVAL;
    }
    if (a->remove_degenerate != 0 && a->remove_degenerate != 1) {
        hs::set_error("%s: remove_degenerate=%d must be 0 or 1", fn, a->remove_degenerate);
        return HS_EINVAL;
    }
    if (hs::check_aligned(fn, a->vertices, "vertices", 4)) return HS_EINVAL;
    if (a->remove_degenerate && a->n_vertices > 0 && a->n_faces > 0 && hs::check_field(fn, a->vertices, "vertices", 4)) return HS_EINVAL;
    if (hs::check_field(fn, a->totals, "totals", 8)) return HS_EINVAL;
    const int64_t V = a->n_vertices, T = a->n_faces;
    const hs::MeshWs w = hs::mesh_ws(V, T);
    hipStream_t s = (hipStream_t)hip_stream;
    const int rc = hs::launch_components(*a, w, s);
    if (rc != HS_OK) return rc;
    char* ws = (char*)a->workspace;
    int32_t* label = (int32_t*)ws;
    uint32_t* size = (uint32_t*)(ws + w.size);
    int32_t* vflag = (int32_t*)(ws + w.vflag);
    int32_t* fflag = (int32_t*)(ws + w.fflag);
    uint32_t* vblocks = (uint32_t*)(ws + w.vblocks);
    uint32_t* fblocks = (uint32_t*)(ws + w.fblocks);
    uint32_t* hist = (uint32_t*)(ws + w.hist);
    hs::SelState* sel = (hs::SelState*)(ws + w.sel);
    const bool select = a->keep_largest > 0 && V > 0 && T > 0;
    if (select) {
        for (int pass = 0; pass < hs::kSelPasses; ++pass) {
            hs::mesh_hist_kernel<<<hs::grid_of(V), hs::kMeshBlock, 0, s>>>(V, pass, label, size, sel, hist);
            HS_LAUNCH_CHECK();
            hs::mesh_pick_kernel<<<1, 64, 0, s>>>(pass, (unsigned long long)a->keep_largest, hist, sel);
            HS_LAUNCH_CHECK();
        }
    }
    if (T > 0) {
        hs::mesh_keep_kernel<<<hs::grid_of(T), hs::kMeshBlock, 0, s>>>(V, T, a->faces, a->vertices, label, size, sel, a->min_faces, select,
                                                                     a->remove_degenerate != 0, fflag, vflag);
        HS_LAUNCH_CHECK();
        hs::mesh_sums_kernel<false><<<hs::grid_of(T), hs::kMeshBlock, 0, s>>>(T, fflag, nullptr, nullptr, fblocks);
        HS_LAUNCH_CHECK();
    }
    if (V > 0) {
        hs::mesh_sums_kernel<true><<<hs::grid_of(V), hs::kMeshBlock, 0, s>>>(V, vflag, label, size, vblocks);
        HS_LAUNCH_CHECK();
    }
    hs::mesh_scan_kernel<<<1, hs::kMeshScanThreads, 0, s>>>(vblocks, w.nvblk, fblocks, w.nfblk, a->totals);
    HS_LAUNCH_CHECK();
    if (V > 0) {
        hs::mesh_base_kernel<<<hs::grid_of(V), hs::kMeshBlock, 0, s>>>(V, vblocks, vflag);
        HS_LAUNCH_CHECK();
    }
    if (T > 0) {
        hs::mesh_base_kernel<<<hs::grid_of(T), hs::kMeshBlock, 0, s>>>(T, fblocks, fflag);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

HS_API int hs_mesh_clean_emit(const hs_mesh_args* a, void* hip_stream) {
    const char* fn = "hs_mesh_clean_emit";
    if (hs::check_args(fn, a) || hs::check_mesh_input(fn, *a)) return HS_EINVAL;
    const int64_t V = a->n_vertices, T = a->n_faces, Vo = a->n_vertices_out, To = a->n_faces_out;
    if (Vo < 0 || Vo > V || To < 0 || To > T) {
        hs::set_error("%s: n_vertices_out=%lld, n_faces_out=%lld outside [0, n_vertices=%lld] and [0, n_faces=%lld]", fn, (long long)Vo,
                      (long long)To, (long long)V, (long long)T);
        return HS_EINVAL;
    }
    if (hs::check_aligned(fn, a->vertices, "vertices", 4) || hs::check_aligned(fn, a->colors, "colors", 4) ||
        hs::check_aligned(fn, a->vertices_out, "vertices_out", 4) || hs::check_aligned(fn, a->faces_out, "faces_out", 4) ||
        hs::check_aligned(fn, a->colors_out, "colors_out", 4) || hs::check_aligned(fn, a->vertex_index, "vertex_index", 4) ||
        hs::check_aligned(fn, a->face_index, "face_index", 4))
        return HS_EINVAL;
    if ((a->colors != nullptr) != (a->colors_out != nullptr)) {
        hs::set_error("%s: %s", fn, a->colors ? "the mesh has colours (colors), the output has none (null colors_out)"
                                              : "colors_out given for a mesh without colours (null colors)");
        return HS_EINVAL;
    }
    if (Vo > 0) {
        const hs::Field f[2] = {{a->vertices, "vertices", 4}, {a->vertices_out, "vertices_out", 4}};
        if (hs::check_fields(fn, f, 2)) return HS_EINVAL;
    }
    if (To > 0 && hs::check_field(fn, a->faces_out, "faces_out", 4)) return HS_EINVAL;
    if (Vo == 0 && To == 0) return HS_OK;
    const hs::MeshWs w = hs::mesh_ws(V, T);
    const char* ws = (const char*)a->workspace;
    const int32_t* vnew = (const int32_t*)(ws + w.vflag);
    const int32_t* fnew = (const int32_t*)(ws + w.fflag);
    hipStream_t s = (hipStream_t)hip_stream;
    if (To > 0) {
        hs::mesh_emit_faces_kernel<<<hs::grid_of(T), hs::kMeshBlock, 0, s>>>(V, T, To, a->faces, fnew, vnew, a->faces_out, a->face_index);
        HS_LAUNCH_CHECK();
    }
    if (Vo > 0) {
        hs::mesh_emit_vertices_kernel<<<hs::grid_of(V), hs::kMeshBlock, 0, s>>>(V, Vo, (const uint32_t*)a->vertices, (const uint32_t*)a->colors,
                                                                              vnew, (uint32_t*)a->vertices_out, (uint32_t*)a->colors_out,
                                                                              a->vertex_index);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

}  // extern "C"
