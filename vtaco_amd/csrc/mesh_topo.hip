// Topology of a triangle mesh on the device: connected components, their table, per-component measures, edge statistics and the
// filter that keeps a subset of the components (DESIGN.md, section "mesh_topo.hip"; tests/mesh_topo_ref.py restates the results in
// numpy).  faces [F,3] i32 and vertices [V,3] f32 as vt_mc_emit leaves them (f64 vertices as well); coordinates are widened exactly and
// every coordinate operation is float64, unfused (-ffp-contract=off).
//   labels        union-find on the device.  labels[v] <= v always and only ever falls.  A hooking launch walks both ends of the edges
//                 (a,b), (b,c) of every face to their roots and, while the roots differ, lowers the larger root with an integer atomicMin
//                 and goes on with (what the atomic found there, the smaller root): no union is lost to a concurrent hook.  A jumping
//                 launch then stores every vertex's root.  The pair is repeated, one launch each, until a hooking launch met no edge
//                 with two roots (a device flag, read once per MT_ROUND_BATCH rounds): the fixed point -- every component under its
//                 smallest index -- is unique, so the arrival order of the atomics cannot show in the result.  Labels that another
//                 workgroup may lower in the same launch are read with relaxed agent-scope atomic loads.
//   table         referenced[v] by plain stores of 1; roots that are referenced are ranked by an exclusive prefix scan.
//   stats         integers by integer atomics.  The two float64 sums are accumulated EXACTLY: a first face pass takes each component's
//                 largest |term| (atomicMax on the bit pattern), a second adds every term as two int64 fixed-point limbs scaled by that
//                 maximum's exponent (2^31 terms of 31 bits each fit an int64; the second limb carries the next 31 bits, rounded to
//                 nearest).  Integer addition is associative, so the sums carry no trace of the order: equal bits from run to run with
//                 no float atomic and no sort.  A term's error is at most 2^-62 of the component's largest term.
//                 bbox: atomicMin / atomicMax on an order-preserving integer image of the float64 coordinate.
//   edges         mesh_edges.h's table: per undirected edge the faces that run lo -> hi and hi -> lo.  A second pass classifies the
//                 occupied slots.
//   filter        two exclusive scans (kept vertices, kept faces), then the copies; order is preserved.
// Every per-component atomic is issued once per (wave, component): lanes of a wave that hold the same component combine first.
// A face with an index outside [0, V) is never dereferenced; it takes no part and sets bit 0 of the status word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mesh_common.h"
#include "mesh_edges.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

enum { ST_BAD = 0, ST_FLAG0 = 4, ST_NCOMP = 8, ST_NV = 9, ST_NF = 10 };     // (MT_STATUS_BYTES of int32 words: mesh_common.h)

#define MT_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- labels -------------------------------------------------------------------------------------------------------------------------
__device__ inline int find_root(int32_t *labels, int v) {
    int p = __hip_atomic_load(labels + v, MT_RLX_AGENT);
    while (p != v) {                              // labels[v] <= v and strictly below v off a root: the walk ends
        v = p;
        p = __hip_atomic_load(labels + v, MT_RLX_AGENT);
    }
    return v;
}

__device__ inline bool link(int32_t *labels, int a, int b) {
    int ra = find_root(labels, a), rb = find_root(labels, b);
    bool met = false;
    while (ra != rb) {
        met = true;
        const int hi = max(ra, rb), lo = min(ra, rb);
        const int old = atomicMin(labels + hi, lo);
        if (old == hi || old == lo) break;        // hi was a root and now hangs under lo, or somebody made the same hook
        ra = find_root(labels, old);              // hi hung under `old` already: old and lo are one component (both < hi: the loop ends)
        rb = find_root(labels, lo);
    }
    return met;
}

__global__ void __launch_bounds__(MT_THREADS) init_labels_kernel(int32_t *labels, int V) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v < V) labels[v] = (int)v;
}

__global__ void __launch_bounds__(MT_THREADS) hook_kernel(const int32_t *faces, int F, int V, int32_t *labels, int32_t *status, int flag) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    if (!ok) { atomicOr(status + ST_BAD, 1); return; }
    const bool m0 = link(labels, a, b);
    const bool m1 = link(labels, b, c);
    if (m0 || m1) __hip_atomic_store(status + flag, 1, MT_RLX_AGENT);
}

__global__ void __launch_bounds__(MT_THREADS) jump_kernel(int32_t *labels, int V) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v >= V) return;
    const int r = find_root(labels, (int)v);
    __hip_atomic_store(labels + v, r, MT_RLX_AGENT);
}

// ---- component table --------------------------------------------------------------------------------------------------------------------
struct RootPred {
    const int32_t *ref, *labels;
    __device__ bool operator()(int64_t v) const { return ref[v] != 0 && labels[v] == (int)v; }
};

__global__ void __launch_bounds__(MT_THREADS) mark_kernel(const int32_t *faces, int F, int V, int32_t *ref, int32_t *status) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    if (!ok) { atomicOr(status + ST_BAD, 1); return; }
    ref[a] = 1; ref[b] = 1; ref[c] = 1;
}

__global__ void __launch_bounds__(MT_THREADS)
table_vertex_kernel(const int32_t *ref, const int32_t *labels, const int32_t *rank, int V, int32_t *comp_of_vertex, int32_t *status) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v >= V) return;
    int c = -1;
    if (ref[v] != 0) {
        const int r = labels[v];
        if ((unsigned)r < (unsigned)V && labels[r] == r && ref[r] != 0) c = rank[r];
        else atomicOr(status + ST_BAD, 2);          // labels that are not vt_mesh_components' of these faces
    }
    comp_of_vertex[v] = c;
}

__global__ void __launch_bounds__(MT_THREADS)
table_face_kernel(const int32_t *faces, int F, int V, const int32_t *comp_of_vertex, int32_t *comp_of_face) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    comp_of_face[f] = ok ? comp_of_vertex[a] : -1;
}

struct FaceMaxOp {                               // n_faces, max area bits, max |volume| bits
    static constexpr int K = 3;
    __device__ static u64 identity(int) { return 0; }
    __device__ static u64 combine(int k, u64 a, u64 b) { return k == 0 ? a + b : (a > b ? a : b); }
    __device__ static void atomic(int k, u64 *p, u64 v) { if (k == 0) atomicAdd(p, v); else atomicMax(p, v); }
};
struct SumOp {                                   // area limbs hi, lo; volume limbs hi, lo (two's complement)
    static constexpr int K = 4;
    __device__ static u64 identity(int) { return 0; }
    __device__ static u64 combine(int, u64 a, u64 b) { return a + b; }
    __device__ static void atomic(int, u64 *p, u64 v) { atomicAdd(p, v); }
};
struct VertOp {                                  // n_vertices, min keys x y z, max keys x y z
    static constexpr int K = 7;
    __device__ static u64 identity(int k) { return (k >= 1 && k <= 3) ? ~0ull : 0ull; }
    __device__ static u64 combine(int k, u64 a, u64 b) { return k == 0 ? a + b : (k <= 3 ? (a < b ? a : b) : (a > b ? a : b)); }
    __device__ static void atomic(int k, u64 *p, u64 v) {
        if (k == 0) atomicAdd(p, v);
        else if (k <= 3) atomicMin(p, v);
        else atomicMax(p, v);
    }
};

// the two terms of a face, each operation one rounding, in this order (tests/mesh_topo_ref.py: face_terms)
template <class T>
__device__ inline void face_terms(const T *verts, int a, int b, int c, double &area, double &vol) {
    double x0, y0, z0, x1, y1, z1, x2, y2, z2;
    load_vertex(verts, a, x0, y0, z0);
    load_vertex(verts, b, x1, y1, z1);
    load_vertex(verts, c, x2, y2, z2);
    const double ux = x1 - x0, uy = y1 - y0, uz = z1 - z0;
    const double wx = x2 - x0, wy = y2 - y0, wz = z2 - z0;
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
    const double cx = y1 * z2 - z1 * y2, cy = z1 * x2 - x1 * z2, cz = x1 * y2 - y1 * x2;
    vol = ((x0 * cx + y0 * cy) + z0 * cz) / 6.0;
}

struct StatsWs { u64 *fmax, *sums, *vert; };      // [C][3], [C][4], [C][7]

__global__ void __launch_bounds__(MT_THREADS) stats_init_kernel(StatsWs ws, int C) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= C) return;
    for (int k = 0; k < 3; ++k) ws.fmax[i * 3 + k] = 0;
    for (int k = 0; k < 4; ++k) ws.sums[i * 4 + k] = 0;
    for (int k = 0; k < 7; ++k) ws.vert[i * 7 + k] = VertOp::identity(k);
}

template <class T>
__global__ void __launch_bounds__(MT_THREADS) stats_vertex_kernel(const T *verts, int V, const int32_t *comp_of_vertex, int C, StatsWs ws) {
    int cur = -1;
    u64 acc[7] = {0, 0, 0, 0, 0, 0, 0};
    const int64_t base = (int64_t)blockIdx.x * MT_CHUNK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        const int64_t v = base + (int64_t)k * MT_THREADS;
        int c = -1;
        u64 x[7] = {1, 0, 0, 0, 0, 0, 0};
        if (v < V) {
            c = comp_of_vertex[v];
            if ((unsigned)c >= (unsigned)C) c = -1;
            else {
                double px, py, pz;
                load_vertex(verts, (int)v, px, py, pz);
                x[1] = x[4] = key_of(px); x[2] = x[5] = key_of(py); x[3] = x[6] = key_of(pz);
            }
        }
        accumulate<7, VertOp>(cur, acc, c, x, ws.vert);
    }
    wave_flush<7, VertOp>(cur, acc, ws.vert);
}

// PASS 0: counts and largest terms; PASS 1: the fixed-point sums against them.  The three indices of a face are read straight from global
// memory here (a wave's three dword loads cover one contiguous 768-byte run between them), not through LDS as the one-face-per-thread kernels do
template <class T, int PASS>
__global__ void __launch_bounds__(MT_THREADS)
stats_face_kernel(const T *verts, int V, const int32_t *faces, int F, const int32_t *comp_of_face, int C, StatsWs ws) {
    constexpr int K = PASS == 0 ? 3 : 4;
    using Op = typename std::conditional<PASS == 0, FaceMaxOp, SumOp>::type;
    u64 *table = PASS == 0 ? ws.fmax : ws.sums;
    int cur = -1;
    u64 acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0;
    const int64_t base = (int64_t)blockIdx.x * MT_CHUNK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        const int64_t f = base + (int64_t)k * MT_THREADS;
        int c = -1;
        u64 x[K];
#pragma unroll
        for (int j = 0; j < K; ++j) x[j] = 0;
        if (f < F) {
            c = comp_of_face[f];
            const int a = faces[f * 3], b = faces[f * 3 + 1], d = faces[f * 3 + 2];
            if ((unsigned)c >= (unsigned)C || (unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)d >= (unsigned)V) c = -1;
            else {
                double area, vol;
                face_terms(verts, a, b, d, area, vol);
                if (PASS == 0) {
                    x[0] = 1;
                    x[1] = (u64)__double_as_longlong(area);
                    x[2] = (u64)__double_as_longlong(fabs(vol));
                } else {
                    limbs_of(area, exponent_of(ws.fmax[(size_t)c * 3 + 1]), x[0], x[1]);
                    limbs_of(vol, exponent_of(ws.fmax[(size_t)c * 3 + 2]), x[2], x[3]);
                }
            }
        }
        accumulate<K, Op>(cur, acc, c, x, table);
    }
    wave_flush<K, Op>(cur, acc, table);
}

template <class T>
__global__ void __launch_bounds__(MT_THREADS)
stats_finish_kernel(StatsWs ws, int C, int32_t *n_faces, int32_t *n_vertices, T *bbox, double *area, double *volume) {
    const int64_t c = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (c >= C) return;
    n_faces[c] = (int32_t)ws.fmax[c * 3];
    n_vertices[c] = (int32_t)ws.vert[c * 7];
    area[c] = sum_of(ws.sums[c * 4], ws.sums[c * 4 + 1], exponent_of(ws.fmax[c * 3 + 1]));
    volume[c] = sum_of(ws.sums[c * 4 + 2], ws.sums[c * 4 + 3], exponent_of(ws.fmax[c * 3 + 2]));
    const bool any = ws.vert[c * 7] != 0;
    for (int k = 0; k < 6; ++k) bbox[c * 6 + k] = any ? (T)value_of(ws.vert[c * 7 + 1 + k]) : (T)0;
}

size_t stats_bytes(int64_t C) { return up256((size_t)C * 3 * 8) + up256((size_t)C * 4 * 8) + up256((size_t)C * 7 * 8); }

template <class T>
void stats_launch(const T *verts, int V, const int32_t *faces, int F, const int32_t *cov, const int32_t *cof, int C, int32_t *n_faces,
                  int32_t *n_vertices, T *bbox, double *area, double *volume, char *wsp, hipStream_t st) {
    StatsWs ws;
    ws.fmax = reinterpret_cast<u64 *>(wsp);
    ws.sums = reinterpret_cast<u64 *>(wsp + up256((size_t)C * 3 * 8));
    ws.vert = reinterpret_cast<u64 *>(wsp + up256((size_t)C * 3 * 8) + up256((size_t)C * 4 * 8));
    hipLaunchKernelGGL(stats_init_kernel, dim3(blocks_of(C, MT_THREADS)), dim3(MT_THREADS), 0, st, ws, C);
    hipLaunchKernelGGL(stats_vertex_kernel<T>, dim3(blocks_of(V, MT_CHUNK)), dim3(MT_THREADS), 0, st, verts, V, cov, C, ws);
    hipLaunchKernelGGL((stats_face_kernel<T, 0>), dim3(blocks_of(F, MT_CHUNK)), dim3(MT_THREADS), 0, st, verts, V, faces, F, cof, C, ws);
    hipLaunchKernelGGL((stats_face_kernel<T, 1>), dim3(blocks_of(F, MT_CHUNK)), dim3(MT_THREADS), 0, st, verts, V, faces, F, cof, C, ws);
    hipLaunchKernelGGL(stats_finish_kernel<T>, dim3(blocks_of(C, MT_THREADS)), dim3(MT_THREADS), 0, st, ws, C, n_faces, n_vertices, bbox, area,
                       volume);
}

// ---- edges ------------------------------------------------------------------------------------------------------------------------------------
// out: [4][C] int32 -- n_edges, n_boundary, n_nonmanifold, n_misoriented
__global__ void __launch_bounds__(MT_THREADS)
edge_count_kernel(const u64 *keys, const u64 *vals, int64_t slots, const int32_t *comp_of_vertex, int V, int C, int32_t *n_edges, int32_t *n_boundary,
                  int32_t *n_nonmanifold, int32_t *n_misoriented) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    int c = -1;
    bool boundary = false, nonmanifold = false, misoriented = false;
    if (i < slots) {
        const u64 key = keys[i];
        if (key != EDGE_EMPTY) {
            const unsigned lo = (unsigned)(key >> 32);
            if (lo < (unsigned)V) c = comp_of_vertex[lo];
            if ((unsigned)c >= (unsigned)C) c = -1;
            const u64 val = vals[i];
            const unsigned fwd = (unsigned)val, bwd = (unsigned)(val >> 32);
            const u64 n = (u64)fwd + bwd;
            boundary = n == 1;
            nonmanifold = n >= 3;
            misoriented = n == 2 && (fwd == 2 || bwd == 2);
        }
    }
    bool live = c >= 0;
    for (;;) {
        const u64 todo = __ballot(live);
        if (todo == 0) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int c0 = __shfl(c, leader);
        const bool mine = live && c == c0;
        const int ne = __popcll(__ballot(mine)), nb = __popcll(__ballot(mine && boundary));
        const int nn = __popcll(__ballot(mine && nonmanifold)), nm = __popcll(__ballot(mine && misoriented));
        if (lane == leader) {
            atomicAdd(n_edges + c0, ne);
            if (nb) atomicAdd(n_boundary + c0, nb);
            if (nn) atomicAdd(n_nonmanifold + c0, nn);
            if (nm) atomicAdd(n_misoriented + c0, nm);
        }
        if (mine) live = false;
    }
}

// ---- filter -------------------------------------------------------------------------------------------------------------------------------------
struct KeepPred {
    const int32_t *comp;
    const uint8_t *keep;
    int C;
    __device__ bool operator()(int64_t i) const {
        const int c = comp[i];
        return (unsigned)c < (unsigned)C && keep[c] != 0;
    }
};

template <class T>
__global__ void __launch_bounds__(MT_THREADS) filter_vertex_kernel(const T *verts, int V, KeepPred kept, int32_t *vertex_map, T *out_verts) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v >= V) return;
    if (!kept(v)) { vertex_map[v] = -1; return; }
    const int at = vertex_map[v];                 // (the scan left the rank here; at <= v < V: inside the capacity-V output)
    for (int k = 0; k < 3; ++k) out_verts[(size_t)at * 3 + k] = verts[(size_t)v * 3 + k];
}

__global__ void __launch_bounds__(MT_THREADS)
filter_face_kernel(const int32_t *faces, int F, int V, KeepPred kept, const int32_t *fpos, const int32_t *vertex_map, int32_t *out_faces,
                   int32_t *status) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok) || !kept(f)) return;
    if (!ok) { atomicOr(status + ST_BAD, 1); return; }
    const int at = fpos[f];                       // at <= f < F
    const int na = vertex_map[a], nb = vertex_map[b], nc = vertex_map[c];
    if (na < 0 || nb < 0 || nc < 0) atomicOr(status + ST_BAD, 2);   // maps that are not the table of these faces
    out_faces[(size_t)at * 3] = na; out_faces[(size_t)at * 3 + 1] = nb; out_faces[(size_t)at * 3 + 2] = nc;
}

template <class T>
void filter_launch(const T *verts, int V, const int32_t *faces, int F, const int32_t *cov, const int32_t *cof, const uint8_t *keep, int C,
                   T *out_verts, int32_t *out_faces, int32_t *vertex_map, int32_t *status, int32_t *bsum, int32_t *fpos, hipStream_t st) {
    const KeepPred kv{cov, keep, C}, kf{cof, keep, C};
    scan_launch(kv, V, bsum, vertex_map, status + ST_NV, st);
    hipLaunchKernelGGL(filter_vertex_kernel<T>, dim3(blocks_of(V, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, V, kv, vertex_map, out_verts);
    scan_launch(kf, F, bsum, fpos, status + ST_NF, st);
    hipLaunchKernelGGL(filter_face_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, faces, F, V, kf, (const int32_t *)fpos,
                       (const int32_t *)vertex_map, out_faces, status);
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && F >= 1 && V <= MT_MAX_V && F <= MT_MAX_F; }

size_t table_bytes(int64_t V) { return MT_STATUS_BYTES + 2 * up256((size_t)V * sizeof(int32_t)) + scan_bytes(V); }
size_t filter_bytes(int64_t V, int64_t F) { return MT_STATUS_BYTES + up256((size_t)F * sizeof(int32_t)) + scan_bytes(V > F ? V : F); }

}  // namespace

extern "C" {

size_t vt_mesh_components_workspace_bytes(int64_t V, int64_t F) { return sizes_ok(V, F) ? MT_STATUS_BYTES : 0; }

int vt_mesh_components(const int32_t *faces, int64_t F, int64_t V, int32_t *labels, int *rounds, void *workspace, size_t workspace_bytes, void *stream) {
    if (!sizes_ok(V, F) || !faces || !labels) return vt_fail(VT_ERR_INVALID, "vt_mesh_components: bad argument (V >= 1, F >= 1)");
    if (!workspace || workspace_bytes < MT_STATUS_BYTES) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_components");
    hipStream_t st = (hipStream_t)stream;
    int32_t *status = static_cast<int32_t *>(workspace);
    int rc = vt_fill32(status, 0u, MT_STATUS_BYTES, st);
    if (rc) return rc;
    hipLaunchKernelGGL(init_labels_kernel, dim3(blocks_of(V, MT_THREADS)), dim3(MT_THREADS), 0, st, labels, (int)V);
    int done = 0;
    for (;;) {                                    // until a hooking round met no edge between two roots: no cap
        for (int r = 0; r < MT_ROUND_BATCH; ++r) {
            hipLaunchKernelGGL(hook_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, faces, (int)F, (int)V, labels, status, ST_FLAG0 + r);
            hipLaunchKernelGGL(jump_kernel, dim3(blocks_of(V, MT_THREADS)), dim3(MT_THREADS), 0, st, labels, (int)V);
        }
        rc = vt_check(hipGetLastError(), "vt_mesh_components");
        if (rc) return rc;
        int32_t h[16];
        rc = read_status(workspace, h, st, "vt_mesh_components");
        if (rc) return rc;
        if (h[ST_BAD]) return vt_fail(VT_ERR_INVALID, "vt_mesh_components: a face index lies outside [0, V)");
        int r = 0;
        while (r < MT_ROUND_BATCH && h[ST_FLAG0 + r] != 0) ++r;
        if (r < MT_ROUND_BATCH) { done += r + 1; break; }       // round r changed nothing (nor did the ones behind it)
        done += MT_ROUND_BATCH;
        rc = vt_fill32(status + ST_FLAG0, 0u, 16, st);
        if (rc) return rc;
    }
    if (rounds) *rounds = done;
    return 0;
}

size_t vt_mesh_component_table_workspace_bytes(int64_t V, int64_t F) { return sizes_ok(V, F) ? table_bytes(V) : 0; }

int vt_mesh_component_table(const int32_t *faces, int64_t F, int64_t V, const int32_t *labels, int32_t *comp_of_vertex, int32_t *comp_of_face,
                            int *n_components, void *workspace, size_t workspace_bytes, void *stream) {
    if (!sizes_ok(V, F) || !faces || !labels || !comp_of_vertex || !comp_of_face || !n_components)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_component_table: bad argument (V >= 1, F >= 1)");
    if (!workspace || workspace_bytes < table_bytes(V)) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_component_table");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    int32_t *status = reinterpret_cast<int32_t *>(ws);
    int32_t *ref = reinterpret_cast<int32_t *>(ws + MT_STATUS_BYTES);
    int32_t *rank = reinterpret_cast<int32_t *>(ws + MT_STATUS_BYTES + up256((size_t)V * 4));
    int32_t *bsum = reinterpret_cast<int32_t *>(ws + MT_STATUS_BYTES + 2 * up256((size_t)V * 4));
    int rc = vt_fill32(ws, 0u, MT_STATUS_BYTES + up256((size_t)V * 4), st);                      // the status words and ref
    if (rc) return rc;
    hipLaunchKernelGGL(mark_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, faces, (int)F, (int)V, ref, status);
    scan_launch(RootPred{ref, labels}, V, bsum, rank, status + ST_NCOMP, st);
    hipLaunchKernelGGL(table_vertex_kernel, dim3(blocks_of(V, MT_THREADS)), dim3(MT_THREADS), 0, st, (const int32_t *)ref, labels, (const int32_t *)rank,
                       (int)V, comp_of_vertex, status);
    hipLaunchKernelGGL(table_face_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, faces, (int)F, (int)V, (const int32_t *)comp_of_vertex,
                       comp_of_face);
    rc = vt_check(hipGetLastError(), "vt_mesh_component_table");
    if (rc) return rc;
    int32_t h[16];
    rc = read_status(workspace, h, st, "vt_mesh_component_table");
    if (rc) return rc;
    if (h[ST_BAD] & 1) return vt_fail(VT_ERR_INVALID, "vt_mesh_component_table: a face index lies outside [0, V)");
    if (h[ST_BAD]) return vt_fail(VT_ERR_INVALID, "vt_mesh_component_table: labels are not vt_mesh_components' labels of these faces");
    *n_components = h[ST_NCOMP];
    return 0;
}

size_t vt_mesh_component_stats_workspace_bytes(int64_t C) { return C >= 1 && C <= MT_MAX_V ? stats_bytes(C) : 0; }

int vt_mesh_component_stats(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, const int32_t *comp_of_vertex,
                            const int32_t *comp_of_face, int64_t C, int32_t *n_faces, int32_t *n_vertices, void *bbox, double *area, double *volume,
                            void *workspace, size_t workspace_bytes, void *stream) {
    if (!sizes_ok(V, F) || C < 1 || C > V || !verts || !faces || !comp_of_vertex || !comp_of_face || !n_faces || !n_vertices || !bbox || !area || !volume)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_component_stats: bad argument (V >= 1, F >= 1, 1 <= C <= V)");
    if (!workspace || workspace_bytes < stats_bytes(C)) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_component_stats");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    if (verts_f64)
        stats_launch(static_cast<const double *>(verts), (int)V, faces, (int)F, comp_of_vertex, comp_of_face, (int)C, n_faces, n_vertices,
                     static_cast<double *>(bbox), area, volume, ws, st);
    else
        stats_launch(static_cast<const float *>(verts), (int)V, faces, (int)F, comp_of_vertex, comp_of_face, (int)C, n_faces, n_vertices,
                     static_cast<float *>(bbox), area, volume, ws, st);
    return vt_check(hipGetLastError(), "vt_mesh_component_stats");
}

size_t vt_mesh_edge_stats_workspace_bytes(int64_t F) { return F >= 1 && F <= MT_MAX_F ? (size_t)edge_slots(F) * 16 : 0; }

int vt_mesh_edge_stats(const int32_t *faces, int64_t F, int64_t V, const int32_t *comp_of_vertex, int64_t C, int32_t *n_edges, int32_t *n_boundary,
                       int32_t *n_nonmanifold, int32_t *n_misoriented, void *workspace, size_t workspace_bytes, void *stream) {
    if (!sizes_ok(V, F) || C < 1 || C > V || !faces || !comp_of_vertex || !n_edges || !n_boundary || !n_nonmanifold || !n_misoriented)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_edge_stats: bad argument (V >= 1, F >= 1, 1 <= C <= V)");
    const EdgeTable t = edge_table_at(workspace, F);
    if (!workspace || workspace_bytes < (size_t)t.slots * 16) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_edge_stats");
    hipStream_t st = (hipStream_t)stream;
    int rc = edge_table_clear(t, st);
    int32_t *outs[4] = {n_edges, n_boundary, n_nonmanifold, n_misoriented};
    for (int k = 0; k < 4 && !rc; ++k) rc = vt_fill32(outs[k], 0u, (size_t)C * 4, st);
    if (rc) return rc;
    // (this workspace has no status words: a face with an index outside [0, V) takes no part and is not reported)
    hipLaunchKernelGGL(edge_insert_kernel<false>, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, faces, (int)F, (int)V, t, (int32_t *)nullptr);
    hipLaunchKernelGGL(edge_count_kernel, dim3(blocks_of(t.slots, MT_THREADS)), dim3(MT_THREADS), 0, st, (const u64 *)t.keys, (const u64 *)t.vals, t.slots,
                       comp_of_vertex, (int)V, (int)C, n_edges, n_boundary, n_nonmanifold, n_misoriented);
    return vt_check(hipGetLastError(), "vt_mesh_edge_stats");
}

size_t vt_mesh_filter_workspace_bytes(int64_t V, int64_t F) { return sizes_ok(V, F) ? filter_bytes(V, F) : 0; }

int vt_mesh_filter(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, const int32_t *comp_of_vertex,
                   const int32_t *comp_of_face, const uint8_t *keep, int64_t C, void *out_verts, int32_t *out_faces, int32_t *vertex_map,
                   int *n_out_verts, int *n_out_faces, void *workspace, size_t workspace_bytes, void *stream) {
    if (!sizes_ok(V, F) || C < 1 || C > V || !verts || !faces || !comp_of_vertex || !comp_of_face || !keep || !out_verts || !out_faces || !vertex_map ||
        !n_out_verts || !n_out_faces)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_filter: bad argument (V >= 1, F >= 1, 1 <= C <= V)");
    if (!workspace || workspace_bytes < filter_bytes(V, F)) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_filter");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    int32_t *status = reinterpret_cast<int32_t *>(ws);
    int32_t *fpos = reinterpret_cast<int32_t *>(ws + MT_STATUS_BYTES);
    int32_t *bsum = reinterpret_cast<int32_t *>(ws + MT_STATUS_BYTES + up256((size_t)F * 4));
    int rc = vt_fill32(status, 0u, MT_STATUS_BYTES, st);
    if (rc) return rc;
    if (verts_f64)
        filter_launch(static_cast<const double *>(verts), (int)V, faces, (int)F, comp_of_vertex, comp_of_face, keep, (int)C,
                      static_cast<double *>(out_verts), out_faces, vertex_map, status, bsum, fpos, st);
    else
        filter_launch(static_cast<const float *>(verts), (int)V, faces, (int)F, comp_of_vertex, comp_of_face, keep, (int)C,
                      static_cast<float *>(out_verts), out_faces, vertex_map, status, bsum, fpos, st);
    rc = vt_check(hipGetLastError(), "vt_mesh_filter");
    if (rc) return rc;
    int32_t h[16];
    rc = read_status(workspace, h, st, "vt_mesh_filter");
    if (rc) return rc;
    if (h[ST_BAD] & 1) return vt_fail(VT_ERR_INVALID, "vt_mesh_filter: a face index lies outside [0, V)");
    if (h[ST_BAD]) return vt_fail(VT_ERR_INVALID, "vt_mesh_filter: the component maps are not vt_mesh_component_table's of these faces");
    *n_out_verts = h[ST_NV];
    *n_out_faces = h[ST_NF];
    return 0;
}

}  // extern "C"
