// Vertex adjacency of a triangle mesh as CSR rows, and the Laplacian-type smoothing filters that walk them (DESIGN.md, section
// "mesh_smooth.hip"; tests/mesh_smooth_ref.py is the definition, and every output equals it bit for bit).  faces [F,3] i32 over V vertices.
//   edge table    mesh_edges.h's table.  Every claimed slot is one undirected edge {a, b}, a != b, however many faces share it.
//   count         one lane per slot: integer atomicAdd on the degrees of a and b; scan_launch (mesh_common.h) over the degrees gives
//                 offsets [V+1], in the caller's array and in the workspace at once, and its total, nnz = 2 E <= 6 F, is the one word
//                 the host reads.
//   fill          one lane per slot again: each end takes the next free place of its row from a per-vertex cursor (integer atomicAdd) and
//                 stores the other end and the edge's boundary bit (edge_uses == 1) in a scratch row.  The order within a row is whatever the
//                 atomics gave, so one lane per entry then counts the row's entries below its own -- they are distinct: the count is the
//                 entry's place in ascending order -- and writes neighbors / boundary_edge there.  boundary_vertex is the OR of the row's bits.
//   filter        positions live in float64 buffers of the workspace for all passes and are rounded once at the end.  One lane per vertex
//                 walks its row in ascending neighbour order: s = s + w x_j per coordinate and sw = sw + w, in double and without FMA (the
//                 tree is built with -ffp-contract=off), m = s / sw.  A pass reads one buffer and writes another.  No float atomic, no LDS
//                 reduction.  A mesh of at most 2 048 vertices runs every pass in one launch of one workgroup, the buffers in LDS and a
//                 barrier between passes; the per-vertex functions are the same, and so are the bits.
// A face with an index outside [0, V) is never dereferenced; it takes no part and sets bit 0 of the status word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_common.h"
#include "mesh_edges.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

enum { ST_BAD = 0, ST_NNZ = 1 };                                  // int32 words of the status block
enum { LAPLACIAN = 0, TAUBIN = 1, HUMPHREY = 2 };
enum { PIN = 0, FREE = 1, LOOP = 2 };
constexpr int64_t SM_MAX_F = 0x7fffffff / 6;                       // nnz <= 6 F stays an int32

// (keys hold indices that passed load_face's test: both ends lie in [0, V))
__global__ void __launch_bounds__(MT_THREADS) degree_kernel(const u64 *keys, int64_t slots, int32_t *deg) {
    const int64_t s = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (s >= slots) return;
    const u64 key = keys[s];
    if (key == EDGE_EMPTY) return;
    atomicAdd(deg + (int)(key >> 32), 1);
    atomicAdd(deg + (int)(unsigned)key, 1);
}

// ---- count ------------------------------------------------------------------------------------------------------------------------------------
struct DegreeFn {                                                  // element V is 0: the scan's word V is the total
    const int32_t *deg;
    int64_t V;
    __device__ int operator()(int64_t i) const { return i < V ? deg[i] : 0; }
};

// ---- fill --------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT_THREADS)
scatter_kernel(const u64 *keys, const u64 *vals, int64_t slots, int32_t *cursor, int nnz, int32_t *raw_nb, uint8_t *raw_be) {
    const int64_t s = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (s >= slots) return;
    const u64 key = keys[s];
    if (key == EDGE_EMPTY) return;
    const int a = (int)(key >> 32), b = (int)(unsigned)key;
    const uint8_t be = edge_uses(vals[s]) == 1;
    const int pa = atomicAdd(cursor + a, 1), pb = atomicAdd(cursor + b, 1);
    if ((unsigned)pa < (unsigned)nnz) { raw_nb[pa] = b; raw_be[pa] = be; }     // (a cursor ends at its row's end: the test never fails on
    if ((unsigned)pb < (unsigned)nnz) { raw_nb[pb] = a; raw_be[pb] = be; }     //  the workspace vt_mesh_adjacency_count left for these faces)
}

// the last v in [0, V) with off[v] <= p: the row that owns entry p (rows in front of it that end at p are empty)
__device__ inline int row_of(const int32_t *off, int V, int p) {
    int lo = 0, hi = V;
    while (hi - lo > 1) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(MT_THREADS)
rank_kernel(const int32_t *off, int V, int nnz, const int32_t *raw_nb, const uint8_t *raw_be, int32_t *neighbors, uint8_t *boundary_edge) {
    const int64_t p = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (p >= nnz) return;
    const int v = row_of(off, V, (int)p);
    const int o = max(off[v], 0), e = min(off[v + 1], nnz);
    const int mine = raw_nb[p];
    int rank = 0;
    for (int k = o; k < e; ++k) rank += raw_nb[k] < mine ? 1 : 0;
    if (o + rank < e) { neighbors[o + rank] = mine; boundary_edge[o + rank] = raw_be[p]; }
}

__global__ void __launch_bounds__(MT_THREADS)
boundary_vertex_kernel(const int32_t *off, int V, int nnz, const uint8_t *raw_be, uint8_t *boundary_vertex) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v >= V) return;
    const int o = max(off[v], 0), e = min(off[v + 1], nnz);
    uint8_t any = 0;
    for (int k = o; k < e; ++k) any |= raw_be[k];
    boundary_vertex[v] = any;
}

// ---- weights ---------------------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(MT_THREADS)
weights_kernel(const T *verts, const int32_t *off, const int32_t *neighbors, int V, int nnz, int scheme, double *w) {
    const int64_t p = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (p >= nnz) return;
    double out = 1.0;
    if (scheme == 1) {
        const int i = row_of(off, V, (int)p), j = neighbors[p];
        out = 0.0;
        if ((unsigned)j < (unsigned)V) {
            double xi, yi, zi, xj, yj, zj;
            load_vertex(verts, i, xi, yi, zi);
            load_vertex(verts, j, xj, yj, zj);
            const double dx = xj - xi, dy = yj - yi, dz = zj - zi;
            const double d = sqrt((dx * dx + dy * dy) + dz * dz);
            if (d > 0.0) out = 1.0 / d;                            // a coincident neighbour, and a NaN distance, weigh nothing
        }
    }
    w[p] = out;
}

// ---- the filter --------------------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(MT_THREADS) to_double_kernel(const T *src, int64_t n, double *dst) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < n) dst[i] = (double)src[i];
}

template <class T>
__global__ void __launch_bounds__(MT_THREADS) from_double_kernel(const double *src, int64_t n, T *dst) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < n) dst[i] = (T)src[i];
}

struct Rows {
    const int32_t *off, *neighbors;
    const uint8_t *boundary_edge, *boundary_vertex;
    const double *w;                                               // nullptr: uniform
    int V, nnz, rule;
};

// the row mean of `src` at vertex i; false when the vertex keeps its position (pinned, an empty row or a zero weight sum)
template <bool WEIGHTED>
__device__ inline bool row_mean(const Rows &r, const double *src, int i, double (&m)[3]) {
    const bool bv = r.rule != FREE && r.boundary_vertex[i] != 0;
    if (bv && r.rule == PIN) return false;
    const bool along = bv && r.rule == LOOP;                       // only the neighbours across boundary edges
    const int o = max(r.off[i], 0), e = min(r.off[i + 1], r.nnz);
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
    for (int k = o; k < e; ++k) {
        if (along && !r.boundary_edge[k]) continue;
        const int j = r.neighbors[k];
        if ((unsigned)j >= (unsigned)r.V) continue;               // (rows that are not vt_mesh_adjacency_fill's)
        const double *p = src + (size_t)j * 3;
        if (WEIGHTED) {
            const double w = r.w[k];
            if (w == 0.0) continue;
            sx = sx + w * p[0]; sy = sy + w * p[1]; sz = sz + w * p[2];
            sw = sw + w;
        } else {
            sx = sx + p[0]; sy = sy + p[1]; sz = sz + p[2];
            sw = sw + 1.0;
        }
    }
    if (!(sw > 0.0)) return false;
    m[0] = sx / sw; m[1] = sy / sw; m[2] = sz / sw;
    return true;
}

// The three per-vertex steps, shared by the many-launch kernels and the single-workgroup kernel (equal expressions: equal bits).
// x <- x + c (m(x) - x)
template <bool WEIGHTED>
__device__ inline void laplacian_vertex(const Rows &r, const double *in, int i, double c, double *out) {
    double m[3];
    const bool moves = row_mean<WEIGHTED>(r, in, i, m);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double xa = in[(size_t)i * 3 + a];
        out[(size_t)i * 3 + a] = moves ? xa + c * (m[a] - xa) : xa;
    }
}

// Humphrey, first half: x <- m(q), b <- x - (alpha o + (1 - alpha) q), o the input positions
template <class T, bool WEIGHTED>
__device__ inline void humphrey_mean_vertex(const Rows &r, const T *orig, const double *q, int i, double alpha, double one_minus_alpha, double *x,
                                            double *b) {
    double m[3];
    const bool moves = row_mean<WEIGHTED>(r, q, i, m);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double qa = q[(size_t)i * 3 + a], oa = (double)orig[(size_t)i * 3 + a];
        const double xa = moves ? m[a] : qa;
        x[(size_t)i * 3 + a] = xa;
        b[(size_t)i * 3 + a] = xa - (alpha * oa + one_minus_alpha * qa);
    }
}

// Humphrey, second half: x <- x - (beta b + (1 - beta) m(b))
template <bool WEIGHTED>
__device__ inline void humphrey_back_vertex(const Rows &r, const double *x, const double *b, int i, double beta, double one_minus_beta, double *out) {
    double m[3];
    const bool moves = row_mean<WEIGHTED>(r, b, i, m);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double xa = x[(size_t)i * 3 + a];
        out[(size_t)i * 3 + a] = moves ? xa - (beta * b[(size_t)i * 3 + a] + one_minus_beta * m[a]) : xa;
    }
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(MT_THREADS) laplacian_kernel(Rows r, const double *in, double c, double *out) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < r.V) laplacian_vertex<WEIGHTED>(r, in, (int)i, c, out);
}

template <class T, bool WEIGHTED>
__global__ void __launch_bounds__(MT_THREADS)
humphrey_mean_kernel(Rows r, const T *orig, const double *q, double alpha, double one_minus_alpha, double *x, double *b) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < r.V) humphrey_mean_vertex<T, WEIGHTED>(r, orig, q, (int)i, alpha, one_minus_alpha, x, b);
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(MT_THREADS)
humphrey_back_kernel(Rows r, const double *x, const double *b, double beta, double one_minus_beta, double *out) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < r.V) humphrey_back_vertex<WEIGHTED>(r, x, b, (int)i, beta, one_minus_beta, out);
}

// Every pass in one launch, for a mesh whose float64 positions fit in LDS (V <= SM_LDS_MAX_V: three buffers of 24 V bytes): one workgroup,
// the buffers in LDS, a barrier where the many-launch form has a kernel boundary.  The rows are still read from memory.
constexpr int SM_LDS_THREADS = 1024;
constexpr int SM_LDS_MAX_V = 2048;                                 // 3 x 24 x 2048 = 147 456 of the 163 840 bytes of LDS

struct Coefficients {
    double lam, mu, alpha, one_minus_alpha, beta, one_minus_beta;
};

template <class T, bool WEIGHTED>
__global__ void __launch_bounds__(SM_LDS_THREADS) smooth_lds_kernel(Rows r, const T *verts, int method, int iterations, Coefficients k, T *out_verts) {
    extern __shared__ double lds[];
    const int n = r.V * 3;
    double *cur = lds, *other = lds + n, *b = lds + 2 * n;        // (b is there for Humphrey only: the launcher asks for 2 n or 3 n doubles)
    for (int i = threadIdx.x; i < n; i += SM_LDS_THREADS) cur[i] = (double)verts[i];
    __syncthreads();
    if (method == HUMPHREY) {
        for (int it = 0; it < iterations; ++it) {
            for (int i = threadIdx.x; i < r.V; i += SM_LDS_THREADS) humphrey_mean_vertex<T, WEIGHTED>(r, verts, cur, i, k.alpha, k.one_minus_alpha, other, b);
            __syncthreads();
            for (int i = threadIdx.x; i < r.V; i += SM_LDS_THREADS) humphrey_back_vertex<WEIGHTED>(r, other, b, i, k.beta, k.one_minus_beta, cur);
            __syncthreads();
        }
    } else {
        const int passes = method == TAUBIN ? 2 * iterations : iterations;
        for (int p = 0; p < passes; ++p) {
            const double c = (method == TAUBIN && (p & 1)) ? k.mu : k.lam;
            for (int i = threadIdx.x; i < r.V; i += SM_LDS_THREADS) laplacian_vertex<WEIGHTED>(r, cur, i, c, other);
            __syncthreads();
            double *t = cur; cur = other; other = t;
        }
    }
    for (int i = threadIdx.x; i < n; i += SM_LDS_THREADS) out_verts[i] = (T)cur[i];
}

// ---- the workspaces -----------------------------------------------------------------------------------------------------------------------------
bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && F >= 1 && V <= MT_MAX_V && F <= SM_MAX_F; }

// status | table | degrees, later the cursors | offsets | the unsorted rows | scan sums
struct AdjWs {
    int32_t *status, *deg, *off, *raw_nb, *bsum;
    EdgeTable t;
    uint8_t *raw_be;
    size_t bytes;
};

AdjWs adj_ws(void *workspace, int64_t V, int64_t F) {
    AdjWs w;
    char *p = static_cast<char *>(workspace);
    size_t at = 0;
    w.status = reinterpret_cast<int32_t *>(p); at += MT_STATUS_BYTES;
    w.t = edge_table_at(p + at, F); at += (size_t)w.t.slots * 16;
    w.deg = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)(V + 1) * 4);
    w.off = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)(V + 1) * 4);
    w.raw_nb = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)F * 6 * 4);
    w.raw_be = reinterpret_cast<uint8_t *>(p + at); at += up256((size_t)F * 6);
    w.bsum = reinterpret_cast<int32_t *>(p + at); at += scan_bytes(V + 1);
    w.bytes = at;
    return w;
}

size_t smooth_bytes(int64_t V) { return 3 * up256((size_t)V * 3 * 8); }

template <class T, bool WEIGHTED>
int smooth_launch(const T *verts, const Rows &r, int method, int iterations, double lam, double mu, double alpha, double beta, T *out_verts,
                  bool one_workgroup, void *workspace, hipStream_t st) {
    if (one_workgroup) {
        const void *fn = reinterpret_cast<const void *>(&smooth_lds_kernel<T, WEIGHTED>);
        const int lds = r.V * 3 * 8 * (method == HUMPHREY ? 3 : 2);                    // at most 147 456 bytes: V <= SM_LDS_MAX_V
        if (lds > 64 * 1024) {
            const hipError_t e = vt_max_dyn_lds(fn, 160 * 1024);
            if (e != hipSuccess) return vt_check(e, "vt_mesh_smooth: hipFuncSetAttribute");
        }
        const Coefficients k{lam, mu, alpha, 1.0 - alpha, beta, 1.0 - beta};
        hipLaunchKernelGGL((smooth_lds_kernel<T, WEIGHTED>), dim3(1), dim3(SM_LDS_THREADS), lds, st, r, verts, method, iterations, k, out_verts);
        return 0;
    }
    const int64_t n = (int64_t)r.V * 3;
    const size_t stride = up256((size_t)n * 8);
    char *p = static_cast<char *>(workspace);
    double *x0 = reinterpret_cast<double *>(p), *x1 = reinterpret_cast<double *>(p + stride), *b = reinterpret_cast<double *>(p + 2 * stride);
    const dim3 block(MT_THREADS), vgrid(blocks_of(r.V, MT_THREADS)), ngrid(blocks_of(n, MT_THREADS));
    hipLaunchKernelGGL(to_double_kernel<T>, ngrid, block, 0, st, verts, n, x0);
    double *cur = x0, *other = x1;                                 // every pass reads `cur` and leaves its result there again
    if (method == HUMPHREY) {
        for (int it = 0; it < iterations; ++it) {                  // q = cur; x in `other`; back into cur
            hipLaunchKernelGGL((humphrey_mean_kernel<T, WEIGHTED>), vgrid, block, 0, st, r, verts, (const double *)cur, alpha, 1.0 - alpha, other, b);
            hipLaunchKernelGGL(humphrey_back_kernel<WEIGHTED>, vgrid, block, 0, st, r, (const double *)other, (const double *)b, beta, 1.0 - beta, cur);
        }
    } else {
        const int passes = method == TAUBIN ? 2 * iterations : iterations;
        for (int k = 0; k < passes; ++k) {
            const double c = (method == TAUBIN && (k & 1)) ? mu : lam;
            hipLaunchKernelGGL(laplacian_kernel<WEIGHTED>, vgrid, block, 0, st, r, (const double *)cur, c, other);
            double *t = cur; cur = other; other = t;
        }
    }
    hipLaunchKernelGGL(from_double_kernel<T>, ngrid, block, 0, st, (const double *)cur, n, out_verts);
    return 0;
}

}  // namespace

extern "C" {

size_t vt_mesh_adjacency_workspace_bytes(int64_t V, int64_t F) { return sizes_ok(V, F) ? adj_ws(nullptr, V, F).bytes : 0; }

int vt_mesh_adjacency_count(const int32_t *faces, int64_t F, int64_t V, int32_t *offsets, int *nnz, void *workspace, size_t workspace_bytes,
                            void *stream) {
    if (F > SM_MAX_F)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_adjacency_count: F is above 357913941 = (2^31 - 1) / 6: the int32 offsets could not hold nnz <= 6 F");
    if (!sizes_ok(V, F) || !faces || !offsets || !nnz) return vt_fail(VT_ERR_INVALID, "vt_mesh_adjacency_count: bad argument (V >= 1, F >= 1)");
    if (!workspace || workspace_bytes < adj_ws(nullptr, V, F).bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_adjacency_count");
    hipStream_t st = (hipStream_t)stream;
    const AdjWs w = adj_ws(workspace, V, F);
    int rc = vt_fill32(w.status, 0u, MT_STATUS_BYTES, st);
    if (!rc) rc = edge_table_clear(w.t, st);
    if (!rc) rc = vt_fill32(w.deg, 0u, up256((size_t)(V + 1) * 4), st);
    if (rc) return rc;
    const dim3 block(MT_THREADS);
    hipLaunchKernelGGL(edge_insert_kernel<true>, dim3(blocks_of(F, MT_THREADS)), block, 0, st, faces, (int)F, (int)V, w.t, w.status + ST_BAD);
    hipLaunchKernelGGL(degree_kernel, dim3(blocks_of(w.t.slots, MT_THREADS)), block, 0, st, (const u64 *)w.t.keys, w.t.slots, w.deg);
    scan_launch(DegreeFn{w.deg, V}, V + 1, w.bsum, offsets, w.status + ST_NNZ, st, w.off);
    rc = vt_check(hipGetLastError(), "vt_mesh_adjacency_count");
    if (rc) return rc;
    int32_t h[32];
    rc = read_status(workspace, h, st, "vt_mesh_adjacency_count");
    if (rc) return rc;
    if (h[ST_BAD]) return vt_fail(VT_ERR_INVALID, "vt_mesh_adjacency_count: a face index lies outside [0, V)");
    if (h[ST_NNZ] < 0 || h[ST_NNZ] > 6 * F) return vt_fail(VT_ERR_INVALID, "vt_mesh_adjacency_count: nnz outside [0, 6 F]");
    *nnz = h[ST_NNZ];
    return 0;
}

int vt_mesh_adjacency_fill(int64_t F, int64_t V, int64_t nnz, int32_t *neighbors, uint8_t *boundary_edge, uint8_t *boundary_vertex, void *workspace,
                           size_t workspace_bytes, void *stream) {
    if (!sizes_ok(V, F) || nnz < 1 || nnz > 6 * F || !neighbors || !boundary_edge || !boundary_vertex)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_adjacency_fill: bad argument (V >= 1, F >= 1, 1 <= nnz <= 6 F)");
    if (!workspace || workspace_bytes < adj_ws(nullptr, V, F).bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_adjacency_fill");
    hipStream_t st = (hipStream_t)stream;
    const AdjWs w = adj_ws(workspace, V, F);
    const dim3 block(MT_THREADS);
    // the cursors start at the rows' offsets (the degrees are not needed again)
    copy_words(w.off, (size_t)V * 4, w.deg, st);
    hipLaunchKernelGGL(scatter_kernel, dim3(blocks_of(w.t.slots, MT_THREADS)), block, 0, st, (const u64 *)w.t.keys, (const u64 *)w.t.vals, w.t.slots, w.deg,
                       (int)nnz, w.raw_nb, w.raw_be);
    hipLaunchKernelGGL(rank_kernel, dim3(blocks_of(nnz, MT_THREADS)), block, 0, st, (const int32_t *)w.off, (int)V, (int)nnz, (const int32_t *)w.raw_nb,
                       (const uint8_t *)w.raw_be, neighbors, boundary_edge);
    hipLaunchKernelGGL(boundary_vertex_kernel, dim3(blocks_of(V, MT_THREADS)), block, 0, st, (const int32_t *)w.off, (int)V, (int)nnz,
                       (const uint8_t *)w.raw_be, boundary_vertex);
    return vt_check(hipGetLastError(), "vt_mesh_adjacency_fill");
}

int vt_mesh_smooth_weights(const void *verts, int verts_f64, int64_t V, const int32_t *offsets, const int32_t *neighbors, int64_t nnz, int scheme,
                           double *w, void *stream) {
    if (V < 1 || V > MT_MAX_V || nnz < 1 || nnz > 0x7fffffff || (scheme != 0 && scheme != 1) || !verts || !offsets || !neighbors || !w)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_smooth_weights: bad argument (V >= 1, nnz >= 1, scheme 0 or 1)");
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(MT_THREADS), grid(blocks_of(nnz, MT_THREADS));
    if (verts_f64)
        hipLaunchKernelGGL(weights_kernel<double>, grid, block, 0, st, static_cast<const double *>(verts), offsets, neighbors, (int)V, (int)nnz, scheme, w);
    else
        hipLaunchKernelGGL(weights_kernel<float>, grid, block, 0, st, static_cast<const float *>(verts), offsets, neighbors, (int)V, (int)nnz, scheme, w);
    return vt_check(hipGetLastError(), "vt_mesh_smooth_weights");
}

size_t vt_mesh_smooth_workspace_bytes(int64_t V) { return V >= 1 && V <= MT_MAX_V ? smooth_bytes(V) : 0; }

int vt_mesh_smooth(const void *verts, int verts_f64, int64_t V, const int32_t *offsets, const int32_t *neighbors, const uint8_t *boundary_edge,
                   const uint8_t *boundary_vertex, int64_t nnz, const double *w, int method, int iterations, double lam, double mu, double alpha,
                   double beta, int boundary, int form, void *out_verts, void *workspace, size_t workspace_bytes, void *stream) {
    if (V < 1 || V > MT_MAX_V || nnz < 0 || nnz > 0x7fffffff || method < 0 || method > 2 || iterations < 0 || boundary < 0 || boundary > 2 || form < 0 ||
        form > 2 || !verts || !out_verts || !offsets || !boundary_vertex || (nnz && (!neighbors || !boundary_edge)))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_smooth: bad argument (V >= 1, nnz >= 0, method 0..2, iterations >= 0, boundary 0..2, form 0..2)");
    if (form == 2 && V > SM_LDS_MAX_V) return vt_fail(VT_ERR_INVALID, "vt_mesh_smooth: form 2 (one workgroup) holds at most 2048 vertices");
    if (!(lam == lam) || !(mu == mu) || !(alpha == alpha) || !(beta == beta)) return vt_fail(VT_ERR_INVALID, "vt_mesh_smooth: a NaN coefficient");
    hipStream_t st = (hipStream_t)stream;
    if (iterations == 0 || nnz == 0) {                             // nothing moves: the input's bits
        copy_words(verts, (size_t)V * 3 * (verts_f64 ? 8 : 4), out_verts, st);
        return vt_check(hipGetLastError(), "vt_mesh_smooth");
    }
    const bool one = form == 2 || (form == 0 && V <= SM_LDS_MAX_V);
    if (!one && (!workspace || workspace_bytes < smooth_bytes(V))) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_smooth");
    const Rows r{offsets, neighbors, boundary_edge, boundary_vertex, w, (int)V, (int)nnz, boundary};
    int rc;
    if (verts_f64) {
        const double *v = static_cast<const double *>(verts);
        double *o = static_cast<double *>(out_verts);
        rc = w ? smooth_launch<double, true>(v, r, method, iterations, lam, mu, alpha, beta, o, one, workspace, st)
               : smooth_launch<double, false>(v, r, method, iterations, lam, mu, alpha, beta, o, one, workspace, st);
    } else {
        const float *v = static_cast<const float *>(verts);
        float *o = static_cast<float *>(out_verts);
        rc = w ? smooth_launch<float, true>(v, r, method, iterations, lam, mu, alpha, beta, o, one, workspace, st)
               : smooth_launch<float, false>(v, r, method, iterations, lam, mu, alpha, beta, o, one, workspace, st);
    }
    return rc ? rc : vt_check(hipGetLastError(), "vt_mesh_smooth");
}

}  // extern "C"
