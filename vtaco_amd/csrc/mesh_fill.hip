// Hole filling of a triangle mesh on the device: the boundary half-edges, their loops, and the cap of every loop (DESIGN.md, section
// "mesh_fill.hip"; tests/mesh_fill_ref.py is the definition, and every output equals it bit for bit).  faces [F,3] i32 over V vertices,
// f32 or f64.  Half-edge h = 3 f + k runs from faces[f][k] (tail) to faces[f][(k+1)%3] (head); flat, its tail is faces[h].
//   edge table    mesh_edges.h's table.  A half-edge is a boundary half-edge when its edge's two counts add up to 1 (its own use).
//                 One byte per half-edge, then scan_launch (mesh_common.h) over the 3 F bytes: the
//                 compacted list keeps half-edge order, so "lowest compacted index" and "lowest half-edge" are one thing from here on.
//   degrees       per vertex the boundary half-edges out of it and into it (integer atomicAdd) and the lowest one out of it (atomicMin).
//                 succ[i] = that one at head(i) when the head has one of each, DEAD otherwise.  succ is injective where defined: only
//                 the one half-edge that enters a regular vertex maps to the one that leaves it.  So the list falls into cycles (the
//                 loops) and paths that end in DEAD (the irregular edges).
//   doubling      state (nxt, mn) per element: mn = the smallest element of the span [i, nxt).  A round reads one buffer and writes the
//                 other: mn = min(mn, mn[nxt]), nxt = nxt[nxt]; after r rounds the span has 2^r elements or has run into DEAD.  With
//                 2^R >= NB a cycle's span covers the cycle (mn = its smallest element, the loop's head) and every path has reached DEAD.
//                 A second run of R rounds over the cycles cut in front of their heads adds up distances: d = the steps to the loop's
//                 last element, so the position of i is d[head] - d[i] and the loop's length d[head] + 1.  All 2 R rounds are enqueued
//                 at once; no round is read back.
//   outputs       one scan_launch with u64 sums over the list, (1 << 32 | length) at the heads: the loop number and the loop's offset of every head.
//   emit          per loop (new vertices << 32 | new faces), scanned; one lane per new face finds its loop by bisection of the scanned
//                 face offsets.  The centroid is mesh_topo.hip's exact sum: the largest |coordinate| of the loop by atomicMax on the bit
//                 pattern, then every coordinate as two int64 fixed-point limbs by integer atomicAdd, rounded once, divided by n in
//                 float64 and rounded to the vertices' type.  No float atomic; equal bits from run to run.
// A face with an index outside [0, V) is never dereferenced; it takes no part and sets bit 0 of the status word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mesh_common.h"
#include "mesh_edges.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

// int32 words of the status block; ST_TOTAL is the index of a 64-bit word (bytes 64..71)
enum { ST_BAD = 0, ST_NB = 8, ST_NFILLED = 9, ST_TOTAL = 8 };
constexpr int DEAD = -1;

// ---- stage 1: the edge table and the boundary flags ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT_THREADS)
edge_flag_kernel(const int32_t *faces, int F, int V, EdgeTable t, uint8_t *flag) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    uint8_t f0 = 0, f1 = 0, f2 = 0;
    if (ok) {
        f0 = edge_uses(t, a, b) == 1;
        f1 = edge_uses(t, b, c) == 1;
        f2 = edge_uses(t, c, a) == 1;
    }
    uint8_t *p = flag + (size_t)f * 3;                         // f < F: inside the 3 F bytes
    p[0] = f0; p[1] = f1; p[2] = f2;
}

struct FlagPred {
    const uint8_t *flag;
    __device__ bool operator()(int64_t h) const { return flag[h] != 0; }
};

__global__ void __launch_bounds__(MT_THREADS) compact_kernel(const uint8_t *flag, const int32_t *pos, int64_t H, int32_t *bhe) {
    const int64_t h = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (h < H && flag[h]) bhe[pos[h]] = (int32_t)h;            // pos[h] < the number of flags <= H: inside the capacity-H list
}

// ---- stage 2: vertex degrees and succ ------------------------------------------------------------------------------------------------------
__device__ inline int head_of(const int32_t *faces, int h) {
    const int k = h % 3;
    return faces[k == 2 ? h - 2 : h + 1];
}

__global__ void __launch_bounds__(MT_THREADS)
degree_kernel(const int32_t *faces, const int32_t *bhe, int NB, int32_t *vout, int32_t *vin, int32_t *vfirst) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= NB) return;
    const int h = bhe[i];
    const int tail = faces[h], head = head_of(faces, h);      // (flagged half-edges belong to faces whose indices lie in [0, V))
    atomicAdd(vout + tail, 1);
    atomicAdd(vin + head, 1);
    atomicMin(vfirst + tail, (int)i);
}

__global__ void __launch_bounds__(MT_THREADS)
succ_kernel(const int32_t *faces, const int32_t *bhe, int NB, const int32_t *vout, const int32_t *vin, const int32_t *vfirst, int32_t *succ) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= NB) return;
    const int head = head_of(faces, bhe[i]);
    succ[i] = (vout[head] == 1 && vin[head] == 1) ? vfirst[head] : DEAD;
}

// ---- stage 3: pointer doubling ---------------------------------------------------------------------------------------------------------------
struct MinOp { __device__ static int combine(int a, int b) { return min(a, b); } };
struct AddOp { __device__ static int combine(int a, int b) { return a + b; } };

__global__ void __launch_bounds__(MT_THREADS) min_init_kernel(const int32_t *succ, int NB, int2 *out) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < NB) out[i] = make_int2(succ[i], (int)i);
}

// one round: `in` is only read, `out` only written (jumping in place would race between workgroups)
template <class Op>
__global__ void __launch_bounds__(MT_THREADS) jump_kernel(const int2 *in, int NB, int2 *out) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= NB) return;
    int2 s = in[i];
    if ((unsigned)s.x < (unsigned)NB) {
        const int2 t = in[s.x];
        s.y = Op::combine(s.y, t.y);
        s.x = t.x;
    }
    out[i] = s;
}

// the cycles cut in front of their heads: (nxt, d), d the steps to the end of the list as far as nxt
__global__ void __launch_bounds__(MT_THREADS) rank_init_kernel(const int32_t *succ, const int2 *mins, int NB, int2 *out) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= NB) return;
    int nxt = DEAD;
    if (mins[i].x != DEAD) {                                   // on a cycle: succ[i] is an element, and on the same cycle
        const int s = succ[i];
        if ((unsigned)s < (unsigned)NB && mins[s].y != s) nxt = s;
    }
    out[i] = make_int2(nxt, nxt == DEAD ? 0 : 1);
}

// ---- stage 4: loop numbers, offsets and the lists --------------------------------------------------------------------------------------------
struct HeadFn {                                                // (1 << 32 | the loop's length) at a loop's head
    const int2 *mins, *ranks;
    __device__ u64 operator()(int64_t i) const {
        const int2 m = mins[i];
        return (m.x != DEAD && m.y == (int)i) ? (1ull << 32 | (u64)(unsigned)(ranks[i].y + 1)) : 0ull;
    }
};

__global__ void __launch_bounds__(MT_THREADS)
loops_write_kernel(const int32_t *faces, const int32_t *bhe, const int2 *mins, const int2 *ranks, const u64 *scan, const u64 *total, int NB,
                   int32_t *loop_offsets, int32_t *loop_vertices, int32_t *loop_half_edges) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= NB) return;
    if (i == 0) loop_offsets[(int)(*total >> 32)] = (int)(unsigned)*total;     // L <= NB: inside the capacity NB + 1
    const int2 m = mins[i];
    if (m.x == DEAD) return;
    const int head = m.y;
    if ((unsigned)head >= (unsigned)NB) return;
    const u64 s = scan[head];
    const int l = (int)(s >> 32), off = (int)(unsigned)s;
    const int at = off + (ranks[head].y - ranks[i].y);
    if ((unsigned)at >= (unsigned)NB || (unsigned)l >= (unsigned)NB) return;    // (cannot happen: the loops' lengths add up to at most NB)
    const int h = bhe[i];
    loop_half_edges[at] = h;
    loop_vertices[at] = faces[h];
    if (head == (int)i) loop_offsets[l] = off;
}

// ---- stage 5: the caps ---------------------------------------------------------------------------------------------------------------------------
struct FillFn {                                                // (new vertices << 32 | new faces) of a loop
    const int32_t *off;
    int method;
    int64_t max_edges;
    __device__ bool filled(int64_t l) const {
        const int n = off[l + 1] - off[l];
        return n >= 3 && (max_edges <= 0 || n <= max_edges);
    }
    __device__ u64 operator()(int64_t l) const {
        const int n = off[l + 1] - off[l];
        if (!filled(l)) return 0;
        if (n == 3) return 1;
        return method == 0 ? (u64)(n - 2) : (1ull << 32 | (u64)n);
    }
};

__global__ void __launch_bounds__(MT_THREADS) filled_count_kernel(FillFn fn, int L, int32_t *status) {
    const int64_t l = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    const int n = __popcll(__ballot(l < L && fn.filled(l)));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(status + ST_NFILLED, n);
}

// the last l in [0, L) with key(l) <= x, key ascending and key(0) <= x
template <class Key>
__device__ inline int last_not_above(Key key, int L, unsigned x) {
    int lo = 0, hi = L;                                        // key(lo) <= x < key(hi) (hi = L: past the end)
    while (hi - lo > 1) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (key(mid) <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(MT_THREADS)
emit_face_kernel(const int32_t *off, const int32_t *loop_vertices, const u64 *fv, int L, int V, int64_t F, int NNF, int32_t *out_faces) {
    const int64_t j = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (j >= NNF) return;
    const int l = last_not_above([fv](int m) { return (unsigned)fv[m]; }, L, (unsigned)j);
    const u64 s = fv[l], e = fv[l + 1];                        // (fv has L + 1 words: the last is the total)
    const int o = off[l], n = off[l + 1] - o;
    int i = (int)j - (int)(unsigned)s;
    if (n < 3 || i < 0 || i >= n) return;                      // (offsets that are not vt_mesh_fill_count's of these loops)
    int a;
    if ((e >> 32) != (s >> 32)) a = V + (int)(s >> 32);        // the loop's new vertex
    else { a = loop_vertices[o]; i += 1; }                     // the fan about v_0: i = 1 .. n - 2
    const int i1 = i + 1 == n ? 0 : i + 1;
    int32_t *p = out_faces + (size_t)(F + j) * 3;
    p[0] = a; p[1] = loop_vertices[o + i1]; p[2] = loop_vertices[o + i];
}

struct MaxOp3 {                                                // the largest |x|, |y|, |z| as bit patterns
    __device__ static u64 identity(int) { return 0; }
    __device__ static u64 combine(int, u64 a, u64 b) { return a > b ? a : b; }
    __device__ static void atomic(int, u64 *p, u64 v) { atomicMax(p, v); }
};
struct SumOp6 {                                                // limbs hi, lo of x, y, z (two's complement)
    __device__ static u64 identity(int) { return 0; }
    __device__ static u64 combine(int, u64 a, u64 b) { return a + b; }
    __device__ static void atomic(int, u64 *p, u64 v) { atomicAdd(p, v); }
};

// PASS 0: the largest |coordinate| per (new vertex, axis); PASS 1: the fixed-point sums against them.  One item per new face: face i of a
// loop with a new vertex stands for the loop's element i, so the loop is found as emit_face_kernel finds it
template <class T, int PASS>
__global__ void __launch_bounds__(MT_THREADS)
centroid_kernel(const T *verts, int V, const int32_t *off, const int32_t *loop_vertices, const u64 *fv, int L, int NNF, int NNV, u64 *cmax, u64 *csum) {
    constexpr int K = PASS == 0 ? 3 : 6;
    using Op = typename std::conditional<PASS == 0, MaxOp3, SumOp6>::type;
    u64 *table = PASS == 0 ? cmax : csum;
    int cur = -1;
    u64 acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0;
    const int64_t base = (int64_t)blockIdx.x * MT_CHUNK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        const int64_t j = base + (int64_t)k * MT_THREADS;
        int c = -1;
        u64 x[K];
#pragma unroll
        for (int a = 0; a < K; ++a) x[a] = 0;
        if (j < NNF) {
            const int l = last_not_above([fv](int m) { return (unsigned)fv[m]; }, L, (unsigned)j);
            const u64 s = fv[l], t = fv[l + 1];
            const int o = off[l], n = off[l + 1] - o, i = (int)j - (int)(unsigned)s;
            if ((t >> 32) != (s >> 32) && (int)(s >> 32) < NNV && i >= 0 && i < n) {
                const int v = loop_vertices[o + i];
                if ((unsigned)v < (unsigned)V) {
                    c = (int)(s >> 32);
                    double p[3];
                    load_vertex(verts, v, p[0], p[1], p[2]);
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        if (PASS == 0) x[a] = (u64)__double_as_longlong(fabs(p[a]));
                        else limbs_of(p[a], exponent_of(cmax[(size_t)c * 3 + a]), x[2 * a], x[2 * a + 1]);
                    }
                }
            }
        }
        accumulate<K, Op>(cur, acc, c, x, table);
    }
    wave_flush<K, Op>(cur, acc, table);
}

template <class T>
__global__ void __launch_bounds__(MT_THREADS)
centroid_finish_kernel(const int32_t *off, const u64 *fv, int L, int V, int NNV, const u64 *cmax, const u64 *csum, T *out_verts) {
    const int64_t l = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (l >= L) return;
    const u64 s = fv[l], t = fv[l + 1];
    const int c = (int)(s >> 32);
    if ((t >> 32) == (s >> 32) || c >= NNV) return;
    const double n = (double)(off[l + 1] - off[l]);
    for (int a = 0; a < 3; ++a) {
        const double sum = sum_of(csum[(size_t)c * 6 + 2 * a], csum[(size_t)c * 6 + 2 * a + 1], exponent_of(cmax[(size_t)c * 3 + a]));
        out_verts[(size_t)(V + c) * 3 + a] = (T)(sum / n);
    }
}

// ---- the workspaces -----------------------------------------------------------------------------------------------------------------------------
bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && F >= 1 && V <= MT_MAX_V && F <= MT_MAX_F; }

// status | table, later the two doubling buffers B, C | pos, later the doubling buffer A | flag | bhe | succ | vout, vin, vfirst | scan sums
struct BoundaryWs {
    int32_t *status;
    EdgeTable t;
    u64 *vsum, *total;
    int2 *bufA, *bufB, *bufC;
    int32_t *pos, *bhe, *succ, *vout, *vin, *vfirst, *bsum;
    uint8_t *flag;
    size_t bytes;
};

BoundaryWs boundary_ws(void *workspace, int64_t V, int64_t F) {
    BoundaryWs w;
    const int64_t H = 3 * F;
    char *p = static_cast<char *>(workspace);
    size_t at = 0;
    w.status = reinterpret_cast<int32_t *>(p);
    w.total = reinterpret_cast<u64 *>(p + ST_TOTAL * 8);
    at += MT_STATUS_BYTES;
    w.t = edge_table_at(p + at, F);
    const size_t table = (size_t)w.t.slots * 16, two = 2 * up256((size_t)H * 8);
    w.bufB = reinterpret_cast<int2 *>(p + at);
    w.bufC = reinterpret_cast<int2 *>(p + at + up256((size_t)H * 8));
    at += table > two ? table : two;
    w.pos = reinterpret_cast<int32_t *>(p + at);
    w.bufA = reinterpret_cast<int2 *>(p + at);
    at += up256((size_t)H * 8);
    w.flag = reinterpret_cast<uint8_t *>(p + at); at += up256((size_t)H);
    w.bhe = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)H * 4);
    w.succ = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)H * 4);
    w.vout = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)V * 4);
    w.vin = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)V * 4);
    w.vfirst = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)V * 4);
    w.bsum = reinterpret_cast<int32_t *>(p + at); at += scan_bytes(H);
    w.vsum = reinterpret_cast<u64 *>(p + at); at += scan_bytes<u64>(H);
    w.bytes = at;
    return w;
}

struct FillWs {
    int32_t *status;
    u64 *fv, *vsum, *cmax, *csum;
    size_t bytes;
};

FillWs fill_ws(void *workspace, int64_t L) {
    FillWs w;
    char *p = static_cast<char *>(workspace);
    size_t at = 0;
    w.status = reinterpret_cast<int32_t *>(p);
    at += MT_STATUS_BYTES;
    w.fv = reinterpret_cast<u64 *>(p + at); at += up256((size_t)(L + 1) * 8);
    w.vsum = reinterpret_cast<u64 *>(p + at); at += scan_bytes<u64>(L);
    w.cmax = reinterpret_cast<u64 *>(p + at); at += up256((size_t)L * 3 * 8);
    w.csum = reinterpret_cast<u64 *>(p + at); at += up256((size_t)L * 6 * 8);
    w.bytes = at;
    return w;
}

int64_t total_of(const int32_t (&h)[32], int word) { return (int64_t)(uint32_t)h[ST_TOTAL * 2 + word]; }     // word 0: low half

template <class T>
void centroid_launch(const T *verts, int V, const int32_t *off, const int32_t *lv, const FillWs &w, int L, int NNF, int NNV, T *out_verts, hipStream_t st) {
    const dim3 grid(blocks_of(NNF, MT_CHUNK)), block(MT_THREADS);
    hipLaunchKernelGGL((centroid_kernel<T, 0>), grid, block, 0, st, verts, V, off, lv, (const u64 *)w.fv, L, NNF, NNV, w.cmax, w.csum);
    hipLaunchKernelGGL((centroid_kernel<T, 1>), grid, block, 0, st, verts, V, off, lv, (const u64 *)w.fv, L, NNF, NNV, w.cmax, w.csum);
    hipLaunchKernelGGL(centroid_finish_kernel<T>, dim3(blocks_of(L, MT_THREADS)), block, 0, st, off, (const u64 *)w.fv, L, V, NNV, (const u64 *)w.cmax,
                       (const u64 *)w.csum, out_verts);
}

}  // namespace

extern "C" {

size_t vt_mesh_boundary_workspace_bytes(int64_t V, int64_t F) { return sizes_ok(V, F) ? boundary_ws(nullptr, V, F).bytes : 0; }

int vt_mesh_boundary(const int32_t *faces, int64_t F, int64_t V, int *n_boundary, void *workspace, size_t workspace_bytes, void *stream) {
    if (!sizes_ok(V, F) || !faces || !n_boundary) return vt_fail(VT_ERR_INVALID, "vt_mesh_boundary: bad argument (V >= 1, F >= 1)");
    if (!workspace || workspace_bytes < boundary_ws(nullptr, V, F).bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_boundary");
    hipStream_t st = (hipStream_t)stream;
    const BoundaryWs w = boundary_ws(workspace, V, F);
    const int64_t H = 3 * F;
    int rc = vt_fill32(w.status, 0u, MT_STATUS_BYTES, st);
    if (!rc) rc = edge_table_clear(w.t, st);
    if (rc) return rc;
    const dim3 block(MT_THREADS), fgrid(blocks_of(F, MT_THREADS));
    hipLaunchKernelGGL(edge_insert_kernel<true>, fgrid, block, 0, st, faces, (int)F, (int)V, w.t, w.status + ST_BAD);
    hipLaunchKernelGGL(edge_flag_kernel, fgrid, block, 0, st, faces, (int)F, (int)V, w.t, w.flag);
    scan_launch(FlagPred{w.flag}, H, w.bsum, w.pos, w.status + ST_NB, st);
    hipLaunchKernelGGL(compact_kernel, dim3(blocks_of(H, MT_THREADS)), block, 0, st, (const uint8_t *)w.flag, (const int32_t *)w.pos, H, w.bhe);
    rc = vt_check(hipGetLastError(), "vt_mesh_boundary");
    if (rc) return rc;
    int32_t h[32];
    rc = read_status(workspace, h, st, "vt_mesh_boundary");
    if (rc) return rc;
    if (h[ST_BAD]) return vt_fail(VT_ERR_INVALID, "vt_mesh_boundary: a face index lies outside [0, V)");
    const int NB = h[ST_NB];
    *n_boundary = NB;
    if (NB <= 0) return 0;
    rc = vt_fill32(w.vout, 0u, 2 * up256((size_t)V * 4), st);      // vout and vin lie back to back
    if (!rc) rc = vt_fill32(w.vfirst, 0x7fffffffu, up256((size_t)V * 4), st);
    if (rc) return rc;
    const dim3 bgrid(blocks_of(NB, MT_THREADS));
    hipLaunchKernelGGL(degree_kernel, bgrid, block, 0, st, faces, (const int32_t *)w.bhe, NB, w.vout, w.vin, w.vfirst);
    hipLaunchKernelGGL(succ_kernel, bgrid, block, 0, st, faces, (const int32_t *)w.bhe, NB, (const int32_t *)w.vout, (const int32_t *)w.vin,
                       (const int32_t *)w.vfirst, w.succ);
    return vt_check(hipGetLastError(), "vt_mesh_boundary");
}

int vt_mesh_boundary_loops(const int32_t *faces, int64_t F, int64_t V, int64_t NB, int32_t *loop_offsets, int32_t *loop_vertices,
                           int32_t *loop_half_edges, int *n_loops, int *n_irregular, void *workspace, size_t workspace_bytes, void *stream) {
    if (!sizes_ok(V, F) || NB < 1 || NB > 3 * F || !faces || !loop_offsets || !loop_vertices || !loop_half_edges || !n_loops || !n_irregular)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_boundary_loops: bad argument (V >= 1, F >= 1, 1 <= NB <= 3 F)");
    if (!workspace || workspace_bytes < boundary_ws(nullptr, V, F).bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_boundary_loops");
    hipStream_t st = (hipStream_t)stream;
    const BoundaryWs w = boundary_ws(workspace, V, F);
    const int n = (int)NB;
    int R = 0;
    while (((int64_t)1 << R) < NB) ++R;                           // 2^R >= NB
    const dim3 block(MT_THREADS), grid(blocks_of(NB, MT_THREADS));
    // the smallest element of every cycle: A -> B -> A ..., the result in `mins`; the buffer it did not end in and C then rank the lists
    int2 *cur = w.bufA, *other = w.bufB;
    hipLaunchKernelGGL(min_init_kernel, grid, block, 0, st, (const int32_t *)w.succ, n, cur);
    for (int r = 0; r < R; ++r) {
        hipLaunchKernelGGL(jump_kernel<MinOp>, grid, block, 0, st, (const int2 *)cur, n, other);
        int2 *t = cur; cur = other; other = t;
    }
    const int2 *mins = cur;
    cur = other; other = w.bufC;
    hipLaunchKernelGGL(rank_init_kernel, grid, block, 0, st, (const int32_t *)w.succ, mins, n, cur);
    for (int r = 0; r < R; ++r) {
        hipLaunchKernelGGL(jump_kernel<AddOp>, grid, block, 0, st, (const int2 *)cur, n, other);
        int2 *t = cur; cur = other; other = t;
    }
    const int2 *ranks = cur;
    u64 *scan = reinterpret_cast<u64 *>(other);
    scan_launch(HeadFn{mins, ranks}, NB, w.vsum, scan, w.total, st);
    hipLaunchKernelGGL(loops_write_kernel, grid, block, 0, st, faces, (const int32_t *)w.bhe, mins, ranks, (const u64 *)scan, (const u64 *)w.total, n,
                       loop_offsets, loop_vertices, loop_half_edges);
    int rc = vt_check(hipGetLastError(), "vt_mesh_boundary_loops");
    if (rc) return rc;
    int32_t h[32];
    rc = read_status(workspace, h, st, "vt_mesh_boundary_loops");
    if (rc) return rc;
    const int64_t L = total_of(h, 1), in_loops = total_of(h, 0);
    if (L > NB || in_loops > NB) return vt_fail(VT_ERR_INVALID, "vt_mesh_boundary_loops: the workspace is not vt_mesh_boundary's of these faces");
    *n_loops = (int)L;
    *n_irregular = (int)(NB - in_loops);
    return 0;
}

size_t vt_mesh_fill_workspace_bytes(int64_t L) { return L >= 1 && L <= MT_MAX_F ? fill_ws(nullptr, L).bytes : 0; }

int vt_mesh_fill_count(const int32_t *loop_offsets, int64_t L, int method, int64_t max_edges, int *n_filled, int *n_new_faces, int *n_new_verts,
                       void *workspace, size_t workspace_bytes, void *stream) {
    if (L < 1 || L > MT_MAX_F || !loop_offsets || (method != 0 && method != 1) || max_edges < 0 || !n_filled || !n_new_faces || !n_new_verts)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_fill_count: bad argument (L >= 1, method 0 or 1, max_edges >= 0)");
    if (!workspace || workspace_bytes < fill_ws(nullptr, L).bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_fill_count");
    hipStream_t st = (hipStream_t)stream;
    const FillWs w = fill_ws(workspace, L);
    int rc = vt_fill32(w.status, 0u, MT_STATUS_BYTES, st);
    if (rc) return rc;
    const FillFn fn{loop_offsets, method, max_edges};
    scan_launch(fn, L, w.vsum, w.fv, w.fv + L, st);
    hipLaunchKernelGGL(filled_count_kernel, dim3(blocks_of(L, MT_THREADS)), dim3(MT_THREADS), 0, st, fn, (int)L, w.status);
    rc = vt_check(hipGetLastError(), "vt_mesh_fill_count");
    if (rc) return rc;
    u64 total = 0;
    int32_t h[32];
    hipError_t e = hipMemcpyAsync(&total, w.fv + L, sizeof total, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return vt_check(e, "vt_mesh_fill_count");
    rc = read_status(workspace, h, st, "vt_mesh_fill_count");     // (one wait for the two copies)
    if (rc) return rc;
    if ((total & 0xffffffffull) > 0x7fffff00ull) return vt_fail(VT_ERR_INVALID, "vt_mesh_fill_count: more than 2^31 new faces");
    *n_filled = h[ST_NFILLED];
    *n_new_faces = (int)(total & 0xffffffffull);
    *n_new_verts = (int)(total >> 32);
    return 0;
}

int vt_mesh_fill_emit(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, const int32_t *loop_offsets,
                      const int32_t *loop_vertices, int64_t L, int method, int64_t n_new_faces, int64_t n_new_verts, void *out_verts,
                      int32_t *out_faces, void *workspace, size_t workspace_bytes, void *stream) {
    if (V < 1 || V > MT_MAX_V || F < 0 || F > MT_MAX_F || L < 1 || L > MT_MAX_F || (method != 0 && method != 1) || n_new_faces < 0 ||
        F + n_new_faces > MT_MAX_F || n_new_verts < 0 || n_new_verts > L || V + n_new_verts > MT_MAX_V || !verts || (F && !faces) || !loop_offsets ||
        !loop_vertices || !out_verts || !out_faces)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_fill_emit: bad argument (V >= 1, F >= 0, L >= 1, the counts vt_mesh_fill_count returned)");
    if (!workspace || workspace_bytes < fill_ws(nullptr, L).bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_fill_emit");
    hipStream_t st = (hipStream_t)stream;
    const FillWs w = fill_ws(workspace, L);
    copy_words(verts, (size_t)V * 3 * (verts_f64 ? 8 : 4), out_verts, st);
    copy_words(faces, (size_t)F * 12, out_faces, st);
    if (n_new_faces)
        hipLaunchKernelGGL(emit_face_kernel, dim3(blocks_of(n_new_faces, MT_THREADS)), dim3(MT_THREADS), 0, st, loop_offsets, loop_vertices,
                           (const u64 *)w.fv, (int)L, (int)V, F, (int)n_new_faces, out_faces);
    if (n_new_verts) {
        int rc = vt_fill32(w.cmax, 0u, up256((size_t)L * 3 * 8) + up256((size_t)L * 6 * 8), st);      // cmax and csum lie back to back
        if (rc) return rc;
        if (verts_f64)
            centroid_launch(static_cast<const double *>(verts), (int)V, loop_offsets, loop_vertices, w, (int)L, (int)n_new_faces, (int)n_new_verts,
                            static_cast<double *>(out_verts), st);
        else
            centroid_launch(static_cast<const float *>(verts), (int)V, loop_offsets, loop_vertices, w, (int)L, (int)n_new_faces, (int)n_new_verts,
                            static_cast<float *>(out_verts), st);
    }
    return vt_check(hipGetLastError(), "vt_mesh_fill_emit");
}

}  // extern "C"
