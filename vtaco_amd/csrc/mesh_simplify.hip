// Mesh simplification by vertex clustering with quadric-error placement (Lindstrom 2000) and vertex welding, on the device (DESIGN.md,
// section "mesh_simplify.hip"; tests/mesh_simplify_ref.py is the definition, restated in numpy, and these kernels equal it bit for bit).
// faces [F,3] i32 and vertices [V,3] f32 or f64; coordinates are widened exactly and every coordinate operation is float64, unfused
// (-ffp-contract=off), in the order the restatement writes.  Every rule that picks among equals picks the lowest index.
//   state         32 int32 words the caller owns and every call of one simplification shares: words 0..11 the bounding box of the referenced
//                 vertices as six order-preserving u64 keys (min x y z, max x y z), word 16 the status bits, 17 K, 18 the face count, 19 the
//                 placement's fallbacks.  The box never leaves the device: every kernel derives lo, L = max(hi - lo), h = L / R from the keys.
//   clusters      referenced[v] by plain stores; an open-addressing table of vertex INDICES, 2 V slots rounded up to a power of two, claimed
//                 by atomicCAS: a slot's occupant stands for its key (the cell triple; for welding the coordinates' bits or rint(x / tol)),
//                 a vertex with the occupant's key lowers the occupant with an integer atomicMin, any other moves on.  The occupants of a
//                 slot all share one key, so the table ends with every key's lowest vertex index whatever the order of arrival.  A lookup
//                 pass gives every vertex its representative, an exclusive scan ranks the representatives: clusters in ascending order
//                 of representative with no sort.
//   faces         corners to cluster ids; a face with two equal ids is dropped; the sorted triple is a 63-bit key (K < 2^21) in a table
//                 of 2 F slots claimed by atomicCAS whose value takes the lowest face index by atomicMin; a face is kept when that is
//                 its own; a scan compacts the kept faces in their order.  The count-only form stops after the scan's totals.
//   quadrics      per (face, distinct cluster among its corners) the upper triangle of [n,d][n,d]^T, per vertex its centre-relative
//                 coordinates: a first pass takes each cluster's largest |term| (atomicMax on the bit pattern), a second adds every term as
//                 two int64 limbs against that exponent (mesh_common.h): exact sums, equal bits from run to run, no float atomic.
//   placement     one thread per cluster: the mean x0, a cyclic 3x3 Jacobi of A in registers (MS_SWEEPS sweeps), eigenvalues at most
//                 MS_EIG_REL of the largest dropped, x = x0 + V pinv(L) V^T (-b - A x0); outside the cell (cell_bound) falls back to x0.
// A face with an index outside [0, V) is never dereferenced; it takes no part and sets bit 0 of the status word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_common.h"
#include "mesh_quadric.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

enum { SS_BOX = 0, SS_BAD = 16, SS_K = 17, SS_NF = 18, SS_FALLBACK = 19, SS_WORDS = 32 };
enum { BAD_INDEX = 1, BAD_NONFINITE = 2, BAD_K = 4, BAD_KEY = 8, BAD_MAP = 16 };
enum { KEY_CELL = 0, KEY_EXACT = 1, KEY_TOL = 2 };
enum { PLACE_QUADRIC = 0, PLACE_MEAN = 1, PLACE_COPY = 2 };

constexpr int MS_MAX_R = 1 << 20;
constexpr int MS_MAX_K = 1 << 21;                // three cluster ids fill 63 bits of a face key
constexpr double MS_SOLVE_SLACK = 0x1p-52 / MS_EIG_REL;
constexpr double MS_BOX_SLACK = 0x1p-51;
constexpr int MS_SUMS = 27;                      // per cluster: 10 quadric values and 3 coordinates as (hi, lo) limbs, the vertex count
constexpr u64 FACE_EMPTY = ~0ull;

#define MS_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

bool ms_sizes_ok(int64_t V, int64_t F) { return V >= 1 && F >= 1 && V <= MT_MAX_V / 2 && F <= MT_MAX_F; }

int64_t pow2_slots(int64_t n) {
    int64_t cap = 1024;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}
int shift_of(int64_t slots) {
    int shift = 64;
    for (int64_t s = slots; s > 1; s >>= 1) --shift;              // slots = 2^(64 - shift)
    return shift;
}

// ---- the grid ---------------------------------------------------------------------------------------------------------------------------
struct Grid {
    double lo[3], L, h;
    int R;
};

__device__ inline Grid grid_of(const int32_t *state, int R) {
    const u64 *box = reinterpret_cast<const u64 *>(state + SS_BOX);
    Grid g;
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.lo[k] = value_of(box[k]);
        d[k] = value_of(box[3 + k]) - g.lo[k];
    }
    g.L = fmax(fmax(d[0], d[1]), d[2]);
    g.h = g.L / (double)R;
    g.R = R;
    return g;
}

// min(R - 1, floor((x - lo) / h)); 0 where the box has no extent (a NaN quotient compares false twice: 0 as well)
__device__ inline int cell_of(double x, double lo, double h, int R) {
    if (h == 0.0) return 0;
    const double t = floor((x - lo) / h);
    return t >= (double)(R - 1) ? R - 1 : (t > 0.0 ? (int)t : 0);
}
__device__ inline double centre_of(int cell, double lo, double h) { return lo + ((double)cell + 0.5) * h; }

// ---- vertex keys ------------------------------------------------------------------------------------------------------------------------
struct Key3 {
    long long k[3];
    bool solo, bad;                               // solo: merges with nothing (a NaN coordinate of a weld); bad: beyond the int64 range
};

template <class T, int MODE>
__device__ inline Key3 vertex_key(const T *verts, int v, const Grid &g, double tol) {
    double p[3];
    load_vertex(verts, v, p[0], p[1], p[2]);
    Key3 key;
    key.solo = key.bad = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (MODE == KEY_CELL) {
            key.k[k] = cell_of(p[k], g.lo[k], g.h, g.R);
        } else if (p[k] != p[k]) {
            key.solo = true;
            key.k[k] = 0;
        } else if (MODE == KEY_EXACT) {
            key.k[k] = p[k] == 0.0 ? 0ll : __double_as_longlong(p[k]);              // -0.0 equals +0.0
        } else {
            const double r = rint(p[k] / tol);
            if (fabs(r) < 0x1p63) key.k[k] = (long long)r;
            else { key.bad = true; key.k[k] = 0; }
        }
    }
    return key;
}

__device__ inline bool same_key(const Key3 &a, const Key3 &b) { return a.k[0] == b.k[0] && a.k[1] == b.k[1] && a.k[2] == b.k[2]; }

__device__ inline u64 slot_of(const Key3 &key, int shift) {
    u64 x = (u64)key.k[0] * 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 29)) + (u64)key.k[1] * 0xC2B2AE3D27D4EB4Full;
    x = (x ^ (x >> 31)) + (u64)key.k[2] * 0x165667B19E3779F9ull;
    x = (x ^ (x >> 30)) * 0x9E3779B97F4A7C15ull;
    return x >> shift;
}

__global__ void __launch_bounds__(MT_THREADS) ms_mark_kernel(const int32_t *faces, int F, int V, int32_t *ref, int32_t *state) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    if (!ok) { atomicOr(state + SS_BAD, BAD_INDEX); return; }
    ref[a] = 1; ref[b] = 1; ref[c] = 1;
}

struct BoxOp {                                   // min keys x y z, max keys x y z
    __device__ static u64 identity(int k) { return k < 3 ? ~0ull : 0ull; }
    __device__ static u64 combine(int k, u64 a, u64 b) { return k < 3 ? (a < b ? a : b) : (a > b ? a : b); }
    __device__ static void atomic(int k, u64 *p, u64 v) {
        if (k < 3) atomicMin(p, v);
        else atomicMax(p, v);
    }
};

// the box of the referenced vertices: one "component" (0), combined per thread and per wave before the six atomics
template <class T>
__global__ void __launch_bounds__(MT_THREADS) box_kernel(const T *verts, int V, const int32_t *ref, int32_t *state) {
    u64 *box = reinterpret_cast<u64 *>(state + SS_BOX);
    int cur = -1;
    u64 acc[6] = {0, 0, 0, 0, 0, 0};
    bool nonfinite = false;
    const int64_t base = (int64_t)blockIdx.x * MT_CHUNK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        const int64_t v = base + (int64_t)k * MT_THREADS;
        int c = -1;
        u64 x[6] = {0, 0, 0, 0, 0, 0};
        if (v < V && ref[v] != 0) {
            double px, py, pz;
            load_vertex(verts, (int)v, px, py, pz);
            if (isfinite(px) && isfinite(py) && isfinite(pz)) {
                c = 0;
                x[0] = x[3] = key_of(px); x[1] = x[4] = key_of(py); x[2] = x[5] = key_of(pz);
            } else {
                nonfinite = true;
            }
        }
        accumulate<6, BoxOp>(cur, acc, c, x, box);
    }
    wave_flush<6, BoxOp>(cur, acc, box);
    if (nonfinite) atomicOr(state + SS_BAD, BAD_NONFINITE);
}

template <class T, int MODE>
__global__ void __launch_bounds__(MT_THREADS)
vinsert_kernel(const T *verts, int V, const int32_t *ref, const int32_t *state, int R, double tol, int32_t *slots, u64 mask, int shift, int32_t *status) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v >= V || ref[v] == 0) return;
    const Grid g = grid_of(state, R);
    const Key3 key = vertex_key<T, MODE>(verts, (int)v, g, tol);
    if (key.solo) return;
    if (key.bad) { atomicOr(status + SS_BAD, BAD_KEY); return; }
    u64 slot = slot_of(key, shift);
    for (u64 probes = 0; probes <= mask; ++probes) {              // (at most V of the >= 2 V slots are ever claimed: a free one is met)
        int cur = __hip_atomic_load(slots + slot, MS_RLX_AGENT);
        if (cur < 0) {
            cur = atomicCAS(slots + slot, -1, (int)v);
            if (cur < 0) return;
        }
        // cur < V: only vertex indices are ever stored; the occupant may fall meanwhile, its key stays
        if (same_key(key, vertex_key<T, MODE>(verts, cur, g, tol))) { atomicMin(slots + slot, (int)v); return; }
        slot = (slot + 1) & mask;
    }
}

template <class T, int MODE>
__global__ void __launch_bounds__(MT_THREADS)
vlookup_kernel(const T *verts, int V, const int32_t *ref, const int32_t *state, int R, double tol, const int32_t *slots, u64 mask, int shift, int32_t *repv) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v >= V) return;
    int rep = -1;
    if (ref[v] != 0) {
        const Grid g = grid_of(state, R);
        const Key3 key = vertex_key<T, MODE>(verts, (int)v, g, tol);
        rep = (int)v;                                            // solo, bad: a cluster of its own
        if (!key.solo && !key.bad) {
            u64 slot = slot_of(key, shift);
            for (u64 probes = 0; probes <= mask; ++probes) {
                const int cur = slots[slot];
                if (cur < 0) break;                              // (not met: the vertex was inserted)
                if (same_key(key, vertex_key<T, MODE>(verts, cur, g, tol))) { rep = cur; break; }
                slot = (slot + 1) & mask;
            }
        }
    }
    repv[v] = rep;
}

struct RepPred {
    const int32_t *repv;
    __device__ bool operator()(int64_t v) const { return repv[v] == (int)v; }
};

__global__ void __launch_bounds__(MT_THREADS)
vfinal_kernel(const int32_t *repv, const int32_t *rank, int V, int32_t *cluster_of_vertex, int32_t *cluster_rep) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v >= V) return;
    const int r = repv[v];                                       // -1, or a vertex index <= v that is its own representative
    int c = -1;
    if ((unsigned)r < (unsigned)V) {
        c = rank[r];                                             // c <= r < V: inside the capacity-V cluster_rep
        if (r == (int)v) cluster_rep[c] = (int)v;
    }
    cluster_of_vertex[v] = c;
}

template <class T, int MODE>
void cluster_launch(const T *verts, int V, const int32_t *faces, int F, int R, double tol, int32_t *cov, int32_t *rep, int32_t *state, char *ws,
                    hipStream_t st) {
    const int64_t slots_n = pow2_slots(V);
    int32_t *ref = reinterpret_cast<int32_t *>(ws);
    int32_t *slots = reinterpret_cast<int32_t *>(ws + up256((size_t)V * 4));
    int32_t *repv = reinterpret_cast<int32_t *>(ws + up256((size_t)V * 4) + (size_t)slots_n * 4);
    int32_t *rank = reinterpret_cast<int32_t *>(ws + 2 * up256((size_t)V * 4) + (size_t)slots_n * 4);
    int32_t *bsum = reinterpret_cast<int32_t *>(ws + 3 * up256((size_t)V * 4) + (size_t)slots_n * 4);
    const int shift = shift_of(slots_n);
    const u64 mask = (u64)(slots_n - 1);
    hipLaunchKernelGGL(ms_mark_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, faces, F, V, ref, state);
    if (MODE == KEY_CELL)
        hipLaunchKernelGGL(box_kernel<T>, dim3(blocks_of(V, MT_CHUNK)), dim3(MT_THREADS), 0, st, verts, V, (const int32_t *)ref, state);
    hipLaunchKernelGGL((vinsert_kernel<T, MODE>), dim3(blocks_of(V, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, V, (const int32_t *)ref,
                       (const int32_t *)state, R, tol, slots, mask, shift, state);
    hipLaunchKernelGGL((vlookup_kernel<T, MODE>), dim3(blocks_of(V, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, V, (const int32_t *)ref,
                       (const int32_t *)state, R, tol, (const int32_t *)slots, mask, shift, repv);
    scan_launch(RepPred{repv}, V, bsum, rank, state + SS_K, st);
    hipLaunchKernelGGL(vfinal_kernel, dim3(blocks_of(V, MT_THREADS)), dim3(MT_THREADS), 0, st, (const int32_t *)repv, (const int32_t *)rank, V, cov, rep);
}

size_t cluster_bytes(int64_t V) { return 3 * up256((size_t)V * 4) + (size_t)pow2_slots(V) * 4 + scan_bytes(V); }

// state: zeros, the box's min keys all ones; ref: zeros; slots: -1
int cluster_prepare(int64_t V, int32_t *state, char *ws, hipStream_t st) {
    int rc = vt_fill32(state, 0u, SS_WORDS * 4, st);
    if (!rc) rc = vt_fill32(state + SS_BOX, 0xffffffffu, 3 * 8, st);
    if (!rc) rc = vt_fill32(ws, 0u, up256((size_t)V * 4), st);
    if (!rc) rc = vt_fill32(ws + up256((size_t)V * 4), 0xffffffffu, (size_t)pow2_slots(V) * 4, st);
    return rc;
}

// ---- faces ------------------------------------------------------------------------------------------------------------------------------
// fslot[f]: -1 dropped; unique: the face's slot of the key table, else 0
__global__ void __launch_bounds__(MT_THREADS)
finsert_kernel(const int32_t *faces, int F, int V, const int32_t *cov, int unique, u64 *keys, int32_t *vals, u64 mask, int shift, int32_t *fslot,
               int32_t *state) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    fslot[f] = -1;
    if (!ok) { atomicOr(state + SS_BAD, BAD_INDEX); return; }
    const int K = state[SS_K];
    if (unique && K >= MS_MAX_K) { atomicOr(state + SS_BAD, BAD_K); return; }
    const int i = cov[a], j = cov[b], k = cov[c];
    if ((unsigned)i >= (unsigned)K || (unsigned)j >= (unsigned)K || (unsigned)k >= (unsigned)K) { atomicOr(state + SS_BAD, BAD_MAP); return; }
    if (i == j || j == k || i == k) return;
    if (!unique) { fslot[f] = 0; return; }
    const int lo = min(i, min(j, k)), hi = max(i, max(j, k)), mid = i + j + k - lo - hi;
    const u64 key = (u64)lo << 42 | (u64)mid << 21 | (u64)hi;
    u64 slot = (key * 0x9E3779B97F4A7C15ull) >> shift;
    for (u64 probes = 0; probes <= mask; ++probes) {             // (at most F of the >= 2 F slots are ever claimed: a free one is met)
        const u64 old = atomicCAS(keys + slot, FACE_EMPTY, key);
        if (old == FACE_EMPTY || old == key) { atomicMin(vals + slot, f); fslot[f] = (int)slot; return; }
        slot = (slot + 1) & mask;
    }
}

struct FaceKeptPred {
    const int32_t *fslot, *vals;
    int unique;
    __device__ bool operator()(int64_t f) const {
        const int s = fslot[f];
        return s >= 0 && (!unique || vals[s] == (int)f);
    }
};

__global__ void __launch_bounds__(MT_THREADS)
fcompact_kernel(const int32_t *faces, int F, int V, const int32_t *cov, FaceKeptPred kept, const int32_t *fpos, int32_t *out_faces) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok) || !ok || !kept(f)) return;
    const int at = fpos[f];                       // at <= f < F
    out_faces[(size_t)at * 3] = cov[a]; out_faces[(size_t)at * 3 + 1] = cov[b]; out_faces[(size_t)at * 3 + 2] = cov[c];
}

size_t faces_bytes(int64_t F) { return (size_t)pow2_slots(F) * 12 + 2 * up256((size_t)F * 4) + scan_bytes(F); }

// ---- quadrics ---------------------------------------------------------------------------------------------------------------------------
struct QuadWs { u64 *big, *sums; };               // [K][2] the largest |quadric term|, |coordinate|; [K][MS_SUMS]

template <class T, int PASS>
__global__ void __launch_bounds__(MT_THREADS) qvertex_kernel(const T *verts, int V, const int32_t *cov, int K, const int32_t *state, int R, QuadWs ws) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v >= V) return;
    const int c = cov[v];
    if ((unsigned)c >= (unsigned)K) return;
    const Grid g = grid_of(state, R);
    double p[3], rel[3];
    load_vertex(verts, (int)v, p[0], p[1], p[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) rel[k] = p[k] - centre_of(cell_of(p[k], g.lo[k], g.h, R), g.lo[k], g.h);
    if (PASS == 0) {
        const double big = fmax(fmax(fabs(rel[0]), fabs(rel[1])), fabs(rel[2]));
        atomicMax(ws.big + (size_t)c * 2 + 1, (u64)__double_as_longlong(big));
    } else {
        const int e = exponent_of(ws.big[(size_t)c * 2 + 1]);
        u64 *sums = ws.sums + (size_t)c * MS_SUMS;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u64 hi, lo;
            limbs_of(rel[k], e, hi, lo);
            atomicAdd(sums + 20 + 2 * k, hi);
            atomicAdd(sums + 21 + 2 * k, lo);
        }
        atomicAdd(sums + 26, 1ull);
    }
}

template <class T, int PASS>
__global__ void __launch_bounds__(MT_THREADS)
qface_kernel(const T *verts, int V, const int32_t *faces, int F, const int32_t *cov, int K, const int32_t *state, int R, QuadWs ws) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, idx[3];
    bool ok;
    if (!load_face(faces, F, V, lds, f, idx[0], idx[1], idx[2], ok) || !ok) return;
    const int id[3] = {cov[idx[0]], cov[idx[1]], cov[idx[2]]};
    if ((unsigned)id[0] >= (unsigned)K || (unsigned)id[1] >= (unsigned)K || (unsigned)id[2] >= (unsigned)K) return;
    const Grid g = grid_of(state, R);
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) load_vertex(verts, idx[k], p[k][0], p[k][1], p[k][2]);
    const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const double wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if ((k >= 1 && id[k] == id[0]) || (k == 2 && id[k] == id[1])) continue;          // once per distinct cluster: its first corner
        double q[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = p[k][a] - centre_of(cell_of(p[k][a], g.lo[a], g.h, R), g.lo[a], g.h);
        const double d = -((nx * q[0] + ny * q[1]) + nz * q[2]);
        const double t[10] = {nx * nx, nx * ny, nx * nz, nx * d, ny * ny, ny * nz, ny * d, nz * nz, nz * d, d * d};
        if (PASS == 0) {
            double big = 0.0;
#pragma unroll
            for (int j = 0; j < 10; ++j) big = fmax(big, fabs(t[j]));
            atomicMax(ws.big + (size_t)id[k] * 2, (u64)__double_as_longlong(big));
        } else {
            const int e = exponent_of(ws.big[(size_t)id[k] * 2]);
            u64 *sums = ws.sums + (size_t)id[k] * MS_SUMS;
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                u64 hi, lo;
                limbs_of(t[j], e, hi, lo);
                atomicAdd(sums + 2 * j, hi);
                atomicAdd(sums + 2 * j + 1, lo);
            }
        }
    }
}

template <class T>
__global__ void __launch_bounds__(MT_THREADS)
place_kernel(const T *verts, int V, const int32_t *rep, int K, int32_t *state, int R, int placement, QuadWs ws, T *out_verts) {
    const int64_t c = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    bool fell = false;
    if (c < K) {
        const int r = rep[c];
        if ((unsigned)r < (unsigned)V) {
            if (placement == PLACE_COPY) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out_verts[c * 3 + k] = verts[(size_t)r * 3 + k];
            } else {
                const Grid g = grid_of(state, R);
                double p[3], centre[3], x0[3], x[3];
                load_vertex(verts, r, p[0], p[1], p[2]);
                const u64 *sums = ws.sums + (size_t)c * MS_SUMS;
                const int ev = exponent_of(ws.big[(size_t)c * 2 + 1]);
                const double n = (double)(long long)sums[26];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    centre[k] = centre_of(cell_of(p[k], g.lo[k], g.h, R), g.lo[k], g.h);
                    x0[k] = sum_of(sums[20 + 2 * k], sums[21 + 2 * k], ev) / n;
                    x[k] = x0[k];
                }
                if (placement == PLACE_QUADRIC) {
                    const int eq = exponent_of(ws.big[(size_t)c * 2]);
                    double q[10], xs[3];
#pragma unroll
                    for (int j = 0; j < 10; ++j) q[j] = sum_of(sums[2 * j], sums[2 * j + 1], eq);
                    quadric_solve(q, x0, xs);
                    const double half = g.h / 2.0;
                    bool inside = true;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {                 // (tests/mesh_simplify_ref.py: cell_bound; a NaN is outside)
                        const double bound = half + (half * MS_SOLVE_SLACK + (fabs(g.lo[k]) + g.L) * MS_BOX_SLACK);
                        inside = inside && fabs(xs[k]) <= bound;
                    }
                    if (inside) { x[0] = xs[0]; x[1] = xs[1]; x[2] = xs[2]; }
                    else fell = true;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) out_verts[c * 3 + k] = (T)(centre[k] + x[k]);
            }
        }
    }
    const u64 fallen = __ballot(fell);
    if (fallen != 0 && (int)(threadIdx.x & 63) == __ffsll((long long)fallen) - 1) atomicAdd(state + SS_FALLBACK, __popcll(fallen));
}

size_t place_bytes(int64_t K) { return up256((size_t)K * 2 * 8) + up256((size_t)K * MS_SUMS * 8); }

template <class T>
void place_launch(const T *verts, int V, const int32_t *faces, int F, int R, const int32_t *cov, const int32_t *rep, int K, int placement, T *out_verts,
                  int32_t *state, char *wsp, hipStream_t st) {
    QuadWs ws;
    ws.big = reinterpret_cast<u64 *>(wsp);
    ws.sums = reinterpret_cast<u64 *>(wsp + up256((size_t)K * 2 * 8));
    if (placement != PLACE_COPY) {
        hipLaunchKernelGGL((qvertex_kernel<T, 0>), dim3(blocks_of(V, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, V, cov, K, (const int32_t *)state, R, ws);
        hipLaunchKernelGGL((qvertex_kernel<T, 1>), dim3(blocks_of(V, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, V, cov, K, (const int32_t *)state, R, ws);
    }
    if (placement == PLACE_QUADRIC) {
        hipLaunchKernelGGL((qface_kernel<T, 0>), dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, V, faces, F, cov, K, (const int32_t *)state, R, ws);
        hipLaunchKernelGGL((qface_kernel<T, 1>), dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, V, faces, F, cov, K, (const int32_t *)state, R, ws);
    }
    hipLaunchKernelGGL(place_kernel<T>, dim3(blocks_of(K, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, V, rep, K, state, R, placement, ws, out_verts);
}

bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" {

size_t vt_mesh_cluster_workspace_bytes(int64_t V, int64_t F) { return ms_sizes_ok(V, F) ? cluster_bytes(V) : 0; }

int vt_mesh_cluster(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int resolution, int32_t *cluster_of_vertex,
                    int32_t *cluster_rep, int32_t *state, void *workspace, size_t workspace_bytes, void *stream) {
    if (!ms_sizes_ok(V, F) || !verts || !faces || !cluster_of_vertex || !cluster_rep || !state || !aligned8(state))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster: bad argument (V >= 1, F >= 1, state 8-byte aligned)");
    if (resolution < 1 || resolution > MS_MAX_R) return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster: resolution must lie in [1, 2^20]");
    if (!workspace || workspace_bytes < cluster_bytes(V)) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_cluster");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    int rc = cluster_prepare(V, state, ws, st);
    if (rc) return rc;
    if (verts_f64)
        cluster_launch<double, KEY_CELL>(static_cast<const double *>(verts), (int)V, faces, (int)F, resolution, 0.0, cluster_of_vertex, cluster_rep, state, ws, st);
    else
        cluster_launch<float, KEY_CELL>(static_cast<const float *>(verts), (int)V, faces, (int)F, resolution, 0.0, cluster_of_vertex, cluster_rep, state, ws, st);
    return vt_check(hipGetLastError(), "vt_mesh_cluster");
}

size_t vt_mesh_weld_workspace_bytes(int64_t V, int64_t F) { return ms_sizes_ok(V, F) ? cluster_bytes(V) : 0; }

int vt_mesh_weld(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, double tol, int32_t *cluster_of_vertex, int32_t *cluster_rep,
                 int32_t *state, void *workspace, size_t workspace_bytes, void *stream) {
    if (!ms_sizes_ok(V, F) || !verts || !faces || !cluster_of_vertex || !cluster_rep || !state || !aligned8(state))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_weld: bad argument (V >= 1, F >= 1, state 8-byte aligned)");
    if (!(tol >= 0.0) || !(tol <= 1.7976931348623157e308)) return vt_fail(VT_ERR_INVALID, "vt_mesh_weld: tol must be finite and >= 0");
    if (!workspace || workspace_bytes < cluster_bytes(V)) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_weld");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    int rc = cluster_prepare(V, state, ws, st);
    if (rc) return rc;
    const int Vi = (int)V, Fi = (int)F;
    if (verts_f64 && tol == 0.0)
        cluster_launch<double, KEY_EXACT>(static_cast<const double *>(verts), Vi, faces, Fi, 1, tol, cluster_of_vertex, cluster_rep, state, ws, st);
    else if (verts_f64)
        cluster_launch<double, KEY_TOL>(static_cast<const double *>(verts), Vi, faces, Fi, 1, tol, cluster_of_vertex, cluster_rep, state, ws, st);
    else if (tol == 0.0)
        cluster_launch<float, KEY_EXACT>(static_cast<const float *>(verts), Vi, faces, Fi, 1, tol, cluster_of_vertex, cluster_rep, state, ws, st);
    else
        cluster_launch<float, KEY_TOL>(static_cast<const float *>(verts), Vi, faces, Fi, 1, tol, cluster_of_vertex, cluster_rep, state, ws, st);
    return vt_check(hipGetLastError(), "vt_mesh_weld");
}

size_t vt_mesh_cluster_faces_workspace_bytes(int64_t F) { return F >= 1 && F <= MT_MAX_F ? faces_bytes(F) : 0; }

int vt_mesh_cluster_faces(const int32_t *faces, int64_t F, int64_t V, const int32_t *cluster_of_vertex, int unique, int32_t *out_faces, int32_t *state,
                          int *n_clusters, int *n_out_faces, void *workspace, size_t workspace_bytes, void *stream) {
    if (!ms_sizes_ok(V, F) || !faces || !cluster_of_vertex || !state || !n_clusters || !n_out_faces)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster_faces: bad argument (V >= 1, F >= 1)");
    if (!workspace || workspace_bytes < faces_bytes(F)) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_cluster_faces");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    const int64_t slots_n = pow2_slots(F);
    u64 *keys = reinterpret_cast<u64 *>(ws);
    int32_t *vals = reinterpret_cast<int32_t *>(ws + (size_t)slots_n * 8);
    int32_t *fslot = reinterpret_cast<int32_t *>(ws + (size_t)slots_n * 12);
    int32_t *fpos = reinterpret_cast<int32_t *>(ws + (size_t)slots_n * 12 + up256((size_t)F * 4));
    int32_t *bsum = reinterpret_cast<int32_t *>(ws + (size_t)slots_n * 12 + 2 * up256((size_t)F * 4));
    int rc = 0;
    if (unique) {
        rc = vt_fill32(keys, 0xffffffffu, (size_t)slots_n * 8, st);
        if (!rc) rc = vt_fill32(vals, 0x7fffffffu, (size_t)slots_n * 4, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(finsert_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, faces, (int)F, (int)V, cluster_of_vertex, unique ? 1 : 0, keys,
                       vals, (u64)(slots_n - 1), shift_of(slots_n), fslot, state);
    const FaceKeptPred kept{fslot, vals, unique ? 1 : 0};
    if (out_faces) {
        scan_launch(kept, F, bsum, fpos, state + SS_NF, st);
        hipLaunchKernelGGL(fcompact_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, faces, (int)F, (int)V, cluster_of_vertex, kept,
                           (const int32_t *)fpos, out_faces);
    } else {                                      // the count alone: the scan's first two launches
        const unsigned nb = blocks_of(F, MT_CHUNK);
        hipLaunchKernelGGL((scan_count_kernel<FaceKeptPred, int32_t>), dim3(nb), dim3(MT_THREADS), 0, st, kept, F, bsum);
        hipLaunchKernelGGL(scan_blocks_kernel<int32_t>, dim3(1), dim3(MT_THREADS), 0, st, bsum, (int)nb, state + SS_NF);
    }
    rc = vt_check(hipGetLastError(), "vt_mesh_cluster_faces");
    if (rc) return rc;
    int32_t h[SS_WORDS];
    hipError_t e = hipMemcpyAsync(h, state, sizeof h, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    rc = vt_check(e, "vt_mesh_cluster_faces");
    if (rc) return rc;
    if (h[SS_BAD] & BAD_INDEX) return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster_faces: a face index lies outside [0, V)");
    if (h[SS_BAD] & BAD_NONFINITE) return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster_faces: a referenced vertex has a non-finite coordinate");
    if (h[SS_BAD] & BAD_KEY) return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster_faces: rint(x / tol) of a referenced vertex lies beyond the int64 range");
    if (h[SS_BAD] & BAD_K) return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster_faces: 2^21 clusters or more; duplicate faces are found among fewer than 2^21 (2097152)");
    if (h[SS_BAD]) return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster_faces: cluster_of_vertex is not the map of these faces");
    *n_clusters = h[SS_K];
    *n_out_faces = h[SS_NF];
    return 0;
}

size_t vt_mesh_cluster_place_workspace_bytes(int64_t K) { return K >= 1 && K <= MT_MAX_V / 2 ? place_bytes(K) : 0; }

int vt_mesh_cluster_place(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int resolution, const int32_t *cluster_of_vertex,
                          const int32_t *cluster_rep, int64_t K, int placement, void *out_verts, int32_t *state, void *workspace, size_t workspace_bytes,
                          void *stream) {
    if (!ms_sizes_ok(V, F) || K < 1 || K > V || !verts || !faces || !cluster_of_vertex || !cluster_rep || !out_verts || !state || !aligned8(state))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster_place: bad argument (V >= 1, F >= 1, 1 <= K <= V, state 8-byte aligned)");
    if (resolution < 1 || resolution > MS_MAX_R) return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster_place: resolution must lie in [1, 2^20]");
    if (placement != PLACE_QUADRIC && placement != PLACE_MEAN && placement != PLACE_COPY)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_cluster_place: placement must be 0 (quadric), 1 (mean) or 2 (the representative's own coordinates)");
    if (!workspace || workspace_bytes < place_bytes(K)) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_cluster_place");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    int rc = placement == PLACE_COPY ? 0 : vt_fill32(ws, 0u, place_bytes(K), st);
    if (!rc) rc = vt_fill32(state + SS_FALLBACK, 0u, 4, st);
    if (rc) return rc;
    if (verts_f64)
        place_launch(static_cast<const double *>(verts), (int)V, faces, (int)F, resolution, cluster_of_vertex, cluster_rep, (int)K, placement,
                     static_cast<double *>(out_verts), state, ws, st);
    else
        place_launch(static_cast<const float *>(verts), (int)V, faces, (int)F, resolution, cluster_of_vertex, cluster_rep, (int)K, placement,
                     static_cast<float *>(out_verts), state, ws, st);
    return vt_check(hipGetLastError(), "vt_mesh_cluster_place");
}

}  // extern "C"
