// Mesh decimation by rounds of independent quadric edge collapses, on the device (DESIGN.md, section "mesh_collapse.hip";
// tests/mesh_collapse_ref.py is the definition, restated in numpy, and these kernels equal it bit for bit).  faces [F,3] i32 and vertices
// [V,3] f32 or f64; coordinates are widened exactly, positions are carried in float64 and rounded once at the end, every operation is
// float64, unfused (-ffp-contract=off), in the order the restatement writes.  Every rule that picks among equals picks the lowest index.
//   prologue      referenced[v] and the bounding box of the referenced vertices (six order-preserving u64 keys in the status block; every
//                 kernel derives the centre c = 0.5 lo + 0.5 hi from them); per vertex the ten plane terms of its faces about c, summed
//                 exactly as two int64 limbs against the exponent of the vertex's largest |term| (mesh_common.h): no float atomic.
//   a round       works on the current, compacted face list; the vertices keep their input indices throughout.
//     tables      mesh_edges.h's table over the faces with three distinct corners, with every edge's lowest half-edge 3 f + k by an
//                 integer atomicMin and every half-edge's slot; one lane per slot counts degrees and pins the ends of an edge that is not
//                 used once in each direction; one 64-bit scan (neighbour count low, face count high) gives both CSR offsets; the rows are
//                 filled through per-vertex cursors and left in the order the atomics gave: nothing below depends on the order in a row.
//     candidates  one lane per slot walks the rows in global memory: |N(u) & N(v)| = 2, not a tetrahedron, the position (mesh_quadric.h's
//                 solve about the midpoint, the midpoint where that is not finite or not better), no surviving face flips; the key
//                 (12 bits of float32(E), 20 hash bits, the lowest half-edge) goes to m1[u], m1[v] by atomicMin on u64.
//     selection   m2[w] = min of m1 over w and its row; an edge is selected when key == m2[u] == m2[v]: no two selected edges have an end
//                 in each other's closed one-ring.  A scan over the half-edges numbers the selected edges by lowest half-edge; the first
//                 ceil((F - target) / 2) are applied by the lane of that half-edge: P[u], Q[u] += Q[v], moved[v] = u.
//     faces       every corner goes through `moved`; a face that had three distinct corners and lost that is dropped; a scan compacts the
//                 rest in their order into the second buffer, which is copied back.  One thread closes the round in the status block.
//   rounds are enqueued MC_ROUND_BATCH at a time with one read of the status block per batch; grids come from the last face count read and
//   every kernel bounds itself by the count on the device; a round that finds the loop over (status word ACTIVE = 0) changes nothing.
//   epilogue      the referenced survivors ranked by a scan, vertices rounded into the input's type, faces and vertex_map on the ranks.
// A face with an index outside [0, V) is never dereferenced: the prologue finds it, the host reads the status and returns before a round.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_common.h"
#include "mesh_edges.h"
#include "mesh_quadric.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

// int32 words of the status block
enum { S_BAD = 0, S_F = 1, S_ACTIVE = 2, S_ROUNDS = 3, S_STALLED = 4, S_NCAND = 5, S_NSEL = 6, S_NKEEP = 7, S_TOTAL = 8, S_NREF = 10, S_BOX = 16 };
enum { BAD_INDEX = 1, BAD_NONFINITE = 2 };
enum { PLACE_OPTIMAL = 0, PLACE_MIDPOINT = 1 };

constexpr int MC_ROUND_BATCH = 4;                                  // rounds enqueued per read of the status block
constexpr int64_t MC_MAX_F = 0x7fffffff / 6;                       // the neighbour rows hold at most 6 F entries
constexpr u64 NO_KEY = ~0ull;
constexpr u64 ONCE_EACH_WAY = 1ull | (1ull << 32);

struct CollapseWs {
    int32_t *state, *fa, *fb, *moved, *ref0, *ref1, *rank, *pinned, *nbr, *vface, *hrank, *fpos;
    double *P, *Q;
    u64 *qbig, *qsums, *m1, *m2, *degs, *off, *cur, *ekey, *bsum, *table;
    uint32_t *hslot, *low;
    int V, target, max_rounds, placement;
    int64_t F0;
    size_t bytes;
};

CollapseWs collapse_ws(void *workspace, int64_t V, int64_t F) {
    CollapseWs w;
    char *p = static_cast<char *>(workspace);
    size_t at = 0;
    auto take = [&](size_t bytes) { char *q = p + at; at += up256(bytes); return q; };
    const int64_t slots = edge_slots(F);
    w.state = reinterpret_cast<int32_t *>(take(MT_STATUS_BYTES));
    // zeroed by one fill in the prologue: the quadric limbs and exponents, the two reference marks
    w.qbig = reinterpret_cast<u64 *>(take((size_t)V * 8));
    w.qsums = reinterpret_cast<u64 *>(take((size_t)V * 20 * 8));
    w.ref0 = reinterpret_cast<int32_t *>(take((size_t)V * 4));
    w.ref1 = reinterpret_cast<int32_t *>(take((size_t)V * 4));
    w.fa = reinterpret_cast<int32_t *>(take((size_t)F * 12));
    w.fb = reinterpret_cast<int32_t *>(take((size_t)F * 12));
    w.P = reinterpret_cast<double *>(take((size_t)V * 24));
    w.Q = reinterpret_cast<double *>(take((size_t)V * 80));
    w.moved = reinterpret_cast<int32_t *>(take((size_t)V * 4));
    w.rank = reinterpret_cast<int32_t *>(take((size_t)V * 4));
    w.pinned = reinterpret_cast<int32_t *>(take((size_t)V * 4));
    w.m1 = reinterpret_cast<u64 *>(take((size_t)V * 8));
    w.m2 = reinterpret_cast<u64 *>(take((size_t)V * 8));
    w.degs = reinterpret_cast<u64 *>(take((size_t)(V + 1) * 8));
    w.off = reinterpret_cast<u64 *>(take((size_t)(V + 1) * 8));
    w.cur = reinterpret_cast<u64 *>(take((size_t)(V + 1) * 8));
    w.nbr = reinterpret_cast<int32_t *>(take((size_t)F * 6 * 4));
    w.vface = reinterpret_cast<int32_t *>(take((size_t)F * 3 * 4));
    w.hslot = reinterpret_cast<uint32_t *>(take((size_t)F * 3 * 4));
    w.hrank = reinterpret_cast<int32_t *>(take((size_t)F * 3 * 4));
    w.fpos = reinterpret_cast<int32_t *>(take((size_t)F * 4));
    w.table = reinterpret_cast<u64 *>(take((size_t)slots * 16));
    w.low = reinterpret_cast<uint32_t *>(take((size_t)slots * 4));
    w.ekey = reinterpret_cast<u64 *>(take((size_t)slots * 8));
    w.bsum = reinterpret_cast<u64 *>(take((size_t)blocks_of(3 * F > V + 1 ? 3 * F : V + 1, MT_CHUNK) * 8));
    w.V = (int)V;
    w.F0 = F;
    w.bytes = at;
    return w;
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && F >= 1 && V <= MT_MAX_V && F <= MC_MAX_F; }

__device__ inline void centre_of_box(const int32_t *state, double (&c)[3]) {
    const u64 *box = reinterpret_cast<const u64 *>(state + S_BOX);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = 0.5 * value_of(box[k]) + 0.5 * value_of(box[3 + k]);
}

__device__ inline bool distinct(int a, int b, int c) { return a != b && b != c && a != c; }

// ---- prologue ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT_THREADS) mark_kernel(const int32_t *faces, const int32_t *count, int F, int V, int32_t *ref, int32_t *state) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, count ? min(*count, F) : F, V, lds, f, a, b, c, ok)) return;
    if (!ok) { atomicOr(state + S_BAD, BAD_INDEX); return; }
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

// P = the vertices widened, moved = the identity, and the box of the referenced vertices
template <class T>
__global__ void __launch_bounds__(MT_THREADS) widen_kernel(const T *verts, int V, const int32_t *ref, double *P, int32_t *moved, int32_t *state) {
    u64 *box = reinterpret_cast<u64 *>(state + S_BOX);
    int cur = -1;
    u64 acc[6] = {0, 0, 0, 0, 0, 0};
    bool nonfinite = false;
    const int64_t base = (int64_t)blockIdx.x * MT_CHUNK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        const int64_t v = base + (int64_t)k * MT_THREADS;
        int c = -1;
        u64 x[6] = {0, 0, 0, 0, 0, 0};
        if (v < V) {
            double px, py, pz;
            load_vertex(verts, (int)v, px, py, pz);
            P[v * 3] = px; P[v * 3 + 1] = py; P[v * 3 + 2] = pz;
            moved[v] = (int)v;
            if (ref[v] != 0) {
                if (isfinite(px) && isfinite(py) && isfinite(pz)) {
                    c = 0;
                    x[0] = x[3] = key_of(px); x[1] = x[4] = key_of(py); x[2] = x[5] = key_of(pz);
                } else {
                    nonfinite = true;
                }
            }
        }
        accumulate<6, BoxOp>(cur, acc, c, x, box);
    }
    wave_flush<6, BoxOp>(cur, acc, box);
    if (nonfinite) atomicOr(state + S_BAD, BAD_NONFINITE);
}

// the ten plane terms of every face, once per corner: PASS 0 the largest |term| per vertex, PASS 1 the limbs against its exponent
template <int PASS>
__global__ void __launch_bounds__(MT_THREADS) qface_kernel(CollapseWs w, int F) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, idx[3];
    bool ok;
    if (!load_face(w.fa, F, w.V, lds, f, idx[0], idx[1], idx[2], ok) || !ok) return;
    double c[3], p[3][3];
    centre_of_box(w.state, c);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) p[k][a] = w.P[(size_t)idx[k] * 3 + a];
    const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const double wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double q0 = p[0][0] - c[0], q1 = p[0][1] - c[1], q2 = p[0][2] - c[2];
    const double d = -((nx * q0 + ny * q1) + nz * q2);
    const double t[10] = {nx * nx, nx * ny, nx * nz, nx * d, ny * ny, ny * nz, ny * d, nz * nz, nz * d, d * d};
    if (PASS == 0) {
        double big = 0.0;
#pragma unroll
        for (int j = 0; j < 10; ++j) big = fmax(big, fabs(t[j]));
        const u64 bits = (u64)__double_as_longlong(big);
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicMax(w.qbig + idx[k], bits);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = exponent_of(w.qbig[idx[k]]);
            u64 *sums = w.qsums + (size_t)idx[k] * 20;
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

__global__ void __launch_bounds__(MT_THREADS) qfinish_kernel(CollapseWs w, int F) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v == 0) {
        w.state[S_F] = F;
        w.state[S_ACTIVE] = F > w.target ? 1 : 0;
    }
    if (v >= w.V) return;
    const int e = exponent_of(w.qbig[v]);
    const u64 *sums = w.qsums + (size_t)v * 20;
#pragma unroll
    for (int j = 0; j < 10; ++j) w.Q[(size_t)v * 10 + j] = sum_of(sums[2 * j], sums[2 * j + 1], e);
}

// ---- a round: tables --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT_THREADS) clear_kernel(CollapseWs w, EdgeTable t) {
    if (!w.state[S_ACTIVE]) return;
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < t.slots) { t.keys[i] = EDGE_EMPTY; t.vals[i] = 0; w.low[i] = NO_SLOT; }
    if (i <= w.V) w.degs[i] = 0;
    if (i < w.V) { w.m1[i] = NO_KEY; w.pinned[i] = 0; }
    if (i == 0) w.state[S_NCAND] = 0;
}

__global__ void __launch_bounds__(MT_THREADS) insert_kernel(CollapseWs w, EdgeTable t) {
    __shared__ int32_t lds[MT_THREADS * 3];
    if (!w.state[S_ACTIVE]) return;
    int f, idx[3];
    bool ok;
    if (!load_face(w.fa, w.state[S_F], w.V, lds, f, idx[0], idx[1], idx[2], ok)) return;
    const bool proper = ok && distinct(idx[0], idx[1], idx[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t s = NO_SLOT;
        if (proper) {
            s = edge_insert(t, idx[k], idx[(k + 1) % 3]);
            if (s != NO_SLOT) atomicMin(w.low + s, (uint32_t)(3 * f + k));
            atomicAdd(w.degs + idx[k], 1ull << 32);
        }
        w.hslot[(size_t)3 * f + k] = s;
    }
}

// (keys hold indices that passed load_face's test: both ends lie in [0, V))
__global__ void __launch_bounds__(MT_THREADS) degree_kernel(CollapseWs w, EdgeTable t) {
    if (!w.state[S_ACTIVE]) return;
    const int64_t s = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (s >= t.slots) return;
    const u64 key = t.keys[s];
    if (key == EDGE_EMPTY) return;
    const int a = (int)(key >> 32), b = (int)(unsigned)key;
    atomicAdd(w.degs + a, 1ull);
    atomicAdd(w.degs + b, 1ull);
    if (t.vals[s] != ONCE_EACH_WAY) { w.pinned[a] = 1; w.pinned[b] = 1; }
}

struct DegreeFn {                                                  // element V is 0: the scan's word V is the total
    const u64 *degs;
    int64_t V;
    __device__ u64 operator()(int64_t i) const { return i < V ? degs[i] : 0ull; }
};

__global__ void __launch_bounds__(MT_THREADS) scatter_edges_kernel(CollapseWs w, EdgeTable t) {
    if (!w.state[S_ACTIVE]) return;
    const int64_t s = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (s >= t.slots) return;
    const u64 key = t.keys[s];
    if (key == EDGE_EMPTY) return;
    const int a = (int)(key >> 32), b = (int)(unsigned)key;
    uint32_t *cur = reinterpret_cast<uint32_t *>(w.cur);
    const uint32_t pa = atomicAdd(cur + 2 * (size_t)a, 1u), pb = atomicAdd(cur + 2 * (size_t)b, 1u);
    const uint64_t cap = (uint64_t)w.F0 * 6;
    if (pa < cap) w.nbr[pa] = b;                                   // (a cursor ends at its row's end: the tests never fail)
    if (pb < cap) w.nbr[pb] = a;
}

__global__ void __launch_bounds__(MT_THREADS) scatter_faces_kernel(CollapseWs w) {
    __shared__ int32_t lds[MT_THREADS * 3];
    if (!w.state[S_ACTIVE]) return;
    int f, idx[3];
    bool ok;
    if (!load_face(w.fa, w.state[S_F], w.V, lds, f, idx[0], idx[1], idx[2], ok) || !ok || !distinct(idx[0], idx[1], idx[2])) return;
    uint32_t *cur = reinterpret_cast<uint32_t *>(w.cur);
    const uint64_t cap = (uint64_t)w.F0 * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t p = atomicAdd(cur + 2 * (size_t)idx[k] + 1, 1u);
        if (p < cap) w.vface[p] = f;
    }
}

// the rows of vertex i: neighbours in [o, e) of nbr with the low words of off, faces with the high words
__device__ inline void nbr_row(const CollapseWs &w, int i, int &o, int &e) {
    o = (int)min((u64)(unsigned)w.off[i], (u64)w.F0 * 6);
    e = (int)min((u64)(unsigned)w.off[i + 1], (u64)w.F0 * 6);
}
__device__ inline void face_row(const CollapseWs &w, int i, int &o, int &e) {
    o = (int)min(w.off[i] >> 32, (u64)w.F0 * 3);
    e = (int)min(w.off[i + 1] >> 32, (u64)w.F0 * 3);
}

// ---- a round: candidates ------------------------------------------------------------------------------------------------------------------
// ((q0 x x + q4 y y + q7 z z) + 2 (q1 x y + q2 x z + q5 y z)) + 2 (q3 x + q6 y + q8 z) + q9
__device__ inline double quadric_energy(const double (&q)[10], const double (&x)[3]) {
    const double s1 = (q[0] * x[0] * x[0] + q[4] * x[1] * x[1]) + q[7] * x[2] * x[2];
    const double s2 = (q[1] * x[0] * x[1] + q[2] * x[0] * x[2]) + q[5] * x[1] * x[2];
    const double s3 = (q[3] * x[0] + q[6] * x[1]) + q[8] * x[2];
    return ((s1 + 2.0 * s2) + 2.0 * s3) + q[9];
}

// the absolute position X and the cost E (before the clamp at 0) of collapsing {u, v}; false when either is not finite
__device__ inline bool edge_position(const CollapseWs &w, const double (&c)[3], int u, int v, double (&X)[3], double &E) {
    double q[10], x0[3], x[3];
#pragma unroll
    for (int j = 0; j < 10; ++j) q[j] = w.Q[(size_t)u * 10 + j] + w.Q[(size_t)v * 10 + j];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double pu = w.P[(size_t)u * 3 + k] - c[k], pv = w.P[(size_t)v * 3 + k] - c[k];
        x0[k] = (pu + pv) * 0.5;
        x[k] = x0[k];
    }
    E = quadric_energy(q, x0);
    if (w.placement == PLACE_OPTIMAL) {
        double xs[3];
        quadric_solve(q, x0, xs);
        const double es = quadric_energy(q, xs);
        const bool back = !(isfinite(xs[0]) && isfinite(xs[1]) && isfinite(xs[2])) || es > E;
        if (!back) { x[0] = xs[0]; x[1] = xs[1]; x[2] = xs[2]; E = es; }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = c[k] + x[k];
    return isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && isfinite(E);
}

// whether a face of vertex i's row holds a and b beside it
__device__ inline bool has_face(const CollapseWs &w, int Fc, int i, int a, int b) {
    int o, e;
    face_row(w, i, o, e);
    for (int k = o; k < e; ++k) {
        const int g = w.vface[k];
        if ((unsigned)g >= (unsigned)Fc) continue;
        const int32_t *fc = w.fa + (size_t)g * 3;
        const int c0 = fc[0], c1 = fc[1], c2 = fc[2];
        if ((c0 == a || c1 == a || c2 == a) && (c0 == b || c1 == b || c2 == b)) return true;
    }
    return false;
}

// whether a face of vertex i's row that does not hold both u and v turns over when its corner i moves to X
__device__ inline bool row_flips(const CollapseWs &w, int Fc, int i, int u, int v, const double (&X)[3]) {
    int o, e;
    face_row(w, i, o, e);
    for (int k = o; k < e; ++k) {
        const int g = w.vface[k];
        if ((unsigned)g >= (unsigned)Fc) continue;
        const int32_t *fc = w.fa + (size_t)g * 3;
        const int id[3] = {fc[0], fc[1], fc[2]};
        const bool hu = id[0] == u || id[1] == u || id[2] == u, hv = id[0] == v || id[1] == v || id[2] == v;
        if (hu && hv) continue;
        double p[3][3], n[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                p[j][a] = (unsigned)id[j] < (unsigned)w.V ? w.P[(size_t)id[j] * 3 + a] : 0.0;
                n[j][a] = id[j] == i ? X[a] : p[j][a];
            }
        const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
        const double wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
        const double ox = uy * wz - uz * wy, oy = uz * wx - ux * wz, oz = ux * wy - uy * wx;
        if (ox == 0.0 && oy == 0.0 && oz == 0.0) continue;        // no area: no vote
        const double ax = n[1][0] - n[0][0], ay = n[1][1] - n[0][1], az = n[1][2] - n[0][2];
        const double bx = n[2][0] - n[0][0], by = n[2][1] - n[0][1], bz = n[2][2] - n[0][2];
        const double mx = ay * bz - az * by, my = az * bx - ax * bz, mz = ax * by - ay * bx;
        const double dot = (mx * ox + my * oy) + mz * oz;
        if (!(dot > 0.0)) return true;
    }
    return false;
}

__device__ inline u64 edge_key_of(double E, int u, int v, int r, uint32_t low) {
    const uint32_t bits = __float_as_uint((float)(E > 0.0 ? E : 0.0)) >> 20;
    uint32_t h = (uint32_t)u * 0x9E3779B1u ^ (uint32_t)v * 0x85EBCA77u ^ (uint32_t)r * 0xC2B2AE3Du;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return (u64)bits << 52 | (u64)(h >> 12) << 32 | (u64)low;
}

// the key of slot s's edge when it is a candidate, NO_KEY otherwise
__device__ inline u64 candidate_key(const CollapseWs &w, const EdgeTable &t, int64_t s, int Fc, int r) {
    const u64 ek = t.keys[s];
    if (ek == EDGE_EMPTY) return NO_KEY;
    const int u = (int)(ek >> 32), v = (int)(unsigned)ek;           // u < v
    if (w.pinned[u] || w.pinned[v]) return NO_KEY;
    int ou, eu, ov, ev, common = 0, a = -1, b = -1;
    nbr_row(w, u, ou, eu);
    nbr_row(w, v, ov, ev);
    for (int i = ou; i < eu; ++i) {
        const int x = w.nbr[i];
        bool both = false;
        for (int j = ov; j < ev; ++j) both = both || w.nbr[j] == x;
        if (both) {
            if (common == 0) a = x; else b = x;
            ++common;
        }
    }
    if (common != 2) return NO_KEY;
    if (has_face(w, Fc, u, a, b) && has_face(w, Fc, v, a, b)) return NO_KEY;
    double c[3], X[3], E;
    centre_of_box(w.state, c);
    if (!edge_position(w, c, u, v, X, E)) return NO_KEY;
    if (row_flips(w, Fc, u, u, v, X) || row_flips(w, Fc, v, u, v, X)) return NO_KEY;
    return edge_key_of(E, u, v, r, w.low[s]);
}

__global__ void __launch_bounds__(MT_THREADS) candidate_kernel(CollapseWs w, EdgeTable t) {
    if (!w.state[S_ACTIVE]) return;
    const int64_t s = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    u64 key = NO_KEY;
    if (s < t.slots) {
        key = candidate_key(w, t, s, w.state[S_F], w.state[S_ROUNDS] + 1);
        w.ekey[s] = key;
        if (key != NO_KEY) {
            const u64 ek = t.keys[s];
            atomicMin(w.m1 + (int)(ek >> 32), key);
            atomicMin(w.m1 + (int)(unsigned)ek, key);
        }
    }
    const u64 found = __ballot(key != NO_KEY);
    if (found != 0 && (int)(threadIdx.x & 63) == __ffsll((long long)found) - 1) atomicAdd(w.state + S_NCAND, __popcll(found));
}

// ---- a round: selection ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT_THREADS) spread_kernel(CollapseWs w) {
    if (!w.state[S_ACTIVE]) return;
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= w.V) return;
    int o, e;
    nbr_row(w, (int)i, o, e);
    u64 m = w.m1[i];
    for (int k = o; k < e; ++k) {
        const int x = w.nbr[k];
        if ((unsigned)x < (unsigned)w.V) m = min(m, w.m1[x]);
    }
    w.m2[i] = m;
}

// half-edge h is the lowest half-edge of a selected edge
struct SelectedPred {
    CollapseWs w;
    EdgeTable t;
    __device__ bool operator()(int64_t h) const {
        if (!w.state[S_ACTIVE] || h >= (int64_t)3 * w.state[S_F]) return false;
        const uint32_t s = w.hslot[h];
        if ((u64)s >= (u64)t.slots || w.low[s] != (uint32_t)h) return false;
        const u64 key = w.ekey[s];
        if (key == NO_KEY) return false;
        const u64 ek = t.keys[s];
        return key == w.m2[(int)(ek >> 32)] && key == w.m2[(int)(unsigned)ek];
    }
};

__global__ void __launch_bounds__(MT_THREADS) apply_kernel(SelectedPred sel) {
    const CollapseWs &w = sel.w;
    const int64_t h = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (!sel(h)) return;
    const int quota = (w.state[S_F] - w.target + 1) / 2;
    if (w.hrank[h] >= quota) return;
    const u64 ek = sel.t.keys[w.hslot[h]];
    const int u = (int)(ek >> 32), v = (int)(unsigned)ek;
    double c[3], X[3], E;
    centre_of_box(w.state, c);
    edge_position(w, c, u, v, X, E);                               // (the candidate's own arithmetic on unchanged inputs: its X again)
#pragma unroll
    for (int k = 0; k < 3; ++k) w.P[(size_t)u * 3 + k] = X[k];
#pragma unroll
    for (int j = 0; j < 10; ++j) w.Q[(size_t)u * 10 + j] = w.Q[(size_t)u * 10 + j] + w.Q[(size_t)v * 10 + j];
    w.moved[v] = u;
}

// ---- a round: faces -------------------------------------------------------------------------------------------------------------------------
struct KeptPred {
    CollapseWs w;
    __device__ bool operator()(int64_t f) const {
        if (!w.state[S_ACTIVE] || f >= w.state[S_F]) return false;
        const int32_t *fc = w.fa + (size_t)f * 3;
        const int a = fc[0], b = fc[1], c = fc[2];
        if ((unsigned)a >= (unsigned)w.V || (unsigned)b >= (unsigned)w.V || (unsigned)c >= (unsigned)w.V) return true;
        return !(distinct(a, b, c) && !distinct(w.moved[a], w.moved[b], w.moved[c]));
    }
};

__global__ void __launch_bounds__(MT_THREADS) compact_kernel(KeptPred kept) {
    const CollapseWs &w = kept.w;
    const int64_t f = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (!kept(f)) return;
    const int at = w.fpos[f];                                      // at <= f < F0
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int x = w.fa[(size_t)f * 3 + k];
        w.fb[(size_t)at * 3 + k] = (unsigned)x < (unsigned)w.V ? w.moved[x] : x;
    }
}

__global__ void __launch_bounds__(MT_THREADS) copy_back_kernel(CollapseWs w) {
    if (!w.state[S_ACTIVE]) return;
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < (int64_t)3 * min(w.state[S_NKEEP], w.state[S_F])) w.fa[i] = w.fb[i];
}

__global__ void round_end_kernel(CollapseWs w) {
    int32_t *st = w.state;
    if (!st[S_ACTIVE]) return;
    if (st[S_NCAND] == 0 || st[S_NKEEP] >= st[S_F]) {              // (with a candidate the smallest key is selected: the second never holds)
        st[S_STALLED] = 1;
        st[S_ACTIVE] = 0;
        return;
    }
    st[S_F] = st[S_NKEEP];
    st[S_ROUNDS] += 1;
    st[S_ACTIVE] = st[S_F] > w.target && st[S_ROUNDS] < w.max_rounds ? 1 : 0;
}

void round_launch(const CollapseWs &w, int64_t F, hipStream_t st) {
    const EdgeTable t = edge_table_at(w.table, F);
    const dim3 block(MT_THREADS), fgrid(blocks_of(F, MT_THREADS)), sgrid(blocks_of(t.slots, MT_THREADS)), vgrid(blocks_of(w.V, MT_THREADS));
    hipLaunchKernelGGL(clear_kernel, dim3(blocks_of(t.slots > w.V + 1 ? t.slots : w.V + 1, MT_THREADS)), block, 0, st, w, t);
    hipLaunchKernelGGL(insert_kernel, fgrid, block, 0, st, w, t);
    hipLaunchKernelGGL(degree_kernel, sgrid, block, 0, st, w, t);
    scan_launch(DegreeFn{w.degs, w.V}, (int64_t)w.V + 1, w.bsum, w.off, reinterpret_cast<u64 *>(w.state + S_TOTAL), st, w.cur);
    hipLaunchKernelGGL(scatter_edges_kernel, sgrid, block, 0, st, w, t);
    hipLaunchKernelGGL(scatter_faces_kernel, fgrid, block, 0, st, w);
    hipLaunchKernelGGL(candidate_kernel, sgrid, block, 0, st, w, t);
    hipLaunchKernelGGL(spread_kernel, vgrid, block, 0, st, w);
    const SelectedPred sel{w, t};
    scan_launch(sel, 3 * F, reinterpret_cast<int32_t *>(w.bsum), w.hrank, w.state + S_NSEL, st);
    hipLaunchKernelGGL(apply_kernel, dim3(blocks_of(3 * F, MT_THREADS)), block, 0, st, sel);
    const KeptPred kept{w};
    scan_launch(kept, F, reinterpret_cast<int32_t *>(w.bsum), w.fpos, w.state + S_NKEEP, st);
    hipLaunchKernelGGL(compact_kernel, fgrid, block, 0, st, kept);
    hipLaunchKernelGGL(copy_back_kernel, dim3(blocks_of(3 * F, MT_THREADS)), block, 0, st, w);
    hipLaunchKernelGGL(round_end_kernel, dim3(1), dim3(1), 0, st, w);
}

// ---- epilogue -------------------------------------------------------------------------------------------------------------------------------
struct ReferencedPred {
    const int32_t *ref;
    __device__ bool operator()(int64_t v) const { return ref[v] != 0; }
};

template <class T>
__global__ void __launch_bounds__(MT_THREADS) out_vertices_kernel(CollapseWs w, T *out_verts, int32_t *vertex_map) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v >= w.V) return;
    if (w.ref1[v]) {
        const int at = w.rank[v];                                  // at <= v < V
#pragma unroll
        for (int k = 0; k < 3; ++k) out_verts[(size_t)at * 3 + k] = (T)w.P[(size_t)v * 3 + k];
    }
    int to = -1;
    if (w.ref0[v]) {
        int root = (int)v;
        for (int hops = 0; hops < w.V; ++hops) {                   // (a merge goes to a vertex that lives on: at most `rounds` hops)
            const int next = w.moved[root];
            if (next == root || (unsigned)next >= (unsigned)w.V) break;
            root = next;
        }
        if (w.ref1[root]) to = w.rank[root];
    }
    vertex_map[v] = to;
}

__global__ void __launch_bounds__(MT_THREADS) out_faces_kernel(CollapseWs w, int32_t *out_faces) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= (int64_t)3 * min((int64_t)w.state[S_F], w.F0)) return;
    const int x = w.fa[i];
    out_faces[i] = (unsigned)x < (unsigned)w.V ? w.rank[x] : -1;
}

template <class T>
int collapse_run(const T *verts, const int32_t *faces, CollapseWs w, T *out_verts, int32_t *out_faces, int32_t *vertex_map, int *n_out_verts,
                 int *n_out_faces, int *rounds, int *stalled, hipStream_t st) {
    const char *where = "vt_mesh_collapse";
    const int V = w.V;
    const int64_t F = w.F0;
    const dim3 block(MT_THREADS), fgrid(blocks_of(F, MT_THREADS)), vgrid(blocks_of(V, MT_THREADS));
    int rc = vt_fill32(w.state, 0u, MT_STATUS_BYTES, st);
    if (!rc) rc = vt_fill32(w.state + S_BOX, 0xffffffffu, 3 * 8, st);
    if (!rc) rc = vt_fill32(w.qbig, 0u, (size_t)(reinterpret_cast<char *>(w.fa) - reinterpret_cast<char *>(w.qbig)), st);
    if (rc) return rc;
    copy_words(faces, (size_t)F * 12, w.fa, st);
    hipLaunchKernelGGL(mark_kernel, fgrid, block, 0, st, (const int32_t *)w.fa, (const int32_t *)nullptr, (int)F, V, w.ref0, w.state);
    hipLaunchKernelGGL(widen_kernel<T>, dim3(blocks_of(V, MT_CHUNK)), block, 0, st, verts, V, (const int32_t *)w.ref0, w.P, w.moved, w.state);
    rc = vt_check(hipGetLastError(), where);
    if (rc) return rc;
    int32_t h[32];
    rc = read_status(w.state, h, st, where);
    if (rc) return rc;
    if (h[S_BAD] & BAD_INDEX) return vt_fail(VT_ERR_INVALID, "vt_mesh_collapse: a face index lies outside [0, V)");
    if (h[S_BAD] & BAD_NONFINITE) return vt_fail(VT_ERR_INVALID, "vt_mesh_collapse: a referenced vertex has a non-finite coordinate");
    hipLaunchKernelGGL(qface_kernel<0>, fgrid, block, 0, st, w, (int)F);
    hipLaunchKernelGGL(qface_kernel<1>, fgrid, block, 0, st, w, (int)F);
    hipLaunchKernelGGL(qfinish_kernel, vgrid, block, 0, st, w, (int)F);
    int64_t Fc = F;
    h[S_ACTIVE] = F > w.target;
    while (h[S_ACTIVE]) {
        for (int k = 0; k < MC_ROUND_BATCH; ++k) round_launch(w, Fc, st);
        rc = vt_check(hipGetLastError(), where);
        if (!rc) rc = read_status(w.state, h, st, where);
        if (rc) return rc;
        if (h[S_F] < 1 || h[S_F] > Fc) return vt_fail(VT_ERR_INVALID, "vt_mesh_collapse: the face count on the device left [1, F]");
        Fc = h[S_F];
    }
    hipLaunchKernelGGL(mark_kernel, dim3(blocks_of(Fc, MT_THREADS)), block, 0, st, (const int32_t *)w.fa, (const int32_t *)(w.state + S_F), (int)Fc, V,
                       w.ref1, w.state);
    scan_launch(ReferencedPred{w.ref1}, V, reinterpret_cast<int32_t *>(w.bsum), w.rank, w.state + S_NREF, st);
    hipLaunchKernelGGL(out_vertices_kernel<T>, vgrid, block, 0, st, w, out_verts, vertex_map);
    hipLaunchKernelGGL(out_faces_kernel, dim3(blocks_of(3 * Fc, MT_THREADS)), block, 0, st, w, out_faces);
    rc = vt_check(hipGetLastError(), where);
    if (!rc) rc = read_status(w.state, h, st, where);
    if (rc) return rc;
    *n_out_verts = h[S_NREF];
    *n_out_faces = h[S_F];
    *rounds = h[S_ROUNDS];
    *stalled = h[S_STALLED];
    return 0;
}

}  // namespace

extern "C" {

size_t vt_mesh_collapse_workspace_bytes(int64_t V, int64_t F) { return sizes_ok(V, F) ? collapse_ws(nullptr, V, F).bytes : 0; }

int vt_mesh_collapse(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int64_t target_faces, int placement, int max_rounds,
                     void *out_verts, int32_t *out_faces, int32_t *vertex_map, int *n_out_verts, int *n_out_faces, int *rounds, int *stalled,
                     void *workspace, size_t workspace_bytes, void *stream) {
    if (F > MC_MAX_F)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_collapse: F is above 357913941 = (2^31 - 1) / 6: the neighbour rows could not hold 6 F entries");
    if (!sizes_ok(V, F) || !verts || !faces || !out_verts || !out_faces || !vertex_map || !n_out_verts || !n_out_faces || !rounds || !stalled)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_collapse: bad argument (V >= 1, F >= 1)");
    if (target_faces < 1 || max_rounds < 1 || (placement != PLACE_OPTIMAL && placement != PLACE_MIDPOINT))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_collapse: target_faces >= 1, max_rounds >= 1, placement 0 (optimal) or 1 (midpoint)");
    if (!workspace || workspace_bytes < collapse_ws(nullptr, V, F).bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_collapse");
    CollapseWs w = collapse_ws(workspace, V, F);
    w.target = (int)(target_faces < F ? target_faces : F);
    w.max_rounds = max_rounds;
    w.placement = placement;
    hipStream_t st = (hipStream_t)stream;
    if (verts_f64)
        return collapse_run(static_cast<const double *>(verts), faces, w, static_cast<double *>(out_verts), out_faces, vertex_map, n_out_verts,
                            n_out_faces, rounds, stalled, st);
    return collapse_run(static_cast<const float *>(verts), faces, w, static_cast<float *>(out_verts), out_faces, vertex_map, n_out_verts, n_out_faces,
                        rounds, stalled, st);
}

}  // extern "C"
