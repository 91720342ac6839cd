// Subdivision of a triangle mesh on the device: mark a set of edges, give each marked edge one new vertex, split each face by how many of
// its edges are marked (DESIGN.md, section "mesh_subdivide.hip"; tests/mesh_subdivide_ref.py is the definition, and every output equals
// it bit for bit).  faces [F,3] i32 over V vertices, f32 or f64.  Half-edge h = 3 f + k runs from faces[f][k] to faces[f][(k+1)%3].
//   edge table    mesh_edges.h's table.  Per slot also the lowest and the highest half-edge on the edge (integer atomicMin / atomicMax),
//                 and per half-edge its slot.
//   marks         mark 0 every edge; mark 1 an edge with (dx dx + dy dy) + dz dz > max_edge^2, d = x_hi - x_lo in double, evaluated once
//                 by the edge's lowest half-edge from the lower index to the higher; mark 2 the edges of the faces with face_mask != 0
//                 (atomicOr).  A half-edge is a first use when it is its edge's lowest half-edge and the edge is marked.
//   numbering     scan_launch over the 3 F first-use bytes: marked edges are numbered in first-seen order, as a dict filled face by face
//                 numbers them.  scan_launch again, over 1 + marks(f), gives every face's output offset.  One host read returns the totals.
//   emit          one lane per face writes its 1 + marks children and their face_parent; one lane per first use writes the edge's
//                 vertex and edge_verts; one lane per original vertex copies it (midpoint) or applies Loop's even rule over its CSR row.
//   backward      g_v[i] = g[i] + 0.5 sum of g[V + e] over the edges at i, as mesh_normals.hip sums: the largest |term| per (vertex,
//                 coordinate) by atomicMax on the bit pattern, then two int64 fixed-point limbs by integer atomicAdd, rounded once.
// No float atomic anywhere: equal bits from run to run.  A face with an index outside [0, V) or with a repeated index is never
// dereferenced; it sets bit 0 of the status word, the count fails and nothing is emitted.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_common.h"
#include "mesh_edges.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

enum { ST_BAD = 0, ST_NMARKED = 1, ST_NOUT = 2, ST_NIRR = 3 };     // int32 words of the status block
enum { MARK_ALL = 0, MARK_LENGTH = 1, MARK_FACES = 2 };
enum { MIDPOINT = 0, LOOP = 1 };
// ---- the edge table ------------------------------------------------------------------------------------------------------------------------
struct Table {                                                     // the shared table, four more words per slot, and per half-edge its slot
    EdgeTable e;
    int32_t *minh, *maxh, *eid, *emark;
    uint32_t *he_slot;
};

__global__ void __launch_bounds__(MT_THREADS)
insert_kernel(const int32_t *faces, int F, int V, int mark, const uint8_t *face_mask, Table t, int32_t *status) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    const int64_t h0 = (int64_t)f * 3;
    if (!ok || a == b || b == c || c == a) {
        atomicOr(status + ST_BAD, 1);
        t.he_slot[h0] = NO_SLOT; t.he_slot[h0 + 1] = NO_SLOT; t.he_slot[h0 + 2] = NO_SLOT;
        return;
    }
    const bool sel = mark == MARK_FACES && face_mask[f] != 0;
    const int tail[3] = {a, b, c}, head[3] = {b, c, a};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t slot = edge_insert(t.e, tail[k], head[k]);
        t.he_slot[h0 + k] = slot;
        if (slot == NO_SLOT) continue;
        atomicMin(t.minh + slot, (int)(h0 + k));
        atomicMax(t.maxh + slot, (int)(h0 + k));
        if (sel) atomicOr(t.emark + slot, 1);
    }
}

// first[h] = 1 when h is the lowest half-edge of a marked edge
template <class T>
__global__ void __launch_bounds__(MT_THREADS) first_kernel(const T *verts, int64_t n, int mark, double max2, Table t, uint8_t *first) {
    const int64_t h = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (h >= n) return;
    const uint32_t slot = t.he_slot[h];
    uint8_t out = 0;
    if (slot != NO_SLOT && t.minh[slot] == (int)h) {
        if (mark == MARK_ALL) out = 1;
        else if (mark == MARK_FACES) out = t.emark[slot] != 0;
        else {
            const u64 key = t.e.keys[slot];                          // (both ends passed load_face's test)
            double x0, y0, z0, x1, y1, z1;
            load_vertex(verts, (int)(key >> 32), x0, y0, z0);
            load_vertex(verts, (int)(unsigned)key, x1, y1, z1);
            const double dx = x1 - x0, dy = y1 - y0, dz = z1 - z0;
            out = ((dx * dx + dy * dy) + dz * dz) > max2;
        }
    }
    first[h] = out;
}

struct ByteFlag {
    const uint8_t *b;
    __device__ bool operator()(int64_t i) const { return b[i] != 0; }
};

// the edge's number at its slot; an edge that is neither interior (1, 1) nor boundary (1, 0) / (0, 1) is counted
__global__ void __launch_bounds__(MT_THREADS) number_kernel(int64_t n, const uint8_t *first, const int32_t *pos, Table t, int32_t *status) {
    const int64_t h = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (h >= n || !first[h]) return;
    const uint32_t slot = t.he_slot[h];
    t.eid[slot] = pos[h];
    const u64 v = t.e.vals[slot];
    const u64 fwd = v & 0xffffffffull, bwd = v >> 32;
    if (!(fwd <= 1 && bwd <= 1)) atomicAdd(status + ST_NIRR, 1);
}

struct ChildrenFn {                                                // 1 + the marked edges of face f
    const uint32_t *he_slot;
    const int32_t *eid;
    __device__ int operator()(int64_t f) const {
        int n = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t slot = he_slot[f * 3 + k];
            n += (slot != NO_SLOT && eid[slot] >= 0) ? 1 : 0;
        }
        return n;
    }
};

// ---- emit ------------------------------------------------------------------------------------------------------------------------------------
__device__ inline void put_face(int32_t *out_faces, int32_t *face_parent, int64_t at, int f, int x, int y, int z) {
    out_faces[at * 3] = x; out_faces[at * 3 + 1] = y; out_faces[at * 3 + 2] = z;
    face_parent[at] = f;
}

template <class T>
__global__ void __launch_bounds__(MT_THREADS)
faces_kernel(const T *verts, const int32_t *faces, int F, int V, Table t, const int32_t *foff, int n_marked, int n_out, int32_t *out_faces,
             int32_t *face_parent) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    if (!ok) return;
    int m[3];                                                      // the new vertex on ab, bc, ca, or -1
    int n = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t slot = t.he_slot[(int64_t)f * 3 + k];
        const int e = slot != NO_SLOT ? t.eid[slot] : -1;
        m[k] = (unsigned)e < (unsigned)n_marked ? V + e : -1;
        n += m[k] >= 0 ? 1 : 0;
    }
    const int64_t o = foff[f];
    if (o < 0 || o + 1 + n > n_out) return;                       // (not the workspace vt_mesh_subdivide_count left for these faces)
    const int idx[3] = {a, b, c};
    if (n == 0) { put_face(out_faces, face_parent, o, f, a, b, c); return; }
    if (n == 3) {
        put_face(out_faces, face_parent, o, f, m[0], m[1], m[2]);
        put_face(out_faces, face_parent, o + 1, f, a, m[0], m[2]);
        put_face(out_faces, face_parent, o + 2, f, b, m[1], m[0]);
        put_face(out_faces, face_parent, o + 3, f, c, m[2], m[1]);
        return;
    }
    if (n == 1) {
        const int k0 = m[0] >= 0 ? 0 : (m[1] >= 0 ? 1 : 2);       // the marked edge (p, q), r opposite
        const int p = idx[k0], q = idx[(k0 + 1) % 3], r = idx[(k0 + 2) % 3], mid = m[k0];
        put_face(out_faces, face_parent, o, f, p, mid, r);
        put_face(out_faces, face_parent, o + 1, f, mid, q, r);
        return;
    }
    const int k0 = m[0] < 0 ? 0 : (m[1] < 0 ? 1 : 2);             // the unmarked edge (p, q); s on qr, u on rp
    const int p = idx[k0], q = idx[(k0 + 1) % 3], r = idx[(k0 + 2) % 3], s = m[(k0 + 1) % 3], u = m[(k0 + 2) % 3];
    double px, py, pz, qx, qy, qz, rx, ry, rz;
    load_vertex(verts, p, px, py, pz);
    load_vertex(verts, q, qx, qy, qz);
    load_vertex(verts, r, rx, ry, rz);
    const double sx = (qx + rx) * 0.5, sy = (qy + ry) * 0.5, sz = (qz + rz) * 0.5;
    const double ux = (rx + px) * 0.5, uy = (ry + py) * 0.5, uz = (rz + pz) * 0.5;
    const double ax = sx - px, ay = sy - py, az = sz - pz;       // diagonal p - s
    const double bx = ux - qx, by = uy - qy, bz = uz - qz;       // diagonal q - u
    const double lps = (ax * ax + ay * ay) + az * az, lqu = (bx * bx + by * by) + bz * bz;
    const bool along_ps = lps < lqu || (!(lqu < lps) && p < q);   // a tie (or a NaN): the diagonal that leaves the lower of p and q
    put_face(out_faces, face_parent, o, f, r, u, s);
    if (along_ps) {
        put_face(out_faces, face_parent, o + 1, f, p, q, s);
        put_face(out_faces, face_parent, o + 2, f, p, s, u);
    } else {
        put_face(out_faces, face_parent, o + 1, f, p, q, u);
        put_face(out_faces, face_parent, o + 2, f, q, s, u);
    }
}

// Loop: both ends of an irregular edge keep their bits
__global__ void __launch_bounds__(MT_THREADS) irregular_ends_kernel(int64_t n, const uint8_t *first, Table t, int V, int32_t *virr) {
    const int64_t h = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (h >= n || !first[h]) return;
    const uint32_t slot = t.he_slot[h];
    const u64 v = t.e.vals[slot], key = t.e.keys[slot];
    if ((v & 0xffffffffull) <= 1 && (v >> 32) <= 1) return;
    const int lo = (int)(key >> 32), hi = (int)(unsigned)key;
    if ((unsigned)lo < (unsigned)V) atomicOr(virr + lo, 1);
    if ((unsigned)hi < (unsigned)V) atomicOr(virr + hi, 1);
}

// one lane per first use: the edge's vertex and its pair
template <class T>
__global__ void __launch_bounds__(MT_THREADS)
edges_kernel(const T *verts, const int32_t *faces, int64_t n, int V, int scheme, const uint8_t *first, const int32_t *pos, Table t, int n_marked,
             T *out_verts, int32_t *edge_verts) {
    const int64_t h = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (h >= n || !first[h]) return;
    const int e = pos[h];
    const uint32_t slot = t.he_slot[h];
    if ((unsigned)e >= (unsigned)n_marked || slot == NO_SLOT) return;
    const u64 key = t.e.keys[slot];
    const int lo = (int)(key >> 32), hi = (int)(unsigned)key;
    if ((unsigned)lo >= (unsigned)V || (unsigned)hi >= (unsigned)V) return;
    edge_verts[(size_t)e * 2] = lo;
    edge_verts[(size_t)e * 2 + 1] = hi;
    T *out = out_verts + ((size_t)V + e) * 3;
    if (scheme == MIDPOINT) {
        const T *a = verts + (size_t)lo * 3, *b = verts + (size_t)hi * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = (a[k] + b[k]) * (T)0.5;
        return;
    }
    double x0[3], x1[3];
    load_vertex(verts, lo, x0[0], x0[1], x0[2]);
    load_vertex(verts, hi, x1[0], x1[1], x1[2]);
    const u64 v = t.e.vals[slot];
    const int h1 = t.maxh[slot];
    if ((v & 0xffffffffull) == 1 && (v >> 32) == 1 && (unsigned)h1 < (unsigned)n && h1 != (int)h) {
        // exactly two half-edges lie on the edge: this one and the highest.  c is opposite in the lo -> hi face, d in the hi -> lo face.
        const int ha = faces[h] == lo ? (int)h : h1, hb = faces[h] == lo ? h1 : (int)h;
        const int c = faces[(ha / 3) * 3 + (ha % 3 + 2) % 3], d = faces[(hb / 3) * 3 + (hb % 3 + 2) % 3];
        if ((unsigned)c < (unsigned)V && (unsigned)d < (unsigned)V) {
            double xc[3], xd[3];
            load_vertex(verts, c, xc[0], xc[1], xc[2]);
            load_vertex(verts, d, xd[0], xd[1], xd[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = (T)(0.375 * (x0[k] + x1[k]) + 0.125 * (xc[k] + xd[k]));
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (T)((x0[k] + x1[k]) * 0.5);
}

// Loop's even rule; a vertex that keeps its place is copied
template <class T>
__global__ void __launch_bounds__(MT_THREADS)
even_kernel(const T *verts, int V, const int32_t *off, const int32_t *neighbors, const uint8_t *boundary_edge, const uint8_t *boundary_vertex, int nnz,
            const int32_t *virr, T *out_verts) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= V) return;
    const T *src = verts + (size_t)i * 3;
    T *out = out_verts + (size_t)i * 3;
    const int o = max(off[i], 0), e = min(off[i + 1], nnz);
    bool keep = virr[i] != 0 || e <= o;
    double r[3] = {0.0, 0.0, 0.0};
    if (!keep) {
        const double x[3] = {(double)src[0], (double)src[1], (double)src[2]};
        if (boundary_vertex[i]) {
            int nb = 0, j = -1, k2 = -1;
            for (int k = o; k < e; ++k) {
                if (!boundary_edge[k]) continue;
                if (nb == 0) j = neighbors[k]; else if (nb == 1) k2 = neighbors[k];
                ++nb;
            }
            if (nb == 2 && (unsigned)j < (unsigned)V && (unsigned)k2 < (unsigned)V) {
                double xj[3], xk[3];
                load_vertex(verts, j, xj[0], xj[1], xj[2]);
                load_vertex(verts, k2, xk[0], xk[1], xk[2]);
#pragma unroll
                for (int a = 0; a < 3; ++a) r[a] = 0.75 * x[a] + 0.125 * (xj[a] + xk[a]);
            } else keep = true;
        } else {
            double s[3] = {0.0, 0.0, 0.0};
            for (int k = o; k < e; ++k) {
                const int j = neighbors[k];
                if ((unsigned)j >= (unsigned)V) { keep = true; break; }     // (rows that are not vt_mesh_adjacency_fill's)
                double xj[3];
                load_vertex(verts, j, xj[0], xj[1], xj[2]);
                s[0] = s[0] + xj[0]; s[1] = s[1] + xj[1]; s[2] = s[2] + xj[2];
            }
            const double n = (double)(e - o);
            const double beta = (e - o) == 3 ? 0.1875 : 3.0 / (8.0 * n);
            const double w = 1.0 - n * beta;
#pragma unroll
            for (int a = 0; a < 3; ++a) r[a] = w * x[a] + beta * s[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = keep ? src[a] : (T)r[a];
}

// ---- the midpoint scheme over a batch, and its gradient -----------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(MT_THREADS) midpoints_kernel(const T *verts, int64_t B, int V, const int32_t *edge_verts, int E, T *out) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    const int64_t per = (int64_t)V + E;
    if (i >= B * per) return;
    const int64_t b = i / per, j = i - b * per;
    const T *src = verts + (size_t)b * V * 3;
    T *dst = out + (size_t)i * 3;
    if (j < V) {
        dst[0] = src[j * 3]; dst[1] = src[j * 3 + 1]; dst[2] = src[j * 3 + 2];
        return;
    }
    const int lo = edge_verts[(j - V) * 2], hi = edge_verts[(j - V) * 2 + 1];
    if ((unsigned)lo >= (unsigned)V || (unsigned)hi >= (unsigned)V) {       // never dereferenced: a NaN the caller cannot miss
        const T nan = (T)__longlong_as_double(0x7ff8000000000000ll);
        dst[0] = nan; dst[1] = nan; dst[2] = nan;
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k] = (src[(size_t)lo * 3 + k] + src[(size_t)hi * 3 + k]) * (T)0.5;
}

// item j < V: the term g[j] of vertex j; item V + e: the term 0.5 g[V + e] of both ends of edge e.
// PASS 0: the largest |term| per (vertex, coordinate); PASS 1: the fixed-point limbs against its exponent.
template <class T, int PASS>
__global__ void __launch_bounds__(MT_THREADS) bwd_terms_kernel(const T *g, int V, const int32_t *edge_verts, int E, u64 *vmax, u64 *sums, int32_t *status) {
    const int64_t j = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (j >= (int64_t)V + E) return;
    int ends[2] = {(int)j, -1};
    double w = 1.0;
    if (j >= V) {
        ends[0] = edge_verts[(j - V) * 2]; ends[1] = edge_verts[(j - V) * 2 + 1];
        w = 0.5;
        if ((unsigned)ends[0] >= (unsigned)V || (unsigned)ends[1] >= (unsigned)V) {
            if (PASS == 0) atomicOr(status + ST_BAD, 1);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double term = w * (double)g[(size_t)j * 3 + k];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int v = ends[s];
            if (v < 0) continue;
            const size_t at = (size_t)v * 3 + k;
            if (PASS == 0) {
                atomicMax(vmax + at, (u64)__double_as_longlong(fabs(term)));      // (a NaN's pattern lies above every number's)
            } else {
                const u64 m = vmax[at];
                if ((m >> 52) >= 0x7ff) continue;                    // a term that is not finite: the sum is NaN (bwd_finish_kernel)
                u64 hi, lo;
                limbs_of(term, exponent_of(m), hi, lo);
                atomicAdd(sums + at * 2, hi);
                atomicAdd(sums + at * 2 + 1, lo);
            }
        }
    }
}

template <class T>
__global__ void __launch_bounds__(MT_THREADS) bwd_finish_kernel(const u64 *vmax, const u64 *sums, int64_t n, T *grad_verts) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= n) return;
    const u64 m = vmax[i];
    double out;
    if ((m >> 52) >= 0x7ff) out = __longlong_as_double(0x7ff8000000000000ll);
    else out = sum_of(sums[i * 2], sums[i * 2 + 1], exponent_of(m));
    grad_verts[i] = (T)out;
}

// ---- the workspaces -----------------------------------------------------------------------------------------------------------------------------
bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && F >= 0 && V <= MT_MAX_V && F <= MT_MAX_F; }

// status | table (keys, counts, lowest and highest half-edge, number, mark) | per half-edge: slot, first use, number | face offsets |
// irregular ends | scan sums
struct SubWs {
    int32_t *status, *pos, *foff, *virr, *bsum;
    uint8_t *first;
    Table t;
    size_t bytes;
};

SubWs sub_ws(void *workspace, int64_t V, int64_t F) {
    SubWs w;
    char *p = static_cast<char *>(workspace);
    size_t at = 0;
    const int64_t F1 = F < 1 ? 1 : F;
    w.status = reinterpret_cast<int32_t *>(p); at += MT_STATUS_BYTES;
    w.t.e = edge_table_at(p + at, F1); at += (size_t)w.t.e.slots * 16;
    const size_t per_slot = (size_t)w.t.e.slots * 4;
    w.t.minh = reinterpret_cast<int32_t *>(p + at); at += per_slot;
    w.t.maxh = reinterpret_cast<int32_t *>(p + at); at += per_slot;
    w.t.eid = reinterpret_cast<int32_t *>(p + at); at += per_slot;
    w.t.emark = reinterpret_cast<int32_t *>(p + at); at += per_slot;
    w.t.he_slot = reinterpret_cast<uint32_t *>(p + at); at += up256((size_t)F1 * 3 * 4);
    w.first = reinterpret_cast<uint8_t *>(p + at); at += up256((size_t)F1 * 3);
    w.pos = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)F1 * 3 * 4);
    w.foff = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)F1 * 4);
    w.virr = reinterpret_cast<int32_t *>(p + at); at += up256((size_t)V * 4);
    w.bsum = reinterpret_cast<int32_t *>(p + at); at += scan_bytes(F1 * 3);
    w.bytes = at;
    return w;
}

size_t bwd_bytes(int64_t V) { return MT_STATUS_BYTES + up256((size_t)V * 3 * 8) + up256((size_t)V * 6 * 8); }

template <class T>
void emit_launch(const T *verts, int64_t V, const int32_t *faces, int64_t F, int64_t n_marked, int64_t n_out, int scheme, const int32_t *offsets,
                 const int32_t *neighbors, const uint8_t *boundary_edge, const uint8_t *boundary_vertex, int64_t nnz, T *out_verts, int32_t *out_faces,
                 int32_t *edge_verts, int32_t *face_parent, const SubWs &w, hipStream_t st) {
    const dim3 block(MT_THREADS), hgrid(blocks_of(F * 3, MT_THREADS));
    if (scheme == LOOP) {
        hipLaunchKernelGGL(irregular_ends_kernel, hgrid, block, 0, st, F * 3, (const uint8_t *)w.first, w.t, (int)V, w.virr);
        hipLaunchKernelGGL(even_kernel<T>, dim3(blocks_of(V, MT_THREADS)), block, 0, st, verts, (int)V, offsets, neighbors, boundary_edge, boundary_vertex,
                           (int)nnz, (const int32_t *)w.virr, out_verts);
    } else {
        copy_words(verts, (size_t)V * 3 * sizeof(T), out_verts, st);
    }
    hipLaunchKernelGGL(faces_kernel<T>, dim3(blocks_of(F, MT_THREADS)), block, 0, st, verts, faces, (int)F, (int)V, w.t, (const int32_t *)w.foff,
                       (int)n_marked, (int)n_out, out_faces, face_parent);
    if (n_marked > 0)
        hipLaunchKernelGGL(edges_kernel<T>, hgrid, block, 0, st, verts, faces, F * 3, (int)V, scheme, (const uint8_t *)w.first, (const int32_t *)w.pos, w.t,
                           (int)n_marked, out_verts, edge_verts);
}

template <class T>
void bwd_launch(const T *g, int64_t V, const int32_t *edge_verts, int64_t E, T *grad_verts, u64 *vmax, u64 *sums, int32_t *status, hipStream_t st) {
    const dim3 block(MT_THREADS), grid(blocks_of(V + E, MT_THREADS));
    hipLaunchKernelGGL((bwd_terms_kernel<T, 0>), grid, block, 0, st, g, (int)V, edge_verts, (int)E, vmax, sums, status);
    hipLaunchKernelGGL((bwd_terms_kernel<T, 1>), grid, block, 0, st, g, (int)V, edge_verts, (int)E, vmax, sums, status);
    hipLaunchKernelGGL(bwd_finish_kernel<T>, dim3(blocks_of(V * 3, MT_THREADS)), block, 0, st, (const u64 *)vmax, (const u64 *)sums, V * 3, grad_verts);
}

}  // namespace

extern "C" {

size_t vt_mesh_subdivide_workspace_bytes(int64_t V, int64_t F) { return sizes_ok(V, F) ? sub_ws(nullptr, V, F).bytes : 0; }

int vt_mesh_subdivide_count(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int mark, double max_edge,
                            const uint8_t *face_mask, int *n_marked, int *n_out_faces, int *n_irregular, void *workspace, size_t workspace_bytes,
                            void *stream) {
    if (!sizes_ok(V, F) || mark < 0 || mark > 2 || !n_marked || !n_out_faces || !n_irregular || (F > 0 && !faces) || (mark == MARK_LENGTH && !verts) ||
        (mark == MARK_FACES && F > 0 && !face_mask))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_subdivide_count: bad argument (V >= 1, F >= 0, mark 0..2; mark 1 needs verts, mark 2 face_mask)");
    if (mark == MARK_LENGTH && !(max_edge > 0.0)) return vt_fail(VT_ERR_INVALID, "vt_mesh_subdivide_count: max_edge must be positive");
    *n_marked = *n_out_faces = *n_irregular = 0;
    if (F == 0) return 0;
    if (!workspace || workspace_bytes < sub_ws(nullptr, V, F).bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_subdivide_count");
    hipStream_t st = (hipStream_t)stream;
    const SubWs w = sub_ws(workspace, V, F);
    int rc = vt_fill32(w.status, 0u, MT_STATUS_BYTES, st);
    if (!rc) rc = edge_table_clear(w.t.e, st);
    if (!rc) rc = vt_fill32(w.t.minh, 0x7fffffffu, (size_t)w.t.e.slots * 4, st);
    if (!rc) rc = vt_fill32(w.t.maxh, 0xffffffffu, (size_t)w.t.e.slots * 4, st);
    if (!rc) rc = vt_fill32(w.t.eid, 0xffffffffu, (size_t)w.t.e.slots * 4, st);
    if (!rc) rc = vt_fill32(w.t.emark, 0u, (size_t)w.t.e.slots * 4, st);
    if (rc) return rc;
    const dim3 block(MT_THREADS), fgrid(blocks_of(F, MT_THREADS)), hgrid(blocks_of(F * 3, MT_THREADS));
    const double max2 = max_edge * max_edge;
    hipLaunchKernelGGL(insert_kernel, fgrid, block, 0, st, faces, (int)F, (int)V, mark, face_mask, w.t, w.status);
    if (verts_f64)
        hipLaunchKernelGGL(first_kernel<double>, hgrid, block, 0, st, static_cast<const double *>(verts), F * 3, mark, max2, w.t, w.first);
    else
        hipLaunchKernelGGL(first_kernel<float>, hgrid, block, 0, st, static_cast<const float *>(verts), F * 3, mark, max2, w.t, w.first);
    scan_launch(ByteFlag{w.first}, F * 3, w.bsum, w.pos, w.status + ST_NMARKED, st);
    hipLaunchKernelGGL(number_kernel, hgrid, block, 0, st, F * 3, (const uint8_t *)w.first, (const int32_t *)w.pos, w.t, w.status);
    scan_launch(ChildrenFn{w.t.he_slot, w.t.eid}, F, w.bsum, w.foff, w.status + ST_NOUT, st);
    rc = vt_check(hipGetLastError(), "vt_mesh_subdivide_count");
    if (rc) return rc;
    int32_t h[16];
    rc = read_status(workspace, h, st, "vt_mesh_subdivide_count");
    if (rc) return rc;
    if (h[ST_BAD]) return vt_fail(VT_ERR_INVALID, "vt_mesh_subdivide_count: a face has an index outside [0, V) or a repeated index");
    if (h[ST_NMARKED] < 0 || h[ST_NMARKED] > 3 * F || h[ST_NOUT] < F || h[ST_NOUT] > 4 * F || V + (int64_t)h[ST_NMARKED] > 0x7fffffff)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_subdivide_count: V + n_marked or the output face count does not fit an int32");
    *n_marked = h[ST_NMARKED];
    *n_out_faces = h[ST_NOUT];
    *n_irregular = h[ST_NIRR];
    return 0;
}

int vt_mesh_subdivide_emit(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int64_t n_marked, int64_t n_out_faces,
                           int scheme, const int32_t *offsets, const int32_t *neighbors, const uint8_t *boundary_edge, const uint8_t *boundary_vertex,
                           int64_t nnz, void *out_verts, int32_t *out_faces, int32_t *edge_verts, int32_t *face_parent, void *workspace,
                           size_t workspace_bytes, void *stream) {
    if (!sizes_ok(V, F) || n_marked < 0 || n_marked > 3 * F || n_out_faces < F || n_out_faces > 4 * F || V + n_marked > 0x7fffffff ||
        (scheme != MIDPOINT && scheme != LOOP) || !verts || !out_verts || (F > 0 && (!faces || !out_faces || !face_parent)) ||
        (n_marked > 0 && !edge_verts))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_subdivide_emit: bad argument (the counts are vt_mesh_subdivide_count's; scheme 0 or 1)");
    if (scheme == LOOP && (nnz < 0 || nnz > 0x7fffffff || !offsets || !boundary_vertex || (nnz && (!neighbors || !boundary_edge))))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_subdivide_emit: scheme 1 needs the rows of vt_mesh_adjacency_count / _fill");
    if (scheme == LOOP && F > 0 && n_marked == 0)
        return vt_fail(VT_ERR_INVALID, "vt_mesh_subdivide_emit: scheme 1 goes with mark 0 only");
    hipStream_t st = (hipStream_t)stream;
    if (F == 0) {                                                  // nothing to split: the vertices' bits
        copy_words(verts, (size_t)V * 3 * (verts_f64 ? 8 : 4), out_verts, st);
        return vt_check(hipGetLastError(), "vt_mesh_subdivide_emit");
    }
    if (!workspace || workspace_bytes < sub_ws(nullptr, V, F).bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_subdivide_emit");
    const SubWs w = sub_ws(workspace, V, F);
    if (scheme == LOOP) {
        const int rc = vt_fill32(w.virr, 0u, up256((size_t)V * 4), st);
        if (rc) return rc;
    }
    if (verts_f64)
        emit_launch<double>(static_cast<const double *>(verts), V, faces, F, n_marked, n_out_faces, scheme, offsets, neighbors, boundary_edge,
                            boundary_vertex, nnz, static_cast<double *>(out_verts), out_faces, edge_verts, face_parent, w, st);
    else
        emit_launch<float>(static_cast<const float *>(verts), V, faces, F, n_marked, n_out_faces, scheme, offsets, neighbors, boundary_edge,
                           boundary_vertex, nnz, static_cast<float *>(out_verts), out_faces, edge_verts, face_parent, w, st);
    return vt_check(hipGetLastError(), "vt_mesh_subdivide_emit");
}

int vt_mesh_subdivide_midpoints(const void *verts, int verts_f64, int64_t B, int64_t V, const int32_t *edge_verts, int64_t E, void *out_verts,
                                void *stream) {
    if (B < 1 || B > 0x7fffffff || V < 1 || E < 0 || V + E > 0x7fffffff || !verts || !out_verts || (E > 0 && !edge_verts))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_subdivide_midpoints: bad argument (B >= 1, V >= 1, E >= 0, V + E < 2^31)");
    if (B * (V + E) > ((int64_t)1 << 38)) return vt_fail(VT_ERR_INVALID, "vt_mesh_subdivide_midpoints: B (V + E) is above 2^38");
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(MT_THREADS), grid(blocks_of(B * (V + E), MT_THREADS));
    if (verts_f64)
        hipLaunchKernelGGL(midpoints_kernel<double>, grid, block, 0, st, static_cast<const double *>(verts), B, (int)V, edge_verts, (int)E,
                           static_cast<double *>(out_verts));
    else
        hipLaunchKernelGGL(midpoints_kernel<float>, grid, block, 0, st, static_cast<const float *>(verts), B, (int)V, edge_verts, (int)E,
                           static_cast<float *>(out_verts));
    return vt_check(hipGetLastError(), "vt_mesh_subdivide_midpoints");
}

size_t vt_mesh_subdivide_bwd_workspace_bytes(int64_t V) { return V >= 1 && V <= MT_MAX_V ? bwd_bytes(V) : 0; }

int vt_mesh_subdivide_bwd(const int32_t *edge_verts, int64_t V, int64_t E, const void *grad_out, int grad_f64, void *grad_verts, void *workspace,
                          size_t workspace_bytes, void *stream) {
    if (V < 1 || V > MT_MAX_V || E < 0 || V + E > 0x7fffffff || !grad_out || !grad_verts || (E > 0 && !edge_verts))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_subdivide_bwd: bad argument (V >= 1, E >= 0, V + E < 2^31)");
    if (!workspace || workspace_bytes < bwd_bytes(V)) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_subdivide_bwd");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    int32_t *status = reinterpret_cast<int32_t *>(ws);
    u64 *vmax = reinterpret_cast<u64 *>(ws + MT_STATUS_BYTES);
    u64 *sums = reinterpret_cast<u64 *>(ws + MT_STATUS_BYTES + up256((size_t)V * 3 * 8));
    const int rc = vt_fill32(ws, 0u, bwd_bytes(V), st);
    if (rc) return rc;
    if (grad_f64) bwd_launch<double>(static_cast<const double *>(grad_out), V, edge_verts, E, static_cast<double *>(grad_verts), vmax, sums, status, st);
    else bwd_launch<float>(static_cast<const float *>(grad_out), V, edge_verts, E, static_cast<float *>(grad_verts), vmax, sums, status, st);
    return vt_check(hipGetLastError(), "vt_mesh_subdivide_bwd");
}

}  // extern "C"
