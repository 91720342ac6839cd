// Fast winding number (Barill et al., "Fast Winding Numbers for Soups and Clouds", SIGGRAPH 2018): an octree over the faces' centroids
// whose cells carry the dipole expansion of their faces to order 2, and a query that walks it.  The reference labels every re-sampled
// query point with igl.fast_winding_number_for_meshes (src/conv_onet/training.py:307, 359, 723, 862); winding.hip evaluates the exact
// sum that call approximates, this file the approximation itself.  The definitions are DESIGN.md's section "winding_fast.hip", restated
// in numpy by tests/winding_fast_ref.py: this file's operations in this file's order.
//   inputs    verts [V,3] f32, faces [F,3] i32 (indices clamped to [0, V) as winding_kernel clamps them), pts [N,3] f32; every number
//             below is float64 on the exactly converted inputs, every product and sum a separate rounding (-ffp-contract=off)
//   tree      octree_common.h's octree with WfSource below: the frame spans the vertices, a face lives in the leaf of its centroid
//             ((a + b) + c) / 3 and carries its corners (9 f32) in list order; pyramids, lists ascending by face index
//   record    36 doubles per occupied cell: p, r, N0, M1[j][i], M2[jk][i] (jk = 00 01 02 11 12 22), total area, face count.  A leaf is
//             summed by one thread over its list, an inner cell by one thread over its children in Morton order: no float atomic, one
//             order, the records are equal from run to run and equal to the restatement's bit for bit
//   query     one lane per query, octree_common.h's walk in Morton order.  A cell with |q - p|^2 > accuracy^2 r^2 adds its expansion, a
//             leaf that is not accepted the Van Oosterom-Strackee solid angles of its faces in list order; w = (far + near) / 4 pi
// No launch function allocates, copies to the host or waits: the one host read of a build (the occupied cells per level and the status
// word, the first 64 bytes of vt_winding_tree_count's workspace: octree_common.h's state words) is the caller's, between the two calls.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "mesh_common.h"
#include "octree_common.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

constexpr int WF_REC = 36;                      // doubles per cell record (288 bytes: 16-byte aligned rows)

__device__ inline int wf_clamp(int v, int V) { return v < 0 ? 0 : (v >= V ? V - 1 : v); }

// octree_common.h's source of a mesh: the frame spans the vertices, a face is binned by its centroid and carries its corners
struct WfSource {
    const float *verts;
    const int32_t *faces;
    int V, F;
    static constexpr size_t PAYLOAD = 9 * sizeof(float);
    __host__ __device__ int coords() const { return V; }
    __host__ __device__ int items() const { return F; }
    __device__ double coord(int, int64_t v, int a) const { return (double)verts[3 * v + a]; }
    __device__ double frame_lo(double x) const { return x; }
    __device__ void point(int, int64_t f, double c[3]) const {
        double p[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int vi = wf_clamp(faces[3 * f + k], V);
#pragma unroll
            for (int a = 0; a < 3; ++a) p[k][a] = (double)verts[3 * (size_t)vi + a];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = ((p[0][a] + p[1][a]) + p[2][a]) / 3.0;
    }
    __device__ void payload(int, int64_t f, char *slot) const {
        float *tri = reinterpret_cast<float *>(slot);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int vi = wf_clamp(faces[3 * f + k], V);
#pragma unroll
            for (int a = 0; a < 3; ++a) tri[3 * k + a] = verts[3 * (size_t)vi + a];
        }
    }
};

bool wf_tree(int64_t F, int L, const int32_t *state, OtTree &t) { return ot_tree(F, L, 1, state, WF_REC, WfSource::PAYLOAD, t); }

// ---- records -----------------------------------------------------------------------------------------------------------------------
struct WfFace { double p[3][3], nv[3], area, cen[3]; };

__device__ inline void wf_face(const float *t, WfFace &f) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) f.p[k][a] = (double)t[3 * k + a];
    double e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { e1[a] = f.p[1][a] - f.p[0][a]; e2[a] = f.p[2][a] - f.p[0][a]; }
    f.nv[0] = 0.5 * (e1[1] * e2[2] - e1[2] * e2[1]);
    f.nv[1] = 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]);
    f.nv[2] = 0.5 * (e1[0] * e2[1] - e1[1] * e2[0]);
    f.area = sqrt((f.nv[0] * f.nv[0] + f.nv[1] * f.nv[1]) + f.nv[2] * f.nv[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) f.cen[a] = ((f.p[0][a] + f.p[1][a]) + f.p[2][a]) / 3.0;
}

// pair n of the symmetric index (j, k): 00 01 02 11 12 22
#define WF_PAIR_J(n) ((n) < 3 ? 0 : ((n) < 5 ? 1 : 2))
#define WF_PAIR_K(n) ((n) < 3 ? (n) : ((n) < 5 ? (n) - 2 : 2))

__global__ void __launch_bounds__(MT_THREADS)
wf_leaf_kernel(const int32_t *pyr_leaf, int64_t cells, const int32_t *loff, const float *tri, double *rec_leaf) {
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m >= cells) return;
    const int rk = pyr_leaf[m];
    if (rk < 0) return;
    const int o = loff[rk], e = loff[rk + 1];
    double A = 0.0, S[3] = {0.0, 0.0, 0.0}, C[3] = {0.0, 0.0, 0.0};
    WfFace f;
    for (int t = o; t < e; ++t) {
        wf_face(tri + (size_t)t * 9, f);
        A = A + f.area;
#pragma unroll
        for (int a = 0; a < 3; ++a) { S[a] = S[a] + f.area * f.cen[a]; C[a] = C[a] + f.cen[a]; }
    }
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = A > 0.0 ? S[a] / A : C[a] / (double)(e - o);
    double n0[3] = {0.0, 0.0, 0.0}, m1[9], m2[18], r2 = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) m1[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 18; ++k) m2[k] = 0.0;
    for (int t = o; t < e; ++t) {
        wf_face(tri + (size_t)t * 9, f);
        double d[3], mid[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            d[a] = f.cen[a] - p[a];
            mid[0][a] = 0.5 * (f.p[0][a] + f.p[1][a]) - p[a];
            mid[1][a] = 0.5 * (f.p[1][a] + f.p[2][a]) - p[a];
            mid[2][a] = 0.5 * (f.p[2][a] + f.p[0][a]) - p[a];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) n0[a] = n0[a] + f.nv[a];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) m1[3 * j + i] = m1[3 * j + i] + d[j] * f.nv[i];
#pragma unroll
        for (int n = 0; n < 6; ++n) {
            const int j = WF_PAIR_J(n), k = WF_PAIR_K(n);
            const double cjk = ((mid[0][j] * mid[0][k] + mid[1][j] * mid[1][k]) + mid[2][j] * mid[2][k]) / 3.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) m2[3 * n + i] = m2[3 * n + i] + cjk * f.nv[i];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double dx = f.p[k][0] - p[0], dy = f.p[k][1] - p[1], dz = f.p[k][2] - p[2];
            const double v = (dx * dx + dy * dy) + dz * dz;
            r2 = v > r2 ? v : r2;
        }
    }
    double *rec = rec_leaf + (size_t)rk * WF_REC;
    rec[0] = p[0]; rec[1] = p[1]; rec[2] = p[2]; rec[3] = sqrt(r2);
#pragma unroll
    for (int a = 0; a < 3; ++a) rec[4 + a] = n0[a];
#pragma unroll
    for (int k = 0; k < 9; ++k) rec[7 + k] = m1[k];
#pragma unroll
    for (int k = 0; k < 18; ++k) rec[16 + k] = m2[k];
    rec[34] = A;
    rec[35] = (double)(e - o);
}

__global__ void __launch_bounds__(MT_THREADS)
wf_inner_kernel(const int32_t *pyr, const int32_t *pyr_child, int64_t cells, const double *rec_child, double *rec_level) {
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m >= cells) return;
    const int rk = pyr[m];
    if (rk < 0) return;
    double A = 0.0, cnt = 0.0, S[3] = {0.0, 0.0, 0.0}, C[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 8; ++k) {
        const int ck = pyr_child[8 * m + k];
        if (ck < 0) continue;
        const double *c = rec_child + (size_t)ck * WF_REC;
        A = A + c[34];
        cnt = cnt + c[35];
#pragma unroll
        for (int a = 0; a < 3; ++a) { S[a] = S[a] + c[34] * c[a]; C[a] = C[a] + c[35] * c[a]; }
    }
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = A > 0.0 ? S[a] / A : C[a] / cnt;
    double n0[3] = {0.0, 0.0, 0.0}, m1[9], m2[18], r = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) m1[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 18; ++k) m2[k] = 0.0;
    for (int k = 0; k < 8; ++k) {
        const int ck = pyr_child[8 * m + k];
        if (ck < 0) continue;
        const double *c = rec_child + (size_t)ck * WF_REC;
        double d[3], cn[3], c1[9];
#pragma unroll
        for (int a = 0; a < 3; ++a) { d[a] = c[a] - p[a]; cn[a] = c[4 + a]; }
#pragma unroll
        for (int a = 0; a < 9; ++a) c1[a] = c[7 + a];
#pragma unroll
        for (int a = 0; a < 3; ++a) n0[a] = n0[a] + cn[a];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) m1[3 * j + i] = m1[3 * j + i] + (c1[3 * j + i] + d[j] * cn[i]);
#pragma unroll
        for (int n = 0; n < 6; ++n) {
            const int j = WF_PAIR_J(n), kk = WF_PAIR_K(n);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                m2[3 * n + i] = m2[3 * n + i] + (((c[16 + 3 * n + i] + d[j] * c1[3 * kk + i]) + d[kk] * c1[3 * j + i]) + (d[j] * d[kk]) * cn[i]);
        }
        const double reach = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + c[3];
        r = reach > r ? reach : r;
    }
    double *rec = rec_level + (size_t)rk * WF_REC;
    rec[0] = p[0]; rec[1] = p[1]; rec[2] = p[2]; rec[3] = r;
#pragma unroll
    for (int a = 0; a < 3; ++a) rec[4 + a] = n0[a];
#pragma unroll
    for (int k = 0; k < 9; ++k) rec[7 + k] = m1[k];
#pragma unroll
    for (int k = 0; k < 18; ++k) rec[16 + k] = m2[k];
    rec[34] = A;
    rec[35] = cnt;
}

// ---- query -------------------------------------------------------------------------------------------------------------------------
// the expansion of record c about rho = p - q, in units of solid angle; r2 = |rho|^2
__device__ inline double wf_expansion(const double *c, double rx, double ry, double rz, double r2, int order) {
    const double r1 = sqrt(r2);
    const double r3 = r2 * r1;
    double out = ((rx * c[4] + ry * c[5]) + rz * c[6]) / r3;
    if (order >= 1) {
        const double r5 = r3 * r2;
        const double *m = c + 7;
        const double tr = (m[0] + m[4]) + m[8];
        double q1 = 0.0;
        q1 = q1 + rx * ((rx * m[0] + ry * m[1]) + rz * m[2]);
        q1 = q1 + ry * ((rx * m[3] + ry * m[4]) + rz * m[5]);
        q1 = q1 + rz * ((rx * m[6] + ry * m[7]) + rz * m[8]);
        out = out + (tr / r3 - 3.0 * q1 / r5);
        if (order >= 2) {
            const double r7 = r5 * r2;
            const double *s = c + 16;                             // s[3 * pair + i]: pairs 00 01 02 11 12 22
            // sA: sum_k rho_k sum_j M2[j][k][j]
            double sA = 0.0;
            sA = sA + rx * ((s[0] + s[4]) + s[8]);                // M2[0][0][0] + M2[1][0][1] + M2[2][0][2]
            sA = sA + ry * ((s[3] + s[10]) + s[14]);              // M2[0][1][0] + M2[1][1][1] + M2[2][1][2]
            sA = sA + rz * ((s[6] + s[13]) + s[17]);              // M2[0][2][0] + M2[1][2][1] + M2[2][2][2]
            double sB = 0.0, sC = 0.0;
            const double rho[3] = {rx, ry, rz};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                sB = sB + rho[i] * ((s[i] + s[9 + i]) + s[15 + i]);
                const double diag = ((rx * rx) * s[i] + (ry * ry) * s[9 + i]) + (rz * rz) * s[15 + i];
                const double off = ((rx * ry) * s[3 + i] + (rx * rz) * s[6 + i]) + (ry * rz) * s[12 + i];
                sC = sC + rho[i] * (diag + 2.0 * off);
            }
            out = out + 0.5 * (15.0 * sC / r7 - 3.0 * (2.0 * sA + sB) / r5);
        }
    }
    return out;
}

// SKIP (VTACO_WINDING_WALK=skip, for A/B runs): a descent reads the eight child words at once and keeps the occupied ones as a byte per
// level in one 64-bit register, so empty children are never visited; the default visits every sibling in turn.  Both visit the occupied
// cells in one order: equal results.  Measured: SKIP is 8 % slower on the 976 125-face mesh's lattices, which is what this file
// is for, and 5 to 16 % faster on small meshes, where the exact kernel wins anyway.
template <bool SKIP>
__global__ void __launch_bounds__(MT_THREADS)
wf_query_kernel(const char *tree, OtAt tree_at, int L, const float *pts, int64_t N, double beta2, int order, void *out, int out_f64, int32_t *stats) {
    const int64_t n = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (n >= N) return;
    const OtView<float> tv = ot_view<float>(tree, tree_at, 0);
    const int32_t *pyr = tv.pyr, *rec_base = reinterpret_cast<const int32_t *>(tree + 64);
    const double px = pts[3 * n], py = pts[3 * n + 1], pz = pts[3 * n + 2];
    double far = 0.0, near = 0.0;
    int accepted = 0, exact = 0;
    // an occupied cell: its expansion, or a descent, or at a leaf its faces
    auto visit = [&](int level, int rk) {
        const double *c = tv.recs + ((size_t)rec_base[level] + rk) * WF_REC;
        const double rx = c[0] - px, ry = c[1] - py, rz = c[2] - pz, r = c[3];
        const double d2 = (rx * rx + ry * ry) + rz * rz;
        if (d2 > beta2 * (r * r)) {
            far = far + wf_expansion(c, rx, ry, rz, d2, order);
            ++accepted;
            return false;
        }
        if (level < L) return true;
        const int o = tv.loff[rk], e = tv.loff[rk + 1];
        exact += e - o;
        for (int t = o; t < e; ++t) {
            const float *v = tv.payload + (size_t)t * 9;
            const double ax = v[0] - px, ay = v[1] - py, az = v[2] - pz;
            const double bx = v[3] - px, by = v[4] - py, bz = v[5] - pz;
            const double cx = v[6] - px, cy = v[7] - py, cz = v[8] - pz;
            const double la = sqrt(ax * ax + ay * ay + az * az), lb = sqrt(bx * bx + by * by + bz * bz), lc = sqrt(cx * cx + cy * cy + cz * cz);
            const double num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
            const double den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la +
                               (cx * ax + cy * ay + cz * az) * lb;
            near = near + 2.0 * atan2(num, den);
        }
        return false;
    };
    if (SKIP) {
        int level = 0;
        unsigned cell = 0, level_at = 0;                          // level_at = (8^level - 1) / 7
        u64 todo = 0;                                             // byte l = the occupied children not yet visited at level l
        for (;;) {
            const int rk = pyr[level_at + cell];
            if (rk >= 0 && visit(level, rk)) {
                level_at = level_at * 8 + 1; ++level; cell *= 8;
                const int32_t *ch = pyr + level_at + cell;
                unsigned occ = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) occ |= ch[k] >= 0 ? 1u << k : 0u;
                todo |= (u64)occ << (8 * level);                  // (not empty: the parent is occupied)
            }
            while (level > 0 && ((todo >> (8 * level)) & 0xffu) == 0) { cell >>= 3; --level; level_at = (level_at - 1) >> 3; }
            if (level == 0) break;
            const unsigned rest = (unsigned)(todo >> (8 * level)) & 0xffu;
            const unsigned k = (unsigned)__ffs((int)rest) - 1u;
            todo &= ~((u64)1 << (8 * level + k));
            cell = (cell & ~7u) | k;
        }
    } else {
        ot_walk(pyr, visit, [](int, unsigned) { return 0u; });
    }
    const double w = (far + near) / (4.0 * 3.14159265358979323846);
    if (out_f64) static_cast<double *>(out)[n] = w;
    else static_cast<float *>(out)[n] = (float)w;
    if (stats) { stats[2 * n] = accepted; stats[2 * n + 1] = exact; }
}

int wf_mesh_args(const char *who, const void *verts, int64_t V, const void *faces, int64_t F, int depth) {
    if (V < 0 || F < 0 || (F > 0 && (!verts || !faces || V <= 0))) return vt_fail(VT_ERR_INVALID, who);
    if (depth < 1 || depth > VT_WN_MAX_DEPTH || F > MT_MAX_F || V > MT_MAX_V) return vt_fail(VT_ERR_UNSUPPORTED, who);
    return 0;
}

}  // namespace

extern "C" {

int vt_winding_tree_default_depth(int64_t F) { return ot_default_depth(F); }

size_t vt_winding_tree_workspace_bytes(int64_t V, int64_t F, int depth) {
    if (V < 0 || F < 0 || F > MT_MAX_F || V > MT_MAX_V || depth < 1 || depth > VT_WN_MAX_DEPTH) return 0;
    return ot_work(F, 1, depth).bytes;
}

int vt_winding_tree_count(const float *verts, int64_t V, const int32_t *faces, int64_t F, int depth, void *workspace, size_t workspace_bytes,
                          void *stream) {
    const char *who = "vt_winding_tree_count: bad argument";
    if (int rc = wf_mesh_args(who, verts, V, faces, F, depth)) return rc;
    if (!workspace) return vt_fail(VT_ERR_INVALID, who);
    const OtWork w = ot_work(F, 1, depth);
    if (workspace_bytes < w.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_winding_tree_count: workspace too small");
    ot_count_enqueue(WfSource{verts, faces, (int)V, (int)F}, 1, depth, w, static_cast<char *>(workspace), (hipStream_t)stream);
    return vt_check(hipGetLastError(), "vt_winding_tree_count");
}

int vt_winding_tree_layout(int64_t F, int depth, const int32_t *state_host, size_t *offsets) {
    if (!state_host || !offsets || F < 0) return vt_fail(VT_ERR_INVALID, "vt_winding_tree_layout: bad argument");
    if (depth < 1 || depth > VT_WN_MAX_DEPTH || F > MT_MAX_F) return vt_fail(VT_ERR_UNSUPPORTED, "vt_winding_tree_layout: depth outside [1, 7]");
    OtTree t;
    if (!wf_tree(F, depth, state_host, t)) return vt_fail(VT_ERR_INVALID, "vt_winding_tree_layout: counts that no tree of this size has");
    offsets[0] = t.pyr; offsets[1] = t.rec; offsets[2] = t.loff; offsets[3] = t.list; offsets[4] = t.payload; offsets[5] = t.bytes;
    return 0;
}

int vt_winding_tree_build(const float *verts, int64_t V, const int32_t *faces, int64_t F, int depth, const int32_t *state_host, void *workspace,
                          size_t workspace_bytes, void *tree, size_t tree_bytes, void *stream) {
    const char *who = "vt_winding_tree_build: bad argument";
    if (int rc = wf_mesh_args(who, verts, V, faces, F, depth)) return rc;
    if (!state_host || !workspace || !tree) return vt_fail(VT_ERR_INVALID, who);
    if (state_host[0] != 0) return vt_fail(VT_ERR_INVALID, "vt_winding_tree_build: a vertex coordinate is not finite");
    OtTree t;
    if (!wf_tree(F, depth, state_host, t)) return vt_fail(VT_ERR_INVALID, "vt_winding_tree_build: counts that no tree of this size has");
    const OtWork w = ot_work(F, 1, depth);
    if (workspace_bytes < w.bytes || tree_bytes < t.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_winding_tree_build: workspace or tree too small");
    if (F == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    char *tr = static_cast<char *>(tree);
    ot_build_enqueue(WfSource{verts, faces, (int)V, (int)F}, 1, depth, w, static_cast<char *>(workspace), t, tr, st);
    const int32_t *pyr = reinterpret_cast<const int32_t *>(tr + t.pyr), *loff = reinterpret_cast<const int32_t *>(tr + t.loff);
    const float *tri = reinterpret_cast<const float *>(tr + t.payload);
    double *recs = reinterpret_cast<double *>(tr + t.rec);
    const int64_t leaf = cells_of(depth);
    hipLaunchKernelGGL(wf_leaf_kernel, dim3(blocks_of(leaf, MT_THREADS)), dim3(MT_THREADS), 0, st, pyr + pyr_off(depth), leaf, loff, tri,
                       recs + (size_t)t.base.v[depth] * WF_REC);
    for (int l = depth - 1; l >= 0; --l)
        hipLaunchKernelGGL(wf_inner_kernel, dim3(blocks_of(cells_of(l), MT_THREADS)), dim3(MT_THREADS), 0, st, pyr + pyr_off(l), pyr + pyr_off(l + 1),
                           cells_of(l), (const double *)(recs + (size_t)t.base.v[l + 1] * WF_REC), recs + (size_t)t.base.v[l] * WF_REC);
    return vt_check(hipGetLastError(), "vt_winding_tree_build");
}

int vt_winding_tree_query(const void *tree, size_t tree_bytes, int64_t F, int depth, const int32_t *state_host, const float *pts, int64_t N,
                          double accuracy, int order, void *out, int out_f64, int32_t *stats, void *stream) {
    const char *who = "vt_winding_tree_query: bad argument";
    if (F < 0 || N < 0 || order < 0 || order > 2 || !(accuracy >= 0.0) || (N > 0 && (!pts || !out))) return vt_fail(VT_ERR_INVALID, who);
    if (depth < 1 || depth > VT_WN_MAX_DEPTH || F > MT_MAX_F || N > (int64_t)0x7fffffff * MT_THREADS)
        return vt_fail(VT_ERR_UNSUPPORTED, "vt_winding_tree_query: depth outside [1, 7]");
    if (N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (F == 0) {
        if (int rc = vt_fill32(out, 0u, (size_t)N * (out_f64 ? 8 : 4), st)) return rc;
        return stats ? vt_fill32(stats, 0u, (size_t)N * 8, st) : 0;
    }
    if (!tree || !state_host) return vt_fail(VT_ERR_INVALID, who);
    OtTree t;
    if (!wf_tree(F, depth, state_host, t)) return vt_fail(VT_ERR_INVALID, "vt_winding_tree_query: counts that no tree of this size has");
    if (tree_bytes < t.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_winding_tree_query: tree too small");
    const char *walk = getenv("VTACO_WINDING_WALK");
    auto kernel = walk && !strcmp(walk, "skip") ? wf_query_kernel<true> : wf_query_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks_of(N, MT_THREADS)), dim3(MT_THREADS), 0, st, static_cast<const char *>(tree),
                       OtAt{t.stride, t.pyr, t.rec, t.loff, t.list, t.payload}, depth, pts, N, accuracy * accuracy, order, out, out_f64, stats);
    return vt_check(hipGetLastError(), "vt_winding_tree_query");
}

}  // extern "C"
