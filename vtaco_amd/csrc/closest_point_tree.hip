// Closest point on a triangle mesh through the face octree of winding_fast.hip: the d2, face and closest of vt_closest_point_mesh, bit for
// bit, without testing every face.  The definitions are DESIGN.md's section "closest_point_tree.hip", restated in numpy by
// tests/closest_point_tree_ref.py: this file's operations in this file's order.
//   inputs    a built winding tree (pyramids, list offsets, lists, the per-level counts the caller read back) and the mesh it was built on
//   boxes     one axis-aligned box per occupied cell of every level, lo[3], hi[3] in float64: a leaf's is the min / max over the exactly
//             converted corners of the faces in its list, an inner cell's the min / max over its occupied children (octree_common.h's
//             ot_inner_box_kernel).  A face with an index
//             outside [0, V) is in no box (status bit 1, as closest_point.hip reports it); a cell of such faces only has lo = +inf, hi = -inf
//   records   closest_point_face.h's 14 doubles per face, in list order: a leaf's faces are contiguous; slot t holds face lists[t]
//   query     one lane per query, float64, octree_common.h's walk.  Per occupied cell lb = ot_box_d2(box, p), e_a = max(lo_a - p_a, 0,
//             p_a - hi_a), lb = (e_x^2 + e_y^2) + e_z^2; the cell and everything under it is skipped when lb - delta > best.  A leaf that is
//             not skipped runs cp_face over its list in list order and takes a face on d2 < best || (d2 == best && face < best_face)
//   delta     2^-40 S^2, S = ot_frame_reach + 4 side = ((m_x + m_y) + m_z) + 4 side, m_a = max(|p_a - lo_a|, |p_a - (lo_a + side)|): S bounds
//             |p - a| + |ab| + |ac| of every face, and the computed d2 undercuts the true squared distance to a cell's box by less than
//             40 u S^2, u = 2^-53 (DESIGN.md derives the count); 2^-40 = 8192 u.  A NaN coordinate makes delta NaN: nothing is skipped
//   seed      before the walk, the leaf reached by descending towards the query's own cell (octree_common.h's binning, clamped into the
//             frame; where the wanted child is empty, the occupied child whose number is nearest, the lower of two) is evaluated, so the
//             walk starts with a finite best; the walk passes over that leaf
//   order     near children first: ot_near_octant, the octant of the query about the cell's centre
// Seed and order change which cells are skipped, never a result: the tie rule does not depend on the order faces are met in.
// VTACO_CLOSEST_TREE_WALK = plain | seed | order | seed+order picks the walk for A/B runs; the default is seed+order.
// No launch function allocates, copies to the host or waits.  All products and sums are separate roundings (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "closest_point_face.h"
#include "mesh_common.h"
#include "octree_common.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

constexpr double CT_SLACK = 0x1p-40;

// ---- build ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT_THREADS)
ct_record_kernel(const float *verts, int V, const int32_t *faces, const int32_t *list, int F, double *rec, int32_t *status) {
    const int64_t t = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (t >= F) return;
    const int f = list[t];
    double *r = rec + (size_t)t * CP_REC;
    if (f < 0 || f >= F) {                                       // (no list of a built tree holds one)
#pragma unroll
        for (int k = 0; k < CP_REC; ++k) r[k] = k == CP_KIND ? CP_SKIP : 0.0;
        return;
    }
    if (!cp_fill_record(verts, V, faces, (size_t)f, r)) atomicOr(status, CP_BAD_INDEX);
}

__global__ void __launch_bounds__(MT_THREADS)
ct_leaf_box_kernel(const int32_t *pyr_leaf, int64_t cells, const int32_t *loff, const int32_t *list, const float *verts, int V, const int32_t *faces,
                   int F, double *box_leaf) {
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m >= cells) return;
    const int rk = pyr_leaf[m];
    if (rk < 0) return;
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    const int o = loff[rk], e = loff[rk + 1];
    for (int t = o; t < e; ++t) {
        const int f = list[t];
        if (f < 0 || f >= F) continue;
        int idx[3];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            idx[k] = faces[3 * (size_t)f + k];
            ok = ok && idx[k] >= 0 && idx[k] < V;
        }
        if (!ok) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double x = (double)verts[3 * (size_t)idx[k] + a];
                lo[a] = x < lo[a] ? x : lo[a];
                hi[a] = x > hi[a] ? x : hi[a];
            }
    }
    double *b = box_leaf + (size_t)rk * OT_BOX;
#pragma unroll
    for (int a = 0; a < 3; ++a) { b[a] = lo[a]; b[3 + a] = hi[a]; }
}

// ---- query ---------------------------------------------------------------------------------------------------------------------------
struct CtBest { double d2; int face, slot; };

// cp_face over the list of leaf rk, in list order; the tie rule is explicit: the walk does not meet faces in ascending order
__device__ inline int ct_leaf(const OtView<float> &tv, const double *recs, int rk, const double *p, CtBest &best) {
    const int o = tv.loff[rk], e = tv.loff[rk + 1];
    for (int t = o; t < e; ++t) {
        const double2 *src = reinterpret_cast<const double2 *>(recs + (size_t)t * CP_REC);
        double r[CP_REC];
#pragma unroll
        for (int k = 0; k < CP_REC / 2; ++k) { const double2 v = src[k]; r[2 * k] = v.x; r[2 * k + 1] = v.y; }
        if (r[CP_KIND] == CP_SKIP) continue;
        double q[3];
        const double d = cp_face(r, p[0], p[1], p[2], q);
        const int f = tv.list[t];
        if (d < best.d2 || (d == best.d2 && f < best.face)) { best.d2 = d; best.face = f; best.slot = t; }
    }
    return e - o;
}

template <bool SEED, bool ORDER>
__global__ void __launch_bounds__(MT_THREADS)
ct_query_kernel(const char *tree, OtAt tree_at, const char *side, OtSide sd, int L, const float *pts, int64_t N, double *d2, int32_t *face,
                double *closest, int32_t *stats) {
    const int64_t n = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (n >= N) return;
    const OtView<float> tv = ot_view<float>(tree, tree_at, 0);
    const OtSideView sv = ot_side_view(side, sd);
    const double p[3] = {(double)pts[3 * n], (double)pts[3 * n + 1], (double)pts[3 * n + 2]};
    const double flo[3] = {tv.frame[0], tv.frame[1], tv.frame[2]}, fside = tv.frame[3];
    const double S = ot_frame_reach(tv.frame, p) + 4.0 * fside;
    const double delta = (S * S) * CT_SLACK;
    CtBest best = {__builtin_inf(), -1, -1};
    int n_boxes = 0, n_faces = 0, seed_rk = -1;
    if (SEED) {
        const unsigned code = ot_code(p[0], p[1], p[2], tv.frame, L);       // (a NaN becomes 0)
        unsigned c = 0, at = 0;
        bool found = true;
        for (int l = 0; l < L; ++l) {
            const int want = (int)((code >> (3 * (L - 1 - l))) & 7u);
            at = at * 8 + 1; c *= 8;
            const int32_t *ch = tv.pyr + at + c;
            int pick = -1, gap = 16;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int g = k > want ? k - want : want - k;
                if (ch[k] >= 0 && g < gap) { gap = g; pick = k; }
            }
            if (pick < 0) { found = false; break; }                // (an occupied cell has an occupied child)
            c += (unsigned)pick;
        }
        if (found) seed_rk = tv.pyr[at + c];
        if (seed_rk >= 0) n_faces += ct_leaf(tv, sv.recs, seed_rk, p, best);
    }
    ot_walk(
        tv.pyr,
        [&](int level, int rk) {
            const double lb = ot_box_d2(sv.boxes + ((size_t)sd.base.v[level] + rk) * OT_BOX, p);
            ++n_boxes;
            if (lb - delta > best.d2) return false;
            if (level < L) return true;
            if (rk != seed_rk) n_faces += ct_leaf(tv, sv.recs, rk, p, best);
            return false;
        },
        [&](int level, unsigned actual) { return ot_near_octant<ORDER>(flo, fside, level, actual, p); });
    d2[n] = best.d2;
    face[n] = best.face;
    if (closest) {
        double q[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
        if (best.slot >= 0) cp_face(sv.recs + (size_t)best.slot * CP_REC, p[0], p[1], p[2], q);
        closest[3 * n] = q[0]; closest[3 * n + 1] = q[1]; closest[3 * n + 2] = q[2];
    }
    if (stats) { stats[2 * n] = n_boxes; stats[2 * n + 1] = n_faces; }
}

int ct_args(const char *who, int64_t F, int depth, const int32_t *state_host, size_t *tree_off, OtSide &s) {
    if (F <= 0 || !state_host) return vt_fail(VT_ERR_INVALID, who);
    if (int rc = vt_winding_tree_layout(F, depth, state_host, tree_off)) return rc;
    ot_side(F, depth, state_host, CP_REC, s);
    return 0;
}

}  // namespace

extern "C" {

int vt_closest_tree_layout(int64_t F, int depth, const int32_t *state_host, size_t *offsets) {
    size_t tree_off[6];
    OtSide s;
    if (!offsets) return vt_fail(VT_ERR_INVALID, "vt_closest_tree_layout: bad argument");
    if (int rc = ct_args("vt_closest_tree_layout: bad argument (a mesh needs F > 0)", F, depth, state_host, tree_off, s)) return rc;
    offsets[0] = s.box; offsets[1] = s.rec; offsets[2] = s.bytes;
    return 0;
}

int vt_closest_tree_build(const float *verts, int64_t V, const int32_t *faces, int64_t F, int depth, const int32_t *state_host, const void *tree,
                          size_t tree_bytes, void *side, size_t side_bytes, void *stream) {
    const char *who = "vt_closest_tree_build: bad argument (a mesh needs V > 0 and F > 0)";
    if (!verts || !faces || V <= 0 || V > MT_MAX_V || !tree || !side) return vt_fail(VT_ERR_INVALID, who);
    size_t off[6];
    OtSide s;
    if (int rc = ct_args(who, F, depth, state_host, off, s)) return rc;
    if (tree_bytes < off[5] || side_bytes < s.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_closest_tree_build: tree or side buffer too small");
    hipStream_t st = (hipStream_t)stream;
    const char *tr = static_cast<const char *>(tree);
    char *sd = static_cast<char *>(side);
    const int32_t *pyr = reinterpret_cast<const int32_t *>(tr + off[0]);
    const int32_t *loff = reinterpret_cast<const int32_t *>(tr + off[2]), *list = reinterpret_cast<const int32_t *>(tr + off[3]);
    double *boxes = reinterpret_cast<double *>(sd + s.box), *recs = reinterpret_cast<double *>(sd + s.rec);
    if (int rc = vt_fill32(sd, 0u, OT_SIDE_HEAD, st)) return rc;
    hipLaunchKernelGGL(ct_record_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, (int)V, faces, list, (int)F, recs,
                       reinterpret_cast<int32_t *>(sd));
    const int64_t leaf = cells_of(depth);
    hipLaunchKernelGGL(ct_leaf_box_kernel, dim3(blocks_of(leaf, MT_THREADS)), dim3(MT_THREADS), 0, st, pyr + pyr_off(depth), leaf, loff, list, verts,
                       (int)V, faces, (int)F, boxes + (size_t)s.base.v[depth] * OT_BOX);
    for (int l = depth - 1; l >= 0; --l)
        hipLaunchKernelGGL(ot_inner_box_kernel, dim3(blocks_of(cells_of(l), MT_THREADS)), dim3(MT_THREADS), 0, st, tr, (size_t)0,
                           off[0] + (size_t)pyr_off(l) * 4, off[0] + (size_t)pyr_off(l + 1) * 4, cells_of(l), sd, (size_t)0,
                           s.box + (size_t)s.base.v[l + 1] * OT_BOX * sizeof(double), s.box + (size_t)s.base.v[l] * OT_BOX * sizeof(double));
    return vt_check(hipGetLastError(), "vt_closest_tree_build");
}

int vt_closest_tree_query(const void *tree, size_t tree_bytes, const void *side, size_t side_bytes, int64_t F, int depth, const int32_t *state_host,
                          const float *pts, int64_t N, double *d2, int32_t *face, double *closest, int32_t *stats, void *stream) {
    const char *who = "vt_closest_tree_query: bad argument (a mesh needs F > 0)";
    if (!tree || !side || N < 0 || (N > 0 && (!pts || !d2 || !face))) return vt_fail(VT_ERR_INVALID, who);
    if (N > (int64_t)0x7fffffff * MT_THREADS) return vt_fail(VT_ERR_UNSUPPORTED, "vt_closest_tree_query: too many queries");
    size_t off[6];
    OtSide s;
    if (int rc = ct_args(who, F, depth, state_host, off, s)) return rc;
    if (tree_bytes < off[5] || side_bytes < s.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_closest_tree_query: tree or side buffer too small");
    if (N == 0) return 0;
    const char *walk = getenv("VTACO_CLOSEST_TREE_WALK");
    auto kernel = ct_query_kernel<true, true>;
    if (walk && walk[0]) {
        if (!strcmp(walk, "plain")) kernel = ct_query_kernel<false, false>;
        else if (!strcmp(walk, "seed")) kernel = ct_query_kernel<true, false>;
        else if (!strcmp(walk, "order")) kernel = ct_query_kernel<false, true>;
        else if (strcmp(walk, "seed+order")) return vt_fail(VT_ERR_INVALID, "vt_closest_tree_query: VTACO_CLOSEST_TREE_WALK must be plain, seed, order or seed+order");
    }
    hipLaunchKernelGGL(kernel, dim3(blocks_of(N, MT_THREADS)), dim3(MT_THREADS), 0, (hipStream_t)stream, static_cast<const char *>(tree),
                       OtAt{0, off[0], off[1], off[2], off[3], off[4]}, static_cast<const char *>(side), s, depth, pts, N, d2, face, closest, stats);
    return vt_check(hipGetLastError(), "vt_closest_tree_query");
}

}  // extern "C"
