// Closest point on a triangle mesh through the face octree of winding_fast.hip: the d2, face and closest of vt_closest_point_mesh, bit for
// bit, without testing every face.  The definitions are DESIGN.md's section "closest_point_tree.hip", restated in numpy by
// tests/closest_point_tree_ref.py: this file's operations in this file's order.
//   inputs    a built winding tree (pyramids, list offsets, lists, the per-level counts the caller read back) and the mesh it was built on
//   boxes     one axis-aligned box per occupied cell of every level, lo[3], hi[3] in float64: a leaf's is the min / max over the exactly
//             converted corners of the faces in its list, an inner cell's the min / max over its occupied children (octree_common.h's
//             ot_inner_box_kernel).  A face with an index
//             outside [0, V) is in no box (status bit 1, as closest_point.hip reports it); a cell of such faces only has lo = +inf, hi = -inf
//   records   closest_point_face.h's 14 doubles per face, in list order: a leaf's faces are contiguous; slot t holds face lists[t]
//   query     one lane per query, float64, winding_fast.hip's walk without a stack: the state is (level, cell), "next" is cell + 1 climbing
//             while cell % 8 == 0, "descend" is (level + 1, 8 cell).  Per occupied cell e_a = max(lo_a - p_a, 0, p_a - hi_a),
//             lb = (e_x^2 + e_y^2) + e_z^2; the cell and everything under it is skipped when lb - delta > best.  A leaf that is not skipped
//             runs cp_face over its list in list order and takes a face on d2 < best || (d2 == best && face < best_face)
//   delta     2^-40 S^2, S = ((m_x + m_y) + m_z) + 4 side, m_a = max(|p_a - lo_a|, |p_a - (lo_a + side)|) over the tree's frame: S bounds
//             |p - a| + |ab| + |ac| of every face, and the computed d2 undercuts the true squared distance to a cell's box by less than
//             40 u S^2, u = 2^-53 (DESIGN.md derives the count); 2^-40 = 8192 u.  A NaN coordinate makes delta NaN: nothing is skipped
//   seed      before the walk, the leaf reached by descending towards the query's own cell (octree_common.h's binning, clamped into the
//             frame; where the wanted child is empty, the occupied child whose number is nearest, the lower of two) is evaluated, so the
//             walk starts with a finite best; the walk passes over that leaf
//   order     the children of a cell are visited as k ^ o, o the octant of the query about the cell's centre
//             lo_a + (i_a + 0.5) (side / 2^level): near children first.  "Next" and "climb" act on k; o is kept per level beside it
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

constexpr int CT_BOX = OT_BOX;                  // doubles per box (48 bytes: 16-byte aligned rows): lo[3], hi[3]
constexpr size_t CT_HEAD = 256;                 // bytes in front of the boxes; the status word is the first
constexpr double CT_SLACK = 0x1p-40;

struct CtSide { size_t box, rec, bytes; OtBase base; };

// the side buffer of a tree with these counts (state_host: vt_winding_tree_count's words, validated by vt_winding_tree_layout first)
void ct_side(int64_t F, int L, const int32_t *state, CtSide &s) {
    int64_t total = 0;
    for (int l = 0; l < OT_LEVELS; ++l) {
        s.base.v[l] = (int)total;
        if (l <= L) total += state[1 + l];
    }
    s.base.v[OT_LEVELS] = (int)total;
    s.box = CT_HEAD;
    s.rec = s.box + up256((size_t)total * CT_BOX * sizeof(double));
    s.bytes = s.rec + up256((size_t)F * CP_REC * sizeof(double));
}

// ---- build ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT_THREADS)
ct_record_kernel(const float *verts, int V, const int32_t *faces, const int32_t *list, int F, double *rec, int32_t *status) {
    const int64_t t = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (t >= F) return;
    const int f = list[t];
    double *r = rec + (size_t)t * CP_REC;
    if (f < 0 || f >= F) {                                       // (no list of a built tree holds one)
#pragma unroll
        for (int k = 0; k < CP_REC; ++k) r[k] = k == 12 ? 2.0 : 0.0;
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
    double *b = box_leaf + (size_t)rk * CT_BOX;
#pragma unroll
    for (int a = 0; a < 3; ++a) { b[a] = lo[a]; b[3 + a] = hi[a]; }
}

// ---- query ---------------------------------------------------------------------------------------------------------------------------
struct CtBest { double d2; int face, slot; };

// cp_face over the list of leaf rk, in list order; the tie rule is explicit: the walk does not meet faces in ascending order
__device__ inline int ct_leaf(const int32_t *loff, const int32_t *list, const double *recs, int rk, double px, double py, double pz, CtBest &best) {
    const int o = loff[rk], e = loff[rk + 1];
    for (int t = o; t < e; ++t) {
        const double2 *src = reinterpret_cast<const double2 *>(recs + (size_t)t * CP_REC);
        double r[CP_REC];
#pragma unroll
        for (int k = 0; k < CP_REC / 2; ++k) { const double2 v = src[k]; r[2 * k] = v.x; r[2 * k + 1] = v.y; }
        if (r[12] == 2.0) continue;
        double q[3];
        const double d = cp_face(r, px, py, pz, q);
        const int f = list[t];
        if (d < best.d2 || (d == best.d2 && f < best.face)) { best.d2 = d; best.face = f; best.slot = t; }
    }
    return e - o;
}

template <bool SEED, bool ORDER>
__global__ void __launch_bounds__(MT_THREADS)
ct_query_kernel(const char *tree, size_t pyr_at, size_t loff_at, size_t list_at, const char *side, size_t box_at, size_t rec_at, OtBase base, int L,
                const float *pts, int64_t N, double *d2, int32_t *face, double *closest, int32_t *stats) {
    const int64_t n = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (n >= N) return;
    const double *frame = reinterpret_cast<const double *>(tree);
    const int32_t *pyr = reinterpret_cast<const int32_t *>(tree + pyr_at);
    const int32_t *loff = reinterpret_cast<const int32_t *>(tree + loff_at);
    const int32_t *list = reinterpret_cast<const int32_t *>(tree + list_at);
    const double *boxes = reinterpret_cast<const double *>(side + box_at);
    const double *recs = reinterpret_cast<const double *>(side + rec_at);
    const double p[3] = {(double)pts[3 * n], (double)pts[3 * n + 1], (double)pts[3 * n + 2]};
    const double flo[3] = {frame[0], frame[1], frame[2]}, fside = frame[3];
    double S = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double u = fabs(p[a] - flo[a]), v = fabs(p[a] - (flo[a] + fside));
        const double m = u > v ? u : v;
        S = a == 0 ? m : S + m;
    }
    S = S + 4.0 * fside;
    const double delta = (S * S) * CT_SLACK;
    CtBest best = {__builtin_inf(), -1, -1};
    int n_boxes = 0, n_faces = 0, seed_rk = -1;
    if (SEED) {
        unsigned code = 0;
        const int cells = 1 << L;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double g = floor((p[a] - flo[a]) / fside * (double)cells);
            g = g > 0.0 ? g : 0.0;                                 // (a NaN becomes 0)
            g = g < (double)(cells - 1) ? g : (double)(cells - 1);
            code |= ot_spread((unsigned)(int)g) << a;
        }
        unsigned c = 0, at = 0;
        bool found = true;
        for (int l = 0; l < L; ++l) {
            const int want = (int)((code >> (3 * (L - 1 - l))) & 7u);
            at = at * 8 + 1; c *= 8;
            const int32_t *ch = pyr + at + c;
            int pick = -1, gap = 16;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int g = k > want ? k - want : want - k;
                if (ch[k] >= 0 && g < gap) { gap = g; pick = k; }
            }
            if (pick < 0) { found = false; break; }                // (an occupied cell has an occupied child)
            c += (unsigned)pick;
        }
        if (found) seed_rk = pyr[at + c];
        if (seed_rk >= 0) n_faces += ct_leaf(loff, list, recs, seed_rk, p[0], p[1], p[2], best);
    }
    int level = 0;
    unsigned cell = 0, flip = 0, level_at = 0;                    // level_at = (8^level - 1) / 7; flip: the octant o of every level, 3 bits each
    for (;;) {
        const unsigned actual = cell ^ flip;
        const int rk = pyr[level_at + actual];
        bool descend = false;
        if (rk >= 0) {
            const double *b = boxes + ((size_t)base.v[level] + rk) * CT_BOX;
            double e[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double x = b[a] - p[a];
                x = x > 0.0 ? x : 0.0;
                const double y = p[a] - b[3 + a];
                e[a] = y > x ? y : x;
            }
            const double lb = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
            ++n_boxes;
            if (!(lb - delta > best.d2)) {
                if (level < L) descend = true;
                else if (rk != seed_rk) n_faces += ct_leaf(loff, list, recs, rk, p[0], p[1], p[2], best);
            }
        }
        if (descend) {
            unsigned o = 0;
            if (ORDER) {
                const double h = fside * (1.0 / (double)(1 << level));
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double centre = flo[a] + ((double)ot_gather(actual >> a) + 0.5) * h;
                    o |= p[a] >= centre ? 1u << a : 0u;
                }
            }
            level_at = level_at * 8 + 1; ++level; cell *= 8; flip = flip * 8 + o;
        } else {
            ++cell;
            while (level > 0 && (cell & 7u) == 0) { cell >>= 3; flip >>= 3; --level; level_at = (level_at - 1) >> 3; }
            if (level == 0) break;
        }
    }
    d2[n] = best.d2;
    face[n] = best.face;
    if (closest) {
        double q[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
        if (best.slot >= 0) cp_face(recs + (size_t)best.slot * CP_REC, p[0], p[1], p[2], q);
        closest[3 * n] = q[0]; closest[3 * n + 1] = q[1]; closest[3 * n + 2] = q[2];
    }
    if (stats) { stats[2 * n] = n_boxes; stats[2 * n + 1] = n_faces; }
}

int ct_args(const char *who, int64_t F, int depth, const int32_t *state_host, size_t *tree_off, CtSide &s) {
    if (F <= 0 || !state_host) return vt_fail(VT_ERR_INVALID, who);
    if (int rc = vt_winding_tree_layout(F, depth, state_host, tree_off)) return rc;
    ct_side(F, depth, state_host, s);
    return 0;
}

}  // namespace

extern "C" {

int vt_closest_tree_layout(int64_t F, int depth, const int32_t *state_host, size_t *offsets) {
    size_t tree_off[6];
    CtSide s;
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
    CtSide s;
    if (int rc = ct_args(who, F, depth, state_host, off, s)) return rc;
    if (tree_bytes < off[5] || side_bytes < s.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_closest_tree_build: tree or side buffer too small");
    hipStream_t st = (hipStream_t)stream;
    const char *tr = static_cast<const char *>(tree);
    char *sd = static_cast<char *>(side);
    const int32_t *pyr = reinterpret_cast<const int32_t *>(tr + off[0]);
    const int32_t *loff = reinterpret_cast<const int32_t *>(tr + off[2]), *list = reinterpret_cast<const int32_t *>(tr + off[3]);
    double *boxes = reinterpret_cast<double *>(sd + s.box), *recs = reinterpret_cast<double *>(sd + s.rec);
    if (int rc = vt_fill32(sd, 0u, CT_HEAD, st)) return rc;
    hipLaunchKernelGGL(ct_record_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, (int)V, faces, list, (int)F, recs,
                       reinterpret_cast<int32_t *>(sd));
    const int64_t leaf = cells_of(depth);
    hipLaunchKernelGGL(ct_leaf_box_kernel, dim3(blocks_of(leaf, MT_THREADS)), dim3(MT_THREADS), 0, st, pyr + pyr_off(depth), leaf, loff, list, verts,
                       (int)V, faces, (int)F, boxes + (size_t)s.base.v[depth] * CT_BOX);
    for (int l = depth - 1; l >= 0; --l)
        hipLaunchKernelGGL(ot_inner_box_kernel, dim3(blocks_of(cells_of(l), MT_THREADS)), dim3(MT_THREADS), 0, st, tr, (size_t)0,
                           off[0] + (size_t)pyr_off(l) * 4, off[0] + (size_t)pyr_off(l + 1) * 4, cells_of(l), sd, (size_t)0,
                           s.box + (size_t)s.base.v[l + 1] * CT_BOX * sizeof(double), s.box + (size_t)s.base.v[l] * CT_BOX * sizeof(double));
    return vt_check(hipGetLastError(), "vt_closest_tree_build");
}

int vt_closest_tree_query(const void *tree, size_t tree_bytes, const void *side, size_t side_bytes, int64_t F, int depth, const int32_t *state_host,
                          const float *pts, int64_t N, double *d2, int32_t *face, double *closest, int32_t *stats, void *stream) {
    const char *who = "vt_closest_tree_query: bad argument (a mesh needs F > 0)";
    if (!tree || !side || N < 0 || (N > 0 && (!pts || !d2 || !face))) return vt_fail(VT_ERR_INVALID, who);
    if (N > (int64_t)0x7fffffff * MT_THREADS) return vt_fail(VT_ERR_UNSUPPORTED, "vt_closest_tree_query: too many queries");
    size_t off[6];
    CtSide s;
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
    hipLaunchKernelGGL(kernel, dim3(blocks_of(N, MT_THREADS)), dim3(MT_THREADS), 0, (hipStream_t)stream, static_cast<const char *>(tree), off[0],
                       off[2], off[3], static_cast<const char *>(side), s.box, s.rec, s.base, depth, pts, N, d2, face, closest, stats);
    return vt_check(hipGetLastError(), "vt_closest_tree_query");
}

}  // extern "C"
