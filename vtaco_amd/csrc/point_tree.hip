// Nearest point of a point set through an octree over the points: the d2 and idx of vt_nn_points (icp.hip), bit for bit, without testing
// every target.  The reference searches a kd-tree there (src/utils/icp.py:50-66, sklearn; src/common.py:142-175, pykdtree).  The
// definitions are DESIGN.md's section "point_tree.hip", restated in numpy by tests/point_tree_ref.py: this file's operations in this
// file's order.  B problems with one M per call; every kernel covers the batch in one launch, the problem index in the grid.
//   tree      octree_common.h's octree with PtSource below: the frame spans the targets (a zero minimum is stored as +0.0), a point lives
//             in the leaf it lies in and is copied in list order: a leaf's points are contiguous, ascending by index
//   boxes     per occupied cell lo[3], hi[3]: a leaf's the min / max of its points, an inner cell's the min / max of its occupied
//             children.  Minimum and maximum do not round; +0.0 is added on the way out, so a zero is stored as +0.0
//   query     one lane per query, float64, octree_common.h's walk.  Per occupied cell lb = ot_box_d2(box, q): e_a = lo_a - q_a when
//             q_a < lo_a, q_a - hi_a when q_a > hi_a, else 0 (computed there as max(lo_a - q_a, 0, q_a - hi_a): the same value for
//             every input, without a branch); lb = (e_x e_x + e_y e_y) + e_z e_z, the operation order of
//             d2 = (dx dx + dy dy) + dz dz, d = q - p.  Rounding is monotone: |fl(q_a - p_a)| >= fl(e_a) >= 0 for every point of the cell,
//             and products and sums of non-negative values keep the order, so the computed lb is <= the computed d2 of every point
//             under the cell: the cell is skipped exactly when lb > best, with no slack term.  A leaf's points are taken in list order
//             on d2 < best || (d2 == best && index < best index): the lowest index among equal minima, as the ascending brute force
//             gives.  A NaN query makes every comparison false: it visits everything and returns (+inf, -1)
//   seed      before the walk the query's own clamped leaf (ot_leaf_of), when occupied, is evaluated; the walk tests its box and passes
//             over it
//   order     near children first: ot_near_octant, the octant of the query about the cell's centre
//   lanes     optionally lane i answers query perm[i], perm the queries in Morton order of the tree's leaves (octree_common.h's count /
//             scan / fill with PtLaneSource, per call): a wave's lanes then walk neighbouring cells.  Outputs stay in query order; no result depends on perm
// Seed and order change which cells are skipped, never a result.  VTACO_POINT_TREE_WALK = plain | seed | order | seed+order picks the
// walk for A/B runs; the default is seed+order.
// No launch function allocates, copies to the host or waits: the one host read of a build (16 int32 per problem, the first 64 B bytes of
// vt_point_tree_count's workspace) is the caller's, between the two calls.  No float atomic, no sort: the trees are equal from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "icp_common.h"
#include "mesh_common.h"
#include "octree_common.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

constexpr int64_t PT_MAX_M = MT_MAX_F;
constexpr int64_t PT_MAX_N = 0x7fffff00;

// octree_common.h's source of B point sets [B][M][3]: the frame spans the points, a point is binned by itself and carried as it is
struct PtSource {
    const double *dst;
    int M;
    static constexpr size_t PAYLOAD = 3 * sizeof(double);
    __host__ __device__ int coords() const { return M; }
    __host__ __device__ int items() const { return M; }
    __device__ double coord(int b, int64_t m, int a) const { return dst[((size_t)b * M + m) * 3 + a]; }
    __device__ double frame_lo(double x) const { return x + 0.0; }       // a zero is stored as +0.0
    __device__ void point(int b, int64_t m, double p[3]) const {
        const double *q = dst + ((size_t)b * M + m) * 3;
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
    __device__ void payload(int b, int64_t m, char *slot) const { point(b, m, reinterpret_cast<double *>(slot)); }
};

// the lane order's source: the queries [B][N][3], moved by T [B][16] when given, binned into the frames of built trees
struct PtLaneSource {
    const double *src, *T;
    int N;
    __host__ __device__ int items() const { return N; }
    __device__ void point(int b, int64_t n, double p[3]) const { load_query(src, T, b, N, n, p); }
};

// the layout of B trees of boxes; a point tree has an occupied cell at every level of every problem
bool pt_tree(int64_t M, int L, int B, const int32_t *state, OtTree &t) {
    for (int b = 0; b < B; ++b)
        for (int l = 0; l <= L; ++l)
            if (state[(size_t)b * OT_STATE + OT_W_COUNT + l] < 1) return false;
    return ot_tree(M, L, B, state, OT_BOX, PtSource::PAYLOAD, t);
}

// ---- boxes -----------------------------------------------------------------------------------------------------------------------------
// grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS)
pt_leaf_box_kernel(char *trees, size_t stride, size_t pyr_leaf_at, int64_t cells, size_t loff_at, size_t pts_at, size_t box_leaf_at) {
    char *tree = trees + (size_t)blockIdx.y * stride;
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m >= cells) return;
    const int rk = reinterpret_cast<const int32_t *>(tree + pyr_leaf_at)[m];
    if (rk < 0) return;
    const int32_t *loff = reinterpret_cast<const int32_t *>(tree + loff_at);
    const double *pts = reinterpret_cast<const double *>(tree + pts_at);
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    const int o = loff[rk], e = loff[rk + 1];
    for (int t = o; t < e; ++t) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = pts[(size_t)t * 3 + a];
            lo[a] = x < lo[a] ? x : lo[a];
            hi[a] = x > hi[a] ? x : hi[a];
        }
    }
    double *bx = reinterpret_cast<double *>(tree + box_leaf_at) + (size_t)rk * OT_BOX;
#pragma unroll
    for (int a = 0; a < 3; ++a) { bx[a] = lo[a] + 0.0; bx[3 + a] = hi[a] + 0.0; }
}

// ---- query ---------------------------------------------------------------------------------------------------------------------------
// the points of leaf rk in list order; the tie rule is explicit: the walk does not meet points in ascending order
__device__ inline int pt_leaf(const OtView<double> &tv, int rk, const double *q, double &best, int &best_m) {
    const int o = tv.loff[rk], e = tv.loff[rk + 1];
    for (int t = o; t < e; ++t) {
        const double *p = tv.payload + (size_t)t * 3;
        const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        const int m = tv.list[t];
        if (d < best || (d == best && m < best_m)) { best = d; best_m = m; }
    }
    return e - o;
}

// grid (query tiles, B).  perm NULL, or [B][N]: lane i of problem b answers query perm[b][i] (vt_point_tree_lanes)
template <bool SEED, bool ORDER>
__global__ void __launch_bounds__(MT_THREADS)
pt_query_kernel(const char *trees, OtAt tree_at, OtBase base, int L, const double *src, const double *T, int N, double *d2, int32_t *idx,
                int32_t *stats, const int32_t *perm, Gate gate) {
    const int b = blockIdx.y;
    if (frozen(gate, b)) return;
    const OtView<double> tv = ot_view<double>(trees, tree_at, b);
    const int lane = blockIdx.x * MT_THREADS + threadIdx.x;
    if (lane >= N) return;
    const int n = perm ? perm[(size_t)b * N + lane] : lane;
    double q[3];
    load_query(src, T, b, N, n, q);
    const double flo[3] = {tv.frame[0], tv.frame[1], tv.frame[2]}, fside = tv.frame[3];
    double best = __builtin_inf();
    int best_m = -1, n_boxes = 0, n_points = 0, seed_rk = -1;
    if (SEED) {
        seed_rk = ot_leaf_of(tv.pyr, tv.frame, L, q);
        if (seed_rk >= 0) n_points += pt_leaf(tv, seed_rk, q, best, best_m);
    }
    ot_walk(
        tv.pyr,
        [&](int level, int rk) {
            const double lb = ot_box_d2(tv.recs + ((size_t)base.v[level] + rk) * OT_BOX, q);
            ++n_boxes;
            if (lb > best) return false;
            if (level < L) return true;
            if (rk != seed_rk) n_points += pt_leaf(tv, rk, q, best, best_m);
            return false;
        },
        [&](int level, unsigned actual) { return ot_near_octant<ORDER>(flo, fside, level, actual, q); });
    const size_t at = (size_t)b * N + n;
    d2[at] = best;
    idx[at] = best_m;
    if (stats) { stats[2 * at] = n_boxes; stats[2 * at + 1] = n_points; }
}

bool pt_sizes_ok(int64_t M, int B) { return M >= 1 && M <= PT_MAX_M && B >= 1 && B <= 65535; }
bool pt_depth_ok(int depth) { return depth >= 1 && depth <= VT_WN_MAX_DEPTH; }

typedef void (*PtQueryFn)(const char *, OtAt, OtBase, int, const double *, const double *, int, double *, int32_t *, int32_t *, const int32_t *, Gate);
const PtQueryFn PT_QUERY[4] = {pt_query_kernel<false, false>, pt_query_kernel<true, false>, pt_query_kernel<false, true>, pt_query_kernel<true, true>};

}  // namespace

// every check of a query, the layout and the walk the environment asks for, once: nothing is enqueued
__attribute__((visibility("hidden")))
int pt_query_plan(size_t tree_bytes, int64_t M, int depth, int B, const int32_t *state_host, int64_t N, PtQueryPlan *plan) {
    if (!pt_sizes_ok(M, B) || N < 1 || N > PT_MAX_N || !state_host || !plan)
        return vt_fail(VT_ERR_INVALID, "vt_point_tree_query: bad argument (N >= 1, M >= 1, 1 <= B <= 65535)");
    if (!pt_depth_ok(depth)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_tree_query: depth outside [1, 7]");
    OtTree t;
    if (!pt_tree(M, depth, B, state_host, t)) return vt_fail(VT_ERR_INVALID, "vt_point_tree_query: counts that no tree of this size has");
    if (tree_bytes < t.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_point_tree_query: tree too small");
    int walk = 3;
    const char *w = getenv("VTACO_POINT_TREE_WALK");
    if (w && w[0]) {
        if (!strcmp(w, "plain")) walk = 0;
        else if (!strcmp(w, "seed")) walk = 1;
        else if (!strcmp(w, "order")) walk = 2;
        else if (strcmp(w, "seed+order")) return vt_fail(VT_ERR_INVALID, "vt_point_tree_query: VTACO_POINT_TREE_WALK must be plain, seed, order or seed+order");
    }
    plan->kernel = walk; plan->depth = depth; plan->B = B; plan->N = N;
    plan->stride = t.stride; plan->pyr = t.pyr; plan->box = t.rec; plan->loff = t.loff; plan->list = t.list; plan->pts = t.payload;
    for (int l = 0; l <= OT_LEVELS; ++l) plan->base[l] = t.base.v[l];
    return 0;
}

__attribute__((visibility("hidden")))
size_t pt_lanes_bytes(int64_t N, int B, int depth) {
    if (N < 1 || N > PT_MAX_N || B < 1 || B > 65535 || !pt_depth_ok(depth)) return 0;
    return ot_work(N, B, depth, false).bytes;
}

__attribute__((visibility("hidden")))
void pt_lanes_enqueue(const PtQueryPlan &plan, const void *tree, const double *src, const double *T, int32_t *perm, void *workspace, void *stream) {
    const int B = plan.B, depth = plan.depth, N = (int)plan.N;
    const OtWork w = ot_work(N, B, depth, false);
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace), *blocks = ws + w.blocks;
    ot_code_enqueue(PtLaneSource{src, T, N}, B, depth, static_cast<const char *>(tree), plan.stride, w, blocks, st);
    ot_scan_launch<OtCount, false>(OtCount{w.cnt}, cells_of(depth), B, blocks, w, w.doff, reinterpret_cast<int32_t *>(ws), OT_W_TOTAL, st);
    ot_fill_enqueue(N, B, depth, w, blocks, reinterpret_cast<char *>(perm), (size_t)N * sizeof(int32_t), st);
}

__attribute__((visibility("hidden")))
void pt_query_enqueue(const PtQueryPlan &plan, const void *tree, const double *src, const double *T, double *d2, int32_t *idx, int32_t *stats,
                      const int32_t *perm, const int32_t *done, const int32_t *iter, int it, void *stream) {
    OtBase base;
    for (int l = 0; l <= OT_LEVELS; ++l) base.v[l] = plan.base[l];
    hipLaunchKernelGGL(PT_QUERY[plan.kernel], dim3(blocks_of(plan.N, MT_THREADS), (unsigned)plan.B), dim3(MT_THREADS), 0, (hipStream_t)stream,
                       static_cast<const char *>(tree), OtAt{plan.stride, plan.pyr, plan.box, plan.loff, plan.list, plan.pts}, base, plan.depth,
                       src, T, (int)plan.N, d2, idx, stats, perm, Gate{done, iter, it});
}

extern "C" {

int vt_point_tree_default_depth(int64_t M) { return ot_default_depth(M); }

size_t vt_point_tree_workspace_bytes(int64_t M, int B, int depth) {
    if (!pt_sizes_ok(M, B) || !pt_depth_ok(depth)) return 0;
    return ot_work(M, B, depth).bytes;
}

int vt_point_tree_count(const double *dst, int64_t M, int B, int depth, void *workspace, size_t workspace_bytes, void *stream) {
    if (!pt_sizes_ok(M, B) || !dst || !workspace) return vt_fail(VT_ERR_INVALID, "vt_point_tree_count: bad argument (M >= 1, 1 <= B <= 65535)");
    if (!pt_depth_ok(depth)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_tree_count: depth outside [1, 7]");
    const OtWork w = ot_work(M, B, depth);
    if (workspace_bytes < w.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_point_tree_count: workspace too small");
    ot_count_enqueue(PtSource{dst, (int)M}, B, depth, w, static_cast<char *>(workspace), (hipStream_t)stream);
    return vt_check(hipGetLastError(), "vt_point_tree_count");
}

int vt_point_tree_layout(int64_t M, int depth, int B, const int32_t *state_host, size_t *offsets) {
    if (!pt_sizes_ok(M, B) || !state_host || !offsets) return vt_fail(VT_ERR_INVALID, "vt_point_tree_layout: bad argument (M >= 1, 1 <= B <= 65535)");
    if (!pt_depth_ok(depth)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_tree_layout: depth outside [1, 7]");
    OtTree t;
    if (!pt_tree(M, depth, B, state_host, t)) return vt_fail(VT_ERR_INVALID, "vt_point_tree_layout: counts that no tree of this size has");
    offsets[0] = t.pyr; offsets[1] = t.rec; offsets[2] = t.loff; offsets[3] = t.list; offsets[4] = t.payload; offsets[5] = t.stride; offsets[6] = t.bytes;
    return 0;
}

int vt_point_tree_build(const double *dst, int64_t M, int B, int depth, const int32_t *state_host, void *workspace, size_t workspace_bytes, void *tree,
                        size_t tree_bytes, void *stream) {
    if (!pt_sizes_ok(M, B) || !dst || !state_host || !workspace || !tree)
        return vt_fail(VT_ERR_INVALID, "vt_point_tree_build: bad argument (M >= 1, 1 <= B <= 65535)");
    if (!pt_depth_ok(depth)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_tree_build: depth outside [1, 7]");
    for (int b = 0; b < B; ++b)
        if (state_host[(size_t)b * OT_STATE] != 0) return vt_fail(VT_ERR_INVALID, "vt_point_tree_build: a target coordinate is not finite");
    OtTree t;
    if (!pt_tree(M, depth, B, state_host, t)) return vt_fail(VT_ERR_INVALID, "vt_point_tree_build: counts that no tree of this size has");
    const OtWork w = ot_work(M, B, depth);
    if (workspace_bytes < w.bytes || tree_bytes < t.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_point_tree_build: workspace or tree too small");
    hipStream_t st = (hipStream_t)stream;
    char *tr = static_cast<char *>(tree);
    ot_build_enqueue(PtSource{dst, (int)M}, B, depth, w, static_cast<char *>(workspace), t, tr, st);
    const unsigned nb = (unsigned)B;
    const int64_t leaf = cells_of(depth);
    hipLaunchKernelGGL(pt_leaf_box_kernel, dim3(blocks_of(leaf, MT_THREADS), nb), dim3(MT_THREADS), 0, st, tr, t.stride,
                       t.pyr + (size_t)pyr_off(depth) * 4, leaf, t.loff, t.payload, t.rec + (size_t)t.base.v[depth] * OT_BOX * sizeof(double));
    for (int l = depth - 1; l >= 0; --l)
        hipLaunchKernelGGL(ot_inner_box_kernel, dim3(blocks_of(cells_of(l), MT_THREADS), nb), dim3(MT_THREADS), 0, st, (const char *)tr, t.stride,
                           t.pyr + (size_t)pyr_off(l) * 4, t.pyr + (size_t)pyr_off(l + 1) * 4, cells_of(l), tr, t.stride,
                           t.rec + (size_t)t.base.v[l + 1] * OT_BOX * sizeof(double), t.rec + (size_t)t.base.v[l] * OT_BOX * sizeof(double));
    return vt_check(hipGetLastError(), "vt_point_tree_build");
}

int vt_point_tree_query(const void *tree, size_t tree_bytes, int64_t M, int depth, int B, const int32_t *state_host, const double *src, int64_t N,
                        const double *T, double *d2, int32_t *idx, int32_t *stats, const int32_t *perm, void *stream) {
    if (!tree || !src || !d2 || !idx) return vt_fail(VT_ERR_INVALID, "vt_point_tree_query: bad argument (a NULL array)");
    PtQueryPlan plan;
    if (int rc = pt_query_plan(tree_bytes, M, depth, B, state_host, N, &plan)) return rc;
    pt_query_enqueue(plan, tree, src, T, d2, idx, stats, perm, nullptr, nullptr, 0, stream);
    return vt_check(hipGetLastError(), "vt_point_tree_query");
}

size_t vt_point_tree_lanes_workspace_bytes(int64_t N, int B, int depth) { return pt_lanes_bytes(N, B, depth); }

int vt_point_tree_lanes(const void *tree, size_t tree_bytes, int64_t M, int depth, int B, const int32_t *state_host, const double *src, int64_t N,
                        const double *T, int32_t *perm, void *workspace, size_t workspace_bytes, void *stream) {
    if (!tree || !src || !perm || !workspace) return vt_fail(VT_ERR_INVALID, "vt_point_tree_lanes: bad argument (a NULL array)");
    PtQueryPlan plan;
    if (int rc = pt_query_plan(tree_bytes, M, depth, B, state_host, N, &plan)) return rc;
    if (workspace_bytes < pt_lanes_bytes(N, B, depth)) return vt_fail(VT_ERR_WORKSPACE, "vt_point_tree_lanes: workspace too small");
    pt_lanes_enqueue(plan, tree, src, T, perm, workspace, stream);
    return vt_check(hipGetLastError(), "vt_point_tree_lanes");
}

}  // extern "C"
