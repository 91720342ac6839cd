// What icp.hip, point_tree.hip and knn.hip share: the loop's per-problem gate, the moved point and the query loader.  Everything lives in
// an unnamed namespace: each translation unit has its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// the loop's per-problem state; a NULL `done` never freezes
struct Gate { const int32_t *done; const int32_t *iter; int it; };
__device__ inline bool frozen(const Gate &g, int b) { return g.done && g.done[b] != 0 && g.iter[b] < g.it; }

__device__ inline void move_point(const double *T, double x, double y, double z, double &ox, double &oy, double &oz) {
    ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// query n of problem b among src [B][N][3], moved by T [B][16] when given
__device__ inline void load_query(const double *src, const double *T, int b, int N, int64_t n, double q[3]) {
    const double *p = src + ((size_t)b * N + n) * 3;
    q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    if (T) move_point(T + (size_t)b * 16, q[0], q[1], q[2], q[0], q[1], q[2]);
}

}  // namespace

// point_tree.hip's query for the loop of icp.hip, in two steps so that every check and the choice of the walk happen once, before
// anything is enqueued.  Internal to the library: hidden, not part of include/vtaco_hip.h.
struct PtQueryPlan { int kernel, depth, B; int64_t N; size_t stride, pyr, box, loff, list, pts; int base[16]; };
__attribute__((visibility("hidden")))
int pt_query_plan(size_t tree_bytes, int64_t M, int depth, int B, const int32_t *state_host, int64_t N, PtQueryPlan *plan);
__attribute__((visibility("hidden")))
void pt_query_enqueue(const PtQueryPlan &plan, const void *tree, const double *src, const double *T, double *d2, int32_t *idx, int32_t *stats,
                      const int32_t *perm, const int32_t *done, const int32_t *iter, int it, void *stream);
// the permutation vt_point_tree_lanes builds; workspace of pt_lanes_bytes(N, B, depth) bytes
__attribute__((visibility("hidden")))
size_t pt_lanes_bytes(int64_t N, int B, int depth);
__attribute__((visibility("hidden")))
void pt_lanes_enqueue(const PtQueryPlan &plan, const void *tree, const double *src, const double *T, int32_t *perm, void *workspace, void *stream);
