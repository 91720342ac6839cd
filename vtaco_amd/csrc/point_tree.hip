// Nearest point of a point set through an octree over the points: the d2 and idx of vt_nn_points (icp.hip), bit for bit, without testing
// every target.  The reference searches a kd-tree there (src/utils/icp.py:50-66, sklearn; src/common.py:142-175, pykdtree).  The
// definitions are DESIGN.md's section "point_tree.hip", restated in numpy by tests/point_tree_ref.py: this file's operations in this
// file's order.  B problems with one M per call; every kernel covers the batch in one launch, the problem index in the grid.
//   frame     lo = the targets' minimum corner, side = their largest extent (1 when 0), n = 2^depth cells per axis, 1 <= depth <= 7
//   binning   a point lives in the leaf clamp((int)floor((p - lo) / side * n), 0, n - 1) per axis; cells are numbered in Morton order
//             (winding_fast.hip's): the children of cell m at level l are 8m .. 8m+7 at level l + 1
//   pyramid   per level a dense int32 [8^l]: the rank of an occupied cell among its level's occupied cells, or -1
//   lists     count, scan, fill through an integer cursor, then every point is placed at its rank inside its leaf: ascending index.
//             The points are copied in list order: a leaf's points are contiguous
//   boxes     per occupied cell lo[3], hi[3]: a leaf's the min / max of its points, an inner cell's the min / max of its occupied
//             children.  Minimum and maximum do not round; +0.0 is added on the way out, so a zero is stored as +0.0
//   query     one lane per query, float64, winding_fast.hip's walk without a stack.  Per occupied cell e_a = lo_a - q_a when
//             q_a < lo_a, q_a - hi_a when q_a > hi_a, else 0; lb = (e_x e_x + e_y e_y) + e_z e_z, the operation order of
//             d2 = (dx dx + dy dy) + dz dz, d = q - p.  Rounding is monotone: |fl(q_a - p_a)| >= fl(e_a) >= 0 for every point of the cell,
//             and products and sums of non-negative values keep the order, so the computed lb is <= the computed d2 of every point
//             under the cell: the cell is skipped exactly when lb > best, with no slack term.  A leaf's points are taken in list order
//             on d2 < best || (d2 == best && index < best index): the lowest index among equal minima, as the ascending brute force
//             gives.  A NaN query makes every comparison false: it visits everything and returns (+inf, -1)
//   seed      before the walk the query's own clamped leaf, when occupied, is evaluated; the walk tests its box and passes over it
//   order     the children of a cell are visited as k ^ o, o the octant of the query about the cell's centre
//             lo_a + (i_a + 0.5) (side / 2^level): near children first
//   lanes     optionally lane i answers query perm[i], perm the queries in Morton order of the tree's leaves (count / scan / fill per
//             call): a wave's lanes then walk neighbouring cells.  Outputs stay in query order; no result depends on perm
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
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

constexpr int PT_LEVELS = VT_WN_MAX_DEPTH + 1;
constexpr int PT_BOX = 6;                       // doubles per box: lo[3], hi[3]
constexpr int PT_STATE = 16;                    // int32 per problem: 0 status, 1..8 occupied cells of level 0..7, 10 the list scan's total
constexpr int PT_W_COUNT = 1;
constexpr int PT_W_TOTAL = 10;
constexpr int PT_BAD_POINT = 1;                 // status bit: a target coordinate that is not finite
constexpr size_t PT_AUX = 128;                  // bytes per problem: the bounding box as ordered keys (6 u64), at byte 64 lo[3] and side
constexpr size_t PT_HEAD = 256;                 // tree header: lo[3], side (doubles at 0), box base per level (int32 at byte 64), depth, M
constexpr int64_t PT_MAX_M = MT_MAX_F;
constexpr int64_t PT_MAX_N = 0x7fffff00;

int64_t cells_of(int l) { return (int64_t)1 << (3 * l); }
int64_t pyr_off(int l) { return (cells_of(l) - 1) / 7; }     // cells of the levels above l

// workspace: the state words of all problems, their frames, then one block per problem
struct PtWork { size_t aux, blocks, blk, codes, cnt, doff, pyr, tmp, bsum, bytes; };
PtWork pt_work(int64_t M, int B, int L) {
    PtWork w;
    const size_t leaf = (size_t)cells_of(L);
    w.aux = up256((size_t)B * PT_STATE * 4);
    w.blocks = w.aux + up256((size_t)B * PT_AUX);
    w.codes = 0;
    w.cnt = w.codes + up256((size_t)M * 4);
    w.doff = w.cnt + up256(leaf * 4);
    w.pyr = w.doff + up256(leaf * 4);
    w.tmp = w.pyr + up256((size_t)pyr_off(L + 1) * 4);
    w.bsum = w.tmp + up256((size_t)M * 4);
    w.blk = w.bsum + scan_bytes((int64_t)leaf);
    w.bytes = w.blocks + (size_t)B * w.blk;
    return w;
}

// the trees: one stride per problem, every array at one offset in all of them.  A level's boxes have room for the largest count of
// that level over the batch: box_base[l] is where level l starts, in boxes
struct PtBase { int v[PT_LEVELS + 1]; };
struct PtTree { size_t pyr, box, loff, list, pts, stride, bytes; PtBase base; };
bool pt_tree(int64_t M, int L, int B, const int32_t *state, PtTree &t) {
    int64_t total = 0;
    int64_t leaves = 0;
    for (int l = 0; l < PT_LEVELS; ++l) {
        t.base.v[l] = (int)total;
        if (l > L) continue;
        int64_t cap = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t c = state[(size_t)b * PT_STATE + PT_W_COUNT + l];
            if (c < 1 || c > cells_of(l) || c > M) return false;
            cap = c > cap ? c : cap;
        }
        total += cap;
        if (l == L) leaves = cap;
    }
    t.base.v[PT_LEVELS] = (int)total;
    if (total > 0x7fffffff) return false;
    t.pyr = PT_HEAD;
    t.box = t.pyr + up256((size_t)pyr_off(L + 1) * 4);
    t.loff = t.box + up256((size_t)total * PT_BOX * sizeof(double));
    t.list = t.loff + up256((size_t)(leaves + 1) * 4);
    t.pts = t.list + up256((size_t)M * 4);
    t.stride = t.pts + up256((size_t)M * 3 * sizeof(double));
    t.bytes = (size_t)B * t.stride;
    return true;
}

template <class T>
__device__ inline T *blk_at(char *blocks, size_t blk, int b, size_t off) { return reinterpret_cast<T *>(blocks + (size_t)b * blk + off); }
template <class T>
__device__ inline const T *blk_at(const char *blocks, size_t blk, int b, size_t off) {
    return reinterpret_cast<const T *>(blocks + (size_t)b * blk + off);
}

// ---- count: frame, codes, pyramids, list offsets -----------------------------------------------------------------------------------
// grid (B)
__global__ void pt_init_kernel(int32_t *state, char *aux) {
    const int b = blockIdx.x;
    if (threadIdx.x < PT_STATE) state[(size_t)b * PT_STATE + threadIdx.x] = 0;
    u64 *keys = reinterpret_cast<u64 *>(aux + (size_t)b * PT_AUX);
    if (threadIdx.x < 3) keys[threadIdx.x] = ~0ull;              // minima
    else if (threadIdx.x < 6) keys[threadIdx.x] = 0ull;          // maxima
}

// grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS) pt_bbox_kernel(const double *dst, int64_t M, int32_t *state, char *aux) {
    __shared__ double lds[6][MT_THREADS];
    const int b = blockIdx.y;
    const double *p = dst + (size_t)b * M * 3;
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    bool bad = false;
    for (int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x; m < M; m += (int64_t)gridDim.x * MT_THREADS) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = p[3 * m + a];
            if (!(fabs(x) < __builtin_inf())) { bad = true; continue; }
            lo[a] = x < lo[a] ? x : lo[a];
            hi[a] = x > hi[a] ? x : hi[a];
        }
    }
    if (bad) atomicOr(state + (size_t)b * PT_STATE, PT_BAD_POINT);
#pragma unroll
    for (int a = 0; a < 3; ++a) { lds[a][threadIdx.x] = lo[a]; lds[3 + a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int d = MT_THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double x = lds[a][threadIdx.x + d], y = lds[3 + a][threadIdx.x + d];
                if (x < lds[a][threadIdx.x]) lds[a][threadIdx.x] = x;
                if (y > lds[3 + a][threadIdx.x]) lds[3 + a][threadIdx.x] = y;
            }
        }
        __syncthreads();
    }
    u64 *keys = reinterpret_cast<u64 *>(aux + (size_t)b * PT_AUX);
    if (threadIdx.x < 3) atomicMin(keys + threadIdx.x, key_of(lds[threadIdx.x][0]));
    else if (threadIdx.x < 6) atomicMax(keys + threadIdx.x, key_of(lds[threadIdx.x][0]));
}

// grid (B), one thread
__global__ void pt_frame_kernel(char *aux) {
    const int b = blockIdx.x;
    const u64 *keys = reinterpret_cast<const u64 *>(aux + (size_t)b * PT_AUX);
    double *frame = reinterpret_cast<double *>(aux + (size_t)b * PT_AUX + 64);
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = value_of(keys[a]) + 0.0, hi = value_of(keys[3 + a]);
        frame[a] = lo;
        const double e = hi - lo;
        ext = e > ext ? e : ext;
    }
    frame[3] = ext > 0.0 ? ext : 1.0;
}

// grid (blocks, B): n int32 words at `off` of every block
__global__ void __launch_bounds__(MT_THREADS) pt_zero_kernel(char *blocks, size_t blk, size_t off, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < n) blk_at<int32_t>(blocks, blk, blockIdx.y, off)[i] = 0;
}

__device__ inline unsigned pt_spread(unsigned x) {          // bit k -> bit 3k, 7 bits
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < VT_WN_MAX_DEPTH; ++k) r |= ((x >> k) & 1u) << (3 * k);
    return r;
}
__device__ inline unsigned pt_gather(unsigned m) {          // bit 3k -> bit k, 7 bits
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < VT_WN_MAX_DEPTH; ++k) r |= ((m >> (3 * k)) & 1u) << k;
    return r;
}

// the leaf of a point: a NaN becomes cell 0, +-inf the first or the last cell
__device__ inline unsigned pt_code(double x, double y, double z, const double *frame, int L) {
    const int n = 1 << L;
    const double p[3] = {x, y, z};
    unsigned code = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double g = floor((p[a] - frame[a]) / frame[3] * (double)n);
        g = g > 0.0 ? g : 0.0;
        g = g < (double)(n - 1) ? g : (double)(n - 1);
        code |= pt_spread((unsigned)(int)g) << a;
    }
    return code;
}

// grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS)
pt_code_kernel(const double *dst, int M, int L, const char *aux, char *blocks, size_t blk, size_t codes_off, size_t cnt_off) {
    const int b = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m >= M) return;
    const double *frame = reinterpret_cast<const double *>(aux + (size_t)b * PT_AUX + 64);
    const double *p = dst + ((size_t)b * M + m) * 3;
    const unsigned code = pt_code(p[0], p[1], p[2], frame, L);
    blk_at<int32_t>(blocks, blk, b, codes_off)[m] = (int32_t)code;
    atomicAdd(blk_at<int32_t>(blocks, blk, b, cnt_off) + code, 1);
}

// what a scan adds per element: 1 for an occupied cell (the pyramids), or the cell's count (the list offsets)
struct PtLeafOcc {
    size_t cnt_off;
    __device__ int operator()(const char *block, int64_t i) const { return reinterpret_cast<const int32_t *>(block + cnt_off)[i] > 0 ? 1 : 0; }
};
struct PtInnerOcc {
    size_t child_off;                                            // the finished pyramid of the level below
    __device__ int operator()(const char *block, int64_t i) const {
        const int32_t *child = reinterpret_cast<const int32_t *>(block + child_off);
        int all = -1;
#pragma unroll
        for (int k = 0; k < 8; ++k) all &= child[8 * i + k];
        return all >= 0 ? 1 : 0;                                 // any child's rank is not negative
    }
};
struct PtCount {
    size_t cnt_off;
    __device__ int operator()(const char *block, int64_t i) const { return reinterpret_cast<const int32_t *>(block + cnt_off)[i]; }
};

// mesh_common.h's three-phase exclusive scan with the problem in blockIdx.y.  grid (chunks, B)
template <class P>
__global__ void __launch_bounds__(MT_THREADS) pt_scan_count_kernel(P val, int64_t n, char *blocks, size_t blk, size_t bsum_off) {
    __shared__ int lds[MT_THREADS];
    const char *block = blocks + (size_t)blockIdx.y * blk;
    const int64_t i0 = (int64_t)blockIdx.x * MT_CHUNK + (int64_t)threadIdx.x * MT_ITEMS;
    int s = 0;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) s += i0 + k < n ? val(block, i0 + k) : 0;
    const int incl = block_inclusive_scan(s, lds);
    if (threadIdx.x == MT_THREADS - 1) blk_at<int32_t>(blocks, blk, blockIdx.y, bsum_off)[blockIdx.x] = incl;
}

// grid (B), one workgroup per problem: bsum[0..nb) becomes its exclusive scan, state[word] the sum
__global__ void __launch_bounds__(MT_THREADS) pt_scan_blocks_kernel(char *blocks, size_t blk, size_t bsum_off, int nb, int32_t *state, int word) {
    __shared__ int lds[MT_THREADS];
    int32_t *bsum = blk_at<int32_t>(blocks, blk, blockIdx.x, bsum_off);
    int carry = 0;
    for (int base = 0; base < nb; base += MT_THREADS) {
        const int i = base + (int)threadIdx.x;
        const int x = i < nb ? bsum[i] : 0;
        const int incl = block_inclusive_scan(x, lds);
        if (i < nb) bsum[i] = carry + incl - x;
        carry += lds[MT_THREADS - 1];
    }
    if (threadIdx.x == 0) state[(size_t)blockIdx.x * PT_STATE + word] = carry;
}

// grid (chunks, B).  MARK: an element that adds nothing gets -1 (a pyramid's empty cell)
template <class P, bool MARK>
__global__ void __launch_bounds__(MT_THREADS) pt_scan_write_kernel(P val, int64_t n, char *blocks, size_t blk, size_t bsum_off, size_t pos_off) {
    __shared__ int lds[MT_THREADS];
    const char *block = blocks + (size_t)blockIdx.y * blk;
    const int64_t i0 = (int64_t)blockIdx.x * MT_CHUNK + (int64_t)threadIdx.x * MT_ITEMS;
    int v[MT_ITEMS];
    int s = 0;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) { v[k] = i0 + k < n ? val(block, i0 + k) : 0; s += v[k]; }
    int at = blk_at<int32_t>(blocks, blk, blockIdx.y, bsum_off)[blockIdx.x] + block_inclusive_scan(s, lds) - s;
    int32_t *pos = blk_at<int32_t>(blocks, blk, blockIdx.y, pos_off);
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        if (i0 + k < n) pos[i0 + k] = (MARK && v[k] == 0) ? -1 : at;
        at += v[k];
    }
}

template <class P, bool MARK>
void pt_scan_launch(P val, int64_t n, int B, char *blocks, const PtWork &w, size_t pos_off, int32_t *state, int word, hipStream_t st) {
    const unsigned nb = blocks_of(n, MT_CHUNK);
    hipLaunchKernelGGL(pt_scan_count_kernel<P>, dim3(nb, (unsigned)B), dim3(MT_THREADS), 0, st, val, n, blocks, w.blk, w.bsum);
    hipLaunchKernelGGL(pt_scan_blocks_kernel, dim3((unsigned)B), dim3(MT_THREADS), 0, st, blocks, w.blk, w.bsum, (int)nb, state, word);
    hipLaunchKernelGGL((pt_scan_write_kernel<P, MARK>), dim3(nb, (unsigned)B), dim3(MT_THREADS), 0, st, val, n, blocks, w.blk, w.bsum, pos_off);
}

// ---- build: header, lists, points in list order, boxes ----------------------------------------------------------------------------
// grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS)
pt_header_kernel(const char *aux, const char *blocks, size_t blk, size_t pyr_off_ws, int64_t words, PtBase base, int L, int M, char *trees,
                 size_t stride, size_t pyr_at) {
    const int b = blockIdx.y;
    char *tree = trees + (size_t)b * stride;
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < words) reinterpret_cast<int32_t *>(tree + pyr_at)[i] = blk_at<int32_t>(blocks, blk, b, pyr_off_ws)[i];
    if (i == 0) {
        const double *frame = reinterpret_cast<const double *>(aux + (size_t)b * PT_AUX + 64);
        double *head = reinterpret_cast<double *>(tree);
#pragma unroll
        for (int k = 0; k < 4; ++k) head[k] = frame[k];
        int32_t *hb = reinterpret_cast<int32_t *>(tree + 64);
#pragma unroll
        for (int k = 0; k <= PT_LEVELS; ++k) hb[k] = base.v[k];
        hb[16] = L; hb[17] = M;
    }
}

// grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS)
pt_list_offsets_kernel(const int32_t *state, const char *blocks, size_t blk, size_t doff_off, int64_t cells, int L, int M, char *trees,
                       size_t stride, size_t pyr_leaf_at, size_t loff_at) {
    const int b = blockIdx.y;
    char *tree = trees + (size_t)b * stride;
    const int32_t *pyr_leaf = reinterpret_cast<const int32_t *>(tree + pyr_leaf_at);
    int32_t *loff = reinterpret_cast<int32_t *>(tree + loff_at);
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m == 0) loff[state[(size_t)b * PT_STATE + PT_W_COUNT + L]] = M;
    if (m < cells && pyr_leaf[m] >= 0) loff[pyr_leaf[m]] = blk_at<int32_t>(blocks, blk, b, doff_off)[m];
}

// grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS) pt_fill_kernel(char *blocks, size_t blk, size_t codes_off, size_t doff_off, size_t cursor_off,
                                                             size_t tmp_off, int M) {
    const int b = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m >= M) return;
    const int code = blk_at<int32_t>(blocks, blk, b, codes_off)[m];
    const int at = blk_at<int32_t>(blocks, blk, b, doff_off)[code] + atomicAdd(blk_at<int32_t>(blocks, blk, b, cursor_off) + code, 1);
    blk_at<int32_t>(blocks, blk, b, tmp_off)[at] = (int32_t)m;
}

// a point's place in its leaf is the number of that leaf's points below it: the lists end ascending however the cursor filled them.
// grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS)
pt_rank_kernel(const double *dst, int M, const char *blocks, size_t blk, size_t codes_off, size_t doff_off, size_t cursor_off, size_t tmp_off,
               char *trees, size_t stride, size_t list_at, size_t pts_at) {
    const int b = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m >= M) return;
    const int code = blk_at<int32_t>(blocks, blk, b, codes_off)[m];
    const int o = blk_at<int32_t>(blocks, blk, b, doff_off)[code], n = blk_at<int32_t>(blocks, blk, b, cursor_off)[code];
    const int32_t *tmp = blk_at<int32_t>(blocks, blk, b, tmp_off);
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += tmp[o + j] < (int32_t)m ? 1 : 0;
    const size_t at = (size_t)o + rank;
    char *tree = trees + (size_t)b * stride;
    reinterpret_cast<int32_t *>(tree + list_at)[at] = (int32_t)m;
    const double *p = dst + ((size_t)b * M + m) * 3;
    double *q = reinterpret_cast<double *>(tree + pts_at) + at * 3;
    q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
}

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
    double *bx = reinterpret_cast<double *>(tree + box_leaf_at) + (size_t)rk * PT_BOX;
#pragma unroll
    for (int a = 0; a < 3; ++a) { bx[a] = lo[a] + 0.0; bx[3 + a] = hi[a] + 0.0; }
}

// grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS)
pt_inner_box_kernel(char *trees, size_t stride, size_t pyr_at, size_t pyr_child_at, int64_t cells, size_t box_child_at, size_t box_level_at) {
    char *tree = trees + (size_t)blockIdx.y * stride;
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m >= cells) return;
    const int rk = reinterpret_cast<const int32_t *>(tree + pyr_at)[m];
    if (rk < 0) return;
    const int32_t *pyr_child = reinterpret_cast<const int32_t *>(tree + pyr_child_at);
    const double *box_child = reinterpret_cast<const double *>(tree + box_child_at);
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    for (int k = 0; k < 8; ++k) {
        const int ck = pyr_child[8 * m + k];
        if (ck < 0) continue;
        const double *c = box_child + (size_t)ck * PT_BOX;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = c[a] < lo[a] ? c[a] : lo[a];
            hi[a] = c[3 + a] > hi[a] ? c[3 + a] : hi[a];
        }
    }
    double *bx = reinterpret_cast<double *>(tree + box_level_at) + (size_t)rk * PT_BOX;
#pragma unroll
    for (int a = 0; a < 3; ++a) { bx[a] = lo[a]; bx[3 + a] = hi[a]; }
}

// ---- query ---------------------------------------------------------------------------------------------------------------------------
// the points of leaf rk in list order; the tie rule is explicit: the walk does not meet points in ascending order
__device__ inline int pt_leaf(const int32_t *loff, const int32_t *list, const double *pts, int rk, double qx, double qy, double qz, double &best,
                              int &best_m) {
    const int o = loff[rk], e = loff[rk + 1];
    for (int t = o; t < e; ++t) {
        const double *p = pts + (size_t)t * 3;
        const double dx = qx - p[0], dy = qy - p[1], dz = qz - p[2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        const int m = list[t];
        if (d < best || (d == best && m < best_m)) { best = d; best_m = m; }
    }
    return e - o;
}

// grid (query tiles, B).  perm NULL, or [B][N]: lane i of problem b answers query perm[b][i] (vt_point_tree_lanes)
template <bool SEED, bool ORDER>
__global__ void __launch_bounds__(MT_THREADS)
pt_query_kernel(const char *trees, size_t stride, size_t pyr_at, size_t box_at, size_t loff_at, size_t list_at, size_t pts_at, PtBase base, int L,
                const double *src, const double *T, int N, double *d2, int32_t *idx, int32_t *stats, const int32_t *perm, Gate gate) {
    const int b = blockIdx.y;
    if (frozen(gate, b)) return;
    const char *tree = trees + (size_t)b * stride;
    const double *frame = reinterpret_cast<const double *>(tree);
    const int32_t *pyr = reinterpret_cast<const int32_t *>(tree + pyr_at);
    const double *boxes = reinterpret_cast<const double *>(tree + box_at);
    const int32_t *loff = reinterpret_cast<const int32_t *>(tree + loff_at);
    const int32_t *list = reinterpret_cast<const int32_t *>(tree + list_at);
    const double *pts = reinterpret_cast<const double *>(tree + pts_at);
    const int lane = blockIdx.x * MT_THREADS + threadIdx.x;
    if (lane >= N) return;
    const int n = perm ? perm[(size_t)b * N + lane] : lane;
    double q[3];
    {
        const double *p = src + ((size_t)b * N + n) * 3;
        q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
        if (T) move_point(T + (size_t)b * 16, q[0], q[1], q[2], q[0], q[1], q[2]);
    }
    const double flo[3] = {frame[0], frame[1], frame[2]}, fside = frame[3];
    double best = __builtin_inf();
    int best_m = -1, n_boxes = 0, n_points = 0, seed_rk = -1;
    if (SEED) {
        seed_rk = pyr[(unsigned)((((int64_t)1 << (3 * L)) - 1) / 7) + pt_code(q[0], q[1], q[2], frame, L)];
        if (seed_rk >= 0) n_points += pt_leaf(loff, list, pts, seed_rk, q[0], q[1], q[2], best, best_m);
    }
    int level = 0;
    unsigned cell = 0, flip = 0, level_at = 0;                    // level_at = (8^level - 1) / 7; flip: the octant o of every level, 3 bits each
    for (;;) {
        const unsigned actual = cell ^ flip;
        const int rk = pyr[level_at + actual];
        bool descend = false;
        if (rk >= 0) {
            const double *bx = boxes + ((size_t)base.v[level] + rk) * PT_BOX;
            double e[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double lo = bx[a], hi = bx[3 + a];
                e[a] = q[a] < lo ? lo - q[a] : (q[a] > hi ? q[a] - hi : 0.0);
            }
            const double lb = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
            ++n_boxes;
            if (!(lb > best)) {
                if (level < L) descend = true;
                else if (rk != seed_rk) n_points += pt_leaf(loff, list, pts, rk, q[0], q[1], q[2], best, best_m);
            }
        }
        if (descend) {
            unsigned o = 0;
            if (ORDER) {
                const double h = fside * (1.0 / (double)(1 << level));
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double centre = flo[a] + ((double)pt_gather(actual >> a) + 0.5) * h;
                    o |= q[a] >= centre ? 1u << a : 0u;
                }
            }
            level_at = level_at * 8 + 1; ++level; cell *= 8; flip = flip * 8 + o;
        } else {
            ++cell;
            while (level > 0 && (cell & 7u) == 0) { cell >>= 3; flip >>= 3; --level; level_at = (level_at - 1) >> 3; }
            if (level == 0) break;
        }
    }
    const size_t at = (size_t)b * N + n;
    d2[at] = best;
    idx[at] = best_m;
    if (stats) { stats[2 * at] = n_boxes; stats[2 * at + 1] = n_points; }
}

// ---- lanes: queries handed to lanes in Morton order of the target frame ------------------------------------------------------------
// grid (query tiles, B): the leaf the (moved) query falls in, clamped into the frame, and the leaf's count
__global__ void __launch_bounds__(MT_THREADS)
pt_lane_code_kernel(const char *trees, size_t stride, int L, const double *src, const double *T, int N, char *blocks, size_t blk, size_t codes_off,
                    size_t cnt_off) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * MT_THREADS + threadIdx.x;
    if (n >= N) return;
    const double *frame = reinterpret_cast<const double *>(trees + (size_t)b * stride);
    const double *p = src + ((size_t)b * N + n) * 3;
    double x = p[0], y = p[1], z = p[2];
    if (T) move_point(T + (size_t)b * 16, x, y, z, x, y, z);
    const unsigned code = pt_code(x, y, z, frame, L);
    blk_at<int32_t>(blocks, blk, b, codes_off)[n] = (int32_t)code;
    atomicAdd(blk_at<int32_t>(blocks, blk, b, cnt_off) + code, 1);
}

// grid (query tiles, B): a permutation whatever order the cursor hands out inside a leaf; no result depends on it
__global__ void __launch_bounds__(MT_THREADS)
pt_lane_fill_kernel(char *blocks, size_t blk, size_t codes_off, size_t doff_off, size_t cursor_off, int N, int32_t *perm) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * MT_THREADS + threadIdx.x;
    if (n >= N) return;
    const int code = blk_at<int32_t>(blocks, blk, b, codes_off)[n];
    const int at = blk_at<int32_t>(blocks, blk, b, doff_off)[code] + atomicAdd(blk_at<int32_t>(blocks, blk, b, cursor_off) + code, 1);
    perm[(size_t)b * N + at] = n;
}

PtWork pt_lane_work(int64_t N, int B, int L) {
    PtWork w;
    const size_t leaf = (size_t)cells_of(L);
    w.aux = w.blocks = up256((size_t)B * PT_STATE * 4);
    w.codes = 0;
    w.cnt = w.codes + up256((size_t)N * 4);
    w.doff = w.cnt + up256(leaf * 4);
    w.pyr = w.tmp = w.bsum = w.doff + up256(leaf * 4);
    w.blk = w.bsum + scan_bytes((int64_t)leaf);
    w.bytes = w.blocks + (size_t)B * w.blk;
    return w;
}

bool pt_sizes_ok(int64_t M, int B) { return M >= 1 && M <= PT_MAX_M && B >= 1 && B <= 65535; }
bool pt_depth_ok(int depth) { return depth >= 1 && depth <= VT_WN_MAX_DEPTH; }

typedef void (*PtQueryFn)(const char *, size_t, size_t, size_t, size_t, size_t, size_t, PtBase, int, const double *, const double *, int, double *,
                          int32_t *, int32_t *, const int32_t *, Gate);
const PtQueryFn PT_QUERY[4] = {pt_query_kernel<false, false>, pt_query_kernel<true, false>, pt_query_kernel<false, true>, pt_query_kernel<true, true>};

}  // namespace

// every check of a query, the layout and the walk the environment asks for, once: nothing is enqueued
__attribute__((visibility("hidden")))
int pt_query_plan(size_t tree_bytes, int64_t M, int depth, int B, const int32_t *state_host, int64_t N, PtQueryPlan *plan) {
    if (!pt_sizes_ok(M, B) || N < 1 || N > PT_MAX_N || !state_host || !plan)
        return vt_fail(VT_ERR_INVALID, "vt_point_tree_query: bad argument (N >= 1, M >= 1, 1 <= B <= 65535)");
    if (!pt_depth_ok(depth)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_tree_query: depth outside [1, 7]");
    PtTree t;
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
    plan->stride = t.stride; plan->pyr = t.pyr; plan->box = t.box; plan->loff = t.loff; plan->list = t.list; plan->pts = t.pts;
    for (int l = 0; l <= PT_LEVELS; ++l) plan->base[l] = t.base.v[l];
    return 0;
}

__attribute__((visibility("hidden")))
size_t pt_lanes_bytes(int64_t N, int B, int depth) {
    if (N < 1 || N > PT_MAX_N || B < 1 || B > 65535 || !pt_depth_ok(depth)) return 0;
    return pt_lane_work(N, B, depth).bytes;
}

__attribute__((visibility("hidden")))
void pt_lanes_enqueue(const PtQueryPlan &plan, const void *tree, const double *src, const double *T, int32_t *perm, void *workspace, void *stream) {
    const int B = plan.B, depth = plan.depth;
    const int64_t N = plan.N, leaf = cells_of(depth);
    const PtWork w = pt_lane_work(N, B, depth);
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace), *blocks = ws + w.blocks;
    const unsigned nb = (unsigned)B, qb = blocks_of(N, MT_THREADS);
    hipLaunchKernelGGL(pt_zero_kernel, dim3(blocks_of(leaf, MT_THREADS), nb), dim3(MT_THREADS), 0, st, blocks, w.blk, w.cnt, leaf);
    hipLaunchKernelGGL(pt_lane_code_kernel, dim3(qb, nb), dim3(MT_THREADS), 0, st, static_cast<const char *>(tree), plan.stride, depth, src, T, (int)N,
                       blocks, w.blk, w.codes, w.cnt);
    pt_scan_launch<PtCount, false>(PtCount{w.cnt}, leaf, B, blocks, w, w.doff, reinterpret_cast<int32_t *>(ws), PT_W_TOTAL, st);
    hipLaunchKernelGGL(pt_zero_kernel, dim3(blocks_of(leaf, MT_THREADS), nb), dim3(MT_THREADS), 0, st, blocks, w.blk, w.cnt, leaf);
    hipLaunchKernelGGL(pt_lane_fill_kernel, dim3(qb, nb), dim3(MT_THREADS), 0, st, blocks, w.blk, w.codes, w.doff, w.cnt, (int)N, perm);
}

__attribute__((visibility("hidden")))
void pt_query_enqueue(const PtQueryPlan &plan, const void *tree, const double *src, const double *T, double *d2, int32_t *idx, int32_t *stats,
                      const int32_t *perm, const int32_t *done, const int32_t *iter, int it, void *stream) {
    PtBase base;
    for (int l = 0; l <= PT_LEVELS; ++l) base.v[l] = plan.base[l];
    hipLaunchKernelGGL(PT_QUERY[plan.kernel], dim3(blocks_of(plan.N, MT_THREADS), (unsigned)plan.B), dim3(MT_THREADS), 0, (hipStream_t)stream,
                       static_cast<const char *>(tree), plan.stride, plan.pyr, plan.box, plan.loff, plan.list, plan.pts, base, plan.depth, src, T,
                       (int)plan.N, d2, idx, stats, perm, Gate{done, iter, it});
}

extern "C" {

int vt_point_tree_default_depth(int64_t M) {
    int L = 1;
    while (L < VT_WN_MAX_DEPTH && cells_of(L) * 8 < M) ++L;
    return L;
}

size_t vt_point_tree_workspace_bytes(int64_t M, int B, int depth) {
    if (!pt_sizes_ok(M, B) || !pt_depth_ok(depth)) return 0;
    return pt_work(M, B, depth).bytes;
}

int vt_point_tree_count(const double *dst, int64_t M, int B, int depth, void *workspace, size_t workspace_bytes, void *stream) {
    if (!pt_sizes_ok(M, B) || !dst || !workspace) return vt_fail(VT_ERR_INVALID, "vt_point_tree_count: bad argument (M >= 1, 1 <= B <= 65535)");
    if (!pt_depth_ok(depth)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_tree_count: depth outside [1, 7]");
    const PtWork w = pt_work(M, B, depth);
    if (workspace_bytes < w.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_point_tree_count: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    int32_t *state = reinterpret_cast<int32_t *>(ws);
    char *aux = ws + w.aux, *blocks = ws + w.blocks;
    const unsigned nb = (unsigned)B;
    hipLaunchKernelGGL(pt_init_kernel, dim3(nb), dim3(64), 0, st, state, aux);
    const unsigned mb = blocks_of(M, MT_THREADS);
    hipLaunchKernelGGL(pt_bbox_kernel, dim3(mb < 1024u ? mb : 1024u, nb), dim3(MT_THREADS), 0, st, dst, M, state, aux);
    hipLaunchKernelGGL(pt_frame_kernel, dim3(nb), dim3(1), 0, st, aux);
    const int64_t leaf = cells_of(depth);
    hipLaunchKernelGGL(pt_zero_kernel, dim3(blocks_of(leaf, MT_THREADS), nb), dim3(MT_THREADS), 0, st, blocks, w.blk, w.cnt, leaf);
    hipLaunchKernelGGL(pt_code_kernel, dim3(mb, nb), dim3(MT_THREADS), 0, st, dst, (int)M, depth, (const char *)aux, blocks, w.blk, w.codes, w.cnt);
    for (int l = depth; l >= 0; --l) {
        const size_t lv = w.pyr + (size_t)pyr_off(l) * 4;
        if (l == depth) pt_scan_launch<PtLeafOcc, true>(PtLeafOcc{w.cnt}, cells_of(l), B, blocks, w, lv, state, PT_W_COUNT + l, st);
        else pt_scan_launch<PtInnerOcc, true>(PtInnerOcc{w.pyr + (size_t)pyr_off(l + 1) * 4}, cells_of(l), B, blocks, w, lv, state, PT_W_COUNT + l, st);
    }
    pt_scan_launch<PtCount, false>(PtCount{w.cnt}, leaf, B, blocks, w, w.doff, state, PT_W_TOTAL, st);
    return vt_check(hipGetLastError(), "vt_point_tree_count");
}

int vt_point_tree_layout(int64_t M, int depth, int B, const int32_t *state_host, size_t *offsets) {
    if (!pt_sizes_ok(M, B) || !state_host || !offsets) return vt_fail(VT_ERR_INVALID, "vt_point_tree_layout: bad argument (M >= 1, 1 <= B <= 65535)");
    if (!pt_depth_ok(depth)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_tree_layout: depth outside [1, 7]");
    PtTree t;
    if (!pt_tree(M, depth, B, state_host, t)) return vt_fail(VT_ERR_INVALID, "vt_point_tree_layout: counts that no tree of this size has");
    offsets[0] = t.pyr; offsets[1] = t.box; offsets[2] = t.loff; offsets[3] = t.list; offsets[4] = t.pts; offsets[5] = t.stride; offsets[6] = t.bytes;
    return 0;
}

int vt_point_tree_build(const double *dst, int64_t M, int B, int depth, const int32_t *state_host, void *workspace, size_t workspace_bytes, void *tree,
                        size_t tree_bytes, void *stream) {
    if (!pt_sizes_ok(M, B) || !dst || !state_host || !workspace || !tree)
        return vt_fail(VT_ERR_INVALID, "vt_point_tree_build: bad argument (M >= 1, 1 <= B <= 65535)");
    if (!pt_depth_ok(depth)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_tree_build: depth outside [1, 7]");
    for (int b = 0; b < B; ++b)
        if (state_host[(size_t)b * PT_STATE] != 0) return vt_fail(VT_ERR_INVALID, "vt_point_tree_build: a target coordinate is not finite");
    PtTree t;
    if (!pt_tree(M, depth, B, state_host, t)) return vt_fail(VT_ERR_INVALID, "vt_point_tree_build: counts that no tree of this size has");
    const PtWork w = pt_work(M, B, depth);
    if (workspace_bytes < w.bytes || tree_bytes < t.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_point_tree_build: workspace or tree too small");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace), *tr = static_cast<char *>(tree);
    const int32_t *state = reinterpret_cast<const int32_t *>(ws);
    char *aux = ws + w.aux, *blocks = ws + w.blocks;
    const unsigned nb = (unsigned)B, mb = blocks_of(M, MT_THREADS);
    const int64_t words = pyr_off(depth + 1), leaf = cells_of(depth);
    const size_t pyr_leaf = t.pyr + (size_t)pyr_off(depth) * 4;
    hipLaunchKernelGGL(pt_header_kernel, dim3(blocks_of(words, MT_THREADS), nb), dim3(MT_THREADS), 0, st, (const char *)aux, (const char *)blocks, w.blk,
                       w.pyr, words, t.base, depth, (int)M, tr, t.stride, t.pyr);
    hipLaunchKernelGGL(pt_list_offsets_kernel, dim3(blocks_of(leaf, MT_THREADS), nb), dim3(MT_THREADS), 0, st, state, (const char *)blocks, w.blk, w.doff,
                       leaf, depth, (int)M, tr, t.stride, pyr_leaf, t.loff);
    hipLaunchKernelGGL(pt_zero_kernel, dim3(blocks_of(leaf, MT_THREADS), nb), dim3(MT_THREADS), 0, st, blocks, w.blk, w.cnt, leaf);
    hipLaunchKernelGGL(pt_fill_kernel, dim3(mb, nb), dim3(MT_THREADS), 0, st, blocks, w.blk, w.codes, w.doff, w.cnt, w.tmp, (int)M);
    hipLaunchKernelGGL(pt_rank_kernel, dim3(mb, nb), dim3(MT_THREADS), 0, st, dst, (int)M, (const char *)blocks, w.blk, w.codes, w.doff, w.cnt, w.tmp, tr,
                       t.stride, t.list, t.pts);
    hipLaunchKernelGGL(pt_leaf_box_kernel, dim3(blocks_of(leaf, MT_THREADS), nb), dim3(MT_THREADS), 0, st, tr, t.stride, pyr_leaf, leaf, t.loff, t.pts,
                       t.box + (size_t)t.base.v[depth] * PT_BOX * sizeof(double));
    for (int l = depth - 1; l >= 0; --l)
        hipLaunchKernelGGL(pt_inner_box_kernel, dim3(blocks_of(cells_of(l), MT_THREADS), nb), dim3(MT_THREADS), 0, st, tr, t.stride,
                           t.pyr + (size_t)pyr_off(l) * 4, t.pyr + (size_t)pyr_off(l + 1) * 4, cells_of(l),
                           t.box + (size_t)t.base.v[l + 1] * PT_BOX * sizeof(double), t.box + (size_t)t.base.v[l] * PT_BOX * sizeof(double));
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
