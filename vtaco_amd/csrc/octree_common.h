// The octree over items binned by a point.  The build half, for B problems by one set of launches, is what winding_fast.hip (faces binned
// by their centroid, B = 1) and point_tree.hip (points binned by themselves) share; the query half is what the five kernels that read a
// built tree share (winding_fast.hip, closest_point_tree.hip, ray_mesh.hip, point_tree.hip, knn.hip).  The definitions are DESIGN.md's
// section "octree_common.h".  Everything lives in an unnamed namespace: each translation unit has its own copy.
//   frame     lo = the minimum corner of the source's coordinates, side = their largest extent (1 when 0), n = 2^depth cells per axis,
//             1 <= depth <= 7.  A coordinate that is not finite sets status bit 1 and is left out
//   binning   an item lives in the leaf clamp((int)floor((p - lo) / side * n), 0, n - 1) per axis of its point p; cells are numbered in
//             Morton order (bit 3k of a cell number is bit k of ix, 3k+1 of iy, 3k+2 of iz): the children of cell m at level l are
//             8m .. 8m+7 at level l + 1
//   pyramid   per level a dense int32 [8^l]: the rank of an occupied cell among its level's occupied cells, or -1
//   lists     count, scan, fill through an integer cursor, then every item is placed at its rank inside its leaf: ascending index.  The
//             source's payload of an item is written at the item's place: a leaf's payloads are contiguous
//   walk      one lane per query, depth first without a stack (ot_walk): the state is (level, cell), "next" is cell + 1 climbing one
//             level while cell % 8 == 0, "descend" is (level + 1, 8 cell).  The children of a cell are read as k ^ o, o an octant chosen
//             at the descent (0: Morton order) and kept per level, 3 bits each, in `flip`; "next" and "climb" act on k.  What is done at
//             an occupied cell and which octant comes first are the caller's two lambdas; OtView and OtSide are what they read
// A source S is a small struct passed by value to the kernels; it is all that differs between two trees:
//   coords(), coord(b, i, a)      the coordinates that span the frame of problem b, as doubles, and how many there are per problem
//   frame_lo(x)                   what is stored for a minimum x (the place where a source may turn a -0.0 into +0.0)
//   items(), point(b, i, p)       the point item i of problem b is binned by, and how many items there are per problem
//   PAYLOAD, payload(b, i, slot)  the bytes per item in list order, and their writer
// A source that only bins (point_tree.hip's lane order) has items() and point() alone.
// Per problem the workspace starts with 16 int32 state words (0 status, 1..8 the occupied cells of level 0..7, 10 the list scan's total):
// the one host read of a build, between ot_count_enqueue and ot_build_enqueue, is the caller's.  Neither function allocates, copies to
// the host or waits.  No float atomic, no sort: the trees are equal from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_common.h"
#include "vtaco_hip.h"

namespace {

constexpr int OT_LEVELS = VT_WN_MAX_DEPTH + 1;
constexpr size_t OT_HEAD = 256;                 // tree header: lo[3], side (doubles at 0), record base per level (int32 at byte 64), depth, items
constexpr int OT_STATE = 16;                    // int32 per problem: 0 status, 1..8 occupied cells of level 0..7, 10 the list scan's total
constexpr int OT_W_COUNT = 1;
constexpr int OT_W_TOTAL = 10;
constexpr int OT_BAD_COORD = 1;                 // status bit: a coordinate that is not finite
constexpr size_t OT_AUX = 128;                  // bytes per problem: the bounding box as ordered keys (6 u64), at byte 64 lo[3] and side
constexpr size_t OT_AUX_FRAME = 64;
constexpr int OT_BOX = 6;                       // doubles per box (48 bytes: 16-byte aligned rows): lo[3], hi[3]
constexpr size_t OT_SIDE_HEAD = 256;            // bytes in front of a side buffer's boxes; the status word is the first

int64_t cells_of(int l) { return (int64_t)1 << (3 * l); }
int64_t pyr_off(int l) { return (cells_of(l) - 1) / 7; }     // cells of the levels above l

// where level l starts among a tree's per-cell records, in records
struct OtBase { int v[OT_LEVELS + 1]; };

__device__ inline unsigned ot_spread(unsigned x) {          // bit k -> bit 3k, 7 bits
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < VT_WN_MAX_DEPTH; ++k) r |= ((x >> k) & 1u) << (3 * k);
    return r;
}
__device__ inline unsigned ot_gather(unsigned m) {          // bit 3k -> bit k, 7 bits
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < VT_WN_MAX_DEPTH; ++k) r |= ((m >> (3 * k)) & 1u) << k;
    return r;
}

// the leaf of a point: a NaN becomes cell 0, +-inf the first or the last cell
__device__ inline unsigned ot_code(double x, double y, double z, const double *frame, int L) {
    const int n = 1 << L;
    const double p[3] = {x, y, z};
    unsigned code = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double g = floor((p[a] - frame[a]) / frame[3] * (double)n);
        g = g > 0.0 ? g : 0.0;
        g = g < (double)(n - 1) ? g : (double)(n - 1);
        code |= ot_spread((unsigned)(int)g) << a;
    }
    return code;
}

int ot_default_depth(int64_t items) {           // the smallest depth in [1, 7] with 8^depth * 8 >= items
    int L = 1;
    while (L < VT_WN_MAX_DEPTH && cells_of(L) * 8 < items) ++L;
    return L;
}

// workspace: the state words of all problems, their aux blocks, then one block per problem.  codes, cnt, doff and bsum are what a
// count / scan / fill needs; `lists` adds what a tree's pyramids and ranked lists need behind them
struct OtWork { size_t aux, blocks, blk, codes, cnt, doff, bsum, pyr, tmp, bytes; };
OtWork ot_work(int64_t items, int B, int L, bool lists = true) {
    OtWork w;
    const size_t leaf = (size_t)cells_of(L);
    w.aux = up256((size_t)B * OT_STATE * 4);
    w.blocks = w.aux + up256((size_t)B * OT_AUX);
    w.codes = 0;
    w.cnt = w.codes + up256((size_t)items * 4);
    w.doff = w.cnt + up256(leaf * 4);
    w.bsum = w.doff + up256(leaf * 4);
    w.pyr = w.bsum + scan_bytes((int64_t)leaf);
    w.tmp = w.pyr + (lists ? up256((size_t)pyr_off(L + 1) * 4) : 0);
    w.blk = w.tmp + (lists ? up256((size_t)items * 4) : 0);
    w.bytes = w.blocks + (size_t)B * w.blk;
    return w;
}

// the trees: one stride per problem, every array at one offset in all of them.  A level's records have room for the largest count of
// that level over the batch: base.v[l] is where level l starts, in records of rec_doubles doubles.  false: counts that no tree has
struct OtTree { size_t pyr, rec, loff, list, payload, stride, bytes; OtBase base; };
bool ot_tree(int64_t items, int L, int B, const int32_t *state, int rec_doubles, size_t payload_bytes, OtTree &t) {
    int64_t total = 0, leaves = 0;
    for (int l = 0; l < OT_LEVELS; ++l) {
        t.base.v[l] = (int)total;
        if (l > L) continue;
        int64_t cap = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t c = state[(size_t)b * OT_STATE + OT_W_COUNT + l];
            if (c < 0 || c > cells_of(l) || c > items) return false;
            cap = c > cap ? c : cap;
        }
        total += cap;
        if (l == L) leaves = cap;
    }
    t.base.v[OT_LEVELS] = (int)total;
    if (total > 0x7fffffff) return false;
    t.pyr = OT_HEAD;
    t.rec = t.pyr + up256((size_t)pyr_off(L + 1) * 4);
    t.loff = t.rec + up256((size_t)total * rec_doubles * sizeof(double));
    t.list = t.loff + up256((size_t)(leaves + 1) * 4);
    t.payload = t.list + up256((size_t)items * 4);
    t.stride = t.payload + up256((size_t)items * payload_bytes);
    t.bytes = (size_t)B * t.stride;
    return true;
}

template <class T>
__device__ inline T *blk_at(char *blocks, size_t blk, int b, size_t off) { return reinterpret_cast<T *>(blocks + (size_t)b * blk + off); }
template <class T>
__device__ inline const T *blk_at(const char *blocks, size_t blk, int b, size_t off) {
    return reinterpret_cast<const T *>(blocks + (size_t)b * blk + off);
}

// ---- query: a built tree as a kernel reads it, and the walk ---------------------------------------------------------------------------
// where a tree keeps its arrays (OtTree's offsets, one set for all problems), and tree b of a buffer through them.  recs: the per-cell
// records (a point tree's boxes, a face tree's expansions), level l from record base l on; payload: P per item in list order
struct OtAt { size_t stride, pyr, rec, loff, list, payload; };
template <class P>
struct OtView { const double *frame, *recs; const int32_t *pyr, *loff, *list; const P *payload; };
template <class P>
__device__ __forceinline__ OtView<P> ot_view(const char *trees, const OtAt &at, int b) {
    return {blk_at<double>(trees, at.stride, b, 0), blk_at<double>(trees, at.stride, b, at.rec), blk_at<int32_t>(trees, at.stride, b, at.pyr),
            blk_at<int32_t>(trees, at.stride, b, at.loff), blk_at<int32_t>(trees, at.stride, b, at.list), blk_at<P>(trees, at.stride, b, at.payload)};
}

// the side buffer closest_point_tree.hip puts beside a face tree and ray_mesh.hip reads too: OT_SIDE_HEAD bytes whose first word is the status,
// one box per occupied cell (level l from box base.v[l] on, in the order of the tree's records), rec_doubles doubles per face in list
// order.  state: vt_winding_tree_count's words, validated by vt_winding_tree_layout first
struct OtSide { size_t box, rec, bytes; OtBase base; };
struct OtSideView { const double *boxes, *recs; };
__device__ __forceinline__ OtSideView ot_side_view(const char *side, const OtSide &s) {
    return {reinterpret_cast<const double *>(side + s.box), reinterpret_cast<const double *>(side + s.rec)};
}
void ot_side(int64_t F, int L, const int32_t *state, int rec_doubles, OtSide &s) {
    int64_t total = 0;
    for (int l = 0; l < OT_LEVELS; ++l) {
        s.base.v[l] = (int)total;
        if (l <= L) total += state[OT_W_COUNT + l];
    }
    s.base.v[OT_LEVELS] = (int)total;
    s.box = OT_SIDE_HEAD;
    s.rec = s.box + up256((size_t)total * OT_BOX * sizeof(double));
    s.bytes = s.rec + up256((size_t)F * rec_doubles * sizeof(double));
}

// the walk of the header comment over the pyramids pyr.  visit(level, rk) is called for every occupied cell (rk >= 0) in the order the
// cells are read and says whether to descend: it tests, counts and evaluates a leaf itself, and returns false at a leaf.
// octant(level, actual), called on a descent only, is the 3-bit o the children of cell `actual` are read with: k ^ o
template <class Visit, class Octant>
__device__ __forceinline__ void ot_walk(const int32_t *pyr, Visit visit, Octant octant) {
    int level = 0;
    unsigned cell = 0, flip = 0, level_at = 0;                    // level_at = (8^level - 1) / 7; flip: the octant o of every level, 3 bits each
    for (;;) {
        const unsigned actual = cell ^ flip;
        const int rk = pyr[level_at + actual];
        if (rk >= 0 && visit(level, rk)) {
            const unsigned o = octant(level, actual);
            level_at = level_at * 8 + 1; ++level; cell *= 8; flip = flip * 8 + o;
        } else {
            ++cell;
            while (level > 0 && (cell & 7u) == 0) { cell >>= 3; flip >>= 3; --level; level_at = (level_at - 1) >> 3; }
            if (level == 0) break;
        }
    }
}

// near children first: the octant of q about the centre flo_a + (i_a + 0.5) (fside / 2^level) of cell `actual`; 0 when !ORDER
template <bool ORDER>
__device__ __forceinline__ unsigned ot_near_octant(const double *flo, double fside, int level, unsigned actual, const double *q) {
    unsigned o = 0;
    if (ORDER) {
        const double h = fside * (1.0 / (double)(1 << level));
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double centre = flo[a] + ((double)ot_gather(actual >> a) + 0.5) * h;
            o |= q[a] >= centre ? 1u << a : 0u;
        }
    }
    return o;
}

// the squared distance from q to the box lo[3], hi[3]: e_a = max(lo_a - q_a, 0, q_a - hi_a), that is lo_a - q_a when q_a < lo_a,
// q_a - hi_a when q_a > hi_a, else 0 (a NaN q_a: 0; an empty box, lo = +inf, hi = -inf: +inf), summed in the operation order of
// d2 = (dx dx + dy dy) + dz dz.  Without a branch: the box's six doubles are read at once, not one after the other's comparison
__device__ __forceinline__ double ot_box_d2(const double *box, const double *q) {
    double e[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double x = box[a] - q[a];
        x = x > 0.0 ? x : 0.0;
        const double y = q[a] - box[3 + a];
        e[a] = y > x ? y : x;
    }
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// the rank of the leaf q is binned into (ot_code: clamped into the frame), or -1 where that leaf is empty
__device__ __forceinline__ int ot_leaf_of(const int32_t *pyr, const double *frame, int L, const double *q) {
    return pyr[(unsigned)((((int64_t)1 << (3 * L)) - 1) / 7) + ot_code(q[0], q[1], q[2], frame, L)];
}

// (m_x + m_y) + m_z, m_a = max(|p_a - lo_a|, |p_a - (lo_a + side)|): no point of the frame is further from p along any axis sum
__device__ __forceinline__ double ot_frame_reach(const double *frame, const double *p) {
    double S = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double u = fabs(p[a] - frame[a]), v = fabs(p[a] - (frame[a] + frame[3]));
        const double m = u > v ? u : v;
        S = a == 0 ? m : S + m;
    }
    return S;
}

// ---- count: frame, codes, pyramids, list offsets -----------------------------------------------------------------------------------
// grid (B)
__global__ void ot_init_kernel(int32_t *state, char *aux) {
    const int b = blockIdx.x;
    if (threadIdx.x < OT_STATE) state[(size_t)b * OT_STATE + threadIdx.x] = 0;
    u64 *keys = reinterpret_cast<u64 *>(aux + (size_t)b * OT_AUX);
    if (threadIdx.x < 3) keys[threadIdx.x] = ~0ull;              // minima
    else if (threadIdx.x < 6) keys[threadIdx.x] = 0ull;          // maxima
}

// grid (blocks, B).  Minimum and maximum do not round: any order gives the same bits
template <class S>
__global__ void __launch_bounds__(MT_THREADS) ot_bbox_kernel(S src, int32_t *state, char *aux) {
    __shared__ double lds[6][MT_THREADS];
    const int b = blockIdx.y;
    const int64_t n = src.coords();
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    bool bad = false;
    for (int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x; m < n; m += (int64_t)gridDim.x * MT_THREADS) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = src.coord(b, m, a);
            if (!(fabs(x) < __builtin_inf())) { bad = true; continue; }
            lo[a] = x < lo[a] ? x : lo[a];
            hi[a] = x > hi[a] ? x : hi[a];
        }
    }
    if (bad) atomicOr(state + (size_t)b * OT_STATE, OT_BAD_COORD);
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
    u64 *keys = reinterpret_cast<u64 *>(aux + (size_t)b * OT_AUX);
    if (threadIdx.x < 3) atomicMin(keys + threadIdx.x, key_of(lds[threadIdx.x][0]));
    else if (threadIdx.x < 6) atomicMax(keys + threadIdx.x, key_of(lds[threadIdx.x][0]));
}

// grid (B), one thread
template <class S>
__global__ void ot_frame_kernel(S src, char *aux) {
    const int b = blockIdx.x;
    const u64 *keys = reinterpret_cast<const u64 *>(aux + (size_t)b * OT_AUX);
    double *frame = reinterpret_cast<double *>(aux + (size_t)b * OT_AUX + OT_AUX_FRAME);
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = src.frame_lo(value_of(keys[a])), hi = value_of(keys[3 + a]);
        frame[a] = lo;
        const double e = hi - lo;
        ext = e > ext ? e : ext;
    }
    frame[3] = ext > 0.0 ? ext : 1.0;
}

// grid (blocks, B): n int32 words at `off` of every block
__global__ void __launch_bounds__(MT_THREADS) ot_zero_kernel(char *blocks, size_t blk, size_t off, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < n) blk_at<int32_t>(blocks, blk, blockIdx.y, off)[i] = 0;
}

// grid (blocks, B): the leaf of every item in the frame of its problem (frames + b frame_stride: lo[3], side), and the leaves' counts
template <class S>
__global__ void __launch_bounds__(MT_THREADS)
ot_code_kernel(S src, int L, const char *frames, size_t frame_stride, char *blocks, size_t blk, size_t codes_off, size_t cnt_off) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= src.items()) return;
    double p[3];
    src.point(b, i, p);
    const unsigned code = ot_code(p[0], p[1], p[2], reinterpret_cast<const double *>(frames + (size_t)b * frame_stride), L);
    blk_at<int32_t>(blocks, blk, b, codes_off)[i] = (int32_t)code;
    atomicAdd(blk_at<int32_t>(blocks, blk, b, cnt_off) + code, 1);
}

// what a scan adds per element: 1 for an occupied cell (the pyramids), or the cell's count (the list offsets)
struct OtLeafOcc {
    size_t cnt_off;
    __device__ int operator()(const char *block, int64_t i) const { return reinterpret_cast<const int32_t *>(block + cnt_off)[i] > 0 ? 1 : 0; }
};
struct OtInnerOcc {
    size_t child_off;                                            // the finished pyramid of the level below
    __device__ int operator()(const char *block, int64_t i) const {
        const int32_t *child = reinterpret_cast<const int32_t *>(block + child_off);
        int all = -1;
#pragma unroll
        for (int k = 0; k < 8; ++k) all &= child[8 * i + k];
        return all >= 0 ? 1 : 0;                                 // any child's rank is not negative
    }
};
struct OtCount {
    size_t cnt_off;
    __device__ int operator()(const char *block, int64_t i) const { return reinterpret_cast<const int32_t *>(block + cnt_off)[i]; }
};

// mesh_common.h's three-phase exclusive scan, of values, with the problem in blockIdx.y.  grid (chunks, B)
template <class P>
__global__ void __launch_bounds__(MT_THREADS) ot_scan_count_kernel(P val, int64_t n, char *blocks, size_t blk, size_t bsum_off) {
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
__global__ void __launch_bounds__(MT_THREADS) ot_scan_blocks_kernel(char *blocks, size_t blk, size_t bsum_off, int nb, int32_t *state, int word) {
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
    if (threadIdx.x == 0) state[(size_t)blockIdx.x * OT_STATE + word] = carry;
}

// grid (chunks, B).  MARK: an element that adds nothing gets -1 (a pyramid's empty cell)
template <class P, bool MARK>
__global__ void __launch_bounds__(MT_THREADS) ot_scan_write_kernel(P val, int64_t n, char *blocks, size_t blk, size_t bsum_off, size_t pos_off) {
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
void ot_scan_launch(P val, int64_t n, int B, char *blocks, const OtWork &w, size_t pos_off, int32_t *state, int word, hipStream_t st) {
    const unsigned nb = blocks_of(n, MT_CHUNK);
    hipLaunchKernelGGL(ot_scan_count_kernel<P>, dim3(nb, (unsigned)B), dim3(MT_THREADS), 0, st, val, n, blocks, w.blk, w.bsum);
    hipLaunchKernelGGL(ot_scan_blocks_kernel, dim3((unsigned)B), dim3(MT_THREADS), 0, st, blocks, w.blk, w.bsum, (int)nb, state, word);
    hipLaunchKernelGGL((ot_scan_write_kernel<P, MARK>), dim3(nb, (unsigned)B), dim3(MT_THREADS), 0, st, val, n, blocks, w.blk, w.bsum, pos_off);
}

// ---- build: header, lists, payloads in list order ------------------------------------------------------------------------------------
// grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS)
ot_header_kernel(const char *aux, const char *blocks, size_t blk, size_t pyr_off_ws, int64_t words, OtBase base, int L, int items, char *trees,
                 size_t stride, size_t pyr_at) {
    const int b = blockIdx.y;
    char *tree = trees + (size_t)b * stride;
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < words) reinterpret_cast<int32_t *>(tree + pyr_at)[i] = blk_at<int32_t>(blocks, blk, b, pyr_off_ws)[i];
    if (i == 0) {
        const double *frame = reinterpret_cast<const double *>(aux + (size_t)b * OT_AUX + OT_AUX_FRAME);
        double *head = reinterpret_cast<double *>(tree);
#pragma unroll
        for (int k = 0; k < 4; ++k) head[k] = frame[k];
        int32_t *hb = reinterpret_cast<int32_t *>(tree + 64);
#pragma unroll
        for (int k = 0; k <= OT_LEVELS; ++k) hb[k] = base.v[k];
        hb[16] = L; hb[17] = items;
    }
}

// grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS)
ot_list_offsets_kernel(const int32_t *state, const char *blocks, size_t blk, size_t doff_off, int64_t cells, int L, int items, char *trees,
                       size_t stride, size_t pyr_leaf_at, size_t loff_at) {
    const int b = blockIdx.y;
    char *tree = trees + (size_t)b * stride;
    const int32_t *pyr_leaf = reinterpret_cast<const int32_t *>(tree + pyr_leaf_at);
    int32_t *loff = reinterpret_cast<int32_t *>(tree + loff_at);
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m == 0) loff[state[(size_t)b * OT_STATE + OT_W_COUNT + L]] = items;
    if (m < cells && pyr_leaf[m] >= 0) loff[pyr_leaf[m]] = blk_at<int32_t>(blocks, blk, b, doff_off)[m];
}

// grid (blocks, B): item i goes to the next free place of its leaf, in int32 [items] at out + b out_stride.  Inside a leaf the order is
// the cursor's: a permutation whatever it is
__global__ void __launch_bounds__(MT_THREADS) ot_fill_kernel(char *blocks, size_t blk, size_t codes_off, size_t doff_off, size_t cursor_off,
                                                             int items, char *out, size_t out_stride) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= items) return;
    const int code = blk_at<int32_t>(blocks, blk, b, codes_off)[i];
    const int at = blk_at<int32_t>(blocks, blk, b, doff_off)[code] + atomicAdd(blk_at<int32_t>(blocks, blk, b, cursor_off) + code, 1);
    blk_at<int32_t>(out, out_stride, b, 0)[at] = (int32_t)i;
}

// an item's place in its leaf is the number of that leaf's items below it: the lists end ascending however the cursor filled them.
// grid (blocks, B)
template <class S>
__global__ void __launch_bounds__(MT_THREADS)
ot_rank_kernel(S src, const char *blocks, size_t blk, size_t codes_off, size_t doff_off, size_t cursor_off, size_t tmp_off, char *trees,
               size_t stride, size_t list_at, size_t payload_at) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= src.items()) return;
    const int code = blk_at<int32_t>(blocks, blk, b, codes_off)[i];
    const int o = blk_at<int32_t>(blocks, blk, b, doff_off)[code], n = blk_at<int32_t>(blocks, blk, b, cursor_off)[code];
    const int32_t *tmp = blk_at<int32_t>(blocks, blk, b, tmp_off);
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += tmp[o + j] < (int32_t)i ? 1 : 0;
    const size_t at = (size_t)o + rank;
    char *tree = trees + (size_t)b * stride;
    reinterpret_cast<int32_t *>(tree + list_at)[at] = (int32_t)i;
    src.payload(b, i, tree + payload_at + at * S::PAYLOAD);
}

// boxes (lo[3], hi[3]: OT_BOX doubles) of the occupied cells of one level from those of their occupied children, the pyramids at
// trees + b stride and the boxes at boxes + b box_stride.  grid (blocks, B)
__global__ void __launch_bounds__(MT_THREADS)
ot_inner_box_kernel(const char *trees, size_t stride, size_t pyr_at, size_t pyr_child_at, int64_t cells, char *boxes, size_t box_stride,
                    size_t box_child_at, size_t box_level_at) {
    const int64_t m = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (m >= cells) return;
    const int rk = blk_at<int32_t>(trees, stride, blockIdx.y, pyr_at)[m];
    if (rk < 0) return;
    const int32_t *pyr_child = blk_at<int32_t>(trees, stride, blockIdx.y, pyr_child_at);
    const double *box_child = blk_at<double>(boxes, box_stride, blockIdx.y, box_child_at);
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    for (int k = 0; k < 8; ++k) {
        const int ck = pyr_child[8 * m + k];
        if (ck < 0) continue;
        const double *c = box_child + (size_t)ck * OT_BOX;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = c[a] < lo[a] ? c[a] : lo[a];
            hi[a] = c[3 + a] > hi[a] ? c[3 + a] : hi[a];
        }
    }
    double *bx = blk_at<double>(boxes, box_stride, blockIdx.y, box_level_at) + (size_t)rk * OT_BOX;
#pragma unroll
    for (int a = 0; a < 3; ++a) { bx[a] = lo[a]; bx[3 + a] = hi[a]; }
}

// ---- the launch sequences ---------------------------------------------------------------------------------------------------------------
// the leaf of every item and the leaves' counts (frames: ot_code_kernel's)
template <class S>
void ot_code_enqueue(const S &src, int B, int L, const char *frames, size_t frame_stride, const OtWork &w, char *blocks, hipStream_t st) {
    const unsigned nb = (unsigned)B;
    const int64_t leaf = cells_of(L);
    hipLaunchKernelGGL(ot_zero_kernel, dim3(blocks_of(leaf, MT_THREADS), nb), dim3(MT_THREADS), 0, st, blocks, w.blk, w.cnt, leaf);
    hipLaunchKernelGGL(ot_code_kernel<S>, dim3(blocks_of(src.items(), MT_THREADS), nb), dim3(MT_THREADS), 0, st, src, L, frames, frame_stride, blocks,
                       w.blk, w.codes, w.cnt);
}

// the items in leaf order (after ot_code_enqueue and the OtCount scan into doff), in int32 [items] at out + b out_stride
void ot_fill_enqueue(int items, int B, int L, const OtWork &w, char *blocks, char *out, size_t out_stride, hipStream_t st) {
    const unsigned nb = (unsigned)B;
    const int64_t leaf = cells_of(L);
    hipLaunchKernelGGL(ot_zero_kernel, dim3(blocks_of(leaf, MT_THREADS), nb), dim3(MT_THREADS), 0, st, blocks, w.blk, w.cnt, leaf);
    hipLaunchKernelGGL(ot_fill_kernel, dim3(blocks_of(items, MT_THREADS), nb), dim3(MT_THREADS), 0, st, blocks, w.blk, w.codes, w.doff, w.cnt, items,
                       out, out_stride);
}

// the count phase: the state words of every problem, and in the workspace the codes, the pyramids and the list offsets by cell.  With
// no item only the state is initialised
template <class S>
void ot_count_enqueue(const S &src, int B, int L, const OtWork &w, char *ws, hipStream_t st) {
    int32_t *state = reinterpret_cast<int32_t *>(ws);
    char *aux = ws + w.aux, *blocks = ws + w.blocks;
    const unsigned nb = (unsigned)B;
    hipLaunchKernelGGL(ot_init_kernel, dim3(nb), dim3(64), 0, st, state, aux);
    if (src.items() == 0) return;
    const unsigned cb = blocks_of(src.coords(), MT_THREADS);
    hipLaunchKernelGGL(ot_bbox_kernel<S>, dim3(cb < 1024u ? cb : 1024u, nb), dim3(MT_THREADS), 0, st, src, state, aux);
    hipLaunchKernelGGL(ot_frame_kernel<S>, dim3(nb), dim3(1), 0, st, src, aux);
    ot_code_enqueue(src, B, L, aux + OT_AUX_FRAME, OT_AUX, w, blocks, st);
    for (int l = L; l >= 0; --l) {
        const size_t lv = w.pyr + (size_t)pyr_off(l) * 4;
        if (l == L) ot_scan_launch<OtLeafOcc, true>(OtLeafOcc{w.cnt}, cells_of(l), B, blocks, w, lv, state, OT_W_COUNT + l, st);
        else ot_scan_launch<OtInnerOcc, true>(OtInnerOcc{w.pyr + (size_t)pyr_off(l + 1) * 4}, cells_of(l), B, blocks, w, lv, state, OT_W_COUNT + l, st);
    }
    ot_scan_launch<OtCount, false>(OtCount{w.cnt}, cells_of(L), B, blocks, w, w.doff, state, OT_W_TOTAL, st);
}

// the build phase, after the caller read the state words and laid the trees out with them: header, pyramids, list offsets, lists and
// payloads of every tree.  The per-cell records are the caller's, after this
template <class S>
void ot_build_enqueue(const S &src, int B, int L, const OtWork &w, char *ws, const OtTree &t, char *trees, hipStream_t st) {
    const int32_t *state = reinterpret_cast<const int32_t *>(ws);
    char *aux = ws + w.aux, *blocks = ws + w.blocks;
    const unsigned nb = (unsigned)B;
    const int items = src.items();
    const int64_t words = pyr_off(L + 1), leaf = cells_of(L);
    hipLaunchKernelGGL(ot_header_kernel, dim3(blocks_of(words, MT_THREADS), nb), dim3(MT_THREADS), 0, st, (const char *)aux, (const char *)blocks, w.blk,
                       w.pyr, words, t.base, L, items, trees, t.stride, t.pyr);
    hipLaunchKernelGGL(ot_list_offsets_kernel, dim3(blocks_of(leaf, MT_THREADS), nb), dim3(MT_THREADS), 0, st, state, (const char *)blocks, w.blk, w.doff,
                       leaf, L, items, trees, t.stride, t.pyr + (size_t)pyr_off(L) * 4, t.loff);
    ot_fill_enqueue(items, B, L, w, blocks, blocks + w.tmp, w.blk, st);
    hipLaunchKernelGGL(ot_rank_kernel<S>, dim3(blocks_of(items, MT_THREADS), nb), dim3(MT_THREADS), 0, st, src, (const char *)blocks, w.blk, w.codes,
                       w.doff, w.cnt, w.tmp, trees, t.stride, t.list, t.payload);
}

}  // namespace
