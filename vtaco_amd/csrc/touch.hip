// Touch session: one touch's tactile assignment MERGED into the id lattice an object keeps across touches (reference
// src/conv_onet/inferencing.py:155-170, 274-313: c_img_all is created at the first touch and every later touch writes its fingers'
// features where its fingers are).  vtaco_amd/conv_onet/inferencing.py drives it.
//
// The session's lattice holds one byte per point: the ROW of the session's feature table (row_base + finger, five rows per touch),
// 255 = no row.  vt_touch_merge evaluates the rule of vt_tactile_assign (tactile_rule.h: the same function, so the same finger,
// bit for bit) at the lattice points and, where it names a finger, stores that touch's row and appends the point to a compacted
// list (lattice id, coordinates): the points whose logit has to be decoded again.  Everything else is left alone.
//
// The list comes out in ASCENDING lattice order on every run -- count, scan, emit:
//   bounds   the lattice index range that can be hit at all: the bounds of the successful fingers' anchors grown by the radius,
//            widened by one index per side (a point outside it is further than the radius from every anchor along one axis)
//   count    per chunk of 1024 consecutive lattice points (256 lanes x 4), the number of hits; chunks outside the range write 0
//            without evaluating anything (at 128^3 a VTacO touch leaves a handful of the 2048 chunks)
//   scan     one workgroup turns the chunk counts into exclusive offsets; the total goes to the caller's device word
//   emit     chunks with hits evaluate the rule again and write ids and list entries at offset + (prefix of the hits inside the
//            chunk: ballots per wave, wave totals through LDS).  No atomics anywhere: the order cannot float.
#include "tactile_rule.h"

namespace {

constexpr int TOUCH_THREADS = 256;
constexpr int TOUCH_PER_LANE = 4;
constexpr int TOUCH_CHUNK = TOUCH_THREADS * TOUCH_PER_LANE;
constexpr int TOUCH_SCAN_THREADS = 1024;
constexpr int TOUCH_WS_HEAD = 8;                                   // ints in front of the chunk counts: the index range (6 used)

struct TouchArgs {
    TactileRule r;
    int nx;
    float box;
    uint32_t total, nchunks;
    int row_base;
    unsigned char *ids;           // [nx^3] in/out
    int *changed_ids;             // [capacity]
    float *changed_pts;           // [capacity][3]
    uint32_t capacity;
    int *count;                   // device word: hits found (may exceed capacity; only the first `capacity` are written)
    int *ws;                      // [0..5] x_lo, x_hi, y_lo, y_hi, z_lo, z_hi; [8 .. 8 + nchunks] chunk counts, then exclusive offsets + total
};

__device__ __forceinline__ DecodeArgs touch_lattice(const TouchArgs &a) {
    DecodeArgs d;
    d.grid = nullptr; d.pts = nullptr; d.c_img = nullptr; d.blob = nullptr; d.out = nullptr; d.out2 = nullptr; d.save = nullptr;
    d.c_direct = nullptr; d.cimg_ids = nullptr; d.cimg_table = nullptr; d.cimg_nf = 0; d.brick = 0; d.N = a.total; d.total = a.total;
    d.lattice_first = 0; d.R = 2; d.nx = a.nx; d.box = a.box; d.divisor = 1.0f; d.status = nullptr; d.clk = nullptr; d.claim = 0;
    return d;
}

// lattice index of coordinate v along one axis, as a double (box * linspace(-0.5, 0.5, nx)[i] ~ v)
__device__ __forceinline__ double touch_index(double v, double box, int nx) { return (v / box + 0.5) * (double)(nx - 1); }

__global__ void __launch_bounds__(TOUCH_THREADS) touch_bounds_kernel(TouchArgs a) {
    __shared__ float fb[VT_TACTILE_MAX_F][6];
    __shared__ int used[VT_TACTILE_MAX_F];
    const int f = (int)threadIdx.x;
    if (f < a.r.F) {
        const int n = a.r.mode == 0 ? 1 : min(a.r.count[f], a.r.K);
        const float *q = a.r.anchors + (size_t)f * a.r.K * 3;
        float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
        for (int k = 0; k < n; ++k)
            for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], q[3 * k + c]); hi[c] = fmaxf(hi[c], q[3 * k + c]); }
        for (int c = 0; c < 3; ++c) { fb[f][c] = lo[c]; fb[f][3 + c] = hi[c]; }
        used[f] = (a.r.success[f] && n > 0) ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
        bool any = false;
        for (int g = 0; g < a.r.F; ++g)
            if (used[g]) {
                any = true;
                for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], fb[g][c]); hi[c] = fmaxf(hi[c], fb[g][3 + c]); }
            }
        const double grow = tactile_grow(a.r), top = (double)(a.nx - 1);
        for (int c = 0; c < 3; ++c) {
            int ilo = 1, ihi = 0;                                   // empty
            if (any) {
                const double dl = floor(touch_index((double)lo[c] - grow, (double)a.box, a.nx)) - 1.0;
                const double dh = ceil(touch_index((double)hi[c] + grow, (double)a.box, a.nx)) + 1.0;
                if (dl <= top && dh >= 0.0 && dl <= dh) {
                    ilo = (int)fmax(dl, 0.0);
                    ihi = (int)fmin(dh, top);
                }
            }
            a.ws[2 * c] = ilo; a.ws[2 * c + 1] = ihi;
        }
    }
}

struct TouchRange {
    int xl, xh, yl, yh, zl, zh;
};

__device__ __forceinline__ TouchRange touch_range(const TouchArgs &a) {
    TouchRange t;
    t.xl = a.ws[0]; t.xh = a.ws[1]; t.yl = a.ws[2]; t.yh = a.ws[3]; t.zl = a.ws[4]; t.zh = a.ws[5];
    return t;
}

// true when no point of the chunk lies in the index range (uniform over the workgroup)
__device__ __forceinline__ bool touch_chunk_outside(const TouchArgs &a, const TouchRange &t, uint32_t chunk) {
    if (t.xl > t.xh || t.yl > t.yh || t.zl > t.zh) return true;
    const uint32_t nx = (uint32_t)a.nx, g0 = chunk * (uint32_t)TOUCH_CHUNK;
    const uint32_t g1 = min(g0 + (uint32_t)TOUCH_CHUNK, a.total) - 1u;
    const int x0 = (int)(g0 / (nx * nx)), x1 = (int)(g1 / (nx * nx));
    if (x1 < t.xl || x0 > t.xh) return true;
    if (x0 == x1) {
        const int y0 = (int)((g0 / nx) % nx), y1 = (int)((g1 / nx) % nx);
        if (y1 < t.yl || y0 > t.yh) return true;
    }
    return false;
}

// the rule at this lane's four points of the chunk: bit j of the result = point base + j takes finger fing[j]
__device__ __forceinline__ unsigned touch_hits(const TouchArgs &a, const TouchRange &t, const DecodeArgs &lat, const float *anc,
                                               const float (*box)[6], uint32_t base, int *fing) {
    const uint32_t nx = (uint32_t)a.nx;
    const double grow = tactile_grow(a.r);
    const uint32_t t0 = base / nx;
    uint32_t z = base - t0 * nx, x = t0 / nx, y = t0 - x * nx;
    unsigned q = 0;
#pragma unroll
    for (int j = 0; j < TOUCH_PER_LANE; ++j) {
        fing[j] = 255;
        if (base + j < a.total && (int)x >= t.xl && (int)x <= t.xh && (int)y >= t.yl && (int)y <= t.yh && (int)z >= t.zl && (int)z <= t.zh) {
            float px, py, pz;
            point_of(lat, base + j, base + j, px, py, pz);
            fing[j] = tactile_finger(a.r, anc, box, grow, px, py, pz);
            if (fing[j] != 255) q |= 1u << j;
        }
        if (++z == nx) { z = 0; if (++y == nx) { y = 0; ++x; } }
    }
    return q;
}

// exclusive prefix of cnt (0..4) over the lanes of the wave, and the wave's total: three ballots (one per bit plane)
__device__ __forceinline__ void touch_wave_prefix(unsigned cnt, unsigned &before, unsigned &sum) {
    const unsigned long long below = (1ull << (threadIdx.x & 63u)) - 1ull;
    before = 0; sum = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const unsigned long long plane = __ballot((cnt >> b) & 1u);
        before += (unsigned)__popcll(plane & below) << b;
        sum += (unsigned)__popcll(plane) << b;
    }
}

__global__ void __launch_bounds__(TOUCH_THREADS) touch_count_kernel(TouchArgs a) {
    extern __shared__ float anc[];
    __shared__ float box[VT_TACTILE_MAX_F][6];
    __shared__ unsigned wsum[TOUCH_THREADS / 64];
    const uint32_t chunk = blockIdx.x;
    const TouchRange t = touch_range(a);
    if (touch_chunk_outside(a, t, chunk)) {                         // the whole workgroup leaves
        if (threadIdx.x == 0) a.ws[TOUCH_WS_HEAD + chunk] = 0;
        return;
    }
    tactile_stage(a.r, anc, box);
    const DecodeArgs lat = touch_lattice(a);
    int fing[TOUCH_PER_LANE];
    const unsigned q = touch_hits(a, t, lat, anc, box, chunk * (uint32_t)TOUCH_CHUNK + threadIdx.x * TOUCH_PER_LANE, fing);
    unsigned before, sum;
    touch_wave_prefix(__popc(q), before, sum);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
        for (int w = 0; w < TOUCH_THREADS / 64; ++w) s += wsum[w];
        a.ws[TOUCH_WS_HEAD + chunk] = (int)s;
    }
}

// ws[8 .. 8 + n): counts -> exclusive offsets; ws[8 + n] and *count: the total
__global__ void __launch_bounds__(TOUCH_SCAN_THREADS) touch_scan_kernel(int *v, uint32_t n, int *count) {
    __shared__ int part[TOUCH_SCAN_THREADS];
    const uint32_t per = (n + TOUCH_SCAN_THREADS - 1) / TOUCH_SCAN_THREADS;
    const uint32_t lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
    int s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += v[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < TOUCH_SCAN_THREADS; off <<= 1) {
        const int add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (uint32_t i = lo; i < hi; ++i) { const int c = v[i]; v[i] = run; run += c; }
    if (threadIdx.x == TOUCH_SCAN_THREADS - 1) { v[n] = part[threadIdx.x]; *count = part[threadIdx.x]; }
}

__global__ void __launch_bounds__(TOUCH_THREADS) touch_emit_kernel(TouchArgs a) {
    extern __shared__ float anc[];
    __shared__ float box[VT_TACTILE_MAX_F][6];
    __shared__ unsigned wsum[TOUCH_THREADS / 64];
    const uint32_t chunk = blockIdx.x;
    const int first = a.ws[TOUCH_WS_HEAD + chunk];
    if (a.ws[TOUCH_WS_HEAD + chunk + 1] == first) return;           // no hit in this chunk: the whole workgroup leaves
    const TouchRange t = touch_range(a);
    tactile_stage(a.r, anc, box);
    const DecodeArgs lat = touch_lattice(a);
    int fing[TOUCH_PER_LANE];
    const uint32_t base = chunk * (uint32_t)TOUCH_CHUNK + threadIdx.x * TOUCH_PER_LANE;
    const unsigned q = touch_hits(a, t, lat, anc, box, base, fing);
    unsigned before, sum;
    touch_wave_prefix(__popc(q), before, sum);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = sum;
    __syncthreads();
    uint32_t slot = (uint32_t)first + before;
    for (unsigned w = 0; w < (threadIdx.x >> 6); ++w) slot += wsum[w];
#pragma unroll
    for (int j = 0; j < TOUCH_PER_LANE; ++j) {
        if ((q >> j) & 1u) {                                        // base + j < total: touch_hits sets no bit past the lattice
            a.ids[base + j] = (unsigned char)(a.row_base + fing[j]);
            if (slot < a.capacity) {                                // past the capacity: counted and merged, not listed
                float px, py, pz;
                point_of(lat, base + j, base + j, px, py, pz);
                a.changed_ids[slot] = (int)(base + j);
                float *o = a.changed_pts + (size_t)slot * 3;
                o[0] = px; o[1] = py; o[2] = pz;
            }
            ++slot;
        }
    }
}

uint32_t touch_chunks(int nx) { return (uint32_t)(((uint64_t)nx * nx * nx + TOUCH_CHUNK - 1) / TOUCH_CHUNK); }

}  // namespace

extern "C" size_t vt_touch_workspace_bytes(int nx) {
    if (nx < 2 || nx > VT_MISE_MAX_N) return 0;
    return ((size_t)TOUCH_WS_HEAD + touch_chunks(nx) + 1) * sizeof(int);
}

extern "C" int vt_touch_merge(const float *anchors, const int *count, const unsigned char *success, int F, int K, int mode, double radius,
                              int nx, float box, int row_base, unsigned char *ids, int *changed_ids, float *changed_pts, int64_t capacity,
                              int *n_changed, void *workspace, size_t workspace_bytes, void *stream) {
    if (!anchors || !count || !success || !ids || !changed_ids || !changed_pts || !n_changed || !workspace)
        return vt_fail(VT_ERR_INVALID, "vt_touch_merge: null argument");
    if (F <= 0 || K <= 0 || row_base < 0 || (mode != 0 && mode != 1)) return vt_fail(VT_ERR_INVALID, "vt_touch_merge: bad argument");
    if (mode == 0 && K != 1) return vt_fail(VT_ERR_INVALID, "vt_touch_merge: nearest-fingertip mode takes one anchor per finger");
    if (nx < 2 || nx > VT_MISE_MAX_N) return vt_fail(VT_ERR_UNSUPPORTED, "vt_touch_merge: nx must be in [2, VT_MISE_MAX_N]");
    if ((int64_t)row_base + F > 254)
        return vt_fail(VT_ERR_UNSUPPORTED, "vt_touch_merge: row_base + F exceeds 254 rows (one byte per point, 255 = no row)");
    if (capacity < 0 || capacity >= ((int64_t)1 << 31)) return vt_fail(VT_ERR_INVALID, "vt_touch_merge: capacity must be in [0, 2^31)");
    const size_t lds = (size_t)F * K * 3 * sizeof(float);
    if (lds > 56 * 1024) return vt_fail(VT_ERR_UNSUPPORTED, "vt_touch_merge: anchor set does not fit 56 KiB of LDS");
    if (workspace_bytes < vt_touch_workspace_bytes(nx)) return vt_fail(VT_ERR_WORKSPACE, "vt_touch_merge: workspace too small (vt_touch_workspace_bytes)");
    TouchArgs a;
    a.r.anchors = anchors; a.r.count = count; a.r.success = success; a.r.F = F; a.r.K = K; a.r.mode = mode; a.r.radius = radius;
    a.nx = nx; a.box = box; a.total = (uint32_t)((uint64_t)nx * nx * nx); a.nchunks = touch_chunks(nx); a.row_base = row_base;
    a.ids = ids; a.changed_ids = changed_ids; a.changed_pts = changed_pts; a.capacity = (uint32_t)capacity; a.count = n_changed;
    a.ws = (int *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(touch_bounds_kernel, dim3(1), dim3(TOUCH_THREADS), 0, st, a);
    int rc = vt_check(hipGetLastError(), "vt_touch_merge: bounds");
    if (rc) return rc;
    hipLaunchKernelGGL(touch_count_kernel, dim3(a.nchunks), dim3(TOUCH_THREADS), lds, st, a);
    rc = vt_check(hipGetLastError(), "vt_touch_merge: count");
    if (rc) return rc;
    hipLaunchKernelGGL(touch_scan_kernel, dim3(1), dim3(TOUCH_SCAN_THREADS), 0, st, a.ws + TOUCH_WS_HEAD, a.nchunks, n_changed);
    rc = vt_check(hipGetLastError(), "vt_touch_merge: scan");
    if (rc) return rc;
    hipLaunchKernelGGL(touch_emit_kernel, dim3(a.nchunks), dim3(TOUCH_THREADS), lds, st, a);
    return vt_check(hipGetLastError(), "vt_touch_merge");
}
