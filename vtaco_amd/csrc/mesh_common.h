// What mesh_topo.hip and mesh_simplify.hip share: the launch constants, faces through LDS, the exclusive prefix scan of a predicate, the
// per-(wave, key) combination in front of an atomic, the order-preserving integer image of a double and the two-limb fixed-point sums.
// Everything lives in an unnamed namespace: each translation unit has its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vt_common.h"

namespace {

typedef unsigned long long u64;

constexpr int MT_THREADS = 256;
constexpr int MT_ITEMS = 4;                      // faces / vertices per thread of the stats passes, elements per thread of a scan
constexpr int MT_CHUNK = MT_THREADS * MT_ITEMS;
constexpr int MT_ROUND_BATCH = 2;                // hooking rounds enqueued per read of their flags
constexpr size_t MT_STATUS_BYTES = 256;          // int32 words at the start of every workspace: see the enum
constexpr int64_t MT_MAX_V = 0x7fffff00;
constexpr int64_t MT_MAX_F = 0x1fffff00;         // 3 F and the 4 F table slots stay below 2^31


size_t up256(size_t x) { return (x + 255) / 256 * 256; }
unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// ---- faces through LDS: contiguous dword reads of the 12-byte records ----------------------------------------------------------
// face blockIdx.x * 256 + threadIdx.x; false past the end.  `ok` is false when an index lies outside [0, V).
__device__ inline bool load_face(const int32_t *faces, int F, int V, int32_t *lds, int &f, int &a, int &b, int &c, bool &ok) {
    const int64_t base = (int64_t)blockIdx.x * MT_THREADS;
    const int cnt = (int)min((int64_t)MT_THREADS, (int64_t)F - base);
    for (int i = threadIdx.x; i < cnt * 3; i += MT_THREADS) lds[i] = faces[base * 3 + i];
    __syncthreads();
    const bool in = (int)threadIdx.x < cnt;
    f = (int)base + (int)threadIdx.x;
    a = b = c = 0;
    ok = false;
    if (in) {
        a = lds[3 * threadIdx.x]; b = lds[3 * threadIdx.x + 1]; c = lds[3 * threadIdx.x + 2];
        ok = (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;
    }
    return in;
}

// ---- exclusive prefix scan of a predicate over [0, n) ---------------------------------------------------------------------------------
__device__ inline int block_inclusive_scan(int x, int *lds) {
    __syncthreads();
    lds[threadIdx.x] = x;
    __syncthreads();
    for (int d = 1; d < MT_THREADS; d <<= 1) {
        const int y = (int)threadIdx.x >= d ? lds[threadIdx.x - d] : 0;
        __syncthreads();
        lds[threadIdx.x] += y;
        __syncthreads();
    }
    return lds[threadIdx.x];
}

template <class P>
__global__ void __launch_bounds__(MT_THREADS) scan_count_kernel(P pred, int64_t n, int32_t *bsum) {
    __shared__ int lds[MT_THREADS];
    const int64_t i0 = (int64_t)blockIdx.x * MT_CHUNK + (int64_t)threadIdx.x * MT_ITEMS;
    int s = 0;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) s += (i0 + k < n && pred(i0 + k)) ? 1 : 0;
    const int incl = block_inclusive_scan(s, lds);
    if (threadIdx.x == MT_THREADS - 1) bsum[blockIdx.x] = incl;
}

// one workgroup: bsum[0..nb) becomes its exclusive scan, *total the sum
__global__ void __launch_bounds__(MT_THREADS) scan_blocks_kernel(int32_t *bsum, int nb, int32_t *total) {
    __shared__ int lds[MT_THREADS];
    int carry = 0;
    for (int base = 0; base < nb; base += MT_THREADS) {
        const int i = base + (int)threadIdx.x;
        const int x = i < nb ? bsum[i] : 0;
        const int incl = block_inclusive_scan(x, lds);
        if (i < nb) bsum[i] = carry + incl - x;
        carry += lds[MT_THREADS - 1];
    }
    if (threadIdx.x == 0) *total = carry;
}

template <class P>
__global__ void __launch_bounds__(MT_THREADS) scan_write_kernel(P pred, int64_t n, const int32_t *bsum, int32_t *pos) {
    __shared__ int lds[MT_THREADS];
    const int64_t i0 = (int64_t)blockIdx.x * MT_CHUNK + (int64_t)threadIdx.x * MT_ITEMS;
    int fl[MT_ITEMS];
    int s = 0;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) { fl[k] = (i0 + k < n && pred(i0 + k)) ? 1 : 0; s += fl[k]; }
    int at = bsum[blockIdx.x] + block_inclusive_scan(s, lds) - s;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        if (i0 + k < n) pos[i0 + k] = at;
        at += fl[k];
    }
}

// pos[i] = the number of j < i with pred(j); *total = the number of all.  bsum: blocks_of(n, MT_CHUNK) int32.
template <class P>
void scan_launch(P pred, int64_t n, int32_t *bsum, int32_t *pos, int32_t *total, hipStream_t st) {
    const unsigned nb = blocks_of(n, MT_CHUNK);
    hipLaunchKernelGGL(scan_count_kernel<P>, dim3(nb), dim3(MT_THREADS), 0, st, pred, n, bsum);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(MT_THREADS), 0, st, bsum, (int)nb, total);
    hipLaunchKernelGGL(scan_write_kernel<P>, dim3(nb), dim3(MT_THREADS), 0, st, pred, n, (const int32_t *)bsum, pos);
}

size_t scan_bytes(int64_t n) { return up256((size_t)blocks_of(n, MT_CHUNK) * sizeof(int32_t)); }

// ---- per-(wave, component) combination ------------------------------------------------------------------------------------------------------
// Every lane holds K 64-bit values for component `cur` (cur < 0: nothing).  Lanes with one component are combined by Op and the first of
// them issues the K atomics on table[cur * K + k].  Called by all lanes of the wave.
template <int K, class Op>
__device__ inline void wave_flush(int cur, const u64 (&acc)[K], u64 *table) {
    const int lane = (int)(threadIdx.x & 63);
    bool live = cur >= 0;
    for (;;) {
        const u64 todo = __ballot(live);
        if (todo == 0) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int c0 = __shfl(cur, leader);
        const bool mine = live && cur == c0;
        u64 v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = mine ? acc[k] : Op::identity(k);
        if (__popcll(__ballot(mine)) > 1) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
                for (int k = 0; k < K; ++k) v[k] = Op::combine(k, v[k], __shfl_xor(v[k], d));
        }
        if (lane == leader) {
#pragma unroll
            for (int k = 0; k < K; ++k) Op::atomic(k, table + (size_t)c0 * K + k, v[k]);
        }
        if (mine) live = false;
    }
}

template <int K, class Op>
__device__ inline void lane_flush(int cur, const u64 (&acc)[K], u64 *table) {
#pragma unroll
    for (int k = 0; k < K; ++k) Op::atomic(k, table + (size_t)cur * K + k, acc[k]);
}

// a thread's MT_ITEMS items in turn (item k of a thread is MT_THREADS past item k - 1, so a wave reads contiguous records each time): values
// of one component stay in registers, a change of component flushes them lane by lane
template <int K, class Op>
__device__ inline void accumulate(int &cur, u64 (&acc)[K], int c, const u64 (&x)[K], u64 *table) {
    if (c < 0) return;
    if (c != cur) {
        if (cur >= 0) lane_flush<K, Op>(cur, acc, table);
        cur = c;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = x[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = Op::combine(k, acc[k], x[k]);
}

// order-preserving image of a double (-0.0 below +0.0) and back
__device__ inline u64 key_of(double x) {
    const u64 u = (u64)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double value_of(u64 k) {
    const u64 u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

template <class T>
__device__ inline void load_vertex(const T *verts, int v, double &x, double &y, double &z) {
    const T *p = verts + (size_t)v * 3;
    x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
}

// x as two fixed-point limbs against the exponent e of the component's largest |term| (|x| < 2^(e+1)):
// hi = trunc(x 2^(30-e)), |hi| <= 2^31; lo = rint((x 2^(30-e) - hi) 2^31), |lo| <= 2^31
__device__ inline int exponent_of(u64 bits) {
    const int e = (int)((bits >> 52) & 0x7ff);
    return (e == 0 ? 1 : e) - 1023;
}
__device__ inline void limbs_of(double x, int e, u64 &hi, u64 &lo) {
    const double s = ldexp(x, 30 - e);
    const double h = trunc(s);
    const double l = rint(ldexp(s - h, 31));
    hi = (u64)(long long)h;
    lo = (u64)(long long)l;
}
__device__ inline double sum_of(u64 hi, u64 lo, int e) {
    const double s = (double)(long long)hi + ldexp((double)(long long)lo, -31);
    return ldexp(s, e - 30);
}

}  // namespace
