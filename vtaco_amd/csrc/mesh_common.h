// What the mesh and octree kernel files share (DESIGN.md, section "mesh_common.h and mesh_edges.h"): the launch constants, faces through
// LDS, the exclusive prefix scan of int32 or 64-bit values, the per-(wave, key) combination in front of an atomic, the order-preserving
// integer image of a double, the two-limb fixed-point sums, and the host's word copy and status read.  The edge table is in mesh_edges.h.
// Everything lives in an unnamed namespace: each translation unit has its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstddef>
#include <type_traits>

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

// ---- exclusive prefix scan of fn(i) over [0, n) -----------------------------------------------------------------------------------------
// S is the summed type, int32_t or u64 (two 32-bit fields scanned at once), taken from the pointers; fn returns the value, and a
// predicate's bool counts as 0 or 1.
template <class S>
__device__ inline S block_inclusive_scan(S x, S *lds) {
    __syncthreads();
    lds[threadIdx.x] = x;
    __syncthreads();
    for (int d = 1; d < MT_THREADS; d <<= 1) {
        const S y = (int)threadIdx.x >= d ? lds[threadIdx.x - d] : 0;
        __syncthreads();
        lds[threadIdx.x] += y;
        __syncthreads();
    }
    return lds[threadIdx.x];
}

template <class Fn, class S>
__global__ void __launch_bounds__(MT_THREADS) scan_count_kernel(Fn fn, int64_t n, S *bsum) {
    __shared__ S lds[MT_THREADS];
    const int64_t i0 = (int64_t)blockIdx.x * MT_CHUNK + (int64_t)threadIdx.x * MT_ITEMS;
    S s = 0;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) s += i0 + k < n ? (S)fn(i0 + k) : 0;
    const S incl = block_inclusive_scan(s, lds);
    if (threadIdx.x == MT_THREADS - 1) bsum[blockIdx.x] = incl;
}

// one workgroup: bsum[0..nb) becomes its exclusive scan, *total the sum
template <class S>
__global__ void __launch_bounds__(MT_THREADS) scan_blocks_kernel(S *bsum, int nb, S *total) {
    __shared__ S lds[MT_THREADS];
    S carry = 0;
    for (int base = 0; base < nb; base += MT_THREADS) {
        const int i = base + (int)threadIdx.x;
        const S x = i < nb ? bsum[i] : 0;
        const S incl = block_inclusive_scan(x, lds);
        if (i < nb) bsum[i] = carry + incl - x;
        carry += lds[MT_THREADS - 1];
    }
    if (threadIdx.x == 0) *total = carry;
}

template <class Fn, class S, class Copy>
__global__ void __launch_bounds__(MT_THREADS) scan_write_kernel(Fn fn, int64_t n, const S *bsum, S *out, Copy copy) {
    __shared__ S lds[MT_THREADS];
    const int64_t i0 = (int64_t)blockIdx.x * MT_CHUNK + (int64_t)threadIdx.x * MT_ITEMS;
    S x[MT_ITEMS];
    S s = 0;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) { x[k] = i0 + k < n ? (S)fn(i0 + k) : 0; s += x[k]; }
    S at = bsum[blockIdx.x] + block_inclusive_scan(s, lds) - s;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        if (i0 + k < n) {
            out[i0 + k] = at;
            if constexpr (!std::is_same<Copy, std::nullptr_t>::value) copy[i0 + k] = at;
        }
        at += x[k];
    }
}

// out[i] = the sum of fn(j) over j < i; *total = the sum over all.  copy: a second S * that gets out's words in the same launch, or
// nullptr for none (the literal: its type decides, so a scan without a copy carries no test for one).
// bsum: blocks_of(n, MT_CHUNK) words of S (scan_bytes<S>).
template <class Fn, class S, class Copy = std::nullptr_t>
void scan_launch(Fn fn, int64_t n, S *bsum, S *out, S *total, hipStream_t st, Copy copy = nullptr) {
    const unsigned nb = blocks_of(n, MT_CHUNK);
    hipLaunchKernelGGL((scan_count_kernel<Fn, S>), dim3(nb), dim3(MT_THREADS), 0, st, fn, n, bsum);
    hipLaunchKernelGGL(scan_blocks_kernel<S>, dim3(1), dim3(MT_THREADS), 0, st, bsum, (int)nb, total);
    hipLaunchKernelGGL((scan_write_kernel<Fn, S, Copy>), dim3(nb), dim3(MT_THREADS), 0, st, fn, n, (const S *)bsum, out, copy);
}

template <class S = int32_t>
size_t scan_bytes(int64_t n) { return up256((size_t)blocks_of(n, MT_CHUNK) * sizeof(S)); }

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

// ---- host helpers ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT_THREADS) copy_words_kernel(const uint32_t *src, int64_t n, uint32_t *dst) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// bytes / 4 dwords from src to dst, on the stream (a launch like its neighbours: no host-side copy engine in between)
void copy_words(const void *src, size_t bytes, void *dst, hipStream_t st) {
    const int64_t n = (int64_t)(bytes / 4);
    if (n) hipLaunchKernelGGL(copy_words_kernel, dim3(blocks_of(n, MT_THREADS)), dim3(MT_THREADS), 0, st, static_cast<const uint32_t *>(src), n,
                              static_cast<uint32_t *>(dst));
}

// the first N status words of a workspace to the host: one copy, one wait
template <int N>
int read_status(const void *workspace, int32_t (&h)[N], hipStream_t st, const char *where) {
    hipError_t e = hipMemcpyAsync(h, workspace, sizeof h, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return vt_check(e, where);
}

}  // namespace
