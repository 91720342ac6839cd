// The three geometric stages of the PointNet++ encoder for gfx950 (reference src/encoder/pointnetpp.py:188-232
// farthest_point_sample, query_ball_point; :84-90 the 3-nearest-neighbour weights of PointNetFeaturePropagation).  They produce
// indices and interpolation weights only -- nothing here is differentiated.  Latency class, no MFMA.  Every squared distance is
// ((dx dx + dy dy) + dz dz) of coordinate differences.
//
//   vt_fps         one workgroup of 1024 threads per cloud runs the reference's loop: the running minimum of the distance to the
//                  chosen set (a [B][N] scratch row, each entry owned by one thread), then the arg-max -- per thread, per wave by
//                  shuffles, over the 16 waves through LDS -- with the lowest index among equal maxima (torch.max(dim)).
//   vt_ball_query  one wave per centre walks the cloud 64 points at a time; a ballot and a prefix count place the points in range in
//                  ascending order until nsample are found.  A short row is filled with its first entry, an empty one with 0.
//   vt_three_nn    one thread per target keeps the three smallest distances (strict <: the lowest index among equals) over the
//                  sources, then w_i = (1 / (d_i + 1e-8)) / sum.  With S == 1 that is index 0, weight 1: the reference's repeat.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vt_common.h"

namespace {

__device__ __forceinline__ float dist2(const float *p, float cx, float cy, float cz) {
    const float dx = p[0] - cx, dy = p[1] - cy, dz = p[2] - cz;
    return (dx * dx + dy * dy) + dz * dz;
}

// the larger value, the lower index among equals
__device__ __forceinline__ void take_max(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

constexpr int FPS_THREADS = 1024;

__global__ void __launch_bounds__(FPS_THREADS)
fps_kernel(const float *xyz, const int64_t *start, int N, int npoint, float *dist, int64_t *out) {
    __shared__ float sval[FPS_THREADS / 64];
    __shared__ int sidx[FPS_THREADS / 64];
    __shared__ int sfar;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const float *x = xyz + (size_t)b * N * 3;
    float *dst = dist + (size_t)b * N;
    int64_t *row = out + (size_t)b * npoint;
    for (int i = tid; i < N; i += FPS_THREADS) dst[i] = 1e10f;
    const int64_t s0 = start[b];
    int far = (int)(s0 < 0 ? 0 : (s0 >= N ? N - 1 : s0));        // a start outside the cloud stays in bounds
    for (int it = 0; it < npoint; ++it) {
        if (tid == 0) row[it] = far;
        const float cx = x[3 * far], cy = x[3 * far + 1], cz = x[3 * far + 2];
        float best = -1.0f;
        int bi = 0x7fffffff;
        for (int i = tid; i < N; i += FPS_THREADS) {
            const float d = dist2(x + 3 * (size_t)i, cx, cy, cz), old = dst[i];
            const float nd = d < old ? d : old;
            dst[i] = nd;
            if (nd > best) { best = nd; bi = i; }                // ascending i: the first of equals stays
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) take_max(best, bi, __shfl_xor(best, off), __shfl_xor(bi, off));
        if (lane == 0) { sval[wave] = best; sidx[wave] = bi; }
        __syncthreads();
        if (wave == 0) {
            float v = lane < FPS_THREADS / 64 ? sval[lane] : -1.0f;
            int i = lane < FPS_THREADS / 64 ? sidx[lane] : 0x7fffffff;
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) take_max(v, i, __shfl_xor(v, off), __shfl_xor(i, off));
            if (lane == 0) sfar = (unsigned)i < (unsigned)N ? i : 0;           // (NaN coordinates: no candidate; stay in bounds)
        }
        __syncthreads();
        far = sfar;
    }
}

__global__ void __launch_bounds__(256)
ball_query_kernel(const float *xyz, const float *centres, int B, int N, int S, float r2, int nsample, int64_t *out) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= (int64_t)B * S) return;                             // whole waves leave: the ballots below see full waves
    const int b = (int)(g / S);
    const float *x = xyz + (size_t)b * N * 3, *c = centres + (size_t)g * 3;
    const float cx = c[0], cy = c[1], cz = c[2];
    int64_t *row = out + (size_t)g * nsample;
    int cnt = 0, first = -1;
    for (int n0 = 0; n0 < N && cnt < nsample; n0 += 64) {
        const int n = n0 + lane;
        const bool in = n < N && dist2(x + 3 * (size_t)(n < N ? n : 0), cx, cy, cz) <= r2;
        const unsigned long long mask = __ballot(in);
        const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
        if (in && pos < nsample) row[pos] = n;
        if (first < 0 && mask) first = n0 + (int)__builtin_ctzll(mask);
        cnt += __popcll(mask);
    }
    if (cnt > nsample) cnt = nsample;
    if (first < 0) first = 0;
    for (int j = cnt + lane; j < nsample; j += 64) row[j] = first;
}

__global__ void __launch_bounds__(256)
three_nn_kernel(const float *tgt, const float *src, int B, int N, int S, int k, int64_t *idx, float *weight) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (int64_t)B * N) return;
    const int b = (int)(g / N);
    const float *t = tgt + (size_t)g * 3, *s = src + (size_t)b * S * 3;
    const float tx = t[0], ty = t[1], tz = t[2];
    const float inf = __builtin_inff();
    float d0 = inf, d1 = inf, d2 = inf;
    int i0 = 0, i1 = 0, i2 = 0;
    for (int j = 0; j < S; ++j) {
        const float d = dist2(s + 3 * (size_t)j, tx, ty, tz);
        if (d < d0) { d2 = d1; i2 = i1; d1 = d0; i1 = i0; d0 = d; i0 = j; }
        else if (d < d1) { d2 = d1; i2 = i1; d1 = d; i1 = j; }
        else if (d < d2) { d2 = d; i2 = j; }
    }
    const float r0 = 1.0f / (d0 + 1e-8f), r1 = k > 1 ? 1.0f / (d1 + 1e-8f) : 0.0f, r2 = k > 2 ? 1.0f / (d2 + 1e-8f) : 0.0f;
    const float norm = (r0 + r1) + r2;
    int64_t *io = idx + (size_t)g * k;
    float *wo = weight + (size_t)g * k;
    io[0] = i0; wo[0] = r0 / norm;
    if (k > 1) { io[1] = i1; wo[1] = r1 / norm; }
    if (k > 2) { io[2] = i2; wo[2] = r2 / norm; }
}

}  // namespace

extern "C" {

int vt_fps(const float *xyz, int B, int N, int npoint, const int64_t *start, float *dist_ws, int64_t *out, void *stream) {
    if (!xyz || !start || !dist_ws || !out) return vt_fail(VT_ERR_INVALID, "vt_fps: null argument");
    if (B <= 0 || N <= 0 || npoint <= 0) return vt_fail(VT_ERR_INVALID, "vt_fps: bad size");
    if (N < npoint) return vt_fail(VT_ERR_INVALID, "vt_fps: the cloud has fewer points than npoint");
    if ((int64_t)B * N >= (int64_t)1 << 31) return vt_fail(VT_ERR_UNSUPPORTED, "vt_fps: B*N must be < 2^31");
    hipLaunchKernelGGL(fps_kernel, dim3((unsigned)B), dim3(FPS_THREADS), 0, (hipStream_t)stream, xyz, start, N, npoint, dist_ws, out);
    return vt_check(hipGetLastError(), "vt_fps");
}

int vt_ball_query(const float *xyz, int B, int N, const float *centres, int S, double radius, int nsample, int64_t *out, void *stream) {
    if (!xyz || !centres || !out) return vt_fail(VT_ERR_INVALID, "vt_ball_query: null argument");
    if (B <= 0 || N <= 0 || S <= 0 || nsample <= 0 || !(radius >= 0.0)) return vt_fail(VT_ERR_INVALID, "vt_ball_query: bad size or radius");
    if ((int64_t)B * N >= (int64_t)1 << 31 || (int64_t)B * S >= (int64_t)1 << 31) return vt_fail(VT_ERR_UNSUPPORTED, "vt_ball_query: B*N and B*S must be < 2^31");
    const int64_t blocks = ((int64_t)B * S + 3) / 4;
    hipLaunchKernelGGL(ball_query_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, xyz, centres, B, N, S,
                       (float)(radius * radius), nsample, out);
    return vt_check(hipGetLastError(), "vt_ball_query");
}

int vt_three_nn(const float *tgt, int B, int N, const float *src, int S, int64_t *idx, float *weight, void *stream) {
    if (!tgt || !src || !idx || !weight) return vt_fail(VT_ERR_INVALID, "vt_three_nn: null argument");
    if (B <= 0 || N <= 0 || S <= 0) return vt_fail(VT_ERR_INVALID, "vt_three_nn: bad size");
    if ((int64_t)B * N >= (int64_t)1 << 31 || (int64_t)B * S >= (int64_t)1 << 31) return vt_fail(VT_ERR_UNSUPPORTED, "vt_three_nn: B*N and B*S must be < 2^31");
    const int k = S < 3 ? S : 3;
    const int64_t blocks = ((int64_t)B * N + 255) / 256;
    hipLaunchKernelGGL(three_nn_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tgt, src, B, N, S, k, idx, weight);
    return vt_check(hipGetLastError(), "vt_three_nn");
}

}  // extern "C"
