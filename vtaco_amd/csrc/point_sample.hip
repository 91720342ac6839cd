// Point-feature sampler of the PointConv baseline's decoder for gfx950 (reference src/conv_onet/models/decoder.py:468-485
// sample_point_feature): every query takes the normalised kernel-weighted sum of the per-point features over the whole cloud,
//     c_m = sum_n w[m,n] fea_n / sum_n w[m,n],   w = exp(-(|p_n - q_m| + 10e-6)^2 / var)  or  1 / (|p_n - q_m| + 10e-6),
// and its backward to the features.  Nothing of size [M,N] is stored.
//
//   forward   out^T [C x 32 queries] = fea^T [C x N] W^T [N x 32] on the exact-f32 matrix instruction (v_mfma_f32_32x32x2_f32): a
//             lane is (query l & 31, cloud point 2 s + (l >> 5)) of k-step s, so it computes exactly the one weight the
//             instruction's B operand wants from it -- a square root and an exponential per lane per 64 matrix cycles -- and
//             reads the A operand (one feature row, 32 channels) from the LDS tile its workgroup staged.  Four waves = 128
//             queries per workgroup; up to four 32-channel blocks per workgroup, the rest over gridDim.y.
//             Gaussian mode is the shifted quotient: a first pass over the cloud finds the query's nearest point, its exponent is
//             subtracted before every exponential.  Where the reference's sum underflows to 0 (nearest point beyond ~10
//             gaussian_val) and it returns NaN, this returns the finite limit; everywhere else the two agree.
//   lattice   the queries box * make_3d_grid(...)[first : first + count] are generated in the kernel (point_of): the same
//             coordinates, hence the same bits as the point form.
//   backward  grad_fea^T [C x 32 cloud points] = grad_c^T [C x M] What [M x 32], What = w / sum recomputed from the saved shift and
//             sum with the forward's own arithmetic.  The queries go in chunks of 512 to separate workgroups, each chunk's partial
//             sum into the workspace, and a last pass adds the chunks in ascending order: no float atomics, the same bits every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "decode_common.h"
#include "points_launch.h"

namespace {

using namespace vt_points;

// ((dx dx + dy dy) + dz dz), the association the geometric stages use too (pointnetpp.hip)
__device__ __forceinline__ float dist2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// the exponent of the Gaussian weight at distance d: -(d + 10e-6)^2 / var
__device__ __forceinline__ float gauss_exponent(float d, float neg_inv_var) {
    const float t = d + 1e-5f;
    return (t * t) * neg_inv_var;
}

// the un-normalised weight at distance d; `shift`: the query's largest exponent (0 in the inverse-distance mode)
__device__ __forceinline__ float weight_of(float d, bool gaussian, float neg_inv_var, float shift) {
    if (gaussian) return expf(gauss_exponent(d, neg_inv_var) - shift);
    return 1.0f / (d + 1e-5f);
}

__device__ __forceinline__ f32x16 div16(const f32x16 &v, float s) {
    f32x16 r;
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = v[i] / s;
    return r;
}

struct SampleArgs {
    DecodeArgs d;            // pts / N (= M, queries per scene) / total / lattice_first / nx / box: the queries (point_of)
    const float *cloud;      // [B][N][3]
    const float *fea;        // [B][N][C]
    float *out;              // [B][M][C]
    float *shift, *sum;      // [B][M]
    uint32_t M, N;
    int C, gaussian;
    float neg_inv_var;
};

constexpr int STAT_TILE = 256;       // cloud points per step of the nearest-point pass

template <int NCB>
__global__ void __launch_bounds__(256)
point_sample_fwd_kernel(SampleArgs a) {
    __shared__ __attribute__((aligned(16))) float sfea[TILE_K][NCB * 32];
    __shared__ float spts[STAT_TILE * 3];
    const int tid = threadIdx.x, lane = tid & 63, l32 = lane & 31, half = lane >> 5, wave = tid >> 6;
    const uint32_t b = blockIdx.z, cg = blockIdx.y, M = a.M, N = a.N;
    const uint32_t m = blockIdx.x * ROWS_PER_BLOCK + wave * ROWS_PER_WAVE + l32;
    const uint32_t mc = m < M ? m : M - 1;                       // lanes past the end compute the last query and write nothing
    const bool gaussian = a.gaussian != 0;
    float qx, qy, qz;
    point_of(a.d, b * M + mc, mc, qx, qy, qz);
    const float *cloud = a.cloud + (size_t)b * N * 3;
    const float *fea = a.fea + (size_t)b * N * a.C + (size_t)cg * NCB * 32;

    float shift = 0.0f;
    if (gaussian) {
        // the nearest cloud point: sqrt, + 10e-6, the square and the scaling are monotone, so its exponent is the largest
        float dmin = __builtin_inff();
        for (uint32_t n0 = 0; n0 < N; n0 += STAT_TILE) {
            __syncthreads();
            for (uint32_t i = tid; i < STAT_TILE * 3; i += 256) {
                const uint64_t idx = (uint64_t)n0 * 3 + i;
                spts[i] = idx < (uint64_t)N * 3 ? cloud[idx] : 0.0f;
            }
            __syncthreads();
            const uint32_t cnt = min((uint32_t)STAT_TILE, N - n0);
            for (uint32_t j = half; j < cnt; j += 2) dmin = fminf(dmin, dist2(spts[3 * j], spts[3 * j + 1], spts[3 * j + 2], qx, qy, qz));
        }
        dmin = fminf(dmin, __shfl_xor(dmin, 32));
        shift = gauss_exponent(sqrtf(dmin), a.neg_inv_var);
    }

    f32x16 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
    float sum = 0.0f;
    for (uint32_t n0 = 0; n0 < N; n0 += TILE_K) {
        __syncthreads();
        for (int i = tid; i < TILE_K * NCB * 8; i += 256) {
            const int row = i / (NCB * 8), c4 = i - row * (NCB * 8);
            const uint32_t n = n0 + row;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};                  // rows past the cloud: a zero operand under a zero weight
            if (n < N) v = reinterpret_cast<const f32x4 *>(fea + (size_t)n * a.C)[c4];
            reinterpret_cast<f32x4 *>(&sfea[row][0])[c4] = v;
        }
        if (tid < TILE_K * 3) {
            const uint64_t idx = (uint64_t)n0 * 3 + tid;
            spts[tid] = idx < (uint64_t)N * 3 ? cloud[idx] : 0.0f;
        }
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < TILE_K / 2; ++s) {
            const int j = 2 * s + half;
            const float d = sqrtf(dist2(spts[3 * j], spts[3 * j + 1], spts[3 * j + 2], qx, qy, qz));
            float w = weight_of(d, gaussian, a.neg_inv_var, shift);
            w = (n0 + j < N) ? w : 0.0f;
            sum += w;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma(sfea[j][cb * 32 + l32], w, acc[cb]);
        }
    }
    sum += __shfl_xor(sum, 32);                                  // even + odd cloud points: the query's whole sum, in both halves
    if (m < M) {
        const size_t g = (size_t)b * M + m;
        float *row = a.out + g * a.C + (size_t)cg * NCB * 32;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) store_acc16(row + cb * 32, div16(acc[cb], sum), half);
        if (cg == 0 && half == 0) { a.shift[g] = shift; a.sum[g] = sum; }
    }
}

struct SampleBwdArgs {
    const float *q;          // [B][M][3]
    const float *cloud;      // [B][N][3]
    const float *shift, *sum;    // [B][M]
    const float *grad_c;     // [B][M][C]
    float *dst;              // grad_fea [B][N][C], or with more than one chunk the partial sums [chunks][B][N][C]
    uint32_t M, N, B;
    int C, gaussian, groups, chunks;
    float neg_inv_var;
};

template <int NCB>
__global__ void __launch_bounds__(256)
point_sample_bwd_kernel(SampleBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float sgc[TILE_K][NCB * 32];
    __shared__ float sq[TILE_K * 3], sshift[TILE_K], ssum[TILE_K];
    const int tid = threadIdx.x, lane = tid & 63, l32 = lane & 31, half = lane >> 5, wave = tid >> 6;
    const uint32_t b = blockIdx.z, chunk = blockIdx.y / a.groups, cg = blockIdx.y - chunk * a.groups, M = a.M, N = a.N;
    const uint32_t n = blockIdx.x * ROWS_PER_BLOCK + wave * ROWS_PER_WAVE + l32;
    const uint32_t nc = n < N ? n : N - 1;
    const bool gaussian = a.gaussian != 0;
    const float *pp = a.cloud + ((size_t)b * N + nc) * 3;
    const float px = pp[0], py = pp[1], pz = pp[2];
    const uint32_t lo = chunk * BWD_CHUNK, hi = min(lo + (uint32_t)BWD_CHUNK, M);
    const float *gc = a.grad_c + (size_t)b * M * a.C + (size_t)cg * NCB * 32;
    const size_t qbase = (size_t)b * M;

    f32x16 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
    for (uint32_t m0 = lo; m0 < hi; m0 += TILE_K) {
        __syncthreads();
        for (int i = tid; i < TILE_K * NCB * 8; i += 256) {
            const int row = i / (NCB * 8), c4 = i - row * (NCB * 8);
            const uint32_t m = m0 + row;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (m < hi) v = reinterpret_cast<const f32x4 *>(gc + (size_t)m * a.C)[c4];
            reinterpret_cast<f32x4 *>(&sgc[row][0])[c4] = v;
        }
        if (tid < TILE_K * 3) {
            const uint32_t m = m0 + tid / 3;
            sq[tid] = m < hi ? a.q[(qbase + m0) * 3 + tid] : 0.0f;
        } else if (tid >= 128 && tid < 128 + TILE_K) {
            const uint32_t m = m0 + (tid - 128);
            sshift[tid - 128] = m < hi ? a.shift[qbase + m] : 0.0f;
            ssum[tid - 128] = m < hi ? a.sum[qbase + m] : 1.0f;
        }
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < TILE_K / 2; ++s) {
            const int j = 2 * s + half;
            const float d = sqrtf(dist2(px, py, pz, sq[3 * j], sq[3 * j + 1], sq[3 * j + 2]));
            float w = weight_of(d, gaussian, a.neg_inv_var, sshift[j]) / ssum[j];
            w = (m0 + j < hi) ? w : 0.0f;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma(sgc[j][cb * 32 + l32], w, acc[cb]);
        }
    }
    if (n < N) {
        float *row = a.dst + (((size_t)chunk * a.B + b) * N + n) * a.C + (size_t)cg * NCB * 32;      // chunk = 0 when there is one
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) store_acc16(row + cb * 32, acc[cb], half);
    }
}

// grad_fea = the chunks' partial sums added in ascending chunk order
__global__ void __launch_bounds__(256)
point_sample_reduce_kernel(const float *part, float *out, uint64_t floats4, int chunks) {
    const f32x4 *p = reinterpret_cast<const f32x4 *>(part);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < floats4; i += (uint64_t)gridDim.x * 256) {
        f32x4 v = p[i];
        for (int k = 1; k < chunks; ++k) v = v + p[(uint64_t)k * floats4 + i];
        reinterpret_cast<f32x4 *>(out)[i] = v;
    }
}

int sample_check(const char *who, int B, int64_t M, int64_t N, int C, double gaussian_val, int gaussian) {
    char msg[160];
    auto fail = [&](int code, const char *what) { snprintf(msg, sizeof msg, "%s: %s", who, what); return vt_fail(code, msg); };
    if (B <= 0 || M < 0 || N < 1) return fail(VT_ERR_INVALID, "bad size (B >= 1, M >= 0, N >= 1)");
    if (!c_ok(C)) return fail(VT_ERR_UNSUPPORTED, "c_dim must be a multiple of 32, at most 256");
    if ((int64_t)B * M >= (int64_t)1 << 31 || (int64_t)B * N >= (int64_t)1 << 31) return fail(VT_ERR_UNSUPPORTED, "B*M and B*N must be < 2^31");
    if (gaussian && !(gaussian_val > 0.0)) return fail(VT_ERR_INVALID, "gaussian mode needs gaussian_val > 0");
    return 0;
}

// -1 / var with var = gaussian_val^2 rounded to f32 as torch rounds the scalar it divides an f32 tensor by
float neg_inv_var_of(double gaussian_val) {
    const float var = (float)(gaussian_val * gaussian_val);
    return (float)(-1.0 / (double)var);
}

}  // namespace

extern "C" {

int vt_point_sample_fwd(const float *q, int64_t M, int lattice_nx, float lattice_box, int64_t lattice_first,
                        const float *cloud, const float *fea, int B, int64_t N, int C, int gaussian, double gaussian_val,
                        float *out, float *shift, float *sum, void *stream) {
    int rc = sample_check("vt_point_sample_fwd", B, M, N, C, gaussian_val, gaussian);
    if (rc) return rc;
    if (!cloud || !fea || !out || !shift || !sum) return vt_fail(VT_ERR_INVALID, "vt_point_sample_fwd: null argument");
    if (((uintptr_t)fea | (uintptr_t)out) & 15) return vt_fail(VT_ERR_INVALID, "vt_point_sample_fwd: fea and out must be 16-byte aligned");
    if (!q && !lattice_ok(lattice_nx, lattice_first, M)) return vt_fail(VT_ERR_INVALID, "vt_point_sample_fwd: lattice range outside nx^3 (2 <= nx <= 1625)");
    if (M == 0) return 0;
    const Channels ch = channels_of(C);
    const int64_t tiles = row_tiles(M);
    if (!grid_ok(tiles, ch.groups, B)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_sample_fwd: B above 65535");
    SampleArgs a{};
    a.d.pts = q; a.d.N = (uint32_t)M; a.d.total = (uint32_t)((int64_t)B * M); a.d.lattice_first = (uint32_t)lattice_first;
    a.d.nx = lattice_nx; a.d.box = lattice_box;
    a.cloud = cloud; a.fea = fea; a.out = out; a.shift = shift; a.sum = sum;
    a.M = (uint32_t)M; a.N = (uint32_t)N; a.C = C; a.gaussian = gaussian ? 1 : 0;
    a.neg_inv_var = gaussian ? neg_inv_var_of(gaussian_val) : 0.0f;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)ch.groups, (unsigned)B);
    switch (ch.ncb) {
        case 4: hipLaunchKernelGGL(point_sample_fwd_kernel<4>, grid, dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(point_sample_fwd_kernel<3>, grid, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL(point_sample_fwd_kernel<2>, grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(point_sample_fwd_kernel<1>, grid, dim3(256), 0, s, a); break;
    }
    return vt_check(hipGetLastError(), "vt_point_sample_fwd");
}

size_t vt_point_sample_bwd_workspace_bytes(int B, int64_t M, int64_t N, int C) {
    return bwd_workspace_bytes(B, M, N, C);
}

int vt_point_sample_bwd(const float *q, int64_t M, const float *cloud, int B, int64_t N, int C, int gaussian, double gaussian_val,
                        const float *shift, const float *sum, const float *grad_c, float *grad_fea,
                        void *workspace, size_t workspace_bytes, void *stream) {
    int rc = sample_check("vt_point_sample_bwd", B, M, N, C, gaussian_val, gaussian);
    if (rc) return rc;
    if (!cloud || !grad_fea || (M > 0 && (!q || !shift || !sum || !grad_c))) return vt_fail(VT_ERR_INVALID, "vt_point_sample_bwd: null argument");
    if (((uintptr_t)grad_c | (uintptr_t)grad_fea | (uintptr_t)workspace) & 15)
        return vt_fail(VT_ERR_INVALID, "vt_point_sample_bwd: grad_c, grad_fea and workspace must be 16-byte aligned");
    const size_t need = bwd_workspace_bytes(B, M, N, C);
    if (need && (!workspace || workspace_bytes < need))
        return vt_fail(VT_ERR_WORKSPACE, "vt_point_sample_bwd: workspace too small (vt_point_sample_bwd_workspace_bytes)");
    const Channels ch = channels_of(C);
    const int64_t chunks = bwd_chunks(M), tiles = row_tiles(N);
    if (!grid_ok(tiles, chunks * ch.groups, B)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_sample_bwd: B or M / 512 x C / 32 above 65535");
    SampleBwdArgs a{};
    a.q = q; a.cloud = cloud; a.shift = shift; a.sum = sum; a.grad_c = grad_c;
    a.dst = chunks > 1 ? (float *)workspace : grad_fea;
    a.M = (uint32_t)M; a.N = (uint32_t)N; a.B = (uint32_t)B; a.C = C; a.gaussian = gaussian ? 1 : 0; a.groups = ch.groups; a.chunks = (int)chunks;
    a.neg_inv_var = gaussian ? neg_inv_var_of(gaussian_val) : 0.0f;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)(chunks * ch.groups), (unsigned)B);      // M == 0: one chunk of no queries writes zeros
    switch (ch.ncb) {
        case 4: hipLaunchKernelGGL(point_sample_bwd_kernel<4>, grid, dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(point_sample_bwd_kernel<3>, grid, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL(point_sample_bwd_kernel<2>, grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(point_sample_bwd_kernel<1>, grid, dim3(256), 0, s, a); break;
    }
    if (chunks > 1) {
        const uint64_t floats4 = (uint64_t)B * N * C / 4;
        uint64_t blocks = (floats4 + 255) / 256;
        const uint64_t cap = (uint64_t)16 * vt_num_cus();
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(point_sample_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float *)workspace, grad_fea, floats4, (int)chunks);
    }
    return vt_check(hipGetLastError(), "vt_point_sample_bwd");
}

}  // extern "C"
