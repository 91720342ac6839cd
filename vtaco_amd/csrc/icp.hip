// Rigid registration of point sets: the reference's src/utils/icp.py (best_fit_transform :5-47, nearest_neighbor :50-66, icp :69-121) for
// 3-D points, B problems per call.  The definitions are DESIGN.md's section "icp.hip", restated in numpy by tests/icp_ref.py
// (kernel_order: this file's operations in this file's order).  Every number is float64; every product, sum, division and square root
// is a separate IEEE rounding in a fixed order (-ffp-contract=off), and no result goes through an atomic: the outputs are bit-reproducible.
//   moved point   T p = (((T00 x + T01 y) + T02 z) + T03, ...), rows 0..2 of the row-major 4x4 T
//   neighbours    d2 = (dx dx + dy dy) + dz dz with d = p - q, minimum over the targets in ascending order with a strict <: the lowest
//                 index among equal minima.  A workgroup takes 256 queries (one per thread) and one slab of targets, staged through
//                 LDS in chunks of 256 points that every lane of a wave reads at the same address (broadcast); one partial minimum per
//                 (query, slab), a finish pass takes them in ascending slab order.  The result does not depend on the slab size.
//   sums          points are cut into chunks of 256; a chunk's sum is the LDS tree s[t] = s[t] + s[t + h], h = 128, 64, ..., 1 (lanes
//                 past the end hold +0.0); one thread per component adds the chunk sums in ascending chunk order, starting from +0.0
//   fit           centroids = sums / N; H[j][k] = sum (a_j - abar_j)(b_k - bbar_k) by the same two stages; one-sided Jacobi on G = H
//                 (V = I): FIT_SWEEPS sweeps over the column pairs (0,1), (0,2), (1,2): alpha = |g_p|^2, beta = |g_q|^2, gamma = g_p.g_q
//                 ((x x + y y) + z z each); gamma == 0 skips; zeta = (beta - alpha) / (2 gamma), t = 1 / (|zeta| + sqrt(1 + zeta zeta)),
//                 negated for zeta < 0, c = 1 / sqrt(1 + t t), s = c t; g_p, g_q <- c g_p - s g_q, s g_p + c g_q, the same on V's columns.
//                 Columns sorted by squared norm, descending (swaps (0,1), (1,2), (0,1) on a strict <).  U is orthonormal by construction,
//                 whatever H's rank: u_0 = g_0 / sqrt(|g_0|^2) (H == 0: R = I); u_1 = w / sqrt(|w|^2), w = g_1 with w - u_0 (u_0.w)
//                 applied twice (w == 0: the axis of u_0's smallest component, made orthogonal to u_0 once); u_2 = u_0 x u_1, negated
//                 when u_2.g_2 < 0 -- the normalised columns of G wherever those are orthogonal to working precision.
//                 R[r][c] = (V[r][0] U[c][0] + V[r][1] U[c][1]) + V[r][2] U[c][2]; det R < 0 negates V's third column and recomputes R;
//                 t_r = bbar_r - ((R_r0 abar_0 + R_r1 abar_1) + R_r2 abar_2)
//   loop          per iteration: neighbours of the working copy, fit, working copy <- T working copy, then mean = (sum of sqrt(d2),
//                 same two stages) / N and done = |prev - mean| < tolerance, else prev = mean.  Every kernel of iteration `it` returns
//                 at once for a problem with done set in an earlier iteration: its points, distances, indices and counter stay.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp_common.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

constexpr int ICP_THREADS = 256;                // queries per workgroup, points per LDS chunk and per reduction chunk
constexpr int NN_MIN_CHUNKS = 2;                // chunks per slab at least: every target set beyond 256 points walks the re-staging loop
constexpr int NN_TARGET_BLOCKS = 2048;          // workgroups wanted per launch: 8 per CU
constexpr int FIT_SUMS = 8;                     // doubles per chunk of the first stage: sum a (3), sum b (3), sum dist, 0
constexpr int FIT_COV = 9;                      // doubles per chunk of the second stage: H row-major
constexpr int FIT_SWEEPS = 10;                  // Jacobi sweeps (a 3x3 settles in 4 to 6; later sweeps rotate at rounding level or skip)

struct NnPlan { int slab_pts, slabs; size_t pidx_off, block_bytes; };

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

NnPlan nn_plan(int64_t N, int64_t M, int B) {
    const int64_t qtiles = (N + ICP_THREADS - 1) / ICP_THREADS * (B > 0 ? B : 1);
    const int64_t chunks = (M + ICP_THREADS - 1) / ICP_THREADS;
    int64_t want = NN_TARGET_BLOCKS / (qtiles > 0 ? qtiles : 1);
    if (want < 1) want = 1;
    int64_t per = (chunks + want - 1) / want;
    if (per < NN_MIN_CHUNKS) per = NN_MIN_CHUNKS;
    NnPlan p;
    p.slab_pts = (int)(per * ICP_THREADS);
    p.slabs = (int)((chunks + per - 1) / per);
    if (p.slabs < 1) p.slabs = 1;
    p.pidx_off = up256((size_t)N * p.slabs * sizeof(double));
    p.block_bytes = p.pidx_off + up256((size_t)N * p.slabs * sizeof(int32_t));
    return p;
}

// grid (query tiles, slabs, B): partial minimum of 256 queries over one slab of targets
__global__ void __launch_bounds__(ICP_THREADS)
nn_slab_kernel(const double *src, const double *T, const double *dst, int N, int M, char *ws, size_t block_bytes, size_t pidx_off, int slab_pts,
               int slabs, Gate gate) {
    __shared__ double lds[ICP_THREADS * 3];
    const int b = blockIdx.z;
    if (frozen(gate, b)) return;
    const int slab = blockIdx.y;
    const int m_begin = slab * slab_pts;
    if (m_begin >= M) return;                     // (uniform over the workgroup; the finish pass does not read this slab)
    const int m_end = min(M, m_begin + slab_pts);
    const int n = blockIdx.x * ICP_THREADS + threadIdx.x;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (n < N) {
        const double *p = src + ((size_t)b * N + n) * 3;
        px = p[0]; py = p[1]; pz = p[2];
        if (T) move_point(T + (size_t)b * 16, px, py, pz, px, py, pz);
    }
    const double *q = dst + (size_t)b * M * 3;
    double best = __builtin_inf();
    int best_m = -1;
    for (int m0 = m_begin; m0 < m_end; m0 += ICP_THREADS) {
        const int cnt = min(ICP_THREADS, m_end - m0);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt * 3; i += ICP_THREADS) lds[i] = q[(size_t)m0 * 3 + i];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double dx = px - lds[3 * j], dy = py - lds[3 * j + 1], dz = pz - lds[3 * j + 2];
            const double d = (dx * dx + dy * dy) + dz * dz;
            if (d < best) { best = d; best_m = m0 + j; }
        }
    }
    if (n < N) {
        char *block = ws + (size_t)b * block_bytes;
        const size_t at = (size_t)n * slabs + slab;
        reinterpret_cast<double *>(block)[at] = best;
        reinterpret_cast<int32_t *>(block + pidx_off)[at] = best_m;
    }
}

// grid (query tiles, 1, B): a query's partials in ascending slab order
__global__ void __launch_bounds__(ICP_THREADS)
nn_finish_kernel(int N, int M, const char *ws, size_t block_bytes, size_t pidx_off, int slab_pts, int slabs, double *d2, int32_t *idx, Gate gate) {
    const int b = blockIdx.z;
    if (frozen(gate, b)) return;
    const int n = blockIdx.x * ICP_THREADS + threadIdx.x;
    if (n >= N) return;
    const char *block = ws + (size_t)b * block_bytes;
    const double *pd2 = reinterpret_cast<const double *>(block) + (size_t)n * slabs;
    const int32_t *pidx = reinterpret_cast<const int32_t *>(block + pidx_off) + (size_t)n * slabs;
    double best = __builtin_inf();
    int best_m = -1;
    for (int s = 0; s < slabs && (int64_t)s * slab_pts < M; ++s) {
        const double d = pd2[s];
        if (d < best) { best = d; best_m = pidx[s]; }
    }
    d2[(size_t)b * N + n] = best;
    idx[(size_t)b * N + n] = best_m;
}

// the chunk sum of K values per thread: s[k][t] = s[k][t] + s[k][t + h], h = 128 ... 1; thread k < K then writes s[k][0] to out[k]
template <int K>
__device__ inline void tree_sums(double (*s)[ICP_THREADS], double *out) {
    for (int h = ICP_THREADS / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int k = 0; k < K; ++k) s[k][threadIdx.x] = s[k][threadIdx.x] + s[k][threadIdx.x + h];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < K) out[threadIdx.x] = s[threadIdx.x][0];
}

// the partner of point n: b[idx[n]] (an index outside [0, M) is clamped into it, never dereferenced as given), or b[n]
__device__ inline const double *partner(const double *bp, const int32_t *idx, int b, int N, int M, int n) {
    int m = n;
    if (idx) {
        m = idx[(size_t)b * N + n];
        m = m < 0 ? 0 : (m >= M ? M - 1 : m);
    }
    return bp + ((size_t)b * M + m) * 3;
}

// grid (chunks, B): per chunk the sums of a, of the partners and (d2 given) of dist = sqrt(d2), which is also written out
__global__ void __launch_bounds__(ICP_THREADS)
fit_sums_kernel(const double *a, const double *bp, const int32_t *idx, int N, int M, const double *d2, double *dist, double *part, int chunks,
                Gate gate) {
    __shared__ double s[7][ICP_THREADS];
    const int b = blockIdx.y;
    if (frozen(gate, b)) return;
    const int n = blockIdx.x * ICP_THREADS + threadIdx.x;
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n < N) {
        const double *pa = a + ((size_t)b * N + n) * 3;
        const double *pb = partner(bp, idx, b, N, M, n);
        v[0] = pa[0]; v[1] = pa[1]; v[2] = pa[2];
        v[3] = pb[0]; v[4] = pb[1]; v[5] = pb[2];
        if (d2) {
            v[6] = sqrt(d2[(size_t)b * N + n]);
            dist[(size_t)b * N + n] = v[6];
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) s[k][threadIdx.x] = v[k];
    double *out = part + ((size_t)b * chunks + blockIdx.x) * FIT_SUMS;
    tree_sums<7>(s, out);
    if (threadIdx.x == 7) out[7] = 0.0;
}

// component k of the chunk records, added in ascending chunk order from +0.0
__device__ inline double chunk_order_sum(const double *rec, int chunks, int stride, int k) {
    double acc = 0.0;
    for (int c = 0; c < chunks; ++c) acc = acc + rec[(size_t)c * stride + k];
    return acc;
}

// grid (chunks, B): the centroids from the first stage's records, then per chunk the nine sums of H
__global__ void __launch_bounds__(ICP_THREADS)
fit_cov_kernel(const double *a, const double *bp, const int32_t *idx, int N, int M, const double *part, double *cov, int chunks, Gate gate) {
    __shared__ double s[9][ICP_THREADS];
    __shared__ double mean[6];
    const int b = blockIdx.y;
    if (frozen(gate, b)) return;
    if (threadIdx.x < 6) mean[threadIdx.x] = chunk_order_sum(part + (size_t)b * chunks * FIT_SUMS, chunks, FIT_SUMS, threadIdx.x) / (double)N;
    __syncthreads();
    const int n = blockIdx.x * ICP_THREADS + threadIdx.x;
    double aa[3] = {0.0, 0.0, 0.0}, bb[3] = {0.0, 0.0, 0.0};
    const bool in = n < N;
    if (in) {
        const double *pa = a + ((size_t)b * N + n) * 3;
        const double *pb = partner(bp, idx, b, N, M, n);
#pragma unroll
        for (int k = 0; k < 3; ++k) { aa[k] = pa[k] - mean[k]; bb[k] = pb[k] - mean[3 + k]; }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[3 * j + k][threadIdx.x] = in ? aa[j] * bb[k] : 0.0;
    tree_sums<9>(s, cov + ((size_t)b * chunks + blockIdx.x) * FIT_COV);
}

__device__ inline double dot3(const double *u, const double *w) { return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]; }

// R (row-major) from H (row-major) by the one-sided Jacobi rule of the file's head
__device__ void kabsch_rotation(const double *H, double *R) {
    double g[3][3], v[3][3];                      // columns: g[j] = G's column j, v[j] = V's column j
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) { g[j][i] = H[3 * i + j]; v[j][i] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < FIT_SWEEPS; ++sweep) {
        for (int pair = 0; pair < 3; ++pair) {
            const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
            const double alpha = dot3(g[p], g[p]), beta = dot3(g[q], g[q]), gamma = dot3(g[p], g[q]);
            if (gamma == 0.0) continue;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            if (zeta < 0.0) t = -t;
            const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
            for (int i = 0; i < 3; ++i) {
                const double gp = g[p][i], gq = g[q][i], vp = v[p][i], vq = v[q][i];
                g[p][i] = c * gp - s * gq; g[q][i] = s * gp + c * gq;
                v[p][i] = c * vp - s * vq; v[q][i] = s * vp + c * vq;
            }
        }
    }
    double n2[3] = {dot3(g[0], g[0]), dot3(g[1], g[1]), dot3(g[2], g[2])};
    auto swap_cols = [&](int x, int y) {
        if (n2[x] < n2[y]) {
            double t = n2[x]; n2[x] = n2[y]; n2[y] = t;
            for (int i = 0; i < 3; ++i) {
                t = g[x][i]; g[x][i] = g[y][i]; g[y][i] = t;
                t = v[x][i]; v[x][i] = v[y][i]; v[y][i] = t;
            }
        }
    };
    swap_cols(0, 1); swap_cols(1, 2); swap_cols(0, 1);
    if (!(n2[0] > 0.0)) {                         // H == 0: numpy's SVD of a zero matrix gives U = V = I
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    double u[3][3];
    const double s0 = sqrt(n2[0]);
    for (int i = 0; i < 3; ++i) u[0][i] = g[0][i] / s0;
    double w[3] = {g[1][0], g[1][1], g[1][2]};     // u_1: g_1 made orthogonal to u_0, twice (the second pass removes what cancellation left)
    for (int pass = 0; pass < 2; ++pass) {
        const double d = dot3(u[0], w);
        for (int i = 0; i < 3; ++i) w[i] = w[i] - u[0][i] * d;
    }
    double wn2 = dot3(w, w);
    if (!(wn2 > 0.0)) {                           // rank 1: the axis of u_0's smallest component (the first among equals), made orthogonal to u_0
        int k = 0;
        if (fabs(u[0][1]) < fabs(u[0][k])) k = 1;
        if (fabs(u[0][2]) < fabs(u[0][k])) k = 2;
        for (int i = 0; i < 3; ++i) w[i] = (i == k ? 1.0 : 0.0) - u[0][i] * u[0][k];
        wn2 = dot3(w, w);
    }
    const double wn = sqrt(wn2);
    for (int i = 0; i < 3; ++i) u[1][i] = w[i] / wn;
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];   // u_2 = +-(u_0 x u_1), on g_2's side
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    if (dot3(u[2], g[2]) < 0.0)
        for (int i = 0; i < 3; ++i) u[2][i] = -u[2][i];
    for (int pass = 0; pass < 2; ++pass) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R[3 * r + c] = (v[0][r] * u[0][c] + v[1][r] * u[1][c]) + v[2][r] * u[2][c];
        const double det = (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!(det < 0.0)) break;                  // (a second pass has det > 0)
        for (int i = 0; i < 3; ++i) v[2][i] = -v[2][i];
    }
}

// grid (B), one wave: the sums in chunk order, the rotation, T; with the loop's state: mean error, convergence, the counter
__global__ void __launch_bounds__(64)
fit_solve_kernel(const double *part, const double *cov, int N, int chunks, double *T, double tolerance, double *prev_error, int32_t *done,
                 int32_t *iter, int it) {
    __shared__ double sum[16];
    const int b = blockIdx.x;
    if (done && done[b] != 0 && iter[b] < it) return;
    if (threadIdx.x < 7) sum[threadIdx.x] = chunk_order_sum(part + (size_t)b * chunks * FIT_SUMS, chunks, FIT_SUMS, threadIdx.x);
    else if (threadIdx.x < 16) sum[threadIdx.x] = chunk_order_sum(cov + (size_t)b * chunks * FIT_COV, chunks, FIT_COV, threadIdx.x - 7);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double mean[6], R[9];
    for (int k = 0; k < 6; ++k) mean[k] = sum[k] / (double)N;
    kabsch_rotation(sum + 7, R);
    double *out = T + (size_t)b * 16;
    for (int r = 0; r < 3; ++r) {
        out[4 * r] = R[3 * r]; out[4 * r + 1] = R[3 * r + 1]; out[4 * r + 2] = R[3 * r + 2];
        out[4 * r + 3] = mean[3 + r] - ((R[3 * r] * mean[0] + R[3 * r + 1] * mean[1]) + R[3 * r + 2] * mean[2]);
    }
    out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
    if (done) {
        const double mean_error = sum[6] / (double)N;
        iter[b] = it;
        if (fabs(prev_error[b] - mean_error) < tolerance) done[b] = 1;
        else prev_error[b] = mean_error;
    }
}

// grid (tiles, B): work = T src (T NULL: a copy); src == work updates in place
__global__ void __launch_bounds__(ICP_THREADS)
move_points_kernel(const double *src, const double *T, double *work, int N, Gate gate) {
    const int b = blockIdx.y;
    if (frozen(gate, b)) return;
    const int n = blockIdx.x * ICP_THREADS + threadIdx.x;
    if (n >= N) return;
    const size_t at = ((size_t)b * N + n) * 3;
    double x = src[at], y = src[at + 1], z = src[at + 2];
    if (T) move_point(T + (size_t)b * 16, x, y, z, x, y, z);
    work[at] = x; work[at + 1] = y; work[at + 2] = z;
}

__global__ void icp_state_kernel(double *prev_error, int32_t *done, int32_t *iter, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) { prev_error[b] = 0.0; done[b] = 0; iter[b] = 0; }
}

unsigned tiles(int64_t n) { return (unsigned)((n + ICP_THREADS - 1) / ICP_THREADS); }

bool sizes_ok(int64_t N, int64_t M, int B) { return N >= 1 && M >= 1 && B >= 1 && N <= 0x7fffff00 && M <= 0x7fffff00 && B <= 65535; }

void nn_launch(const double *src, const double *T, const double *dst, int N, int M, int B, double *d2, int32_t *idx, char *ws, const NnPlan &pl,
               Gate gate, hipStream_t stream) {
    hipLaunchKernelGGL(nn_slab_kernel, dim3(tiles(N), (unsigned)pl.slabs, (unsigned)B), dim3(ICP_THREADS), 0, stream, src, T, dst, N, M, ws,
                       pl.block_bytes, pl.pidx_off, pl.slab_pts, pl.slabs, gate);
    hipLaunchKernelGGL(nn_finish_kernel, dim3(tiles(N), 1u, (unsigned)B), dim3(ICP_THREADS), 0, stream, N, M, (const char *)ws, pl.block_bytes,
                       pl.pidx_off, pl.slab_pts, pl.slabs, d2, idx, gate);
}

size_t fit_bytes(int64_t N, int B) { return up256((size_t)B * tiles(N) * (FIT_SUMS + FIT_COV) * sizeof(double)); }

// d2 / dist / the state are the loop's; a plain fit passes NULLs
void fit_launch(const double *a, const double *bp, const int32_t *idx, int N, int M, int B, const double *d2, double *dist, double *T, char *ws,
                double tolerance, double *prev_error, int32_t *done, int32_t *iter, int it, hipStream_t stream) {
    const int chunks = (int)tiles(N);
    double *part = reinterpret_cast<double *>(ws);
    double *cov = part + (size_t)B * chunks * FIT_SUMS;
    const Gate gate{done, iter, it};
    hipLaunchKernelGGL(fit_sums_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(ICP_THREADS), 0, stream, a, bp, idx, N, M, d2, dist, part, chunks, gate);
    hipLaunchKernelGGL(fit_cov_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(ICP_THREADS), 0, stream, a, bp, idx, N, M, (const double *)part, cov,
                       chunks, gate);
    hipLaunchKernelGGL(fit_solve_kernel, dim3((unsigned)B), dim3(64), 0, stream, (const double *)part, (const double *)cov, N, chunks, T, tolerance,
                       prev_error, done, iter, it);
}

// the loop's own buffers, then the neighbour search's (nn_bytes: 0 for the tree, which needs none)
struct IcpPlan { size_t work_off, d2_off, t_off, prev_off, done_off, fit_off, nn_off, bytes; };

IcpPlan icp_plan(int64_t N, int B, size_t nn_bytes) {
    IcpPlan p;
    p.work_off = 0;
    p.d2_off = p.work_off + up256((size_t)B * N * 3 * sizeof(double));
    p.t_off = p.d2_off + up256((size_t)B * N * sizeof(double));
    p.prev_off = p.t_off + up256((size_t)B * 16 * sizeof(double));
    p.done_off = p.prev_off + up256((size_t)B * sizeof(double));
    p.fit_off = p.done_off + up256((size_t)B * sizeof(int32_t));
    p.nn_off = p.fit_off + fit_bytes(N, B);
    p.bytes = p.nn_off + nn_bytes;
    return p;
}

// icp.py:102-121 enqueued in full.  nn(work, d2, idx, gate) enqueues the neighbour search of one iteration and returns its error code;
// fit, move, the state and the gate are the same whatever searches
template <class Nn>
int icp_loop(const double *A, int N, const double *Bp, int M, int B, const double *init_pose, int max_iterations, double tolerance, double *T,
             double *distances, int32_t *idx, int32_t *iterations, char *ws, const IcpPlan &pl, hipStream_t st, Nn nn) {
    double *work = reinterpret_cast<double *>(ws + pl.work_off), *d2 = reinterpret_cast<double *>(ws + pl.d2_off);
    double *Tit = reinterpret_cast<double *>(ws + pl.t_off), *prev = reinterpret_cast<double *>(ws + pl.prev_off);
    int32_t *done = reinterpret_cast<int32_t *>(ws + pl.done_off);
    hipLaunchKernelGGL(icp_state_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, prev, done, iterations, B);
    hipLaunchKernelGGL(move_points_kernel, dim3(tiles(N), (unsigned)B), dim3(ICP_THREADS), 0, st, A, init_pose, work, N, Gate{nullptr, nullptr, 0});
    for (int it = 0; it < max_iterations; ++it) {
        const Gate gate{done, iterations, it};
        if (int rc = nn(work, d2, idx, gate)) return rc;
        fit_launch(work, Bp, idx, N, M, B, d2, distances, Tit, ws + pl.fit_off, tolerance, prev, done, iterations, it, st);
        hipLaunchKernelGGL(move_points_kernel, dim3(tiles(N), (unsigned)B), dim3(ICP_THREADS), 0, st, (const double *)work, (const double *)Tit, work, N,
                           gate);
    }
    fit_launch(A, work, nullptr, N, N, B, nullptr, nullptr, T, ws + pl.fit_off, 0.0, nullptr, nullptr, nullptr, 0, st);
    return 0;
}

}  // namespace

extern "C" {

size_t vt_nn_points_workspace_bytes(int64_t N, int64_t M, int B) {
    if (!sizes_ok(N, M, B)) return 0;
    return (size_t)B * nn_plan(N, M, B).block_bytes;
}

int vt_nn_points_slab_points(int64_t N, int64_t M, int B) {
    if (!sizes_ok(N, M, B)) return 0;
    return nn_plan(N, M, B).slab_pts;
}

int vt_nn_points(const double *src, int64_t N, const double *dst, int64_t M, int B, const double *T, double *d2, int32_t *idx, void *workspace,
                 size_t workspace_bytes, void *stream) {
    if (!sizes_ok(N, M, B) || !src || !dst || !d2 || !idx)
        return vt_fail(VT_ERR_INVALID, "vt_nn_points: bad argument (N >= 1, M >= 1, 1 <= B <= 65535)");
    const NnPlan pl = nn_plan(N, M, B);
    if (pl.slabs > 65535) return vt_fail(VT_ERR_UNSUPPORTED, "vt_nn_points");
    if (!workspace || workspace_bytes < (size_t)B * pl.block_bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_nn_points");
    nn_launch(src, T, dst, (int)N, (int)M, B, d2, idx, static_cast<char *>(workspace), pl, Gate{nullptr, nullptr, 0}, (hipStream_t)stream);
    return vt_check(hipGetLastError(), "vt_nn_points");
}

size_t vt_icp_fit_workspace_bytes(int64_t N, int B) {
    if (!sizes_ok(N, 1, B)) return 0;
    return fit_bytes(N, B);
}

int vt_icp_fit(const double *a, const double *b, int64_t N, int64_t M, const int32_t *idx, int B, double *T, void *workspace, size_t workspace_bytes,
               void *stream) {
    if (!sizes_ok(N, M, B) || !a || !b || !T || (!idx && M != N))
        return vt_fail(VT_ERR_INVALID, "vt_icp_fit: bad argument (N >= 1, M >= 1, 1 <= B <= 65535; without idx, M == N)");
    if (!workspace || workspace_bytes < fit_bytes(N, B)) return vt_fail(VT_ERR_WORKSPACE, "vt_icp_fit");
    fit_launch(a, b, idx, (int)N, (int)M, B, nullptr, nullptr, T, static_cast<char *>(workspace), 0.0, nullptr, nullptr, nullptr, 0, (hipStream_t)stream);
    return vt_check(hipGetLastError(), "vt_icp_fit");
}

size_t vt_icp_workspace_bytes(int64_t N, int64_t M, int B) {
    if (!sizes_ok(N, M, B)) return 0;
    return icp_plan(N, B, (size_t)B * nn_plan(N, M, B).block_bytes).bytes;
}

int vt_icp(const double *A, int64_t N, const double *Bp, int64_t M, int B, const double *init_pose, int max_iterations, double tolerance, double *T,
           double *distances, int32_t *idx, int32_t *iterations, void *workspace, size_t workspace_bytes, void *stream) {
    if (!sizes_ok(N, M, B) || !A || !Bp || !T || !distances || !idx || !iterations || max_iterations < 1 || !(tolerance >= 0.0))
        return vt_fail(VT_ERR_INVALID, "vt_icp: bad argument (N >= 1, M >= 1, 1 <= B <= 65535, max_iterations >= 1, tolerance >= 0)");
    const NnPlan nn = nn_plan(N, M, B);
    const IcpPlan pl = icp_plan(N, B, (size_t)B * nn.block_bytes);
    if (nn.slabs > 65535) return vt_fail(VT_ERR_UNSUPPORTED, "vt_icp");
    if (!workspace || workspace_bytes < pl.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_icp");
    char *ws = static_cast<char *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)N, m = (int)M;
    if (int rc = icp_loop(A, n, Bp, m, B, init_pose, max_iterations, tolerance, T, distances, idx, iterations, ws, pl, st,
                          [&](const double *work, double *d2, int32_t *ix, Gate gate) {
                              nn_launch(work, nullptr, Bp, n, m, B, d2, ix, ws + pl.nn_off, nn, gate, st);
                              return 0;
                          }))
        return rc;
    return vt_check(hipGetLastError(), "vt_icp");
}

// the tree loop's workspace: the loop's own buffers, then the lane permutation [B][N] and what building it needs
size_t icp_tree_nn_bytes(int64_t N, int B, int depth) { return up256((size_t)B * N * sizeof(int32_t)) + pt_lanes_bytes(N, B, depth); }

size_t vt_icp_tree_workspace_bytes(int64_t N, int B, int depth) {
    if (!sizes_ok(N, 1, B) || depth < 1 || depth > VT_WN_MAX_DEPTH) return 0;
    return icp_plan(N, B, icp_tree_nn_bytes(N, B, depth)).bytes;
}

int vt_icp_tree(const double *A, int64_t N, const double *Bp, int64_t M, int B, const void *tree, size_t tree_bytes, int depth,
                const int32_t *state_host, int morton_lanes, const double *init_pose, int max_iterations, double tolerance, double *T,
                double *distances, int32_t *idx, int32_t *iterations, void *workspace, size_t workspace_bytes, void *stream) {
    if (!sizes_ok(N, M, B) || !A || !Bp || !tree || !state_host || !T || !distances || !idx || !iterations || max_iterations < 1 || !(tolerance >= 0.0))
        return vt_fail(VT_ERR_INVALID, "vt_icp_tree: bad argument (N >= 1, M >= 1, 1 <= B <= 65535, max_iterations >= 1, tolerance >= 0)");
    PtQueryPlan plan;                             // the tree's own checks (depth, counts, size, the walk asked for) before anything is enqueued
    if (int rc = pt_query_plan(tree_bytes, M, depth, B, state_host, N, &plan)) return rc;
    const IcpPlan pl = icp_plan(N, B, icp_tree_nn_bytes(N, B, depth));
    if (!workspace || workspace_bytes < pl.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_icp_tree");
    char *ws = static_cast<char *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    int32_t *perm = morton_lanes ? reinterpret_cast<int32_t *>(ws + pl.nn_off) : nullptr;
    char *lanes_ws = ws + pl.nn_off + up256((size_t)B * N * sizeof(int32_t));
    if (int rc = icp_loop(A, (int)N, Bp, (int)M, B, init_pose, max_iterations, tolerance, T, distances, idx, iterations, ws, pl, st,
                          [&](const double *work, double *d2, int32_t *ix, Gate gate) {
                              // the lane order is taken once, from the working copy the loop starts with: a rigid motion keeps the
                              // lanes of a wave neighbours of each other, which is all the order is for
                              if (perm && gate.it == 0) pt_lanes_enqueue(plan, tree, work, nullptr, perm, lanes_ws, st);
                              pt_query_enqueue(plan, tree, work, nullptr, d2, ix, nullptr, perm, gate.done, gate.iter, gate.it, st);
                              return 0;
                          }))
        return rc;
    return vt_check(hipGetLastError(), "vt_icp_tree");
}

}  // extern "C"
