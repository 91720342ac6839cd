// Voxel-input encoder front end for gfx950: the 1 -> C Conv3d (kernel 3 with zero padding 1, or kernel 1), ReLU and the scatter-mean
// of the voxel features onto the feature grid or the canonical planes of reference src/encoder/voxels.py:56-119, in one launch, and the
// weight / bias gradient of that composition.
//
// A voxel's coordinate is linspace(-0.5, 0.5, D)[i] per axis, so its cell index is a per-axis table a_k[i_k] that depends on the volume's
// shape alone and never decreases with i_k: the voxels that land in an output cell are a box [lo1,hi1) x [lo2,hi2) x [lo3,hi3).  The
// scatter-mean is therefore a gather: a thread owns one (cell, channel), walks the cell's box in (i1, i2, i3) order, recomputes the
// voxel's feature from the 27 taps of x and its channel's 27 weights (registers), sums, divides once.  No atomics, no clear pass (an
// empty box writes 0.0f), no [B,C,D^3] intermediate; the order of every sum is fixed, so results are bit-identical from run to run and
// a scene's result does not depend on the batch around it.  A plane cell's box is its two ranges times the whole dropped axis.
//
// Latency / bandwidth class, no MFMA: 27 FMAs per (voxel, channel).  The lanes of a cell run over its channels, so the taps of x are
// the same address for all of them (one broadcast load) and the channels-last grid is written in contiguous rows; along i3 (the
// contiguous axis of x) a 3x9 register window slides, so a step loads 9 new taps instead of 27.
//
// Backward (dW, dbias; x is data): stage 1 walks the voxels in chunks of consecutive flat indices, one chunk per workgroup, recomputes
// the pre-activation in the forward's order, and where it is positive (torch's ReLU gradient: 0 at 0) adds g[cell] / n of every output
// the voxel fed -- grid first, then xz, xy, yz -- times the taps into 28 per-thread sums; the workgroup's voxel slots are summed in
// slot order through LDS into one partial row per workgroup.  Stage 2 sums the rows in workgroup order.  No float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "vt_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BWD_BLOCKS = 512;

// the projected axes of plane 0 (xz), 1 (xy), 2 (yz) as axes of the volume: u (fastest, the array's last dimension), v, and the
// dropped one (normalize_coordinate: xz -> (p0, p2), xy -> (p0, p1), yz -> (p1, p2); p_k is the coordinate along x's dimension k + 1)
__device__ __forceinline__ int plane_u(int k) { return k == 2 ? 1 : 0; }
__device__ __forceinline__ int plane_v(int k) { return k == 1 ? 1 : 2; }

struct Box {
    int lo[3], hi[3];
    __device__ __forceinline__ int count() const { return (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]); }
};

// ranges: [3 axes][R][2] = lo, hi of the voxel indices whose table entry is r; clipped to the volume so that a bad table cannot
// send a load outside x
__device__ __forceinline__ void axis_range(const int *ranges, int R, int axis, int r, int D, int &lo, int &hi) {
    const int *p = ranges + ((size_t)axis * R + r) * 2;
    lo = max(p[0], 0);
    hi = min(p[1], D);
    if (hi < lo) hi = lo;
}

// x[i1][i2][i3] of one scene with zero padding
__device__ __forceinline__ float tap(const float *xb, int D1, int D2, int D3, int j1, int j2, int j3) {
    const bool in = (unsigned)j1 < (unsigned)D1 && (unsigned)j2 < (unsigned)D2 && (unsigned)j3 < (unsigned)D3;
    return in ? xb[((size_t)j1 * D2 + j2) * D3 + j3] : 0.0f;
}

// the nine taps (t1, t2) of the column at j3
__device__ __forceinline__ void column(const float *xb, int D1, int D2, int D3, int i1, int i2, int j3, float (&col)[9]) {
#pragma unroll
    for (int t1 = 0; t1 < 3; ++t1)
#pragma unroll
        for (int t2 = 0; t2 < 3; ++t2) col[t1 * 3 + t2] = tap(xb, D1, D2, D3, i1 + t1 - 1, i2 + t2 - 1, j3);
}

// bias + sum W x over the taps in (t1, t2, t3) order, one fused multiply-add per tap: the forward and the backward share it
__device__ __forceinline__ float pre3(const float (&w)[27], float bias, const float (&c0)[9], const float (&c1)[9], const float (&c2)[9]) {
    float pre = bias;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        pre = fmaf(w[t * 3 + 0], c0[t], pre);
        pre = fmaf(w[t * 3 + 1], c1[t], pre);
        pre = fmaf(w[t * 3 + 2], c2[t], pre);
    }
    return pre;
}

// sum of relu(conv) over the voxels of a box, in (i1, i2, i3) order
template <int K>
__device__ __forceinline__ float box_sum(const float *xb, int D1, int D2, int D3, const Box &bx, const float (&w)[27], float bias) {
    float s = 0.0f;
    for (int i1 = bx.lo[0]; i1 < bx.hi[0]; ++i1)
        for (int i2 = bx.lo[1]; i2 < bx.hi[1]; ++i2) {
            if (K == 1) {
                const float *row = xb + ((size_t)i1 * D2 + i2) * D3;
                for (int i3 = bx.lo[2]; i3 < bx.hi[2]; ++i3) {
                    const float pre = fmaf(w[0], row[i3], bias);
                    s += pre > 0.0f ? pre : 0.0f;
                }
            } else {
                float c0[9], c1[9], c2[9];
                column(xb, D1, D2, D3, i1, i2, bx.lo[2] - 1, c0);
                column(xb, D1, D2, D3, i1, i2, bx.lo[2], c1);
                for (int i3 = bx.lo[2]; i3 < bx.hi[2]; ++i3) {
                    column(xb, D1, D2, D3, i1, i2, i3 + 1, c2);
                    const float pre = pre3(w, bias, c0, c1, c2);
                    s += pre > 0.0f ? pre : 0.0f;
#pragma unroll
                    for (int t = 0; t < 9; ++t) { c0[t] = c1[t]; c1[t] = c2[t]; }
                }
            }
        }
    return s;
}

struct FwdArgs {
    const float *x, *w, *bias;
    const int *ranges;
    float *out;
    int B, D1, D2, D3, C, R;
    int plane_id[3], n_planes;      // planes form: the stacked planes' ids in output order
    uint64_t cells;                 // grid: B R^3; planes: n_planes B R^2
};

// thread -> (cell slot of the workgroup, channel); THREADS / C cells per workgroup (C = 96: two cells, 64 idle lanes)
template <int K, bool PLANES>
__global__ void __launch_bounds__(THREADS)
voxel_encode_kernel(FwdArgs a) {
    const int per_block = THREADS / a.C;
    const int slot = (int)threadIdx.x / a.C, c = (int)threadIdx.x % a.C;
    const uint64_t cell = (uint64_t)blockIdx.x * per_block + slot;
    if (slot >= per_block || cell >= a.cells) return;
    const int R = a.R, D[3] = {a.D1, a.D2, a.D3};
    Box bx;
    int b;
    size_t out_at;
    if (PLANES) {
        const uint64_t RR = (uint64_t)R * R;
        const int u = (int)(cell % R), v = (int)((cell / R) % R);
        const uint64_t img = cell / RR;                    // plane slot * B + scene
        const int k = a.plane_id[img / a.B];
        b = (int)(img % a.B);
        const int au = plane_u(k), av = plane_v(k), ad = 3 - au - av;
        axis_range(a.ranges, R, au, u, D[au], bx.lo[au], bx.hi[au]);
        axis_range(a.ranges, R, av, v, D[av], bx.lo[av], bx.hi[av]);
        bx.lo[ad] = 0; bx.hi[ad] = D[ad];
        out_at = ((size_t)img * a.C + c) * RR + (size_t)v * R + u;
    } else {
        const uint64_t RRR = (uint64_t)R * R * R;
        const uint64_t in = cell % RRR;                    // a1 + R (a2 + R a3)
        b = (int)(cell / RRR);
        const int r1 = (int)(in % R), r2 = (int)((in / R) % R), r3 = (int)(in / ((uint64_t)R * R));
        axis_range(a.ranges, R, 0, r1, D[0], bx.lo[0], bx.hi[0]);
        axis_range(a.ranges, R, 1, r2, D[1], bx.lo[1], bx.hi[1]);
        axis_range(a.ranges, R, 2, r3, D[2], bx.lo[2], bx.hi[2]);
        out_at = (size_t)cell * a.C + c;
    }
    const int n = bx.count();
    float val = 0.0f;
    if (n > 0) {
        float w[27];
#pragma unroll
        for (int t = 0; t < K * K * K; ++t) w[t] = a.w[(size_t)c * (K * K * K) + t];
        const float *xb = a.x + (size_t)b * a.D1 * a.D2 * a.D3;
        val = box_sum<K>(xb, a.D1, a.D2, a.D3, bx, w, a.bias[c]) / (float)n;
    }
    a.out[out_at] = val;
}

struct BwdArgs {
    const float *x, *w, *bias;
    const float *ggrid;             // [B][Rg^3][C] or null
    const int *gindex, *granges;    // a1 | a2 | a3 and [3][Rg][2]
    const float *gplanes;           // [n_planes B][C][Rp][Rp] or null
    const int *pindex, *pranges;
    float *part;                    // [blocks][C][28]
    int B, D1, D2, D3, C, Rg, Rp;
    int plane_id[3], n_planes;
    uint64_t voxels, chunk;         // B D1 D2 D3; voxels per workgroup
};

__device__ __forceinline__ int table_at(const int *t, int i, int R) { return min(max(t[i], 0), R - 1); }
__device__ __forceinline__ int range_len(const int *ranges, int R, int axis, int r, int D) {
    int lo, hi;
    axis_range(ranges, R, axis, r, D, lo, hi);
    return hi - lo;
}

template <int K>
__global__ void __launch_bounds__(THREADS)
voxel_encode_bwd_partial_kernel(BwdArgs a) {
    constexpr int KK = K * K * K;
    __shared__ float red[THREADS * 28];
    const int per_block = THREADS / a.C;
    const int slot = (int)threadIdx.x / a.C, c = (int)threadIdx.x % a.C;
    const bool active = slot < per_block;
    const int D[3] = {a.D1, a.D2, a.D3};
    const uint64_t per_scene = (uint64_t)a.D1 * a.D2 * a.D3;
    float acc[KK], accb = 0.0f;
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[t] = 0.0f;
    if (active) {
        float w[27];
#pragma unroll
        for (int t = 0; t < KK; ++t) w[t] = a.w[(size_t)c * KK + t];
        const float bias = a.bias[c];
        const uint64_t v0 = (uint64_t)blockIdx.x * a.chunk, v1 = min(v0 + a.chunk, a.voxels);
        for (uint64_t v = v0 + slot; v < v1; v += per_block) {
            const int b = (int)(v / per_scene);
            const uint64_t in = v % per_scene;
            const int i[3] = {(int)(in / ((uint64_t)a.D2 * a.D3)), (int)((in / a.D3) % a.D2), (int)(in % a.D3)};
            const float *xb = a.x + (size_t)b * per_scene;
            float c0[9], c1[9], c2[9], pre;
            if (K == 1) {
                c1[0] = xb[in];
                pre = fmaf(w[0], c1[0], bias);
            } else {
                column(xb, a.D1, a.D2, a.D3, i[0], i[1], i[2] - 1, c0);
                column(xb, a.D1, a.D2, a.D3, i[0], i[1], i[2], c1);
                column(xb, a.D1, a.D2, a.D3, i[0], i[1], i[2] + 1, c2);
                pre = pre3(w, bias, c0, c1, c2);
            }
            if (!(pre > 0.0f)) continue;
            float g = 0.0f;
            if (a.ggrid) {
                const int R = a.Rg;
                const int r1 = table_at(a.gindex, i[0], R), r2 = table_at(a.gindex + a.D1, i[1], R), r3 = table_at(a.gindex + a.D1 + a.D2, i[2], R);
                const int n = range_len(a.granges, R, 0, r1, D[0]) * range_len(a.granges, R, 1, r2, D[1]) * range_len(a.granges, R, 2, r3, D[2]);
                const size_t cell = (size_t)r1 + (size_t)R * ((size_t)r2 + (size_t)R * r3);
                g += a.ggrid[(((size_t)b * R * R * R) + cell) * a.C + c] / (float)max(n, 1);
            }
            if (a.gplanes) {
                const int R = a.Rp;
                const int off[3] = {0, a.D1, a.D1 + a.D2};
                for (int s = 0; s < a.n_planes; ++s) {
                    const int k = a.plane_id[s];
                    const int au = plane_u(k), av = plane_v(k), ad = 3 - au - av;
                    const int u = table_at(a.pindex + off[au], i[au], R), vv = table_at(a.pindex + off[av], i[av], R);
                    const int n = range_len(a.pranges, R, au, u, D[au]) * range_len(a.pranges, R, av, vv, D[av]) * D[ad];
                    g += a.gplanes[(((size_t)s * a.B + b) * a.C + c) * R * R + (size_t)vv * R + u] / (float)max(n, 1);
                }
            }
            if (K == 1) {
                acc[0] = fmaf(g, c1[0], acc[0]);
            } else {
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    acc[t * 3 + 0] = fmaf(g, c0[t], acc[t * 3 + 0]);
                    acc[t * 3 + 1] = fmaf(g, c1[t], acc[t * 3 + 1]);
                    acc[t * 3 + 2] = fmaf(g, c2[t], acc[t * 3 + 2]);
                }
            }
            accb += g;
        }
#pragma unroll
        for (int t = 0; t < KK; ++t) red[(size_t)threadIdx.x * 28 + t] = acc[t];
        red[(size_t)threadIdx.x * 28 + KK] = accb;
    }
    __syncthreads();
    if (active && slot == 0) {
        float *row = a.part + ((size_t)blockIdx.x * a.C + c) * 28;
        for (int t = 0; t <= KK; ++t) {
            float s = red[(size_t)c * 28 + t];
            for (int k = 1; k < per_block; ++k) s += red[((size_t)k * a.C + c) * 28 + t];
            row[t] = s;
        }
    }
}

// dW[c][t] / dbias[c] = the workgroups' partial rows summed in workgroup order
__global__ void __launch_bounds__(THREADS)
voxel_encode_bwd_reduce_kernel(const float *part, int blocks, int C, int KK, float *dweight, float *dbias) {
    const int i = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (i >= C * (KK + 1)) return;
    const int c = i / (KK + 1), t = i % (KK + 1);
    float s = 0.0f;
    for (int k = 0; k < blocks; ++k) s += part[((size_t)k * C + c) * 28 + t];
    if (t < KK) dweight[(size_t)c * KK + t] = s;
    else dbias[c] = s;
}

int shape_check(const char *who, int B, int D1, int D2, int D3, int C, int ksize, int R) {
    static thread_local char msg[160];
    auto fail = [&](int code, const char *what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return vt_fail(code, msg);
    };
    if (B <= 0 || D1 < 2 || D2 < 2 || D3 < 2 || R < 1) return fail(VT_ERR_INVALID, "B >= 1, every volume dimension >= 2 and R >= 1 are required");
    if (ksize != 1 && ksize != 3) return fail(VT_ERR_UNSUPPORTED, "the conv's kernel size must be 1 or 3");
    if (C < 32 || C > 128 || C % 32) return fail(VT_ERR_UNSUPPORTED, "C must be a multiple of 32 up to 128");
    if (D1 > 4096 || D2 > 4096 || D3 > 4096 || R > 1024 || B > 65535) return fail(VT_ERR_UNSUPPORTED, "volume dimensions up to 4096, R up to 1024, B up to 65535");
    return 0;
}

int plane_slots(int plane_mask, int (&ids)[3]) {
    int n = 0;
    for (int k = 0; k < 3; ++k)
        if (plane_mask & (1 << k)) ids[n++] = k;
    for (int k = n; k < 3; ++k) ids[k] = 0;
    return n;
}

uint64_t bwd_chunk(uint64_t voxels) {
    uint64_t blocks = (voxels + THREADS - 1) / THREADS;
    if (blocks > MAX_BWD_BLOCKS) blocks = MAX_BWD_BLOCKS;
    if (blocks < 1) blocks = 1;
    return (voxels + blocks - 1) / blocks;
}

}  // namespace

extern "C" {

int vt_voxel_encode_grid(const float *x, int B, int D1, int D2, int D3, const float *weight, const float *bias, int C, int ksize,
                         const int *ranges, int R, float *grid_cl, void *stream) {
    int rc = shape_check("vt_voxel_encode_grid", B, D1, D2, D3, C, ksize, R);
    if (rc) return rc;
    if (!x || !weight || !bias || !ranges || !grid_cl) return vt_fail(VT_ERR_INVALID, "vt_voxel_encode_grid: null argument");
    FwdArgs a{};
    a.x = x; a.w = weight; a.bias = bias; a.ranges = ranges; a.out = grid_cl;
    a.B = B; a.D1 = D1; a.D2 = D2; a.D3 = D3; a.C = C; a.R = R;
    a.cells = (uint64_t)B * R * R * R;
    const uint64_t blocks = (a.cells + (THREADS / C) - 1) / (THREADS / C);
    if (blocks > 0x7fffffffull) return vt_fail(VT_ERR_UNSUPPORTED, "vt_voxel_encode_grid: B R^3 cells exceed one launch");
    hipStream_t s = (hipStream_t)stream;
    if (ksize == 3) hipLaunchKernelGGL((voxel_encode_kernel<3, false>), dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL((voxel_encode_kernel<1, false>), dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
    return vt_check(hipGetLastError(), "vt_voxel_encode_grid");
}

int vt_voxel_encode_planes(const float *x, int B, int D1, int D2, int D3, const float *weight, const float *bias, int C, int ksize,
                           const int *ranges, int R, int plane_mask, float *planes, void *stream) {
    int rc = shape_check("vt_voxel_encode_planes", B, D1, D2, D3, C, ksize, R);
    if (rc) return rc;
    if (!x || !weight || !bias || !ranges || !planes) return vt_fail(VT_ERR_INVALID, "vt_voxel_encode_planes: null argument");
    if (plane_mask < 1 || plane_mask > 7) return vt_fail(VT_ERR_INVALID, "vt_voxel_encode_planes: plane_mask must name at least one of xz (1), xy (2), yz (4)");
    FwdArgs a{};
    a.x = x; a.w = weight; a.bias = bias; a.ranges = ranges; a.out = planes;
    a.B = B; a.D1 = D1; a.D2 = D2; a.D3 = D3; a.C = C; a.R = R;
    a.n_planes = plane_slots(plane_mask, a.plane_id);
    a.cells = (uint64_t)a.n_planes * B * R * R;
    const uint64_t blocks = (a.cells + (THREADS / C) - 1) / (THREADS / C);
    if (blocks > 0x7fffffffull) return vt_fail(VT_ERR_UNSUPPORTED, "vt_voxel_encode_planes: the planes' cells exceed one launch");
    hipStream_t s = (hipStream_t)stream;
    if (ksize == 3) hipLaunchKernelGGL((voxel_encode_kernel<3, true>), dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL((voxel_encode_kernel<1, true>), dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
    return vt_check(hipGetLastError(), "vt_voxel_encode_planes");
}

size_t vt_voxel_encode_bwd_workspace_bytes(int B, int D1, int D2, int D3, int C) {
    if (B <= 0 || D1 < 2 || D2 < 2 || D3 < 2 || C < 32 || C > 128 || C % 32) return 0;
    const uint64_t voxels = (uint64_t)B * D1 * D2 * D3, chunk = bwd_chunk(voxels);
    return (size_t)((voxels + chunk - 1) / chunk) * C * 28 * sizeof(float);
}

int vt_voxel_encode_bwd(const float *x, int B, int D1, int D2, int D3, const float *weight, const float *bias, int C, int ksize,
                        const float *grad_grid_cl, const int *grid_index, const int *grid_ranges, int Rg,
                        const float *grad_planes, const int *plane_index, const int *plane_ranges, int Rp, int plane_mask,
                        float *grad_weight, float *grad_bias, void *workspace, size_t workspace_bytes, void *stream) {
    if (!grad_grid_cl && !grad_planes) return vt_fail(VT_ERR_INVALID, "vt_voxel_encode_bwd: give the gradient of the grid, of the planes, or both");
    int rc = shape_check("vt_voxel_encode_bwd", B, D1, D2, D3, C, ksize, grad_grid_cl ? Rg : Rp);
    if (!rc && grad_grid_cl && grad_planes) rc = shape_check("vt_voxel_encode_bwd", B, D1, D2, D3, C, ksize, Rp);
    if (rc) return rc;
    if (!x || !weight || !bias || !grad_weight || !grad_bias || !workspace) return vt_fail(VT_ERR_INVALID, "vt_voxel_encode_bwd: null argument");
    if (grad_grid_cl && (!grid_index || !grid_ranges)) return vt_fail(VT_ERR_INVALID, "vt_voxel_encode_bwd: the grid's gradient needs its index and range tables");
    if (grad_planes && (!plane_index || !plane_ranges || plane_mask < 1 || plane_mask > 7))
        return vt_fail(VT_ERR_INVALID, "vt_voxel_encode_bwd: the planes' gradient needs their tables and a plane_mask of xz (1), xy (2), yz (4)");
    if (workspace_bytes < vt_voxel_encode_bwd_workspace_bytes(B, D1, D2, D3, C))
        return vt_fail(VT_ERR_WORKSPACE, "vt_voxel_encode_bwd: workspace too small (vt_voxel_encode_bwd_workspace_bytes)");
    BwdArgs a{};
    a.x = x; a.w = weight; a.bias = bias;
    a.ggrid = grad_grid_cl; a.gindex = grid_index; a.granges = grid_ranges;
    a.gplanes = grad_planes; a.pindex = plane_index; a.pranges = plane_ranges;
    a.part = (float *)workspace;
    a.B = B; a.D1 = D1; a.D2 = D2; a.D3 = D3; a.C = C; a.Rg = Rg; a.Rp = Rp;
    a.n_planes = grad_planes ? plane_slots(plane_mask, a.plane_id) : 0;
    a.voxels = (uint64_t)B * D1 * D2 * D3;
    a.chunk = bwd_chunk(a.voxels);
    const unsigned blocks = (unsigned)((a.voxels + a.chunk - 1) / a.chunk);
    const int KK = ksize * ksize * ksize;
    hipStream_t s = (hipStream_t)stream;
    if (ksize == 3) hipLaunchKernelGGL((voxel_encode_bwd_partial_kernel<3>), dim3(blocks), dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL((voxel_encode_bwd_partial_kernel<1>), dim3(blocks), dim3(THREADS), 0, s, a);
    hipLaunchKernelGGL(voxel_encode_bwd_reduce_kernel, dim3((unsigned)((C * (KK + 1) + THREADS - 1) / THREADS)), dim3(THREADS), 0, s,
                       (const float *)a.part, (int)blocks, C, KK, grad_weight, grad_bias);
    return vt_check(hipGetLastError(), "vt_voxel_encode_bwd");
}

}  // extern "C"
