// Plane-feature sampler of the occupancy decoder for gfx950: feat = (base?) + xz? + xy? + yz?, the bilinear (or nearest)
// sample of each canonical feature plane at the query points, summed in the order the reference walks its keys
// (reference src/conv_onet/models/decoder.py:55-60 sample_plane_feature, :135-147 the sum; src/common.py:268-291
// normalize_coordinate), and its backward to the planes.
//
// Bandwidth / latency class, no MFMA.  The planes arrive [B][C][R][R] (channel stride R*R: a gather of C channels at one pixel
// would touch C cache lines), so every call first lays them out channels-last in a workspace ([B][R][R][C]: 0.5 MB per plane at
// 64^2 x 32); after that a corner is one contiguous row of C floats and every lane reads 16 bytes of it.
//
//   point form    one lane per (point, 4 channels): up to 12 corner rows per point, summed plane by plane.
//   lattice form  on the lattice box * make_3d_grid(...) a plane's sample depends on two of the three lattice indices only, so
//                 the nx^2 distinct samples of each plane are computed once into a table (the same device function as the
//                 point form, fed the same coordinates: the same bits) and every lattice point is the ordered sum of up to
//                 three table rows -- 3 coalesced rows from L2-resident tables instead of 12 scattered corner rows.
//   backward      the points are grouped by bilinear cell (vt_plane_build_multi at resolution R - 1, all present planes in one
//                 launch); one wave per cell sums its points' four corner contributions in ascending point order and issues
//                 its atomics once per cell, 128 contiguous bytes per corner, into a channels-last accumulator in the
//                 workspace, which a last pass writes out as [B][C][R][R] (the outputs are written, never accumulated into).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "decode_common.h"

namespace {

// reference src/common.py:283-290 in f32 (divisor 1 + padding + 10e-6, upper clamp 1 - 10e-6: not the 3-D constants), then
// ATen's align_corners=True un-normalisation of 2 q - 1 and the border clip: the continuous pixel coordinate in [0, R - 1]
__device__ __forceinline__ float plane_coord(float v, float divisor, float clamp_hi, int R) {
    float q = v / divisor + 0.5f;
    q = (q >= 1.0f) ? clamp_hi : q;
    q = (q < 0.0f) ? 0.0f : q;
    const float g = 2.0f * q - 1.0f;
    const float f = ((g + 1.0f) / 2.0f) * (float)(R - 1);
    return fminf(fmaxf(f, 0.0f), (float)(R - 1));
}

// the four pixels and weights of ATen's 2-D grid_sample (align_corners, border); 'nearest': pixel (x0, y0) alone, rounded half to even
struct Bil {
    int x0, x1, y0, y1;
    float w[4];          // (y0,x0) (y0,x1) (y1,x0) (y1,x1)
};
// u: the first projected axis (indexes W, the last dimension), v: the second (indexes H)
__device__ __forceinline__ Bil bil_setup(float u, float v, float divisor, float clamp_hi, int R, bool nearest) {
    Bil t;
    const float fx = plane_coord(u, divisor, clamp_hi, R), fy = plane_coord(v, divisor, clamp_hi, R);
    if (nearest) {
        t.x0 = t.x1 = (int)rintf(fx); t.y0 = t.y1 = (int)rintf(fy);
        t.w[0] = 1.0f; t.w[1] = t.w[2] = t.w[3] = 0.0f;
        return t;
    }
    const float x0f = floorf(fx), y0f = floorf(fy);
    t.x0 = (int)x0f; t.y0 = (int)y0f;
    t.x1 = min(t.x0 + 1, R - 1); t.y1 = min(t.y0 + 1, R - 1);
    const float wx0 = (x0f + 1.0f) - fx, wy0 = (y0f + 1.0f) - fy;
    // a pixel beyond the border is skipped by ATen; its weight is 0 there anyway
    const float wx1 = (t.x0 + 1 <= R - 1) ? fx - x0f : 0.0f, wy1 = (t.y0 + 1 <= R - 1) ? fy - y0f : 0.0f;
    t.w[0] = wx0 * wy0; t.w[1] = wx1 * wy0; t.w[2] = wx0 * wy1; t.w[3] = wx1 * wy1;
    return t;
}

// four channels of one plane's sample; cl: the scene's channels-last plane [R][R][C]
__device__ __forceinline__ f32x4 bil_sample(const float *cl, const Bil &t, int R, int C, int c4, bool nearest) {
    auto row = [&](int y, int x) { return reinterpret_cast<const f32x4 *>(cl + ((size_t)y * R + x) * C)[c4]; };
    const f32x4 v00 = row(t.y0, t.x0);
    if (nearest) return v00;
    const f32x4 v01 = row(t.y0, t.x1), v10 = row(t.y1, t.x0), v11 = row(t.y1, t.x1);
    return ((v00 * t.w[0] + v01 * t.w[1]) + v10 * t.w[2]) + v11 * t.w[3];
}

// plane k = 0 (xz), 1 (xy), 2 (yz): the point's coordinates it projects (ops.voxel.PLANES, vt_plane_build)
__device__ __forceinline__ int axis0(int k) { return k == 2 ? 1 : 0; }
__device__ __forceinline__ int axis1(int k) { return k == 1 ? 1 : 2; }

struct PlaneArgs {
    DecodeArgs d;            // pts / N / total / lattice_first / nx / box: the query points (point_of)
    const float *cl[3];      // channels-last copies [B][R][R][C] of xz, xy, yz; null = absent
    float *table[3];         // lattice form: [B][nx^2][C] per present plane
    const float *base;       // [B][N][C] or null
    float *feat;             // [B][N][C]
    int R, C, nearest;
    float divisor, clamp_hi;
};

// [n][C][RR] -> [n][RR][C] for up to three planes (blockIdx.y), one thread per output element
struct LayoutArgs {
    const float *src[3];
    float *dst[3];
    uint32_t n, C, RR;
};
__global__ void __launch_bounds__(256)
planes_to_cl_kernel(LayoutArgs a) {
    const float *src = a.src[blockIdx.y];
    float *dst = a.dst[blockIdx.y];
    if (!src) return;
    const uint64_t total = (uint64_t)a.n * a.RR * a.C;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t c = (uint32_t)(i % a.C);
        const uint64_t t = i / a.C;
        const uint32_t pix = (uint32_t)(t % a.RR), b = (uint32_t)(t / a.RR);
        dst[i] = src[((uint64_t)b * a.C + c) * a.RR + pix];
    }
}
// [n][RR][C] -> [n][C][RR] (the backward's accumulators out to the caller's gradients: every element written)
__global__ void __launch_bounds__(256)
planes_from_cl_kernel(LayoutArgs a) {
    const float *src = a.src[blockIdx.y];
    float *dst = a.dst[blockIdx.y];
    if (!src) return;
    const uint64_t total = (uint64_t)a.n * a.RR * a.C;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t pix = (uint32_t)(i % a.RR);
        const uint64_t t = i / a.RR;
        const uint32_t c = (uint32_t)(t % a.C), b = (uint32_t)(t / a.C);
        dst[i] = src[((uint64_t)b * a.RR + pix) * a.C + c];
    }
}

// thread -> (point slot of the block, 4-channel group): C / 4 lanes share a point
__device__ __forceinline__ bool slot_of(int C, uint32_t &slot, int &c4, uint32_t &per_block) {
    const uint32_t c4n = (uint32_t)C >> 2;
    per_block = 256u / c4n;
    slot = threadIdx.x / c4n;
    c4 = (int)(threadIdx.x - slot * c4n);
    return slot < per_block;
}

// point form: feat[g] = base[g]? + sum over the present planes, in the order xz, xy, yz
__global__ void __launch_bounds__(256)
sample_planes_kernel(PlaneArgs a) {
    uint32_t slot, per_block;
    int c4;
    if (!slot_of(a.C, slot, c4, per_block)) return;
    const bool nearest = a.nearest != 0;
    const size_t plane_floats = (size_t)a.R * a.R * a.C;
    for (uint64_t g64 = (uint64_t)blockIdx.x * per_block + slot; g64 < a.d.total; g64 += (uint64_t)gridDim.x * per_block) {
        const uint32_t g = (uint32_t)g64, b = g / a.d.N, n = g - b * a.d.N;
        float p[3];
        point_of(a.d, g, n, p[0], p[1], p[2]);
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        bool have = false;
        if (a.base) { acc = reinterpret_cast<const f32x4 *>(a.base + (size_t)g * a.C)[c4]; have = true; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!a.cl[k]) continue;
            const Bil t = bil_setup(p[axis0(k)], p[axis1(k)], a.divisor, a.clamp_hi, a.R, nearest);
            const f32x4 s = bil_sample(a.cl[k] + (size_t)b * plane_floats, t, a.R, a.C, c4, nearest);
            acc = have ? acc + s : s;
            have = true;
        }
        reinterpret_cast<f32x4 *>(a.feat + (size_t)g * a.C)[c4] = acc;
    }
}

// lattice form, pass 1: table_k[b][u * nx + v] = plane k's sample at the lattice coordinates (lin(u), lin(v)) of its two axes
__global__ void __launch_bounds__(256)
sample_planes_table_kernel(PlaneArgs a, uint32_t B) {
    uint32_t slot, per_block;
    int c4;
    if (!slot_of(a.C, slot, c4, per_block)) return;
    const int k = blockIdx.y;
    if (!a.cl[k]) return;
    const bool nearest = a.nearest != 0;
    const uint32_t nx = (uint32_t)a.d.nx, nn = nx * nx;
    const uint64_t entries = (uint64_t)B * nn;
    const size_t plane_floats = (size_t)a.R * a.R * a.C;
    for (uint64_t e = (uint64_t)blockIdx.x * per_block + slot; e < entries; e += (uint64_t)gridDim.x * per_block) {
        const uint32_t b = (uint32_t)(e / nn), r = (uint32_t)(e - (uint64_t)b * nn), u = r / nx, v = r - u * nx;
        float pu, pv, unused;
        lattice_point(a.d, u, v, 0u, pu, pv, unused);
        const Bil t = bil_setup(pu, pv, a.divisor, a.clamp_hi, a.R, nearest);
        reinterpret_cast<f32x4 *>(a.table[k] + e * a.C)[c4] = bil_sample(a.cl[k] + (size_t)b * plane_floats, t, a.R, a.C, c4, nearest);
    }
}

// lattice form, pass 2: lattice point (ix, iy, iz) = base? + xz[ix, iz] + xy[ix, iy] + yz[iy, iz], the point form's order
__global__ void __launch_bounds__(256)
sample_planes_sum_kernel(PlaneArgs a) {
    uint32_t slot, per_block;
    int c4;
    if (!slot_of(a.C, slot, c4, per_block)) return;
    const uint32_t nx = (uint32_t)a.d.nx, nn = nx * nx;
    for (uint64_t g64 = (uint64_t)blockIdx.x * per_block + slot; g64 < a.d.total; g64 += (uint64_t)gridDim.x * per_block) {
        const uint32_t g = (uint32_t)g64, b = g / a.d.N, n = g - b * a.d.N;
        const uint32_t m = a.d.lattice_first + n, tq = m / nx, iz = m - tq * nx, ix = tq / nx, iy = tq - ix * nx;
        const uint32_t row[3] = {ix * nx + iz, ix * nx + iy, iy * nx + iz};
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        bool have = false;
        if (a.base) { acc = reinterpret_cast<const f32x4 *>(a.base + (size_t)g * a.C)[c4]; have = true; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!a.table[k]) continue;
            const f32x4 s = reinterpret_cast<const f32x4 *>(a.table[k] + ((size_t)b * nn + row[k]) * a.C)[c4];
            acc = have ? acc + s : s;
            have = true;
        }
        reinterpret_cast<f32x4 *>(a.feat + (size_t)g * a.C)[c4] = acc;
    }
}

// backward: one wave per bilinear cell (blockIdx.y = the 32-channel slice, blockIdx.z = the plane).  order / seg_lo / seg_hi: the
// plane's [B][N] arrays of vt_plane_build_multi at resolution R - 1.  A point whose own pixels differ from its cell head's (a
// 'nearest' point that rounds the other way, a coordinate on a cell boundary) issues its own atomics: the sums do not depend
// on the partition.  acc_cl: the plane's zeroed channels-last accumulator [B][R][R][C].
struct PlaneBwdArgs {
    const float *pts, *grad_feat;
    const int *order, *seg_lo, *seg_hi;      // [K][B][N], the present planes in the order xz, xy, yz
    float *acc_cl[3];                        // by slot 0 .. K-1
    int plane_id[3];                         // slot -> 0 (xz), 1 (xy), 2 (yz)
    uint32_t N, total;
    int R, C, nearest;
    float divisor, clamp_hi;
};
__global__ void __launch_bounds__(256)
sample_planes_bwd_kernel(PlaneBwdArgs a) {
    const int lane = threadIdx.x & 63, ch = (lane & 31) + 32 * blockIdx.y, half = lane >> 5;
    const int slot = blockIdx.z, k = a.plane_id[slot], R = a.R, C = a.C;
    const bool nearest = a.nearest != 0;
    const size_t off = (size_t)slot * a.total;
    const int *order = a.order + off, *seg_lo = a.seg_lo + off, *seg_hi = a.seg_hi + off;
    const int a0 = axis0(k), a1 = axis1(k);
    for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < a.total; g += gridDim.x * 4) {
        const uint32_t b = g / a.N, t = g - b * a.N;
        const int lo = seg_lo[g], hi = seg_hi[g];
        const int *ord = order + (size_t)b * a.N;
        if ((uint32_t)ord[lo] != t) continue;                       // not the first point of its cell: the head's wave does the cell
        const float *ph = a.pts + (size_t)g * 3;
        const Bil head = bil_setup(ph[a0], ph[a1], a.divisor, a.clamp_hi, R, nearest);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float *gb = a.acc_cl[slot] + (size_t)b * R * R * C + ch;
        for (int j = lo + half; j < hi; j += 2) {
            const uint32_t n = (uint32_t)ord[j], gn = b * a.N + n;
            const float *pp = a.pts + (size_t)gn * 3;
            const Bil tr = bil_setup(pp[a0], pp[a1], a.divisor, a.clamp_hi, R, nearest);
            const float v = a.grad_feat[(size_t)gn * C + ch];
            const bool same = tr.x0 == head.x0 && tr.y0 == head.y0 && tr.x1 == head.x1 && tr.y1 == head.y1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (same) acc[q] = fmaf(tr.w[q], v, acc[q]);
                else if (tr.w[q] != 0.0f) {
                    const int yy = (q & 2) ? tr.y1 : tr.y0, xx = (q & 1) ? tr.x1 : tr.x0;
                    atomicAdd(gb + ((size_t)yy * R + xx) * C, tr.w[q] * v);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += __shfl_xor(acc[q], 32);       // even + odd positions of the cell
        if (half == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (acc[q] == 0.0f) continue;
                const int yy = (q & 2) ? head.y1 : head.y0, xx = (q & 1) ? head.x1 : head.x0;
                atomicAdd(gb + ((size_t)yy * R + xx) * C, acc[q]);
            }
        }
    }
}

constexpr int VT_PLANES_MAX_R = 1024;
constexpr int VT_PLANES_MAX_NX = 1625;      // 1625^3 < 2^32 <= 1626^3

// the arguments every entry checks, before any GPU call
int planes_check(const char *who, int n_planes, int B, int R, int C, int64_t N, int flags) {
    char msg[128];
    auto fail = [&](int code, const char *what) { snprintf(msg, sizeof msg, "%s: %s", who, what); return vt_fail(code, msg); };
    if (n_planes == 0) return fail(VT_ERR_INVALID, "no plane given (xz, xy and yz are all null)");
    if (B <= 0 || R < 2 || N < 0) return fail(VT_ERR_INVALID, "bad size");
    if (R > VT_PLANES_MAX_R) return fail(VT_ERR_UNSUPPORTED, "plane resolution above 1024");
    if (C <= 0 || (C & 31) || C > 256) return fail(VT_ERR_UNSUPPORTED, "c_dim must be a multiple of 32, at most 256");
    if ((int64_t)B * N >= (int64_t)1 << 31) return fail(VT_ERR_UNSUPPORTED, "B*N must be < 2^31");
    if (flags & ~(VT_PLANES_NEAREST | VT_PLANES_LATTICE_POINTS | VT_PLANES_PREPARED)) return fail(VT_ERR_INVALID, "unknown flag");
    return 0;
}

unsigned blocks_for(uint64_t rows, unsigned per_block) {
    uint64_t blocks = (rows + per_block - 1) / per_block;
    const uint64_t cap = (uint64_t)16 * vt_num_cus();
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks ? blocks : 1);
}

}  // namespace

extern "C" {

size_t vt_sample_planes_workspace_bytes(int B, int R, int C, int n_planes, int lattice_nx) {
    if (B <= 0 || R < 2 || C <= 0 || n_planes < 1 || n_planes > 3) return 0;
    size_t floats = (size_t)n_planes * B * R * R * C;
    if (lattice_nx >= 2) floats += (size_t)n_planes * B * lattice_nx * lattice_nx * C;
    return floats * sizeof(float);
}

int vt_sample_planes(const float *xz, const float *xy, const float *yz, int B, int R, int C,
                     const float *pts, int64_t N, int lattice_nx, float lattice_box, int64_t lattice_first,
                     double padding, int flags, const float *base, float *feat,
                     void *workspace, size_t workspace_bytes, void *stream) {
    const float *src[3] = {xz, xy, yz};
    const int n_planes = (xz ? 1 : 0) + (xy ? 1 : 0) + (yz ? 1 : 0);
    int rc = planes_check("vt_sample_planes", n_planes, B, R, C, N, flags);
    if (rc) return rc;
    if (!feat || !workspace) return vt_fail(VT_ERR_INVALID, "vt_sample_planes: null argument");
    if (((uintptr_t)feat | (uintptr_t)base | (uintptr_t)workspace) & 15) return vt_fail(VT_ERR_INVALID, "vt_sample_planes: base, feat and workspace must be 16-byte aligned");
    if (!pts) {
        // (the kernels carry lattice indices in 32 bits, as vt_sample_grid and the decode kernels do: nx^3 must fit)
        if (lattice_nx < 2) return vt_fail(VT_ERR_INVALID, "vt_sample_planes: lattice mode needs nx >= 2");
        if (lattice_nx > VT_PLANES_MAX_NX) return vt_fail(VT_ERR_UNSUPPORTED, "vt_sample_planes: lattice nx above 1625 (nx^3 must stay below 2^32)");
        const int64_t all = (int64_t)lattice_nx * lattice_nx * lattice_nx;
        if (lattice_first < 0 || lattice_first + N > all) return vt_fail(VT_ERR_INVALID, "vt_sample_planes: lattice range outside nx^3");
    }
    const bool tables = !pts && !(flags & VT_PLANES_LATTICE_POINTS);
    const size_t cl_floats = (size_t)B * R * R * C, tab_floats = tables ? (size_t)B * lattice_nx * lattice_nx * C : 0;
    if (workspace_bytes < (size_t)n_planes * (cl_floats + tab_floats) * sizeof(float))
        return vt_fail(VT_ERR_WORKSPACE, "vt_sample_planes: workspace too small (vt_sample_planes_workspace_bytes)");
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    PlaneArgs a{};
    a.d.pts = pts; a.d.N = (uint32_t)N; a.d.total = (uint32_t)((int64_t)B * N); a.d.lattice_first = (uint32_t)lattice_first;
    a.d.nx = lattice_nx; a.d.box = lattice_box; a.d.R = R;
    a.base = base; a.feat = feat; a.R = R; a.C = C; a.nearest = (flags & VT_PLANES_NEAREST) ? 1 : 0;
    a.divisor = (float)(1.0 + padding + 10e-6); a.clamp_hi = (float)(1.0 - 10e-6);      // src/common.py:283, 288, rounded to f32 as torch does
    LayoutArgs l{};
    l.n = (uint32_t)B; l.C = (uint32_t)C; l.RR = (uint32_t)R * (uint32_t)R;
    float *w = (float *)workspace;
    for (int k = 0; k < 3; ++k) {
        l.src[k] = src[k]; l.dst[k] = nullptr; a.cl[k] = nullptr; a.table[k] = nullptr;
        if (src[k]) { l.dst[k] = w; a.cl[k] = w; w += cl_floats; }
    }
    for (int k = 0; k < 3; ++k)
        if (src[k] && tables) { a.table[k] = w; w += tab_floats; }
    // VT_PLANES_PREPARED: the workspace still holds what an earlier call with the same planes (and lattice nx, box) left there
    const bool prepared = (flags & VT_PLANES_PREPARED) != 0;
    if (!prepared) hipLaunchKernelGGL(planes_to_cl_kernel, dim3(blocks_for(cl_floats, 256), 3), dim3(256), 0, s, l);
    const unsigned per_block = 256u / ((unsigned)C >> 2);
    if (tables) {
        if (!prepared) hipLaunchKernelGGL(sample_planes_table_kernel, dim3(blocks_for((uint64_t)B * lattice_nx * lattice_nx, per_block), 3), dim3(256), 0, s, a, (uint32_t)B);
        hipLaunchKernelGGL(sample_planes_sum_kernel, dim3(blocks_for(a.d.total, per_block)), dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(sample_planes_kernel, dim3(blocks_for(a.d.total, per_block)), dim3(256), 0, s, a);
    }
    return vt_check(hipGetLastError(), "vt_sample_planes");
}

size_t vt_sample_planes_bwd_workspace_bytes(int B, int64_t N, int R, int C, int n_planes) {
    if (B <= 0 || N < 0 || R < 2 || C <= 0 || n_planes < 1 || n_planes > 3) return 0;
    return (size_t)n_planes * ((size_t)B * R * R * C * sizeof(float) + 4 * (size_t)B * (size_t)N * sizeof(int));
}

int vt_sample_planes_bwd(int B, int R, int C, const float *pts, int64_t N, double padding, int flags,
                         const float *grad_feat, float *grad_xz, float *grad_xy, float *grad_yz,
                         void *workspace, size_t workspace_bytes, void *stream) {
    float *dst[3] = {grad_xz, grad_xy, grad_yz};
    const int n_planes = (grad_xz ? 1 : 0) + (grad_xy ? 1 : 0) + (grad_yz ? 1 : 0);
    int rc = planes_check("vt_sample_planes_bwd", n_planes, B, R, C, N, flags);
    if (rc) return rc;
    if (flags & (VT_PLANES_LATTICE_POINTS | VT_PLANES_PREPARED)) return vt_fail(VT_ERR_INVALID, "vt_sample_planes_bwd: only VT_PLANES_NEAREST applies to the backward");
    if (!pts || !grad_feat || !workspace) return vt_fail(VT_ERR_INVALID, "vt_sample_planes_bwd: null argument");
    if ((uintptr_t)workspace & 15) return vt_fail(VT_ERR_INVALID, "vt_sample_planes_bwd: workspace must be 16-byte aligned");
    if (workspace_bytes < vt_sample_planes_bwd_workspace_bytes(B, N, R, C, n_planes))
        return vt_fail(VT_ERR_WORKSPACE, "vt_sample_planes_bwd: workspace too small (vt_sample_planes_bwd_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const size_t cl_floats = (size_t)B * R * R * C, idx_ints = (size_t)n_planes * B * (size_t)N;
    float *acc = (float *)workspace;
    int *ints = (int *)(acc + (size_t)n_planes * cl_floats);
    PlaneBwdArgs a{};
    LayoutArgs l{};
    l.n = (uint32_t)B; l.C = (uint32_t)C; l.RR = (uint32_t)R * (uint32_t)R;
    int ids[3] = {0, 0, 0}, slot = 0;
    for (int k = 0; k < 3; ++k) {
        l.src[k] = nullptr; l.dst[k] = dst[k]; a.acc_cl[k] = nullptr; a.plane_id[k] = 0;
        if (dst[k]) { l.src[k] = acc + (size_t)slot * cl_floats; a.acc_cl[slot] = acc + (size_t)slot * cl_floats; a.plane_id[slot] = k; ids[slot] = k; ++slot; }
    }
    rc = vt_fill32(acc, 0u, (size_t)n_planes * cl_floats * sizeof(float), s);
    if (rc) return rc;
    if (N > 0) {
        // a point's bin at resolution R - 1 is the cell whose four pixels it touches
        rc = vt_plane_build_multi(pts, B, (int)N, R - 1, padding, n_planes, ids, ints, ints + idx_ints, ints + 2 * idx_ints, ints + 3 * idx_ints, stream);
        if (rc) return rc;
        a.pts = pts; a.grad_feat = grad_feat;
        a.order = ints + idx_ints; a.seg_lo = ints + 2 * idx_ints; a.seg_hi = ints + 3 * idx_ints;
        a.N = (uint32_t)N; a.total = (uint32_t)((int64_t)B * N); a.R = R; a.C = C; a.nearest = (flags & VT_PLANES_NEAREST) ? 1 : 0;
        a.divisor = (float)(1.0 + padding + 10e-6); a.clamp_hi = (float)(1.0 - 10e-6);
        int64_t blocks = ((int64_t)a.total + 3) / 4;
        const int64_t cap = 32 * vt_num_cus();
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(sample_planes_bwd_kernel, dim3((unsigned)blocks, (unsigned)(C / 32), (unsigned)n_planes), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(planes_from_cl_kernel, dim3(blocks_for(cl_floats, 256), 3), dim3(256), 0, s, l);
    return vt_check(hipGetLastError(), "vt_sample_planes_bwd");
}

}  // extern "C"
