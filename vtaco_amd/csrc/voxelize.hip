// Mesh -> occupancy volume, for VoxelGrid.from_mesh (src/utils/voxels.py:16-42, 201-216).  The reference calls voxelize_surface and
// voxelize_interior there, which it never defines (upstream they were Cython extensions); the definitions here are DESIGN.md's section
// "voxelize.hip", restated in numpy by tests/voxelize_ref.py.
//   grid units  g = ((v - loc) / scale + 0.5) * res per component, in that order, float64 from the float32 vertices;
//               voxel (i, j, k) is the closed box [i, i+1] x [j, j+1] x [k, k+1] with centre (i+.5, j+.5, k+.5)
//   surface     box / triangle overlap by the 13-axis separating-axis test (equality = overlap) over the triangle's clipped bounding box
//   interior    parity of the crossings of the +z ray from every voxel centre, accumulated per triangle with XOR
//   fill        scipy.ndimage.binary_fill_holes (6-connectivity): `outside` spreads from the grid's boundary in line sweeps
// All predicates are plain float64 products and sums (the tree is built with -ffp-contract=off; no fma, no fast-math): two triangles
// that share an edge must see exactly opposite edge functions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

constexpr int VX_THREADS = 256;
constexpr int VX_WAVE = 64;
constexpr int VX_TRIS = VX_THREADS / VX_WAVE;      // one wave per triangle, four triangles per workgroup

struct VxFrame { double lx, ly, lz, scale, res; };

__device__ inline double vx_grid(float v, double loc, double scale, double res) { return (((double)v - loc) / scale + 0.5) * res; }

// the triangle `tri` in grid units; false when a vertex index is outside [0, V) (the host refuses such meshes; this keeps reads in bounds)
__device__ inline bool vx_load(const float *verts, int V, const int32_t *faces, int tri, const VxFrame &fr, int idx[3], double p[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        idx[k] = faces[3 * (size_t)tri + k];
        if (idx[k] < 0 || idx[k] >= V) return false;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k][0] = vx_grid(verts[3 * (size_t)idx[k]], fr.lx, fr.scale, fr.res);
        p[k][1] = vx_grid(verts[3 * (size_t)idx[k] + 1], fr.ly, fr.scale, fr.res);
        p[k][2] = vx_grid(verts[3 * (size_t)idx[k] + 2], fr.lz, fr.scale, fr.res);
    }
    return true;
}

__device__ inline double vx_min3(double a, double b, double c) { return fmin(a, fmin(b, c)); }
__device__ inline double vx_max3(double a, double b, double c) { return fmax(a, fmax(b, c)); }

// clamp a double that may be far outside the int range (or NaN: -> lo) before the cast
__device__ inline int vx_clampi(double x, int lo, int hi) { return x >= (double)lo ? (x <= (double)hi ? (int)x : hi) : lo; }

// true when the axis (ax, ay, az) separates the box of half-width .5 at the origin from the triangle q (already relative to the centre)
__device__ inline bool vx_separates(double ax, double ay, double az, const double q[3][3]) {
    const double d0 = q[0][0] * ax + q[0][1] * ay + q[0][2] * az;
    const double d1 = q[1][0] * ax + q[1][1] * ay + q[1][2] * az;
    const double d2 = q[2][0] * ax + q[2][1] * ay + q[2][2] * az;
    const double r = 0.5 * (fabs(ax) + fabs(ay) + fabs(az));
    return vx_min3(d0, d1, d2) > r || vx_max3(d0, d1, d2) < -r;
}

__global__ void __launch_bounds__(VX_THREADS)
voxelize_surface_kernel(const float *verts, int V, const int32_t *faces, int F, VxFrame fr, int res, uint8_t *occ) {
    const int tri = blockIdx.x * VX_TRIS + threadIdx.x / VX_WAVE, lane = threadIdx.x % VX_WAVE;
    if (tri >= F) return;
    int idx[3];
    double p[3][3];
    if (!vx_load(verts, V, faces, tri, fr, idx, p)) return;
    int lo[3], n[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {                                  // closed boxes: i + 1 >= min and i <= max
        lo[a] = vx_clampi(ceil(vx_min3(p[0][a], p[1][a], p[2][a])) - 1.0, 0, res);
        const int hi = vx_clampi(floor(vx_max3(p[0][a], p[1][a], p[2][a])), -1, res - 1);
        n[a] = hi - lo[a] + 1;
        if (n[a] <= 0) return;
    }
    double e[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { e[0][a] = p[1][a] - p[0][a]; e[1][a] = p[2][a] - p[1][a]; e[2][a] = p[0][a] - p[2][a]; }
    const double nx = e[0][1] * e[1][2] - e[0][2] * e[1][1], ny = e[0][2] * e[1][0] - e[0][0] * e[1][2], nz = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    const int cells = n[0] * n[1] * n[2];                          // <= 512^3 = 2^27
    for (int c = lane; c < cells; c += VX_WAVE) {
        const int k = c % n[2], ij = c / n[2];
        const int j = ij % n[1], i = ij / n[1];
        const int vi = lo[0] + i, vj = lo[1] + j, vk = lo[2] + k;
        const double cx = vi + 0.5, cy = vj + 0.5, cz = vk + 0.5;
        double q[3][3];
#pragma unroll
        for (int m = 0; m < 3; ++m) { q[m][0] = p[m][0] - cx; q[m][1] = p[m][1] - cy; q[m][2] = p[m][2] - cz; }
        bool sep = vx_separates(1.0, 0.0, 0.0, q) || vx_separates(0.0, 1.0, 0.0, q) || vx_separates(0.0, 0.0, 1.0, q) || vx_separates(nx, ny, nz, q);
#pragma unroll
        for (int m = 0; m < 3; ++m) {                              // e_m x (1,0,0), e_m x (0,1,0), e_m x (0,0,1)
            sep = sep || vx_separates(0.0, e[m][2], -e[m][1], q) || vx_separates(-e[m][2], 0.0, e[m][0], q) || vx_separates(e[m][1], -e[m][0], 0.0, q);
        }
        if (!sep) occ[((size_t)vi * res + vj) * res + vk] = 1;     // every writer stores 1: the order cannot matter
    }
}

// the edge function of the edge the triangle walks ia -> ib at the centre (cx, cy), as a sign in {-1, +1} and a value: evaluated on the
// canonical direction (lower vertex index first) and negated when the walk is the other way; an exact 0 is decided as if the centre sat
// at (+eps, +eps^2): the sign of -(by - ay), then of (bx - ax)
__device__ inline int vx_edge(int ia, int ib, const double *pa, const double *pb, double cx, double cy, double *value) {
    const bool flip = ia > ib;
    const double ax = flip ? pb[0] : pa[0], ay = flip ? pb[1] : pa[1], bx = flip ? pa[0] : pb[0], by = flip ? pa[1] : pb[1];
    const double dx = bx - ax, dy = by - ay;
    const double val = dx * (cy - ay) - dy * (cx - ax);
    const double tie = dy != 0.0 ? -dy : dx;
    const double dec = val != 0.0 ? val : tie;
    const int s = dec > 0.0 ? 1 : -1;
    *value = flip ? -val : val;
    return flip ? -s : s;
}

__global__ void __launch_bounds__(VX_THREADS)
voxelize_interior_kernel(const float *verts, int V, const int32_t *faces, int F, VxFrame fr, int res, int words, uint32_t *bits) {
    const int tri = blockIdx.x * VX_TRIS + threadIdx.x / VX_WAVE, lane = threadIdx.x % VX_WAVE;
    if (tri >= F) return;
    int idx[3];
    double p[3][3];
    if (!vx_load(verts, V, faces, tri, fr, idx, p)) return;
    const double A = (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0]);
    if (!(A != 0.0) || A != A) return;                             // projected area 0 (or NaN): no crossing
    const int sa = A > 0.0 ? 1 : -1;
    int lo[2], n[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {                                  // centres i + .5 inside [min, max]
        lo[a] = vx_clampi(ceil(vx_min3(p[0][a], p[1][a], p[2][a]) - 0.5), 0, res);
        const int hi = vx_clampi(floor(vx_max3(p[0][a], p[1][a], p[2][a]) - 0.5), -1, res - 1);
        n[a] = hi - lo[a] + 1;
        if (n[a] <= 0) return;
    }
    const int cols = n[0] * n[1];
    for (int c = lane; c < cols; c += VX_WAVE) {
        const int j = c % n[1], i = c / n[1];
        const int vi = lo[0] + i, vj = lo[1] + j;
        const double cx = vi + 0.5, cy = vj + 0.5;
        double e0, e1, e2;
        const int s0 = vx_edge(idx[1], idx[2], p[1], p[2], cx, cy, &e0);
        const int s1 = vx_edge(idx[2], idx[0], p[2], p[0], cx, cy, &e1);
        const int s2 = vx_edge(idx[0], idx[1], p[0], p[1], cx, cy, &e2);
        if (s0 != sa || s1 != sa || s2 != sa) continue;
        const double z = (e0 * p[0][2] + e1 * p[1][2] + e2 * p[2][2]) / A;
        const int cnt = vx_clampi(ceil(z - 0.5), 0, res);          // the rays from the centres k + .5 < z cross: flip k < cnt
        uint32_t *col = bits + ((size_t)vi * res + vj) * words;
        for (int w = 0; w * 32 < cnt; ++w) {
            const int left = cnt - w * 32;
            atomicXor(col + w, left >= 32 ? 0xffffffffu : ((1u << left) - 1u));
        }
    }
}

// one sweep of the fill: one thread per grid line along `axis`, forward or backward.  Beyond the grid is outside; an unoccupied voxel
// next to an outside one (along the line) becomes outside.  Lines are disjoint, so a launch has no two writers of one byte.
__global__ void __launch_bounds__(VX_THREADS)
voxel_fill_sweep_kernel(const uint8_t *occ, int res, int axis, int backward, uint8_t *outside, int32_t *changed) {
    const int line = blockIdx.x * VX_THREADS + threadIdx.x;
    if (line >= res * res) return;
    const int a = line / res, b = line % res;
    const size_t r = (size_t)res;
    size_t base, step;
    if (axis == 0) { base = (size_t)a * r + b; step = r * r; }          // lines along x: (y, z) = (a, b)
    else if (axis == 1) { base = (size_t)a * r * r + b; step = r; }     // along y: (x, z)
    else { base = ((size_t)a * r + b) * r; step = 1; }                  // along z: (x, y)
    bool prev = true, any = false;
    for (int t = 0; t < res; ++t) {
        const size_t v = base + (size_t)(backward ? res - 1 - t : t) * step;
        if (occ[v]) { prev = false; continue; }
        const bool was = outside[v] != 0;
        if (prev && !was) { outside[v] = 1; any = true; }
        prev = prev || was;
    }
    if (any) *changed = 1;
}

int vx_check_args(const char *who, const void *verts, int V, const void *faces, int F, const double *loc, double scale, int res, const void *out) {
    if (res < 1 || res > VT_VOXELIZE_MAX_RES) return vt_fail(VT_ERR_INVALID, who);
    if (V < 0 || F < 0 || !loc || !out || !(scale > 0.0) || ((V > 0 && F > 0) && (!verts || !faces))) return vt_fail(VT_ERR_INVALID, who);
    return 0;
}

}  // namespace

extern "C" {

int vt_voxelize_surface(const float *verts, int V, const int32_t *faces, int F, const double *loc, double scale, int res, uint8_t *occ, void *stream) {
    if (int rc = vx_check_args("vt_voxelize_surface: bad argument (1 <= res <= 512, scale > 0)", verts, V, faces, F, loc, scale, res, occ)) return rc;
    if (V == 0 || F == 0) return 0;
    const VxFrame fr{loc[0], loc[1], loc[2], scale, (double)res};
    hipLaunchKernelGGL(voxelize_surface_kernel, dim3((unsigned)((F + VX_TRIS - 1) / VX_TRIS)), dim3(VX_THREADS), 0, (hipStream_t)stream,
                       verts, V, faces, F, fr, res, occ);
    return vt_check(hipGetLastError(), "vt_voxelize_surface");
}

int vt_voxelize_interior(const float *verts, int V, const int32_t *faces, int F, const double *loc, double scale, int res, uint32_t *bits, void *stream) {
    if (int rc = vx_check_args("vt_voxelize_interior: bad argument (1 <= res <= 512, scale > 0)", verts, V, faces, F, loc, scale, res, bits)) return rc;
    if (V == 0 || F == 0) return 0;
    const VxFrame fr{loc[0], loc[1], loc[2], scale, (double)res};
    hipLaunchKernelGGL(voxelize_interior_kernel, dim3((unsigned)((F + VX_TRIS - 1) / VX_TRIS)), dim3(VX_THREADS), 0, (hipStream_t)stream,
                       verts, V, faces, F, fr, res, (res + 31) / 32, bits);
    return vt_check(hipGetLastError(), "vt_voxelize_interior");
}

int vt_voxel_fill(const uint8_t *occ, int res, uint8_t *outside, int32_t *changed, void *stream) {
    if (res < 1 || res > VT_VOXELIZE_MAX_RES || !occ || !outside || !changed) return vt_fail(VT_ERR_INVALID, "vt_voxel_fill: bad argument (1 <= res <= 512)");
    const unsigned blocks = (unsigned)((res * res + VX_THREADS - 1) / VX_THREADS);
    for (int axis = 0; axis < 3; ++axis)
        for (int backward = 0; backward < 2; ++backward)
            hipLaunchKernelGGL(voxel_fill_sweep_kernel, dim3(blocks), dim3(VX_THREADS), 0, (hipStream_t)stream, occ, res, axis, backward, outside, changed);
    return vt_check(hipGetLastError(), "vt_voxel_fill");
}

}  // extern "C"
