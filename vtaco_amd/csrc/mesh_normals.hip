// Normals of a triangle mesh on the device: unit face normals and vertex normals weighted by face area or by corner angle (DESIGN.md,
// section "mesh_normals.hip"; tests/mesh_normals_ref.py restates the rule in numpy).  faces [F,3] i32 and vertices [V,3] f32 or f64 as
// vt_mc_emit leaves them; coordinates are widened exactly and every operation is float64, unfused (-ffp-contract=off).
//   face          c = (v1 - v0) x (v2 - v0), l2 = (cx cx + cy cy) + cz cz.  The face is degenerate unless l2 is positive and finite; its
//                 normal is c / sqrt(l2), (0,0,0) when degenerate.
//   terms         a live face adds one term to each of its three vertices: 'area' the raw cross product c, 'angle' the unit normal
//                 times the interior angle at that corner, atan2(sqrt(l2), e1 . e2) with e1, e2 the two edges that leave the corner.
//   sums          EXACT, as the component sums of mesh_topo.hip: a first face pass takes every vertex's largest |term component|
//                 (atomicMax on the bit pattern), a second adds each component as two int64 fixed-point limbs scaled by that maximum's
//                 exponent.  Integer addition is associative: no float atomic, equal bits from run to run and under any order of the
//                 faces.  A term's error is at most 2^-62 of the vertex's largest term component; 2^31 faces may meet in a vertex.
//   vertex        the three sums stay in the fixed-point scale (|s| < 2^63, squares cannot overflow or vanish) and are normalised
//                 there: s / sqrt((sx sx + sy sy) + sz sz); (0,0,0) for a vertex no live face touches or whose terms cancel exactly.
// A face with an index outside [0, V) is never dereferenced; it sets bit 0 of the status word and the call fails.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_common.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

enum { ST_BAD = 0 };                             // (MT_STATUS_BYTES of int32 words: mesh_common.h)
enum { W_AREA = 0, W_ANGLE = 1 };

struct FaceGeom {
    double cx, cy, cz;                           // the raw cross product
    double nx, ny, nz;                           // the unit normal, zero when degenerate
    double len;
    bool live;
    double px[3], py[3], pz[3];
};

template <class T>
__device__ inline void face_geom(const T *verts, int a, int b, int c, FaceGeom &g) {
    load_vertex(verts, a, g.px[0], g.py[0], g.pz[0]);
    load_vertex(verts, b, g.px[1], g.py[1], g.pz[1]);
    load_vertex(verts, c, g.px[2], g.py[2], g.pz[2]);
    const double ux = g.px[1] - g.px[0], uy = g.py[1] - g.py[0], uz = g.pz[1] - g.pz[0];
    const double wx = g.px[2] - g.px[0], wy = g.py[2] - g.py[0], wz = g.pz[2] - g.pz[0];
    g.cx = uy * wz - uz * wy; g.cy = uz * wx - ux * wz; g.cz = ux * wy - uy * wx;
    const double l2 = (g.cx * g.cx + g.cy * g.cy) + g.cz * g.cz;
    g.live = l2 > 0.0 && l2 < __longlong_as_double(0x7ff0000000000000ll);
    g.len = g.live ? sqrt(l2) : 0.0;
    g.nx = g.live ? g.cx / g.len : 0.0;
    g.ny = g.live ? g.cy / g.len : 0.0;
    g.nz = g.live ? g.cz / g.len : 0.0;
}

// the term of corner k (0, 1, 2) of a live face
template <int WEIGHT>
__device__ inline void corner_term(const FaceGeom &g, int k, double &tx, double &ty, double &tz) {
    if (WEIGHT == W_AREA) { tx = g.cx; ty = g.cy; tz = g.cz; return; }
    const int k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const double e1x = g.px[k1] - g.px[k], e1y = g.py[k1] - g.py[k], e1z = g.pz[k1] - g.pz[k];
    const double e2x = g.px[k2] - g.px[k], e2y = g.py[k2] - g.py[k], e2z = g.pz[k2] - g.pz[k];
    const double dot = (e1x * e2x + e1y * e2y) + e1z * e2z;
    const double ang = atan2(g.len, dot);
    tx = ang * g.nx; ty = ang * g.ny; tz = ang * g.nz;
}

// PASS 0: the face normals and every vertex's largest |term component|; PASS 1: the fixed-point sums against them.
// vmax [V] u64 (null: face normals only), sums [V][6] u64: limbs hi, lo of x, y, z.
template <class T, int WEIGHT, int PASS>
__global__ void __launch_bounds__(MT_THREADS)
normals_face_kernel(const T *verts, int V, const int32_t *faces, int F, T *face_normals, u64 *vmax, u64 *sums, int32_t *status) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    if (!ok) {
        if (PASS == 0) {
            atomicOr(status + ST_BAD, 1);
            if (face_normals)
                for (int k = 0; k < 3; ++k) face_normals[(size_t)f * 3 + k] = (T)0;
        }
        return;
    }
    FaceGeom g;
    face_geom(verts, a, b, c, g);
    if (PASS == 0 && face_normals) {
        face_normals[(size_t)f * 3] = (T)g.nx; face_normals[(size_t)f * 3 + 1] = (T)g.ny; face_normals[(size_t)f * 3 + 2] = (T)g.nz;
    }
    if (!g.live || !vmax) return;
    const int idx[3] = {a, b, c};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double tx, ty, tz;
        corner_term<WEIGHT>(g, k, tx, ty, tz);
        const int v = idx[k];                     // (0 <= v < V: ok)
        if (PASS == 0) {
            const double m = fmax(fmax(fabs(tx), fabs(ty)), fabs(tz));
            atomicMax(vmax + v, (u64)__double_as_longlong(m));
        } else {
            const int e = exponent_of(vmax[v]);
            u64 hi, lo;
            limbs_of(tx, e, hi, lo); atomicAdd(sums + (size_t)v * 6, hi); atomicAdd(sums + (size_t)v * 6 + 1, lo);
            limbs_of(ty, e, hi, lo); atomicAdd(sums + (size_t)v * 6 + 2, hi); atomicAdd(sums + (size_t)v * 6 + 3, lo);
            limbs_of(tz, e, hi, lo); atomicAdd(sums + (size_t)v * 6 + 4, hi); atomicAdd(sums + (size_t)v * 6 + 5, lo);
        }
    }
}

template <class T>
__global__ void __launch_bounds__(MT_THREADS) normals_vertex_kernel(const u64 *sums, int V, T *vertex_normals) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v >= V) return;
    const u64 *s = sums + (size_t)v * 6;
    const double sx = sum_of(s[0], s[1], 30), sy = sum_of(s[2], s[3], 30), sz = sum_of(s[4], s[5], 30);    // (e = 30: the limbs' own scale)
    const double l2 = (sx * sx + sy * sy) + sz * sz;
    const double len = sqrt(l2);
    const bool any = l2 > 0.0;
    vertex_normals[(size_t)v * 3] = any ? (T)(sx / len) : (T)0;
    vertex_normals[(size_t)v * 3 + 1] = any ? (T)(sy / len) : (T)0;
    vertex_normals[(size_t)v * 3 + 2] = any ? (T)(sz / len) : (T)0;
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && F >= 1 && V <= MT_MAX_V && F <= MT_MAX_F; }

size_t normals_bytes(int64_t V) { return MT_STATUS_BYTES + up256((size_t)V * 8) + up256((size_t)V * 6 * 8); }

template <class T, int WEIGHT>
void normals_launch(const T *verts, int V, const int32_t *faces, int F, T *fn, T *vn, u64 *vmax, u64 *sums, int32_t *status, hipStream_t st) {
    const dim3 grid(blocks_of(F, MT_THREADS)), block(MT_THREADS);
    hipLaunchKernelGGL((normals_face_kernel<T, WEIGHT, 0>), grid, block, 0, st, verts, V, faces, F, fn, vn ? vmax : (u64 *)nullptr, sums, status);
    if (!vn) return;
    hipLaunchKernelGGL((normals_face_kernel<T, WEIGHT, 1>), grid, block, 0, st, verts, V, faces, F, (T *)nullptr, vmax, sums, status);
    hipLaunchKernelGGL(normals_vertex_kernel<T>, dim3(blocks_of(V, MT_THREADS)), block, 0, st, (const u64 *)sums, V, vn);
}

}  // namespace

extern "C" {

size_t vt_mesh_normals_workspace_bytes(int64_t V, int64_t F) { return sizes_ok(V, F) ? normals_bytes(V) : 0; }

int vt_mesh_normals(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int weight, void *face_normals,
                    void *vertex_normals, void *workspace, size_t workspace_bytes, void *stream) {
    if (!sizes_ok(V, F) || !verts || !faces || (!face_normals && !vertex_normals) || (weight != W_AREA && weight != W_ANGLE))
        return vt_fail(VT_ERR_INVALID, "vt_mesh_normals: bad argument (V >= 1, F >= 1, weight 0 or 1, at least one output)");
    if (!workspace || workspace_bytes < normals_bytes(V)) return vt_fail(VT_ERR_WORKSPACE, "vt_mesh_normals");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    int32_t *status = reinterpret_cast<int32_t *>(ws);
    u64 *vmax = reinterpret_cast<u64 *>(ws + MT_STATUS_BYTES);
    u64 *sums = reinterpret_cast<u64 *>(ws + MT_STATUS_BYTES + up256((size_t)V * 8));
    int rc = vt_fill32(ws, 0u, vertex_normals ? normals_bytes(V) : MT_STATUS_BYTES, st);
    if (rc) return rc;
    if (verts_f64) {
        const double *p = static_cast<const double *>(verts);
        double *fn = static_cast<double *>(face_normals), *vn = static_cast<double *>(vertex_normals);
        if (weight == W_AREA) normals_launch<double, W_AREA>(p, (int)V, faces, (int)F, fn, vn, vmax, sums, status, st);
        else normals_launch<double, W_ANGLE>(p, (int)V, faces, (int)F, fn, vn, vmax, sums, status, st);
    } else {
        const float *p = static_cast<const float *>(verts);
        float *fn = static_cast<float *>(face_normals), *vn = static_cast<float *>(vertex_normals);
        if (weight == W_AREA) normals_launch<float, W_AREA>(p, (int)V, faces, (int)F, fn, vn, vmax, sums, status, st);
        else normals_launch<float, W_ANGLE>(p, (int)V, faces, (int)F, fn, vn, vmax, sums, status, st);
    }
    rc = vt_check(hipGetLastError(), "vt_mesh_normals");
    if (rc) return rc;
    int32_t h[16];
    hipError_t e = hipMemcpyAsync(h, workspace, sizeof h, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    rc = vt_check(e, "vt_mesh_normals");
    if (rc) return rc;
    if (h[ST_BAD]) return vt_fail(VT_ERR_INVALID, "vt_mesh_normals: a face index lies outside [0, V)");
    return 0;
}

}  // extern "C"
