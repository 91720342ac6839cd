// Closest point on a triangle mesh, for the hand metrics of the reference's eval_step (src/conv_onet/training.py:399-419: the penetration
// depth of the predicted hand is trimesh.proximity.closest_point over the hand vertices the winding number puts inside the object) and
// for mesh-against-mesh distances.  The definitions are DESIGN.md's section "closest_point.hip", restated in numpy by
// tests/closest_point_ref.py (by_regions: this file's operations in this file's order).
//   inputs      verts [V,3] f32, faces [F,3] i32, pts [N,3] f32; every number below is float64 on the exactly converted inputs
//   prepare     one record per face, gathered once: corner a, edges ab = b - a and ac = c - a, ab.ab, ab.ac, ac.ac, and a kind:
//               0 regular, 1 degenerate (the normal ab x ac is exactly zero: a repeated index or collinear corners; the face is then the
//               union of its three edges), 2 skipped (an index outside [0, V): reported through the status word, never dereferenced)
//   regular     the seven Voronoi regions of the closed triangle from d1 = ab.ap, d2 = ac.ap and the record's three products
//               (d3 = d1 - ab.ab, d4 = d2 - ab.ac, d5 = d1 - ab.ac, d6 = d2 - ac.ac), tested in the order a, b, ab, c, ac, bc, inside;
//               the region picks two numerators and one denominator, (v, w) = (nv / den, nw / den), q = (a + ab v) + ac w,
//               d2 = ((p - q)_x^2 + (p - q)_y^2) + (p - q)_z^2.  A denominator that is not > 0 (cancellation far from a sliver)
//               gives the corner a: never NaN
//   minimum     over the faces in ascending order with a strict <: equal minima give the lowest face index
// Work is tiled both ways: a workgroup takes 256 queries (one per thread) and one slab of faces, staged through LDS in chunks of 256
// records that every lane of a wave reads at the same address (broadcast); it writes one partial minimum per (query, slab).  The finish
// pass takes a query's partials in ascending slab order and recomputes the point on the winning face.  No atomics on a result: the
// outputs are bit-reproducible and do not depend on the slab size.  All products and sums are separate roundings (-ffp-contract=off).
// Replaces: trimesh.proximity.closest_point(mesh, points) of the reference's eval_step (src/conv_onet/training.py:413-416).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "closest_point_face.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

constexpr int CP_THREADS = 256;                 // queries per workgroup, and records per LDS chunk
constexpr int CP_MIN_CHUNKS = 2;                // chunks per slab at least: every mesh beyond 256 faces walks the re-staging loop
constexpr int CP_TARGET_BLOCKS = 2048;          // workgroups wanted per launch: 8 per CU
constexpr size_t CP_HEAD = 256;                 // bytes in front of a scene's workspace block; the call's status word is the first of block 0

struct CpScene { const float *verts; const int32_t *faces; int V, F; };        // vt_winding_number_scenes' record
static_assert(sizeof(CpScene) == 24, "scene records are 24 bytes");

struct CpPlan { int slab_faces, slabs; size_t rec_off, pd2_off, pface_off, block_bytes; };

// how F faces and N queries (times B scenes) are cut: slabs of whole chunks, as many as fill the device, at least CP_MIN_CHUNKS chunks each
CpPlan cp_plan(int64_t F, int64_t N, int B) {
    const int64_t qtiles = (N + CP_THREADS - 1) / CP_THREADS * (B > 0 ? B : 1);
    const int64_t chunks = (F + CP_THREADS - 1) / CP_THREADS;
    int64_t want = CP_TARGET_BLOCKS / (qtiles > 0 ? qtiles : 1);
    if (want < 1) want = 1;
    int64_t per = (chunks + want - 1) / want;
    if (per < CP_MIN_CHUNKS) per = CP_MIN_CHUNKS;
    CpPlan p;
    p.slab_faces = (int)(per * CP_THREADS);
    p.slabs = (int)((chunks + per - 1) / per);
    if (p.slabs < 1) p.slabs = 1;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    p.rec_off = CP_HEAD;
    p.pd2_off = p.rec_off + up((size_t)F * CP_REC * sizeof(double));
    p.pface_off = p.pd2_off + up((size_t)N * p.slabs * sizeof(double));
    p.block_bytes = p.pface_off + up((size_t)N * p.slabs * sizeof(int32_t));
    return p;
}

__global__ void __launch_bounds__(CP_THREADS)
closest_point_prepare_kernel(const float *verts, int V, const int32_t *faces, int F, const CpScene *scenes, int max_F, char *ws, size_t block_bytes,
                             size_t rec_off) {
    int32_t *status = reinterpret_cast<int32_t *>(ws);
    if (scenes) {
        const CpScene sc = scenes[blockIdx.y];
        verts = sc.verts; V = sc.V; faces = sc.faces; F = sc.F;
        if (V <= 0 || F <= 0 || F > max_F || !verts || !faces) {
            if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, CP_BAD_SCENE);
            return;
        }
    }
    const int f = blockIdx.x * CP_THREADS + threadIdx.x;
    if (f >= F) return;
    double *rec = reinterpret_cast<double *>(ws + (size_t)blockIdx.y * block_bytes + rec_off) + (size_t)f * CP_REC;
    if (!cp_fill_record(verts, V, faces, (size_t)f, rec)) atomicOr(status, CP_BAD_INDEX);
}

// the scene's mesh size, clamped to what the workspace holds (a refused scene has no faces)
__device__ inline int cp_scene_faces(const CpScene *scenes, int F, int max_F) {
    if (!scenes) return F;
    const CpScene sc = scenes[blockIdx.z];
    return (sc.V <= 0 || sc.F <= 0 || sc.F > max_F || !sc.verts || !sc.faces) ? 0 : sc.F;
}

// grid (query tiles, slabs, scenes): partial minimum of 256 queries over one slab of faces
__global__ void __launch_bounds__(CP_THREADS)
closest_point_slab_kernel(int F, const CpScene *scenes, int max_F, const float *pts, int64_t N, char *ws, size_t block_bytes, size_t rec_off,
                          size_t pd2_off, size_t pface_off, int slab_faces, int slabs) {
    __shared__ __attribute__((aligned(16))) double lds[CP_THREADS * CP_REC];
    F = cp_scene_faces(scenes, F, max_F);
    const int slab = blockIdx.y;
    const int f_begin = slab * slab_faces;
    if (f_begin >= F) return;                     // (uniform over the workgroup; the finish pass does not read this slab)
    const int f_end = min(F, f_begin + slab_faces);
    char *block = ws + (size_t)blockIdx.z * block_bytes;
    const double *rec = reinterpret_cast<const double *>(block + rec_off);
    const int64_t n = (int64_t)blockIdx.x * CP_THREADS + threadIdx.x;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (n < N) {
        const float *p = pts + ((size_t)blockIdx.z * N + n) * 3;
        px = p[0]; py = p[1]; pz = p[2];
    }
    double best = __builtin_inf();
    int best_f = -1;
    for (int f0 = f_begin; f0 < f_end; f0 += CP_THREADS) {
        const int cnt = min(CP_THREADS, f_end - f0);
        __syncthreads();
        const double2 *src = reinterpret_cast<const double2 *>(rec + (size_t)f0 * CP_REC);
        double2 *dst = reinterpret_cast<double2 *>(lds);
        for (int i = threadIdx.x; i < cnt * (CP_REC / 2); i += CP_THREADS) dst[i] = src[i];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double *r = lds + j * CP_REC;
            if (r[CP_KIND] == CP_SKIP) continue;
            double q[3];
            const double d = cp_face(r, px, py, pz, q);
            if (d < best) { best = d; best_f = f0 + j; }
        }
    }
    if (n < N) {
        const size_t at = (size_t)n * slabs + slab;
        reinterpret_cast<double *>(block + pd2_off)[at] = best;
        reinterpret_cast<int32_t *>(block + pface_off)[at] = best_f;
    }
}

// grid (query tiles, 1, scenes): a query's partials in ascending slab order, then the point on the winning face
__global__ void __launch_bounds__(CP_THREADS)
closest_point_finish_kernel(int F, const CpScene *scenes, int max_F, const float *pts, int64_t N, const char *ws, size_t block_bytes, size_t rec_off,
                            size_t pd2_off, size_t pface_off, int slab_faces, int slabs, double *d2, int32_t *face, double *closest) {
    F = cp_scene_faces(scenes, F, max_F);
    const int64_t n = (int64_t)blockIdx.x * CP_THREADS + threadIdx.x;
    if (n >= N) return;
    const char *block = ws + (size_t)blockIdx.z * block_bytes;
    const double *pd2 = reinterpret_cast<const double *>(block + pd2_off) + (size_t)n * slabs;
    const int32_t *pface = reinterpret_cast<const int32_t *>(block + pface_off) + (size_t)n * slabs;
    double best = __builtin_inf();
    int best_f = -1;
    for (int s = 0; s < slabs && (int64_t)s * slab_faces < F; ++s) {
        const double d = pd2[s];
        if (d < best) { best = d; best_f = pface[s]; }
    }
    const size_t at = (size_t)blockIdx.z * N + n;
    d2[at] = best;
    face[at] = best_f;
    if (closest) {
        double q[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
        if (best_f >= 0 && best_f < F) {
            const float *p = pts + at * 3;
            cp_face(reinterpret_cast<const double *>(block + rec_off) + (size_t)best_f * CP_REC, p[0], p[1], p[2], q);
        }
        closest[3 * at] = q[0]; closest[3 * at + 1] = q[1]; closest[3 * at + 2] = q[2];
    }
}

int cp_run(const char *who, const float *verts, int V, const int32_t *faces, int F, const CpScene *scenes, int B, const float *pts, int64_t N,
           double *d2, int32_t *face, double *closest, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    const CpPlan pl = cp_plan(F, N, B);
    const int64_t qtiles = (N + CP_THREADS - 1) / CP_THREADS;
    if (qtiles > 0x7fffffff || pl.slabs > 65535 || B > 65535) return vt_fail(VT_ERR_UNSUPPORTED, who);
    if (!workspace || workspace_bytes < (size_t)B * pl.block_bytes) return vt_fail(VT_ERR_WORKSPACE, who);
    char *ws = static_cast<char *>(workspace);
    if (int rc = vt_fill32(ws, 0u, 4, stream)) return rc;
    hipLaunchKernelGGL(closest_point_prepare_kernel, dim3((unsigned)((F + CP_THREADS - 1) / CP_THREADS), (unsigned)B), dim3(CP_THREADS), 0, stream,
                       verts, V, faces, F, scenes, F, ws, pl.block_bytes, pl.rec_off);
    hipLaunchKernelGGL(closest_point_slab_kernel, dim3((unsigned)qtiles, (unsigned)pl.slabs, (unsigned)B), dim3(CP_THREADS), 0, stream,
                       F, scenes, F, pts, N, ws, pl.block_bytes, pl.rec_off, pl.pd2_off, pl.pface_off, pl.slab_faces, pl.slabs);
    hipLaunchKernelGGL(closest_point_finish_kernel, dim3((unsigned)qtiles, 1u, (unsigned)B), dim3(CP_THREADS), 0, stream,
                       F, scenes, F, pts, N, (const char *)ws, pl.block_bytes, pl.rec_off, pl.pd2_off, pl.pface_off, pl.slab_faces, pl.slabs,
                       d2, face, closest);
    return vt_check(hipGetLastError(), who);
}

}  // namespace

extern "C" {

size_t vt_closest_point_mesh_workspace_bytes(int F, int64_t N) {
    if (F <= 0 || N < 0) return 0;
    return cp_plan(F, N, 1).block_bytes;
}

int vt_closest_point_mesh_slab_faces(int F, int64_t N, int B) {
    if (F <= 0 || N < 0 || B <= 0) return 0;
    return cp_plan(F, N, B).slab_faces;
}

int vt_closest_point_mesh(const float *verts, int V, const int32_t *faces, int F, const float *pts, int64_t N, double *d2, int32_t *face,
                          double *closest, void *workspace, size_t workspace_bytes, void *stream) {
    if (!verts || !faces || V <= 0 || F <= 0 || N < 0 || (N > 0 && (!pts || !d2 || !face)))
        return vt_fail(VT_ERR_INVALID, "vt_closest_point_mesh: bad argument (a mesh needs V > 0 and F > 0)");
    if (N == 0) return 0;
    return cp_run("vt_closest_point_mesh", verts, V, faces, F, nullptr, 1, pts, N, d2, face, closest, workspace, workspace_bytes, (hipStream_t)stream);
}

int vt_closest_point_mesh_scenes(const void *scenes, int B, int max_F, const float *pts, int64_t N, double *d2, int32_t *face, double *closest,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    if (!scenes || B < 0 || max_F <= 0 || N < 0 || (B > 0 && N > 0 && (!pts || !d2 || !face)))
        return vt_fail(VT_ERR_INVALID, "vt_closest_point_mesh_scenes: bad argument (max_F > 0)");
    if (B == 0 || N == 0) return 0;
    return cp_run("vt_closest_point_mesh_scenes", nullptr, 0, nullptr, max_F, reinterpret_cast<const CpScene *>(scenes), B, pts, N, d2, face, closest,
                  workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
