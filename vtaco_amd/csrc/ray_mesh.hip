// What a ray hits first on a triangle mesh -- trimesh's mesh.ray.intersects_first / intersects_location -- and the sensor camera built on
// it: the inverse of vt_contact_points' unprojection, so that a mesh can be rendered into the depth images the tactile side consumes.
// The definitions are DESIGN.md's section "ray_mesh.hip", restated in numpy by tests/ray_mesh_ref.py: this file's operations in this
// file's order.  The ray / face rule is ray_face.h's; both kernels below call it.
//   vt_ray_mesh         brute force, the definition: every ray against every face.  Work is tiled both ways as in closest_point.hip: a
//                       workgroup takes 256 rays (one per thread) and one slab of faces, staged through LDS in chunks of 256 records
//                       (the corners as doubles and a kind: 2 = an index outside [0, V), reported through the status word and never
//                       dereferenced) that every lane of a wave reads at one address; it writes one partial minimum per (ray, slab).  The
//                       finish pass takes a ray's partials in ascending slab order.  Faces are met in ascending order with a strict <:
//                       equal s give the lowest face index.  No atomic on a result: bit-reproducible, independent of the slab size
//   vt_ray_tree_query   the same s and face from a walk of winding_fast.hip's octree with closest_point_tree.hip's side buffer (one tight
//                       box per occupied cell, the kind of every face in list order); the corners come from the tree's F x 9 f32 in list
//                       order.  One lane per ray, octree_common.h's walk.  An occupied cell and everything under it is skipped when
//                       the segment [t_min, min(t_max, best)] misses the cell's box grown by E:
//                         x0_a = (lo_a - o_a) - E, x1_a = (hi_a - o_a) + E;  d_a == 0: skipped when x0_a > 0 or x1_a < 0;  otherwise
//                         (near_a, far_a) = (x0_a, x1_a) (1 / d_a), exchanged when d_a < 0;  enter = t_min, exit = min(t_max, best),
//                         enter = near_a where near_a > enter, exit = far_a where far_a < exit;  skipped when enter > exit
//                       Every comparison is false for a NaN: a NaN constrains nothing and skips nothing.  A leaf that is not skipped runs
//                       rf_face over its list in list order and takes a face on
//                       s < best || (s == best && face < best_face): the walk does not meet faces in ascending order
//   E                   2^-40 S, S = ot_frame_reach = (m_x + m_y) + m_z, m_a = max(|o_a - lo_a|, |o_a - (lo_a + side)|): S bounds
//                       |corner_a - o_a| of every face, and the point o + s d of a computed hit lies within (19 + 12 k) u S of the face's
//                       box, u = 2^-53, k the face's aspect seen along the ray (DESIGN.md derives it); 2^-40 = 8192 u covers k <= 681
//   order               the children of a cell are visited as k ^ o, o_a = (d_a < 0): near children first, one o for the whole ray
//   invalid rays        (ray_face.h) write (+inf, -1, NaN weights, no statistics) before any walk
// VTACO_RAY_TREE_WALK = plain | order picks the walk for A/B runs; the default is order.  The order changes which cells are skipped,
// never a result.  Lanes take rays in index order: a wave is 64 consecutive pixels of an image row.  Handing a wave an 8 x 8 pixel tile
// instead was measured and not kept (profiles/ray_mesh_tile_ab.json: five 320 x 240 images, 0.17 against 0.21 ms at 576 faces, but 2.74
// against 2.13 ms at 65 536 and 1.27 against 1.19 ms on the 976 125-face scene mesh).
//   vt_camera_rays      pose records [n_images][16] f64 {M 3x3, t, centroid, scale} as vt_contact_points reads them: per image the origin
//                       (t - centroid) / scale, per pixel (u, v) the direction M (1, -(u - W/2) / f, -(v - H/2) / f) / scale,
//                       f = H / (2 tan(fov / 2)).  The camera-axis component is 1: the s of a hit IS the planar depth
//   vt_depth_from_hits  depth = min(s, origin) clamped below at near, as f32; a miss gives origin (+inf without one)
// No launch function allocates, copies to the host or waits.  All products and sums are separate roundings (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "closest_point_face.h"
#include "mesh_common.h"
#include "octree_common.h"
#include "ray_face.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

constexpr int RM_REC = 10;                      // doubles per face record (80 bytes: 16-byte aligned rows): a, b, c, kind
constexpr int RM_MIN_CHUNKS = 2;                // chunks per slab at least: every mesh beyond 256 faces walks the re-staging loop
constexpr int RM_TARGET_BLOCKS = 2048;          // workgroups wanted per launch: 8 per CU
constexpr size_t RM_HEAD = 256;                 // bytes in front of the workspace; the call's status word is the first
constexpr int RM_BAD_INDEX = 1;                 // status bit (closest_point_face.h's CP_BAD_INDEX)
constexpr double RT_SLACK = 0x1p-40;

struct RmPlan { int slab_faces, slabs; size_t rec_off, ps_off, pface_off, bytes; };

// how F faces and N rays are cut: slabs of whole chunks, as many as fill the device, at least RM_MIN_CHUNKS chunks each
RmPlan rm_plan(int64_t F, int64_t N) {
    const int64_t tiles = (N + MT_THREADS - 1) / MT_THREADS;
    const int64_t chunks = (F + MT_THREADS - 1) / MT_THREADS;
    int64_t want = RM_TARGET_BLOCKS / (tiles > 0 ? tiles : 1);
    if (want < 1) want = 1;
    int64_t per = (chunks + want - 1) / want;
    if (per < RM_MIN_CHUNKS) per = RM_MIN_CHUNKS;
    RmPlan p;
    p.slab_faces = (int)(per * MT_THREADS);
    p.slabs = (int)((chunks + per - 1) / per);
    if (p.slabs < 1) p.slabs = 1;
    p.rec_off = RM_HEAD;
    p.ps_off = p.rec_off + up256((size_t)F * RM_REC * sizeof(double));
    p.pface_off = p.ps_off + up256((size_t)N * p.slabs * sizeof(double));
    p.bytes = p.pface_off + up256((size_t)N * p.slabs * sizeof(int32_t));
    return p;
}

__global__ void __launch_bounds__(MT_THREADS)
rm_prepare_kernel(const float *verts, int V, const int32_t *faces, int F, double *rec, int32_t *status) {
    const int f = blockIdx.x * MT_THREADS + threadIdx.x;
    if (f >= F) return;
    double *r = rec + (size_t)f * RM_REC;
    int idx[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        idx[k] = faces[3 * (size_t)f + k];
        ok = ok && idx[k] >= 0 && idx[k] < V;
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < RM_REC; ++k) r[k] = k == 9 ? 2.0 : 0.0;
        atomicOr(status, RM_BAD_INDEX);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) r[3 * k + a] = (double)verts[3 * (size_t)idx[k] + a];
    r[9] = 0.0;
}

__device__ inline bool rm_load_ray(const double *origins, int64_t per_origin, const double *dirs, int64_t n, RfRay &ray) {
    const double *op = origins + 3 * (n / per_origin), *dp = dirs + 3 * n;
    const double o[3] = {op[0], op[1], op[2]}, d[3] = {dp[0], dp[1], dp[2]};
    rf_setup(o, d, ray);
    return ray.ok;
}

// grid (ray tiles, slabs): partial minimum of 256 rays over one slab of faces
__global__ void __launch_bounds__(MT_THREADS)
rm_slab_kernel(int F, const double *origins, int64_t per_origin, const double *dirs, int64_t N, double t_min, double t_max, const double *rec,
               double *ps, int32_t *pface, int slab_faces, int slabs) {
    __shared__ __attribute__((aligned(16))) double lds[MT_THREADS * RM_REC];
    const int slab = blockIdx.y;
    const int f_begin = slab * slab_faces;
    if (f_begin >= F) return;                     // (uniform over the workgroup; the finish pass does not read this slab)
    const int f_end = min(F, f_begin + slab_faces);
    const int64_t n = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    RfRay ray;
    ray.ok = false;
    if (n < N) rm_load_ray(origins, per_origin, dirs, n, ray);
    double best = __builtin_inf();
    int best_f = -1;
    for (int f0 = f_begin; f0 < f_end; f0 += MT_THREADS) {
        const int cnt = min(MT_THREADS, f_end - f0);
        __syncthreads();
        const double2 *src = reinterpret_cast<const double2 *>(rec + (size_t)f0 * RM_REC);
        double2 *dst = reinterpret_cast<double2 *>(lds);
        for (int i = threadIdx.x; i < cnt * (RM_REC / 2); i += MT_THREADS) dst[i] = src[i];
        __syncthreads();
        if (!ray.ok) continue;
        for (int j = 0; j < cnt; ++j) {
            const double *r = lds + j * RM_REC;
            if (r[9] == 2.0) continue;
            double s;
            if (rf_face(ray, r, r + 3, r + 6, t_min, t_max, s) && s < best) { best = s; best_f = f0 + j; }
        }
    }
    if (n < N) {
        const size_t at = (size_t)n * slabs + slab;
        ps[at] = best;
        pface[at] = best_f;
    }
}

// a ray's partials in ascending slab order, then the weights on the winning face
__global__ void __launch_bounds__(MT_THREADS)
rm_finish_kernel(int F, const double *origins, int64_t per_origin, const double *dirs, int64_t N, double t_min, double t_max, const double *rec,
                 const double *ps, const int32_t *pface, int slab_faces, int slabs, double *s_out, int32_t *face, double *bary) {
    const int64_t n = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (n >= N) return;
    double best = __builtin_inf();
    int best_f = -1;
    for (int sl = 0; sl < slabs && (int64_t)sl * slab_faces < F; ++sl) {
        const double v = ps[(size_t)n * slabs + sl];
        if (v < best) { best = v; best_f = pface[(size_t)n * slabs + sl]; }
    }
    s_out[n] = best;
    face[n] = best_f;
    if (bary) {
        double w[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
        RfRay ray;
        if (best_f >= 0 && best_f < F && rm_load_ray(origins, per_origin, dirs, n, ray)) {
            const double *r = rec + (size_t)best_f * RM_REC;
            double s, uvw[4];
            if (rf_face(ray, r, r + 3, r + 6, t_min, t_max, s, uvw)) { w[0] = uvw[0] / uvw[3]; w[1] = uvw[1] / uvw[3]; w[2] = uvw[2] / uvw[3]; }
        }
        bary[3 * n] = w[0]; bary[3 * n + 1] = w[1]; bary[3 * n + 2] = w[2];
    }
}

// ---- the tree walk -------------------------------------------------------------------------------------------------------------------------
struct RtBest { double s; int face, slot; };

__device__ inline void rt_corners(const float *tri, int t, double p[9]) {
    const float *c = tri + (size_t)t * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) p[k] = (double)c[k];
}

// rf_face over the list of leaf rk, in list order; the tie rule is explicit
__device__ inline int rt_leaf(const OtView<float> &tv, const double *recs, int rk, const RfRay &ray, double t_min, double t_max, RtBest &best) {
    const int o = tv.loff[rk], e = tv.loff[rk + 1];
    for (int t = o; t < e; ++t) {
        if (recs[(size_t)t * CP_REC + CP_KIND] == CP_SKIP) continue;
        double p[9], s;
        rt_corners(tv.payload, t, p);
        if (!rf_face(ray, p, p + 3, p + 6, t_min, t_max, s)) continue;
        const int f = tv.list[t];
        if (s < best.s || (s == best.s && f < best.face)) { best.s = s; best.face = f; best.slot = t; }
    }
    return e - o;
}

template <bool ORDER>
__global__ void __launch_bounds__(MT_THREADS)
rt_query_kernel(const char *tree, OtAt tree_at, const char *side, OtSide sd, int L, const double *origins, int64_t per_origin, const double *dirs,
                int64_t N, double t_min, double t_max, double *s_out, int32_t *face, double *bary, int32_t *stats) {
    const int64_t n = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (n >= N) return;
    const OtView<float> tv = ot_view<float>(tree, tree_at, 0);
    const OtSideView sv = ot_side_view(side, sd);
    const double *op = origins + 3 * (n / per_origin), *dp = dirs + 3 * n;
    const double o[3] = {op[0], op[1], op[2]}, d[3] = {dp[0], dp[1], dp[2]};
    RfRay ray;
    rf_setup(o, d, ray);
    RtBest best = {__builtin_inf(), -1, -1};
    int n_boxes = 0, n_faces = 0;
    if (ray.ok) {
        double inv[3];
        unsigned oct = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            inv[a] = 1.0 / d[a];
            if (ORDER) oct |= d[a] < 0.0 ? 1u << a : 0u;
        }
        const double E = ot_frame_reach(tv.frame, o) * RT_SLACK;
        ot_walk(
            tv.pyr,
            [&](int level, int rk) {
                const double *b = sv.boxes + ((size_t)sd.base.v[level] + rk) * OT_BOX;
                double enter = t_min, exit = best.s < t_max ? best.s : t_max;
                bool skip = false;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double x0 = (b[a] - o[a]) - E, x1 = (b[3 + a] - o[a]) + E;
                    if (d[a] == 0.0) {
                        skip = skip || x0 > 0.0 || x1 < 0.0;
                    } else {
                        const double u = x0 * inv[a], v = x1 * inv[a];
                        const double near = d[a] < 0.0 ? v : u, far = d[a] < 0.0 ? u : v;
                        enter = near > enter ? near : enter;
                        exit = far < exit ? far : exit;
                    }
                }
                skip = skip || enter > exit;
                ++n_boxes;
                if (skip) return false;
                if (level < L) return true;
                n_faces += rt_leaf(tv, sv.recs, rk, ray, t_min, t_max, best);
                return false;
            },
            [&](int, unsigned) { return oct; });
    }
    s_out[n] = best.s;
    face[n] = best.face;
    if (bary) {
        double w[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
        if (best.slot >= 0) {
            double p[9], s, uvw[4];
            rt_corners(tv.payload, best.slot, p);
            if (rf_face(ray, p, p + 3, p + 6, t_min, t_max, s, uvw)) { w[0] = uvw[0] / uvw[3]; w[1] = uvw[1] / uvw[3]; w[2] = uvw[2] / uvw[3]; }
        }
        bary[3 * n] = w[0]; bary[3 * n + 1] = w[1]; bary[3 * n + 2] = w[2];
    }
    if (stats) { stats[2 * n] = n_boxes; stats[2 * n + 1] = n_faces; }
}

// ---- the camera ------------------------------------------------------------------------------------------------------------------------------
struct RmPose { double m[9], t[3], centroid[3], scale; };         // contact.hip's ContactPose
static_assert(sizeof(RmPose) == 128, "pose records are 16 doubles");

// grid (pixel tiles, images)
__global__ void __launch_bounds__(MT_THREADS)
rm_camera_kernel(const RmPose *pose, int width, int height, double f, double *origins, double *dirs) {
    const int img = blockIdx.y, npix = width * height;
    const RmPose ps = pose[img];
    const int pix = blockIdx.x * MT_THREADS + threadIdx.x;
    if (pix == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) origins[3 * (size_t)img + i] = (ps.t[i] - ps.centroid[i]) / ps.scale;
    }
    if (pix >= npix) return;
    const int u = pix % width, v = pix / width;
    const double c1 = (-((double)u - width / 2.0)) / f, c2 = (-((double)v - height / 2.0)) / f;
    double *out = dirs + ((size_t)img * npix + pix) * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = ((ps.m[3 * i] + ps.m[3 * i + 1] * c1) + ps.m[3 * i + 2] * c2) / ps.scale;
}

__global__ void __launch_bounds__(MT_THREADS)
rm_depth_kernel(const double *s, const double *origin, int64_t npix, int64_t N, double near, float *depth) {
    const int64_t n = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (n >= N) return;
    double z = s[n];
    if (origin) { const double g = origin[n % npix]; z = z < g ? z : g; }
    z = z < near ? near : z;
    depth[n] = (float)z;
}

int rm_ray_args(const char *who, const double *origins, int64_t per_origin, const double *dirs, int64_t N, const double *s, const int32_t *face) {
    if (N < 0 || per_origin < 1 || (N > 0 && (!origins || !dirs || !s || !face))) return vt_fail(VT_ERR_INVALID, who);
    if (N > (int64_t)0x7fffffff * MT_THREADS) return vt_fail(VT_ERR_UNSUPPORTED, who);
    return 0;
}

}  // namespace

extern "C" {

size_t vt_ray_mesh_workspace_bytes(int F, int64_t N) {
    if (F <= 0 || N < 0) return 0;
    return rm_plan(F, N).bytes;
}

int vt_ray_mesh(const float *verts, int V, const int32_t *faces, int F, const double *origins, int64_t rays_per_origin, const double *dirs, int64_t N,
                double t_min, double t_max, double *s, int32_t *face, double *bary, void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "vt_ray_mesh: bad argument (a mesh needs V > 0 and F > 0, rays_per_origin >= 1)";
    if (!verts || !faces || V <= 0 || F <= 0) return vt_fail(VT_ERR_INVALID, who);
    if (int rc = rm_ray_args(who, origins, rays_per_origin, dirs, N, s, face)) return rc;
    if (N == 0) return 0;
    const RmPlan pl = rm_plan(F, N);
    const int64_t tiles = (N + MT_THREADS - 1) / MT_THREADS;
    if (pl.slabs > 65535) return vt_fail(VT_ERR_UNSUPPORTED, "vt_ray_mesh: too many faces for this many rays");
    if (!workspace || workspace_bytes < pl.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_ray_mesh: workspace too small (vt_ray_mesh_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    double *rec = reinterpret_cast<double *>(ws + pl.rec_off), *ps = reinterpret_cast<double *>(ws + pl.ps_off);
    int32_t *pface = reinterpret_cast<int32_t *>(ws + pl.pface_off);
    if (int rc = vt_fill32(ws, 0u, 4, st)) return rc;
    hipLaunchKernelGGL(rm_prepare_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, st, verts, V, faces, F, rec, reinterpret_cast<int32_t *>(ws));
    hipLaunchKernelGGL(rm_slab_kernel, dim3((unsigned)tiles, (unsigned)pl.slabs), dim3(MT_THREADS), 0, st, F, origins, rays_per_origin, dirs, N, t_min,
                       t_max, (const double *)rec, ps, pface, pl.slab_faces, pl.slabs);
    hipLaunchKernelGGL(rm_finish_kernel, dim3((unsigned)tiles), dim3(MT_THREADS), 0, st, F, origins, rays_per_origin, dirs, N, t_min, t_max,
                       (const double *)rec, (const double *)ps, (const int32_t *)pface, pl.slab_faces, pl.slabs, s, face, bary);
    return vt_check(hipGetLastError(), "vt_ray_mesh");
}

int vt_ray_tree_query(const void *tree, size_t tree_bytes, const void *side, size_t side_bytes, int64_t F, int depth, const int32_t *state_host,
                      const double *origins, int64_t rays_per_origin, const double *dirs, int64_t N, double t_min, double t_max, double *s,
                      int32_t *face, double *bary, int32_t *stats, void *stream) {
    const char *who = "vt_ray_tree_query: bad argument (a mesh needs F > 0, rays_per_origin >= 1)";
    if (!tree || !side || F <= 0 || !state_host) return vt_fail(VT_ERR_INVALID, who);
    if (int rc = rm_ray_args(who, origins, rays_per_origin, dirs, N, s, face)) return rc;
    size_t off[6];
    if (int rc = vt_winding_tree_layout(F, depth, state_host, off)) return rc;
    OtSide sd;
    ot_side(F, depth, state_host, CP_REC, sd);
    if (tree_bytes < off[5] || side_bytes < sd.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_ray_tree_query: tree or side buffer too small");
    if (N == 0) return 0;
    const char *walk = getenv("VTACO_RAY_TREE_WALK");
    auto kernel = rt_query_kernel<true>;
    if (walk && walk[0]) {
        if (!strcmp(walk, "plain")) kernel = rt_query_kernel<false>;
        else if (strcmp(walk, "order")) return vt_fail(VT_ERR_INVALID, "vt_ray_tree_query: VTACO_RAY_TREE_WALK must be plain or order");
    }
    hipLaunchKernelGGL(kernel, dim3(blocks_of(N, MT_THREADS)), dim3(MT_THREADS), 0, (hipStream_t)stream, static_cast<const char *>(tree),
                       OtAt{0, off[0], off[1], off[2], off[3], off[4]}, static_cast<const char *>(side), sd, depth, origins, rays_per_origin, dirs, N,
                       t_min, t_max, s, face, bary, stats);
    return vt_check(hipGetLastError(), "vt_ray_tree_query");
}

int vt_camera_rays(const double *pose, int n_images, int width, int height, double fov_deg, double *origins, double *dirs, void *stream) {
    if (n_images < 0 || width <= 0 || height <= 0 || !(fov_deg > 0.0 && fov_deg < 180.0) || (n_images > 0 && (!pose || !origins || !dirs)))
        return vt_fail(VT_ERR_INVALID, "vt_camera_rays: bad argument (width, height > 0, 0 < fov < 180)");
    if (n_images > 65535 || (int64_t)width * height > 0x7fffff00) return vt_fail(VT_ERR_UNSUPPORTED, "vt_camera_rays: too many images or pixels");
    if (n_images == 0) return 0;
    const double f = height / (2.0 * tan(fov_deg * 3.14159265358979323846 / 180.0 / 2.0));
    hipLaunchKernelGGL(rm_camera_kernel, dim3(blocks_of((int64_t)width * height, MT_THREADS), (unsigned)n_images), dim3(MT_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const RmPose *>(pose), width, height, f, origins, dirs);
    return vt_check(hipGetLastError(), "vt_camera_rays");
}

int vt_depth_from_hits(const double *s, const double *depth_origin, int64_t n_pixels, int64_t N, double near, float *depth, void *stream) {
    if (N < 0 || n_pixels <= 0 || (N > 0 && (!s || !depth))) return vt_fail(VT_ERR_INVALID, "vt_depth_from_hits: bad argument (n_pixels > 0)");
    if (N > (int64_t)0x7fffffff * MT_THREADS) return vt_fail(VT_ERR_UNSUPPORTED, "vt_depth_from_hits: too many rays");
    if (N == 0) return 0;
    hipLaunchKernelGGL(rm_depth_kernel, dim3(blocks_of(N, MT_THREADS)), dim3(MT_THREADS), 0, (hipStream_t)stream, s, depth_origin, n_pixels, N, near, depth);
    return vt_check(hipGetLastError(), "vt_depth_from_hits");
}

}  // extern "C"
