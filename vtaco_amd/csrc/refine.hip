// Mesh refinement on the decoder's field jet: one RMSprop iteration of the Convolutional Occupancy Networks generator's refine_mesh
// (DESIGN.md, section "field_jet / refine"; tests/refine_ref.py states it in float64 autograd).  Per iteration, with one point per face:
//   vt_refine_sample      p_f = (eps_0 v_0 + eps_1 v_1) + eps_2 v_2 in float32, eps given or drawn here: Dirichlet(1/2,1/2,1/2) as
//                         z_i^2 / sum z_j^2, z standard normal by Box-Muller from a counter hash of (seed, step, face, i).  No state:
//                         any launch order gives equal bits.
//   (vt_decode_jet)       the field's jet at p_f (field_jet.hip)
//   vt_refine_face_grad   with s = sigmoid(f), s' = s (1 - s), s'' = s' (1 - 2 s), g = s' grad f, m = |g|, n_t = -g / (m + 1e-10),
//                         n = c / (|c| + 1e-10), c = (v1 - v0) x (v2 - v1), d = n - n_t:
//                             L = mean_F (s - t)^2 + w mean_F |d|^2
//                             u = dL/dg = (2 w / F) (d / (m + 1e-10) - (d . g) g / (m (m + 1e-10)^2))       (second term 0 at m = 0)
//                             dL/dp = (2 / F) (s - t) g + s'' (grad f . u) grad f + s' H_f u                 (H_f: zero diagonal)
//                             q = dL/dc = r / (|c| + 1e-10) - (r . c) c / (|c| (|c| + 1e-10)^2),  r = (2 w / F) d
//                             dL/dv0 = eps_0 dL/dp - b x q,  dL/dv1 = eps_1 dL/dp + b x q - q x a,  dL/dv2 = eps_2 dL/dp + q x a
//                         (a = v1 - v0, b = v2 - v1), all in float64 from the float32 inputs.  Summed per vertex EXACTLY, as
//                         mesh_normals.hip sums its terms: pass 0 takes each vertex's largest |term component|, pass 1 adds two
//                         int64 fixed-point limbs scaled by that maximum's exponent.  No float atomic: equal bits under any face
//                         order.  A zero-area face is finite: the 1e-10 in the denominators does that.
//   vt_refine_step        g = float32 of the sums (which it zeroes for the next iteration), then torch.optim.RMSprop's defaults:
//                         sq = 0.99 sq + 0.01 g^2,  v -= lr g / (sqrt(sq) + 1e-8), evaluated in float64 from the float32 g, sq
//                         and v and rounded once each.
// A face with an index outside [0, V) is never dereferenced: it contributes nothing and its point is the origin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_common.h"
#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

// ---- counter-based randomness: splitmix64's finaliser over the packed counter -----------------------------------------------------
__device__ inline u64 mix64(u64 x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// standard normal of (seed, step, face, i): two 32-bit uniforms, u1 in (0, 1], u2 in [0, 1)
__device__ inline double normal_of(u64 seed, u64 step, u64 face, int i) {
    const u64 k = mix64(mix64(mix64(seed) ^ step) ^ (face * 4 + (u64)i));
    const double u1 = ((double)(uint32_t)(k >> 32) + 1.0) * 0x1p-32;
    const double u2 = (double)(uint32_t)k * 0x1p-32;
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

__global__ void __launch_bounds__(MT_THREADS)
refine_sample_kernel(const float *verts, int V, const int32_t *faces, int F, const float *eps_in, u64 seed, u64 step, float *eps, float *pts) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    float e0, e1, e2;
    if (eps_in) {
        e0 = eps_in[(size_t)f * 3]; e1 = eps_in[(size_t)f * 3 + 1]; e2 = eps_in[(size_t)f * 3 + 2];
    } else {
        const double z0 = normal_of(seed, step, (u64)f, 0), z1 = normal_of(seed, step, (u64)f, 1), z2 = normal_of(seed, step, (u64)f, 2);
        const double s0 = z0 * z0, s1 = z1 * z1, s2 = z2 * z2, sum = (s0 + s1) + s2;
        const bool any = sum > 0.0;
        e0 = any ? (float)(s0 / sum) : 1.0f / 3.0f;
        e1 = any ? (float)(s1 / sum) : 1.0f / 3.0f;
        e2 = any ? (float)(s2 / sum) : 1.0f / 3.0f;
    }
    if (eps != eps_in) { eps[(size_t)f * 3] = e0; eps[(size_t)f * 3 + 1] = e1; eps[(size_t)f * 3 + 2] = e2; }
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (ok) {
        const float *p0 = verts + (size_t)a * 3, *p1 = verts + (size_t)b * 3, *p2 = verts + (size_t)c * 3;
        px = (e0 * p0[0] + e1 * p1[0]) + e2 * p2[0];
        py = (e0 * p0[1] + e1 * p1[1]) + e2 * p2[1];
        pz = (e0 * p0[2] + e1 * p1[2]) + e2 * p2[2];
    }
    pts[(size_t)f * 3] = px; pts[(size_t)f * 3 + 1] = py; pts[(size_t)f * 3 + 2] = pz;
}

struct FaceGradArgs {
    const float *verts;
    const int32_t *faces;
    const float *eps;        // [F][3]
    const float *jet;        // [F][8]
    float *terms;            // [F][2] (target, normal) or null
    u64 *vmax;               // [V]
    u64 *sums;               // [V][6]: limbs hi, lo of x, y, z
    int V, F;
    double threshold, weight;
};

// PASS 0: the loss terms and every vertex's largest |gradient term component|; PASS 1: the fixed-point sums against them.
template <int PASS>
__global__ void __launch_bounds__(MT_THREADS) refine_face_grad_kernel(FaceGradArgs A) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, ia, ib, ic;
    bool ok;
    if (!load_face(A.faces, A.F, A.V, lds, f, ia, ib, ic, ok)) return;
    if (!ok) {
        if (PASS == 0 && A.terms) { A.terms[(size_t)f * 2] = 0.0f; A.terms[(size_t)f * 2 + 1] = 0.0f; }
        return;
    }
    const double EPS = 1e-10;
    double v0[3], v1[3], v2[3];
    load_vertex(A.verts, ia, v0[0], v0[1], v0[2]);
    load_vertex(A.verts, ib, v1[0], v1[1], v1[2]);
    load_vertex(A.verts, ic, v2[0], v2[1], v2[2]);
    const float *jr = A.jet + (size_t)f * 8;
    const double fv = jr[0], gx = jr[1], gy = jr[2], gz = jr[3], hxy = jr[4], hxz = jr[5], hyz = jr[6];
    const double e0 = A.eps[(size_t)f * 3], e1 = A.eps[(size_t)f * 3 + 1], e2 = A.eps[(size_t)f * 3 + 2];
    const double invF = 1.0 / (double)A.F;

    const double s = 1.0 / (1.0 + exp(-fv)), s1 = s * (1.0 - s), s2 = s1 * (1.0 - 2.0 * s);
    const double g[3] = {s1 * gx, s1 * gy, s1 * gz};
    const double m = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    const double a[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, b[3] = {v2[0] - v1[0], v2[1] - v1[1], v2[2] - v1[2]};
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double l = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = c[k] / (l + EPS) + g[k] / (m + EPS);        // n - n_t
    if (PASS == 0 && A.terms) {
        A.terms[(size_t)f * 2] = (float)((s - A.threshold) * (s - A.threshold));
        A.terms[(size_t)f * 2 + 1] = (float)((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    }
    const double w2 = 2.0 * A.weight * invF;
    // u = dL/dg
    const double dg = (d[0] * g[0] + d[1] * g[1]) + d[2] * g[2];
    const double ku = m > 0.0 ? dg / (m * (m + EPS) * (m + EPS)) : 0.0;
    double u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = w2 * (d[k] / (m + EPS) - ku * g[k]);
    // dL/dp
    const double gu = (gx * u[0] + gy * u[1]) + gz * u[2];
    const double hu[3] = {hxy * u[1] + hxz * u[2], hxy * u[0] + hyz * u[2], hxz * u[0] + hyz * u[1]};
    const double kt = 2.0 * invF * (s - A.threshold);
    const double gf[3] = {gx, gy, gz};
    double dp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) dp[k] = kt * g[k] + (s2 * gu * gf[k] + s1 * hu[k]);
    // q = dL/dc
    const double rc = (d[0] * c[0] + d[1] * c[1]) + d[2] * c[2];
    const double kq = l > 0.0 ? rc / (l * (l + EPS) * (l + EPS)) : 0.0;
    double q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = w2 * (d[k] / (l + EPS) - kq * c[k]);
    const double bq[3] = {b[1] * q[2] - b[2] * q[1], b[2] * q[0] - b[0] * q[2], b[0] * q[1] - b[1] * q[0]};       // dL/da
    const double qa[3] = {q[1] * a[2] - q[2] * a[1], q[2] * a[0] - q[0] * a[2], q[0] * a[1] - q[1] * a[0]};       // dL/db
    const int idx[3] = {ia, ib, ic};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ek = k == 0 ? e0 : (k == 1 ? e1 : e2);
        double t[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = ek * dp[j] + (k == 0 ? -bq[j] : (k == 1 ? bq[j] - qa[j] : qa[j]));
        const int v = idx[k];
        if (PASS == 0) {
            const double mx = fmax(fmax(fabs(t[0]), fabs(t[1])), fabs(t[2]));
            if (mx < __longlong_as_double(0x7ff0000000000000ll)) atomicMax(A.vmax + v, (u64)__double_as_longlong(mx));
        } else {
            const int e = exponent_of(A.vmax[v]);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (!(fabs(t[j]) < __longlong_as_double(0x7ff0000000000000ll))) continue;       // (a NaN jet: no term)
                u64 hi, lo;
                limbs_of(t[j], e, hi, lo);
                atomicAdd(A.sums + (size_t)v * 6 + 2 * j, hi);
                atomicAdd(A.sums + (size_t)v * 6 + 2 * j + 1, lo);
            }
        }
    }
}

__global__ void __launch_bounds__(MT_THREADS)
refine_step_kernel(float *verts, int V, u64 *vmax, u64 *sums, float *sq, double lr, double alpha, double eps, float *grad) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= (int64_t)V * 3) return;
    const int64_t v = i / 3;
    const int j = (int)(i - v * 3);
    const int e = exponent_of(vmax[v]);
    u64 *s = sums + (size_t)v * 6 + 2 * j;
    const float g = (float)sum_of(s[0], s[1], e);
    s[0] = 0; s[1] = 0;
    if (grad) grad[i] = g;
    // the update in float64 from the float32 state: one rounding each for sq and the vertex
    const double gd = (double)g, q = alpha * (double)sq[i] + (1.0 - alpha) * (gd * gd);
    sq[i] = (float)q;
    verts[i] = (float)((double)verts[i] - lr * (gd / (sqrt(q) + eps)));
}

// (the maxima are cleared behind the step that read them: three threads of a vertex read vmax[v] above, in one kernel)
__global__ void __launch_bounds__(MT_THREADS) refine_clear_kernel(u64 *vmax, int V) {
    const int64_t v = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (v < V) vmax[v] = 0;
}

bool mesh_ok(int64_t V, int64_t F) { return V >= 1 && F >= 1 && V <= MT_MAX_V && F <= MT_MAX_F; }

struct RefineWs {
    size_t pts, eps, jet, vmax, sums, jet_ws, bytes;
};
RefineWs refine_layout(int64_t V, int64_t F, int composed) {
    RefineWs w;
    size_t at = 0;
    w.pts = at; at += up256((size_t)F * 3 * sizeof(float));
    w.eps = at; at += up256((size_t)F * 3 * sizeof(float));
    w.jet = at; at += up256((size_t)F * 8 * sizeof(float));
    w.vmax = at; at += up256((size_t)V * 8);
    w.sums = at; at += up256((size_t)V * 6 * 8);
    w.jet_ws = at; at += composed ? up256(vt_decode_jet_composed_workspace_bytes(1, F)) : 0;
    w.bytes = at;
    return w;
}

}  // namespace

extern "C" {

int vt_refine_sample(const float *verts, int64_t V, const int32_t *faces, int64_t F, const float *eps_in, uint64_t seed, uint64_t step,
                     float *eps, float *pts, void *stream) {
    if (!mesh_ok(V, F) || !verts || !faces || !eps || !pts) return vt_fail(VT_ERR_INVALID, "vt_refine_sample: bad argument (V >= 1, F >= 1)");
    hipLaunchKernelGGL(refine_sample_kernel, dim3(blocks_of(F, MT_THREADS)), dim3(MT_THREADS), 0, (hipStream_t)stream, verts, (int)V, faces,
                       (int)F, eps_in, (u64)seed, (u64)step, eps, pts);
    return vt_check(hipGetLastError(), "vt_refine_sample");
}

size_t vt_refine_accum_bytes(int64_t V) { return V >= 1 && V <= MT_MAX_V ? up256((size_t)V * 8) + up256((size_t)V * 6 * 8) : 0; }

int vt_refine_face_grad(const float *verts, int64_t V, const int32_t *faces, int64_t F, const float *eps, const float *jet,
                        double threshold, double normal_weight, float *terms, void *accum, size_t accum_bytes, void *stream) {
    if (!mesh_ok(V, F) || !verts || !faces || !eps || !jet) return vt_fail(VT_ERR_INVALID, "vt_refine_face_grad: bad argument (V >= 1, F >= 1)");
    if (!accum || accum_bytes < vt_refine_accum_bytes(V)) return vt_fail(VT_ERR_WORKSPACE, "vt_refine_face_grad");
    FaceGradArgs A;
    A.verts = verts; A.faces = faces; A.eps = eps; A.jet = jet; A.terms = terms; A.V = (int)V; A.F = (int)F;
    A.vmax = static_cast<u64 *>(accum);
    A.sums = reinterpret_cast<u64 *>(static_cast<char *>(accum) + up256((size_t)V * 8));
    A.threshold = threshold; A.weight = normal_weight;
    const dim3 grid(blocks_of(F, MT_THREADS)), block(MT_THREADS);
    hipLaunchKernelGGL(refine_face_grad_kernel<0>, grid, block, 0, (hipStream_t)stream, A);
    hipLaunchKernelGGL(refine_face_grad_kernel<1>, grid, block, 0, (hipStream_t)stream, A);
    return vt_check(hipGetLastError(), "vt_refine_face_grad");
}

int vt_refine_step(float *verts, int64_t V, void *accum, size_t accum_bytes, float *sq, double lr, double alpha, double eps, float *grad,
                   void *stream) {
    if (V < 1 || V > MT_MAX_V || !verts || !sq) return vt_fail(VT_ERR_INVALID, "vt_refine_step: bad argument (V >= 1)");
    if (!accum || accum_bytes < vt_refine_accum_bytes(V)) return vt_fail(VT_ERR_WORKSPACE, "vt_refine_step");
    u64 *vmax = static_cast<u64 *>(accum);
    u64 *sums = reinterpret_cast<u64 *>(static_cast<char *>(accum) + up256((size_t)V * 8));
    hipLaunchKernelGGL(refine_step_kernel, dim3(blocks_of(V * 3, MT_THREADS)), dim3(MT_THREADS), 0, (hipStream_t)stream, verts, (int)V, vmax,
                       sums, sq, lr, alpha, eps, grad);
    hipLaunchKernelGGL(refine_clear_kernel, dim3(blocks_of(V, MT_THREADS)), dim3(MT_THREADS), 0, (hipStream_t)stream, vmax, (int)V);
    return vt_check(hipGetLastError(), "vt_refine_step");
}

size_t vt_refine_workspace_bytes(int64_t V, int64_t F, int composed_jet) {
    return mesh_ok(V, F) ? refine_layout(V, F, composed_jet).bytes : 0;
}

int vt_refine(const float *grid_cl, int R, int C, float *verts, int64_t V, const int32_t *faces, int64_t F, const float *blob,
              const float *blob_t, double padding, double threshold, double normal_weight, double lr, int steps, uint64_t seed,
              uint64_t first_step, const float *eps_given, float *sq, int composed_jet, float *terms, void *workspace, size_t workspace_bytes,
              void *stream) {
    if (!mesh_ok(V, F) || !grid_cl || !verts || !faces || !blob || !blob_t || !sq || steps < 0)
        return vt_fail(VT_ERR_INVALID, "vt_refine: bad argument (V >= 1, F >= 1, steps >= 0)");
    if (eps_given && steps > 1) return vt_fail(VT_ERR_INVALID, "vt_refine: a given eps is one step's");
    const RefineWs w = refine_layout(V, F, composed_jet);
    if (!workspace || workspace_bytes < w.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_refine");
    if (steps == 0) return 0;
    char *ws = static_cast<char *>(workspace);
    float *pts = reinterpret_cast<float *>(ws + w.pts), *eps = reinterpret_cast<float *>(ws + w.eps), *jet = reinterpret_cast<float *>(ws + w.jet);
    void *accum = ws + w.vmax;                                       // (vmax then sums, as vt_refine_accum_bytes lays them out)
    const size_t accum_bytes = w.jet_ws - w.vmax;
    int rc = vt_fill32(accum, 0u, accum_bytes, (hipStream_t)stream);
    if (rc) return rc;
    for (int it = 0; it < steps; ++it) {
        rc = vt_refine_sample(verts, V, faces, F, eps_given, seed, first_step + (uint64_t)it, eps, pts, stream);
        if (rc) return rc;
        rc = composed_jet ? vt_decode_jet_composed(grid_cl, 1, R, C, pts, F, blob, blob_t, padding, jet, ws + w.jet_ws, w.bytes - w.jet_ws, stream)
                          : vt_decode_jet(grid_cl, 1, R, C, pts, F, blob, blob_t, padding, jet, stream);
        if (rc) return rc;
        rc = vt_refine_face_grad(verts, V, faces, F, eps, jet, threshold, normal_weight, terms ? terms + (size_t)it * F * 2 : nullptr, accum,
                                 accum_bytes, stream);
        if (rc) return rc;
        rc = vt_refine_step(verts, V, accum, accum_bytes, sq, lr, 0.99, 1e-8, nullptr, stream);
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
