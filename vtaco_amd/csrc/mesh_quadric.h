// The quadric minimiser that mesh_simplify.hip and mesh_collapse.hip share (sections "mesh_simplify.hip" and "mesh_collapse.hip"):
// a cyclic Jacobi of the symmetric 3x3 in registers and the pseudo-inverse solve about a given point.  tests/mesh_simplify_ref.py (jacobi,
// solve) is the definition.  Everything lives in an unnamed namespace, as in mesh_common.h.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int MS_SWEEPS = 8;
constexpr double MS_EIG_REL = 1e-3;              // Lindstrom's threshold

// one rotation of the cyclic Jacobi on the symmetric a (both triangles kept) and the eigenvector columns v; R is the third index
template <int P, int Q, int R>
__device__ inline void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
}

// x = x0 + V pinv(Lambda) V^T (-b - A x0) over the eigenvalues above MS_EIG_REL of the largest (tests/mesh_simplify_ref.py: solve)
__device__ inline void quadric_solve(const double (&q)[10], const double (&x0)[3], double (&x)[3]) {
    double a[3][3] = {{q[0], q[1], q[2]}, {q[1], q[4], q[5]}, {q[2], q[5], q[7]}};
    const double b[3] = {q[3], q[6], q[8]};
    double g[3], v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = (-b[i]) - ((a[i][0] * x0[0] + a[i][1] * x0[1]) + a[i][2] * x0[2]);
    for (int sweep = 0; sweep < MS_SWEEPS; ++sweep) {
        jacobi_rotate<0, 1, 2>(a, v);
        jacobi_rotate<0, 2, 1>(a, v);
        jacobi_rotate<1, 2, 0>(a, v);
    }
    const double lam[3] = {a[0][0], a[1][1], a[2][2]};
    const double bound = MS_EIG_REL * fmax(fmax(lam[0], lam[1]), lam[2]);
    double coef[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double proj = (v[0][k] * g[0] + v[1][k] * g[1]) + v[2][k] * g[2];
        coef[k] = lam[k] > bound ? proj / lam[k] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = x0[i] + ((v[i][0] * coef[0] + v[i][1] * coef[1]) + v[i][2] * coef[2]);
}

}  // namespace
