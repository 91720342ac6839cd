// The ray / face rule ray_mesh.hip's brute-force kernel and its tree walk share: both call these very functions, so a (ray, face) pair
// gives one s and one set of weights whichever kernel meets it.  Rays are o + s d in float64; d is NOT normalised and s is in units of d.
// The rule is the watertight test of Woop, Benthin and Wald (2013), two-sided.  Every product and sum is a separate rounding
// (-ffp-contract=off); tests/ray_mesh_ref.py (pairs) restates the operations in this order.
//   per ray   kz = the axis of the largest |d_a| (the lowest among equals), kx, ky the next two cyclically, swapped when d[kz] < 0;
//             Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  A direction that is all zero or has a component that is not
//             finite, or an origin that is not finite, makes the ray invalid: it misses every face and no face is read for it
//   per face  corners exactly converted from f32; A = a - o, Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], the same for B and C;
//             U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax; a miss when one of them is < 0 and another > 0;
//             det = (U + V) + W, a miss when det == 0 (degenerate and edge-on faces);
//             s = ((U (Sz A[kz]) + V (Sz B[kz])) + W (Sz C[kz])) / det; a hit when t_min <= s <= t_max (a NaN is a miss)
// What the rule guarantees:
//   * no leaks   zeros are accepted on both sides of an edge, and the two faces of a shared edge compute that edge's function from the
//                same two products (the sheared corners depend on the ray and the corner alone, not on the face): fl(p - q) in one,
//                fl(q - p) in the other, exact negatives.  A ray therefore cannot be strictly outside both across their common edge
//   * no NaN     a NaN in U, V, W or det passes every comparison above and ends in "NaN is a miss"; s is written only for a hit
//   * repeated corners give U = -V, W = 0 (or a rotation of it) exactly, so det == 0: never a hit
// Not guaranteed: that a face seen edge-on to within rounding (collinear corners in general position, a sliver whose U, V, W are all
// rounding noise) misses; DESIGN.md, "ray_mesh.hip", says what the tree's slack covers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct RfRay {
    double ox, oy, oz;          // o[kx], o[ky], o[kz]
    double Sx, Sy, Sz;
    int kx, ky, kz;
    bool ok;
};

__device__ inline double rf_pick(double x, double y, double z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

__device__ inline bool rf_finite(double x) { return fabs(x) < __builtin_inf(); }        // false for a NaN

__device__ inline void rf_setup(const double o[3], const double d[3], RfRay &r) {
    const double a0 = fabs(d[0]), a1 = fabs(d[1]), a2 = fabs(d[2]);
    r.ok = rf_finite(o[0]) && rf_finite(o[1]) && rf_finite(o[2]) && rf_finite(d[0]) && rf_finite(d[1]) && rf_finite(d[2]) &&
           (a0 > 0.0 || a1 > 0.0 || a2 > 0.0);
    int kz = 0;
    double m = a0;
    if (a1 > m) { kz = 1; m = a1; }
    if (a2 > m) { kz = 2; m = a2; }
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const double dz = rf_pick(d[0], d[1], d[2], kz);
    if (dz < 0.0) { const int t = kx; kx = ky; ky = t; }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.Sx = rf_pick(d[0], d[1], d[2], kx) / dz;
    r.Sy = rf_pick(d[0], d[1], d[2], ky) / dz;
    r.Sz = 1.0 / dz;
    r.ox = rf_pick(o[0], o[1], o[2], kx); r.oy = rf_pick(o[0], o[1], o[2], ky); r.oz = rf_pick(o[0], o[1], o[2], kz);
}

// the face with corners a, b, c (three doubles each) against a valid ray: true for a hit, with its parameter s.  uvw, when given, takes
// U, V, W and det (the weights are U / det, V / det, W / det), for a hit only
__device__ inline bool rf_face(const RfRay &r, const double *a, const double *b, const double *c, double t_min, double t_max, double &s,
                               double *uvw = nullptr) {
    const double Az = rf_pick(a[0], a[1], a[2], r.kz) - r.oz, Bz = rf_pick(b[0], b[1], b[2], r.kz) - r.oz, Cz = rf_pick(c[0], c[1], c[2], r.kz) - r.oz;
    const double Ax = (rf_pick(a[0], a[1], a[2], r.kx) - r.ox) - r.Sx * Az, Ay = (rf_pick(a[0], a[1], a[2], r.ky) - r.oy) - r.Sy * Az;
    const double Bx = (rf_pick(b[0], b[1], b[2], r.kx) - r.ox) - r.Sx * Bz, By = (rf_pick(b[0], b[1], b[2], r.ky) - r.oy) - r.Sy * Bz;
    const double Cx = (rf_pick(c[0], c[1], c[2], r.kx) - r.ox) - r.Sx * Cz, Cy = (rf_pick(c[0], c[1], c[2], r.ky) - r.oy) - r.Sy * Cz;
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;
    const double det = (U + V) + W;
    if (det == 0.0) return false;
    const double t = ((U * (r.Sz * Az) + V * (r.Sz * Bz)) + W * (r.Sz * Cz)) / det;
    if (!(t >= t_min && t <= t_max)) return false;
    s = t;
    if (uvw) { uvw[0] = U; uvw[1] = V; uvw[2] = W; uvw[3] = det; }
    return true;
}
