// The face arithmetic closest_point.hip and closest_point_tree.hip share: the 14-double face record, the code that fills it, and the
// squared distance from a point to a face.  Both files call these very functions, so a (query, face) pair gives one d2 and one q
// whichever kernel meets it.  Every product and sum is a separate rounding (-ffp-contract=off); tests/closest_point_ref.py
// (pairs_by_regions) restates the operations in this order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int CP_REC = 14;                      // doubles per face record (112 bytes: 16-byte aligned rows): a, ab, ac, d00, d01, d11, kind, 0
constexpr int CP_KIND = 12;                     // the record's kind slot: 0 regular, 1 degenerate, CP_SKIP
constexpr double CP_SKIP = 2.0;                 // the kind of a face with an index outside [0, V): never dereferenced, met by no query
constexpr int CP_BAD_INDEX = 1;                 // status bits
constexpr int CP_BAD_SCENE = 2;

// the record of face f: kind (rec[CP_KIND]) 0 regular, 1 degenerate (ab x ac is exactly zero), CP_SKIP (an index outside [0, V)).
// false for CP_SKIP: the caller reports it
__device__ inline bool cp_fill_record(const float *verts, int V, const int32_t *faces, size_t f, double *rec) {
    int idx[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        idx[k] = faces[3 * f + k];
        ok = ok && idx[k] >= 0 && idx[k] < V;
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < CP_REC; ++k) rec[k] = k == CP_KIND ? CP_SKIP : 0.0;
        return false;
    }
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) p[k][a] = (double)verts[3 * (size_t)idx[k] + a];
    const double abx = p[1][0] - p[0][0], aby = p[1][1] - p[0][1], abz = p[1][2] - p[0][2];
    const double acx = p[2][0] - p[0][0], acy = p[2][1] - p[0][1], acz = p[2][2] - p[0][2];
    const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    rec[0] = p[0][0]; rec[1] = p[0][1]; rec[2] = p[0][2];
    rec[3] = abx; rec[4] = aby; rec[5] = abz;
    rec[6] = acx; rec[7] = acy; rec[8] = acz;
    rec[9] = (abx * abx + aby * aby) + abz * abz;
    rec[10] = (abx * acx + aby * acy) + abz * acz;
    rec[11] = (acx * acx + acy * acy) + acz * acz;
    rec[CP_KIND] = (nx == 0.0 && ny == 0.0 && nz == 0.0) ? 1.0 : 0.0;
    rec[13] = 0.0;
    return true;
}

// the point of the segment o + t e, t in [0, 1], nearest p, and its squared distance; ew = e.(p - o), ee = e.e (ee == 0: the point o)
__device__ inline double cp_segment(double px, double py, double pz, double ox, double oy, double oz, double ex, double ey, double ez,
                                    double ew, double ee, double q[3]) {
    double t = ee > 0.0 ? ew / ee : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    q[0] = ox + ex * t; q[1] = oy + ey * t; q[2] = oz + ez * t;
    const double dx = px - q[0], dy = py - q[1], dz = pz - q[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// squared distance from p to the face of record r (kind 0 or 1), and the point q that attains it
__device__ inline double cp_face(const double *r, double px, double py, double pz, double q[3]) {
    const double ax = r[0], ay = r[1], az = r[2], abx = r[3], aby = r[4], abz = r[5], acx = r[6], acy = r[7], acz = r[8];
    const double d00 = r[9], d01 = r[10], d11 = r[11];
    const double apx = px - ax, apy = py - ay, apz = pz - az;
    const double d1 = (abx * apx + aby * apy) + abz * apz;
    const double d2 = (acx * apx + acy * apy) + acz * apz;
    if (r[CP_KIND] != 0.0) {                           // degenerate: the nearest of the edges ab, ac, bc (the first among equals)
        double best = cp_segment(px, py, pz, ax, ay, az, abx, aby, abz, d1, d00, q);
        double t[3];
        const double dac = cp_segment(px, py, pz, ax, ay, az, acx, acy, acz, d2, d11, t);
        if (dac < best) { best = dac; q[0] = t[0]; q[1] = t[1]; q[2] = t[2]; }
        const double bx = ax + abx, by = ay + aby, bz = az + abz, ex = acx - abx, ey = acy - aby, ez = acz - abz;
        const double wx = px - bx, wy = py - by, wz = pz - bz;
        const double dbc = cp_segment(px, py, pz, bx, by, bz, ex, ey, ez, (ex * wx + ey * wy) + ez * wz, (ex * ex + ey * ey) + ez * ez, t);
        if (dbc < best) { best = dbc; q[0] = t[0]; q[1] = t[1]; q[2] = t[2]; }
        return best;
    }
    const double d3 = d1 - d00, d4 = d2 - d01, d5 = d1 - d01, d6 = d2 - d11;
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    // lowest priority first, every later region overrides: inside, bc, ac, c, ab, b, a
    double nv = vb, nw = vc, den = (va + vb) + vc;
    bool on_bc = false;
    if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) { nv = 0.0; nw = e43; den = e43 + e56; on_bc = true; }
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { nv = 0.0; nw = d2; den = d2 - d6; on_bc = false; }
    if (d6 >= 0.0 && d5 <= d6) { nv = 0.0; nw = 1.0; den = 1.0; on_bc = false; }
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { nv = d1; nw = 0.0; den = d1 - d3; on_bc = false; }
    if (d3 >= 0.0 && d4 <= d3) { nv = 1.0; nw = 0.0; den = 1.0; on_bc = false; }
    if (d1 <= 0.0 && d2 <= 0.0) { nv = 0.0; nw = 0.0; den = 1.0; on_bc = false; }
    if (!(den > 0.0)) { nv = 0.0; nw = 0.0; den = 1.0; on_bc = false; }
    const double w = nw / den;
    const double v = on_bc ? 1.0 - w : nv / den;
    q[0] = (ax + abx * v) + acx * w; q[1] = (ay + aby * v) + acy * w; q[2] = (az + abz * v) + acz * w;
    const double dx = px - q[0], dy = py - q[1], dz = pz - q[2];
    return (dx * dx + dy * dy) + dz * dz;
}
