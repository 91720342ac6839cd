// The tactile assignment rule of one query point, shared by vt_tactile_assign (tactile.hip: a fresh id per point) and
// vt_touch_merge (touch.hip: a touch merged into a session's id lattice).  Reference src/conv_onet/generation.py:186-200
// (mode 0: nearest fingertip within the radius, if that finger's touch succeeded) and :245-255 (mode 1: within the radius of any
// of a finger's contact points; later fingers overwrite earlier ones).  Distances in double, like scipy's cdist.
#pragma once
#include "decode_common.h"

namespace {

constexpr int VT_TACTILE_MAX_F = 256;

struct TactileRule {
    const float *anchors;         // [F][K][3]
    const int *count;             // [F] valid anchors per finger (<= K)
    const unsigned char *success; // [F] touch_success
    int F, K, mode;               // mode 0: nearest fingertip (K = 1), 1: any contact point within radius
    double radius;
};

// Stage the anchors in LDS (anc: F*K*3 floats) and, in mode 1, every finger's bounds of its valid anchors (box).  A contact
// cloud is a few millimetres across and the radius two lattice cells: a point outside the cloud's bounds grown by the radius
// cannot be within it of any anchor (|d| >= |dx|), so all but a few hundred of the 2 M lattice points skip the finger's anchor
// loop after six compares (1.2 ms -> 0.03 ms at 128^3; the result is the loop's, bit for bit).  Ends with a barrier.
__device__ __forceinline__ void tactile_stage(const TactileRule &r, float *anc, float (*box)[6]) {
    for (int i = threadIdx.x; i < r.F * r.K * 3; i += blockDim.x) anc[i] = r.anchors[i];
    __syncthreads();
    if (r.mode == 1 && (int)threadIdx.x < r.F) {
        const float *q = anc + (size_t)threadIdx.x * r.K * 3;
        float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
        for (int k = 0; k < r.count[threadIdx.x]; ++k)
            for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], q[3 * k + c]); hi[c] = fmaxf(hi[c], q[3 * k + c]); }
        for (int c = 0; c < 3; ++c) { box[threadIdx.x][c] = lo[c]; box[threadIdx.x][3 + c] = hi[c]; }
    }
    __syncthreads();
}

__device__ __forceinline__ double tactile_grow(const TactileRule &r) { return r.radius * (1.0 + 1e-9); }

// the finger of point (px, py, pz), 255 = none
__device__ __forceinline__ int tactile_finger(const TactileRule &r, const float *anc, const float (*box)[6], double grow,
                                              float px, float py, float pz) {
    int id = 255;
    if (r.mode == 0) {
        double best = 1e300;
        int arg = 0;
        for (int f = 0; f < r.F; ++f) {
            const double dx = (double)px - (double)anc[f * 3], dy = (double)py - (double)anc[f * 3 + 1], dz = (double)pz - (double)anc[f * 3 + 2];
            const double dist = sqrt(dx * dx + dy * dy + dz * dz);
            if (dist < best) { best = dist; arg = f; }          // first minimum, like np.argmin
        }
        if (best < r.radius && r.success[arg]) id = arg;
    } else {
        for (int f = 0; f < r.F; ++f) {
            if (!r.success[f]) continue;
            if ((double)px < (double)box[f][0] - grow || (double)px > (double)box[f][3] + grow ||
                (double)py < (double)box[f][1] - grow || (double)py > (double)box[f][4] + grow ||
                (double)pz < (double)box[f][2] - grow || (double)pz > (double)box[f][5] + grow) continue;
            const float *q = anc + (size_t)f * r.K * 3;
            bool hit = false;
            for (int k = 0; k < r.count[f] && !hit; ++k) {
                const double dx = (double)q[3 * k] - (double)px, dy = (double)q[3 * k + 1] - (double)py, dz = (double)q[3 * k + 2] - (double)pz;
                hit = sqrt(dx * dx + dy * dy + dz * dz) < r.radius;
            }
            if (hit) id = f;                                    // later fingers overwrite earlier ones
        }
    }
    return id;
}

}  // namespace
