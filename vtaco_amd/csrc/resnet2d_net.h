// resnet2d_net.h -- the kernels both eval-mode tactile ResNets launch besides their convs (resnet2d.hip: BasicBlock nets; resnet2d_bneck.hip:
// Bottleneck nets): the BatchNorm-folding pack, the stem with its max-pool, the tail.  See resnet2d.hip for the description.
#pragma once
#include "resnet2d_conv.h"

namespace {

// ---- pack: BatchNorm folded in f64, fragment order ---------------------------------------------------------------------------------
// conv fragments [Cout / 32][Cin / 8][ntaps][64 lanes][4]: lane l, slot j = W'[cb * 32 + l % 32][chunk * 8 + 4 (l / 32) + j][tap]
// stem fragments [2][21 rows = (c, ky)][64 lanes][4]:      lane l, slot j = W'[cb * 32 + l % 32][c][ky][kx = 2 j + l / 32] (kx 7: zero)
struct RnPack {
    const float *w, *gamma, *beta, *mean, *var;
    double eps;
    float *frag, *bias;
    int Cout, Cin, ntaps, stem;
};

__global__ void __launch_bounds__(256) resnet_pack_kernel(RnPack p) {
    const long long nf = p.stem ? RN_STEM_FRAG : (long long)p.Cout * p.Cin * p.ntaps;
    const int n_chunks = p.Cin / 8;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nf + p.Cout; e += (long long)gridDim.x * 256) {
        if (e >= nf) {
            const int co = (int)(e - nf);
            const double s = (double)p.gamma[co] / sqrt((double)p.var[co] + p.eps);
            p.bias[co] = (float)((double)p.beta[co] - (double)p.mean[co] * s);
            continue;
        }
        const int j = (int)(e & 3), l = (int)((e >> 2) & 63);
        long long q = e >> 8;
        int co;
        double v;
        if (p.stem) {
            const int r = (int)(q % RN_STEM_ROWS), cb = (int)(q / RN_STEM_ROWS);
            const int kx = 2 * j + (l >> 5), c = r / 7, ky = r % 7;
            co = cb * 32 + (l & 31);
            v = kx < 7 ? (double)p.w[((co * 3 + c) * 7 + ky) * 7 + kx] : 0.0;
        } else {
            const int t = (int)(q % p.ntaps); q /= p.ntaps;
            const int chunk = (int)(q % n_chunks), cb = (int)(q / n_chunks);
            const int ci = chunk * 8 + 4 * (l >> 5) + j;
            co = cb * 32 + (l & 31);
            v = (double)p.w[((size_t)co * p.Cin + ci) * p.ntaps + t];
        }
        const double s = (double)p.gamma[co] / sqrt((double)p.var[co] + p.eps);
        p.frag[e] = (float)(v * s);
    }
}

__global__ void __launch_bounds__(256) resnet_copy_kernel(const float *src, float *dst, long long n) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) dst[e] = src[e];
}

// ---- stem: 7x7 stride 2 + bias + ReLU + 3x3 stride-2 max-pool ------------------------------------------------------------------------
struct RnStem {
    const float *x;          // [n_img][3][H][W]
    const float *wfrag, *bias;
    float *out;              // [n_img][Hp][Wp][64]
    int H, W, Hs, Ws, Hp, Wp, tiles_x, tiles_y;
};

constexpr int RN_ST_PITCH = 65;      // LDS floats per stem pixel (odd: the 32 pixels of an accumulator row hit 32 banks)

__global__ void __launch_bounds__(192) resnet_stem_kernel(RnStem p) {
    __shared__ float s[81 * RN_ST_PITCH];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5, lp = lane & 31;
    const int tile = blockIdx.x;
    const int tx = tile % p.tiles_x, ty = (tile / p.tiles_x) % p.tiles_y, img = tile / (p.tiles_x * p.tiles_y);
    // this lane's stem pixel: slot sidx of the 9 x 9 patch under the tile's 4 x 4 pooled pixels
    const int sidx = wave * 32 + lp, ly = sidx / 9, lx = sidx % 9;
    const int sy = 8 * ty - 1 + ly, sx = 8 * tx - 1 + lx;
    const bool svalid = sidx < 81 && sy >= 0 && sy < p.Hs && sx >= 0 && sx < p.Ws;
    f32x16 acc[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
    const f32x4 *wf = reinterpret_cast<const f32x4 *>(p.wfrag) + lane;
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            const int iy = 2 * sy - 3 + ky;
            const bool rowok = svalid && iy >= 0 && iy < p.H;
            const int iyc = iy < 0 ? 0 : iy >= p.H ? p.H - 1 : iy;
            const float *row = p.x + (unsigned)(((img * 3 + c) * p.H + iyc) * p.W);
            float b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kx = 2 * j + h, ix = 2 * sx - 3 + kx;
                const bool ok = rowok && kx < 7 && ix >= 0 && ix < p.W;
                const float v = row[ix < 0 ? 0 : ix >= p.W ? p.W - 1 : ix];
                b[j] = ok ? v : 0.f;
            }
            const int r = c * 7 + ky;
            const f32x4 a0 = wf[(0 * RN_STEM_ROWS + r) * 64], a1 = wf[(1 * RN_STEM_ROWS + r) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0] = mfma(a0[j], b[j], acc[0]);
                acc[1] = mfma(a1[j], b[j], acc[1]);
            }
        }
    }
    // bias + ReLU into LDS; a stem pixel outside the image holds 0: every pool window has its centre inside, and the values are >= 0
    if (sidx < 81) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cb * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                const float v = fmaxf(acc[cb][r] + p.bias[co], 0.f);
                s[sidx * RN_ST_PITCH + co] = svalid ? v : 0.f;
            }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 16 * 64; o += 192) {
        const int c = o & 63, pp = o >> 6, py = pp >> 2, px = pp & 3;
        const int gy = ty * 4 + py, gx = tx * 4 + px;
        if (gy >= p.Hp || gx >= p.Wp) continue;
        float m = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, s[((2 * py + dy) * 9 + 2 * px + dx) * RN_ST_PITCH + c]);
        p.out[(unsigned)(((img * p.Hp + gy) * p.Wp + gx) * 64 + c)] = m;
    }
}

// ---- tail: global average pool, linear, fc --------------------------------------------------------------------------------------------
struct RnTail {
    const float *in;         // [n_img][HW][FEAT]
    const float *lw, *lb, *fw, *fb;
    float *out;              // [n_img][classes]
    int HW, classes;
};

template <int FEAT>
__global__ void __launch_bounds__(256) resnet_tail_kernel(RnTail p) {
    __shared__ double pooled[FEAT];
    __shared__ double hid[RN_LIN];
    const int img = blockIdx.x;
    for (int c = threadIdx.x; c < FEAT; c += 256) {
        double sum = 0.0;
        const float *q = p.in + (unsigned)(img * p.HW * FEAT + c);
        for (int px = 0; px < p.HW; ++px) sum += (double)q[(unsigned)(px * FEAT)];
        pooled[c] = (double)(float)(sum / (double)p.HW);               // (the reference's pooled tensor is f32)
    }
    __syncthreads();
    if (threadIdx.x < RN_LIN) {
        double a = (double)p.lb[threadIdx.x];
        const float *w = p.lw + threadIdx.x * FEAT;
        for (int k = 0; k < FEAT; ++k) a = fma((double)w[k], pooled[k], a);
        hid[threadIdx.x] = (double)(float)a;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < p.classes; o += 256) {
        double a = (double)p.fb[o];
        const float *w = p.fw + (size_t)o * RN_LIN;
        for (int k = 0; k < RN_LIN; ++k) a = fma((double)w[k], hid[k], a);
        p.out[(size_t)img * p.classes + o] = (float)a;
    }
}

int rn_pack_conv(const float *w, const vt_resnet_bn &bn, float *frag, float *bias, int Cout, int Cin, int ntaps, int stem, hipStream_t s) {
    if (!w || !rn_bn_ok(bn)) return vt_fail(VT_ERR_INVALID, "vt_resnet_pack: null conv weight or BatchNorm tensor");
    RnPack p;
    p.w = w; p.gamma = bn.weight; p.beta = bn.bias; p.mean = bn.running_mean; p.var = bn.running_var; p.eps = bn.eps;
    p.frag = frag; p.bias = bias; p.Cout = Cout; p.Cin = Cin; p.ntaps = ntaps; p.stem = stem;
    hipLaunchKernelGGL(resnet_pack_kernel, dim3(128), dim3(256), 0, s, p);
    return 0;
}

}  // namespace
