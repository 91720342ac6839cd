// unet2d_train.hip -- the tactile depth estimator (reference ``UNet``, src/layers.py:322-450) in TRAIN mode: the forward with batch
// statistics and the backward for every parameter, on hand-written kernels.  vt_tactile_unet_train_fwd, vt_tactile_unet_bwd.
//
// The input is x [S * G][Cin][H][W], scene-major: images s * G .. s * G + G - 1 are one statistics group (the reference calls the net
// once per scene on its G = 5 images, so every BatchNorm sees one scene's images alone).  Per 3x3 conv:
//
//   conv      z = conv(a_in) + b with the eval path's implicit-GEMM template (unet2d_conv.h, epilogue TU_RAW: no ReLU), exact-f32 matrix
//             core, the raw weights packed into fragment order at every call.  The first conv reads x as channels-last padded to 8
//             channels, so it is the same template.
//   stats     per (group, channel) sum and sum of squares of z in f64: slices of TT_SLICE pixels of ONE group (tt_reduce_kernel), the
//             slices combined one after the other (tt_finalize_kernel) -> mean, biased variance, 1 / sqrt(var + eps).
//   bn+relu   a = relu(gamma (z - mean) rstd + beta); a down block's second conv also writes the 2x2 max-pool.
//   A block's ONE bn module follows both convs: gamma and beta are shared, each use has its own statistics.
//   Then the transposed 2x2/2 conv (template TU_UP), the two-source first conv of an up block (no concat), conv_final + sigmoid.
//   Running statistics: one kernel, per block and channel, for each scene in order and per scene conv1's use then conv2's:
//   running = (1 - m) running + m batch (unbiased variance) -- what S sequential module calls do.
//
// Backward (from dout [S * G][classes][H][W]; no gradient for the images), per conv in reverse:
//   g = (sum of the incoming gradients, the max-pool's routed to the first maximum of its window) * (a > 0)
//   sums of g and g xhat per (group, channel) with the same slice scheme -> dbeta, dgamma (conv2's use first, conv1's added) and
//   dz = gamma rstd (g - mean(g) - xhat mean(g xhat))
//   bias gradient: the sum of dz, same scheme.
//   weight gradient (tt_wgrad_kernel): dW[co][ci][tap] = sum over pixels dz[px][co] a_in[px + tap][ci] on the matrix core, A = 32 output
//   channels, B = 32 input channels, k = pixels; a wave owns 8 rows of one image and all taps; the per-(image, row block) partials
//   are combined in f64 in image order (tt_wcombine_kernel).  The transposed conv's weight gradient is the same kernel with its 4
//   parities as taps.
//   data gradient: the same conv template with flipped, transposed weights (TU_RAW); the transposed conv's is a 2x2 stride-2 conv
//   (TU_S2D).
//
// Every sum has a fixed order that depends on neither S nor the launch; no floating-point atomics.  The results are bit-reproducible,
// a scene's outputs and statistics do not depend on the other scenes of the call, and scenes whose dout is zero add exact zeros.
//
// Covered (vt_tactile_unet_train_supported): what vt_tactile_unet_supported covers with start_filts a power of two (8, 16, 32, 64):
// depth 1..5, in_channels 1..4, num_classes 1..4, 1 <= n_img <= 1024, H and W multiples of 2^(depth-1) up to 2048,
// n_img * H * W * start_filts < 2^31; group >= 1 dividing n_img; at least 2 values per group and channel at the bottom level.
#include "unet2d_conv.h"

namespace {

constexpr int TT_SLICE = 4096;     // pixels of one group per partial of a per-channel sum
constexpr int TT_ROWS = 8;         // image rows per partial of a weight gradient

struct TtDims { TuDims d; int G, S; };

inline bool tt_dims_ok(const TtDims &t) {
    const TuDims &d = t.d;
    if (!tu_dims_ok(d)) return false;
    if (d.sf != 8 && d.sf != 16 && d.sf != 32 && d.sf != 64) return false;
    if (t.G < 1 || d.n_img % t.G) return false;
    return (long long)t.G * (d.H >> (d.depth - 1)) * (d.W >> (d.depth - 1)) >= 2;
}

// ---- workspace (floats; every offset a multiple of 4) ---------------------------------------------------------------------------------
struct TtStat { long long f, d; };                      // floats [2][S][C]: mean, rstd; doubles [2][S][C]: mean, biased variance
struct TtWs {
    long long xcl, dt;
    long long dz[VT_TACTILE_UNET_MAX_DEPTH][2], da[VT_TACTILE_UNET_MAX_DEPTH][2], pooled[VT_TACTILE_UNET_MAX_DEPTH];
    long long up[VT_TACTILE_UNET_MAX_DEPTH], uz[VT_TACTILE_UNET_MAX_DEPTH][2], ua[VT_TACTILE_UNET_MAX_DEPTH][2];
    long long gx[VT_TACTILE_UNET_MAX_DEPTH], gy[VT_TACTILE_UNET_MAX_DEPTH], gz[VT_TACTILE_UNET_MAX_DEPTH];
    TtStat dstat[VT_TACTILE_UNET_MAX_DEPTH][2], ustat[VT_TACTILE_UNET_MAX_DEPTH][2];
    long long m12, red, wpart, frag, bias, total;
};
inline long long tt_up4(long long n) { return (n + 3) / 4 * 4; }
inline int tt_nsl(const TtDims &t, int lvl) { return (int)(((long long)t.G * (t.d.H >> lvl) * (t.d.W >> lvl) + TT_SLICE - 1) / TT_SLICE); }
inline long long tt_chunks(const TtDims &t, int h) { return (long long)t.d.n_img * ((h + TT_ROWS - 1) / TT_ROWS); }

inline TtWs tt_workspace(const TtDims &t) {
    const TuDims &d = t.d;
    TtWs w{};
    long long off = 0;
    auto take = [&](long long n) { const long long o = off; off += tt_up4(n); return o; };
    const long long P = (long long)d.n_img * d.H * d.W;
    const int cmax = d.sf << (d.depth - 1);
    w.xcl = take(P * 8);
    w.dt = take(P * d.classes);
    long long red = 0, wpart = 0;
    for (int i = 0; i < d.depth; ++i) {
        const int c = d.sf << i, h = d.H >> i;
        const long long n = (long long)d.n_img * h * (d.W >> i) * c;
        const bool bottom = i == d.depth - 1;
        auto stat = [&](TtStat &s) { s.f = take(2ll * t.S * c); s.d = take(4ll * t.S * c); };
        for (int k = 0; k < 2; ++k) { w.dz[i][k] = take(n); w.da[i][k] = take(n); stat(w.dstat[i][k]); }
        w.gx[i] = take(n); w.gy[i] = take(n);
        if (!bottom) {
            w.pooled[i] = take(n / 4);
            w.up[i] = take(n);
            for (int k = 0; k < 2; ++k) { w.uz[i][k] = take(n); w.ua[i][k] = take(n); stat(w.ustat[i][k]); }
            w.gz[i] = take(n);
        }
        const long long r = 2ll * t.S * tt_nsl(t, i) * 2 * c * (i == 0 ? VT_TACTILE_UNET_MAX_CLASSES : 1);     // doubles, as floats
        if (r > red) red = r;
        // weight-gradient partials: the 3x3 convs of this level (K up to 2 c through two launches of c) and the up-conv ending here
        long long p = tt_chunks(t, h) * c * (long long)(i == 0 ? (c > 8 ? c : 8) : c) * 9;
        if (p > wpart) wpart = p;
        if (!bottom) { p = tt_chunks(t, h / 2) * 2ll * c * c * 4; if (p > wpart) wpart = p; }
    }
    w.m12 = take(2ll * t.S * cmax);
    w.red = take(red);
    w.wpart = take(wpart);
    w.frag = take(tu_frag_floats(cmax, cmax, 9));
    w.bias = take(tu_ncb(cmax) * 32);
    w.total = off;
    return w;
}

// ---- packing: raw weights -> fragments [ncb][Cin / 8][ntaps][64 lanes][4] (tapmajor: [ncb][ntaps][Cin / 8][64][4]) -------------------
// lane l, slot j = w[base + o * so + k * sk + tap'], o = cb * 32 + l % 32 (output), k = chunk * 8 + 4 (l / 32) + j (input), tap' = tap or,
// flipped, ntaps - 1 - tap; zero for o >= Cout or k >= CinReal.  The bias is copied behind it, zero padded to 32 ncb.
struct TtPack { const float *w, *b; float *frag, *bias; int Cout, Cin, CinReal, ntaps, so, sk, base, flip, tapmajor; };

__global__ void __launch_bounds__(256) tt_pack_kernel(TtPack p) {
    const int ncb = (p.Cout + 31) / 32, n_chunks = p.Cin / 8;
    const long long nf = (long long)ncb * n_chunks * p.ntaps * 256, nb = ncb * 32;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nf + nb; e += (long long)gridDim.x * 256) {
        if (e >= nf) {
            const int co = (int)(e - nf);
            p.bias[co] = p.b && co < p.Cout ? p.b[co] : 0.f;
            continue;
        }
        const int j = (int)(e & 3), l = (int)((e >> 2) & 63);
        long long q = e >> 8;
        int t, chunk, cb;
        if (p.tapmajor) { chunk = (int)(q % n_chunks); q /= n_chunks; t = (int)(q % p.ntaps); cb = (int)(q / p.ntaps); }
        else { t = (int)(q % p.ntaps); q /= p.ntaps; chunk = (int)(q % n_chunks); cb = (int)(q / n_chunks); }
        const int k = chunk * 8 + 4 * (l >> 5) + j, o = cb * 32 + (l & 31);
        float v = 0.f;
        if (o < p.Cout && k < p.CinReal) v = p.w[(size_t)p.base + (size_t)o * p.so + (size_t)k * p.sk + (p.flip ? p.ntaps - 1 - t : t)];
        p.frag[e] = v;
    }
}

// x [n][cin][H][W] -> [n][H][W][8], channels past cin zero
__global__ void __launch_bounds__(256) tt_to_cl_kernel(const float *x, float *out, int cin, int HW, int P) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= P) return;
    const int img = pix / HW, r = pix % HW;
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < cin; ++c) lo[c] = x[(size_t)(img * cin + c) * HW + r];
    f32x4 *o = reinterpret_cast<f32x4 *>(out + (size_t)pix * 8);
    o[0] = lo; o[1] = hi;
}

// ---- per-channel sums ---------------------------------------------------------------------------------------------------------------------
enum { TT_STATS = 0, TT_BNBWD = 1, TT_SUM = 2, TT_FINAL = 3 };
// part [classes or 1][groups][nsl][2][C] doubles
struct TtRed { const float *v, *z, *mean, *rstd; double *part; int C, Pg, nsl, groups, HW, classes; };

template <int MODE>
__global__ void __launch_bounds__(256) tt_reduce_kernel(TtRed p) {
    __shared__ double sh[2][256];
    const int CBk = p.C < 256 ? p.C : 256, PL = 256 / CBk;            // (C is a power of two >= 8)
    const int cl = threadIdx.x % CBk, pl = threadIdx.x / CBk, c = blockIdx.y * CBk + cl;
    const int g = blockIdx.x / p.nsl, s = blockIdx.x % p.nsl, k = blockIdx.z;
    const int j0 = s * TT_SLICE, j1 = j0 + TT_SLICE < p.Pg ? j0 + TT_SLICE : p.Pg;
    double s0 = 0.0, s1 = 0.0;
    float mu = 0.f, rs = 0.f;
    if (MODE == TT_BNBWD) { mu = p.mean[g * p.C + c]; rs = p.rstd[g * p.C + c]; }
    for (int j = j0 + pl; j < j1; j += PL) {
        const int pix = g * p.Pg + j;
        const size_t idx = (size_t)pix * p.C + c;
        if (MODE == TT_STATS) { const double v = p.z[idx]; s0 += v; s1 += v * v; }
        else if (MODE == TT_BNBWD) { const float gg = p.v[idx], xh = (p.z[idx] - mu) * rs; s0 += gg; s1 += (double)gg * (double)xh; }
        else if (MODE == TT_SUM) s0 += p.v[idx];
        else {
            const int img = pix / p.HW, r = pix % p.HW;
            const double dd = p.v[(size_t)(img * p.classes + k) * p.HW + r];
            s0 += dd * (double)p.z[idx]; s1 += dd;
        }
    }
    sh[0][threadIdx.x] = s0; sh[1][threadIdx.x] = s1;
    __syncthreads();
    if (pl == 0) {
        for (int q = 1; q < PL; ++q) { s0 += sh[0][q * CBk + cl]; s1 += sh[1][q * CBk + cl]; }
        double *o = p.part + ((((size_t)k * p.groups + g) * p.nsl + s) * 2) * p.C + c;
        o[0] = s0; o[p.C] = s1;
    }
}

struct TtFin {
    const double *part; int mode, C, Pg, nsl, groups, accumulate; double eps;
    float *o0, *o1; double *od;      // STATS: mean, rstd [groups][C], od [2][groups][C] (mean, biased variance); BNBWD: mean(g), mean(g xhat)
    float *p0, *p1;                  // BNBWD: dbeta, dgamma [C]; SUM: the sum [C]; FINAL: dW [k][C], db [k]
};

__global__ void __launch_bounds__(64) tt_finalize_kernel(TtFin p) {
    const int c = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y;
    if (c >= p.C) return;
    double t0 = 0.0, t1 = 0.0;
    for (int g = 0; g < p.groups; ++g) {
        double s0 = 0.0, s1 = 0.0;
        const double *src = p.part + (((size_t)k * p.groups + g) * p.nsl * 2) * p.C + c;
        for (int s = 0; s < p.nsl; ++s) { s0 += src[(size_t)s * 2 * p.C]; s1 += src[(size_t)s * 2 * p.C + p.C]; }
        if (p.mode == TT_STATS) {
            const double mean = s0 / p.Pg;
            double var = s1 / p.Pg - mean * mean;
            var = var > 0.0 ? var : 0.0;
            p.o0[g * p.C + c] = (float)mean;
            p.o1[g * p.C + c] = (float)(1.0 / sqrt(var + p.eps));
            p.od[g * p.C + c] = mean;
            p.od[(size_t)p.groups * p.C + g * p.C + c] = var;
        } else if (p.mode == TT_BNBWD) {
            p.o0[g * p.C + c] = (float)(s0 / p.Pg);
            p.o1[g * p.C + c] = (float)(s1 / p.Pg);
        }
        t0 += s0; t1 += s1;
    }
    if (p.mode == TT_BNBWD) {
        p.p0[c] = p.accumulate ? p.p0[c] + (float)t0 : (float)t0;
        p.p1[c] = p.accumulate ? p.p1[c] + (float)t1 : (float)t1;
    } else if (p.mode == TT_SUM) {
        p.p0[c] = (float)t0;
    } else if (p.mode == TT_FINAL) {
        p.p0[k * p.C + c] = (float)t0;
        if (c == 0) p.p1[k] = (float)t1;
    }
}

// ---- BatchNorm + ReLU (+ 2x2 max-pool) ----------------------------------------------------------------------------------------------------
struct TtBn { const float *z, *mean, *rstd, *gamma, *beta; float *a, *pooled; int C, H, W, n_img, G; };

__device__ __forceinline__ f32x4 tt_bn4(const f32x4 z, const f32x4 mu, const f32x4 rs, const f32x4 ga, const f32x4 be) {
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = fmaxf(fmaf((z[i] - mu[i]) * rs[i], ga[i], be[i]), 0.f);
    return r;
}

template <bool POOL>
__global__ void __launch_bounds__(256) tt_bn_relu_kernel(TtBn p) {
    const int q4 = p.C >> 2, Hh = POOL ? p.H >> 1 : p.H, Wh = POOL ? p.W >> 1 : p.W;
    const unsigned total = (unsigned)p.n_img * Hh * Wh * q4, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int cq = idx % q4, pix = idx / q4, x = pix % Wh, y = (pix / Wh) % Hh, img = pix / (Wh * Hh), g = img / p.G;
    const f32x4 mu = *reinterpret_cast<const f32x4 *>(p.mean + g * p.C + 4 * cq), rs = *reinterpret_cast<const f32x4 *>(p.rstd + g * p.C + 4 * cq);
    const f32x4 ga = *reinterpret_cast<const f32x4 *>(p.gamma + 4 * cq), be = *reinterpret_cast<const f32x4 *>(p.beta + 4 * cq);
    if (!POOL) {
        const size_t o = (size_t)pix * p.C + 4 * cq;
        *reinterpret_cast<f32x4 *>(p.a + o) = tt_bn4(*reinterpret_cast<const f32x4 *>(p.z + o), mu, rs, ga, be);
    } else {
        f32x4 m;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const size_t o = ((size_t)(img * p.H + 2 * y + (w >> 1)) * p.W + 2 * x + (w & 1)) * p.C + 4 * cq;
            const f32x4 a = tt_bn4(*reinterpret_cast<const f32x4 *>(p.z + o), mu, rs, ga, be);
            *reinterpret_cast<f32x4 *>(p.a + o) = a;
#pragma unroll
            for (int i = 0; i < 4; ++i) m[i] = w == 0 ? a[i] : fmaxf(m[i], a[i]);
        }
        *reinterpret_cast<f32x4 *>(p.pooled + (size_t)pix * p.C + 4 * cq) = m;
    }
}

// g = (g + da2 + the pool's gradient where this pixel is the first maximum of its window) * (a > 0), in place
struct TtG { float *g; const float *da2, *a, *dpool; int C, H, W, n_img; };

__global__ void __launch_bounds__(256) tt_make_g_kernel(TtG p) {
    const int q4 = p.C >> 2;
    const unsigned total = (unsigned)p.n_img * p.H * p.W * q4, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int cq = idx % q4, pix = idx / q4;
    const size_t o = (size_t)pix * p.C + 4 * cq;
    f32x4 v = *reinterpret_cast<const f32x4 *>(p.g + o);
    const f32x4 a = *reinterpret_cast<const f32x4 *>(p.a + o);
    if (p.da2) { const f32x4 d = *reinterpret_cast<const f32x4 *>(p.da2 + o); v += d; }
    if (p.dpool) {
        const int x = pix % p.W, y = (pix / p.W) % p.H, img = pix / (p.W * p.H), me = (y & 1) * 2 + (x & 1);
        f32x4 w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w[k] = *reinterpret_cast<const f32x4 *>(p.a + ((size_t)(img * p.H + (y & ~1) + (k >> 1)) * p.W + (x & ~1) + (k & 1)) * p.C + 4 * cq);
        const f32x4 dp = *reinterpret_cast<const f32x4 *>(p.dpool + ((size_t)(img * (p.H >> 1) + (y >> 1)) * (p.W >> 1) + (x >> 1)) * p.C + 4 * cq);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int first = 0;
            float m = w[0][i];
#pragma unroll
            for (int k = 1; k < 4; ++k) if (w[k][i] > m) { m = w[k][i]; first = k; }
            if (first == me) v[i] += dp[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = a[i] > 0.f ? v[i] : 0.f;
    *reinterpret_cast<f32x4 *>(p.g + o) = v;
}

// dz = gamma rstd (g - mean(g) - xhat mean(g xhat)), in place
struct TtBnB { float *g; const float *z, *mean, *rstd, *gamma, *m1, *m2; int C, HW, n_img, G; };

__global__ void __launch_bounds__(256) tt_bn_bwd_kernel(TtBnB p) {
    const int q4 = p.C >> 2;
    const unsigned total = (unsigned)p.n_img * p.HW * q4, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int cq = idx % q4, pix = idx / q4, g = (pix / p.HW) / p.G;
    const size_t o = (size_t)pix * p.C + 4 * cq;
    const int s = g * p.C + 4 * cq;
    const f32x4 mu = *reinterpret_cast<const f32x4 *>(p.mean + s), rs = *reinterpret_cast<const f32x4 *>(p.rstd + s);
    const f32x4 m1 = *reinterpret_cast<const f32x4 *>(p.m1 + s), m2 = *reinterpret_cast<const f32x4 *>(p.m2 + s);
    const f32x4 ga = *reinterpret_cast<const f32x4 *>(p.gamma + 4 * cq), z = *reinterpret_cast<const f32x4 *>(p.z + o);
    f32x4 v = *reinterpret_cast<const f32x4 *>(p.g + o);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float xh = (z[i] - mu[i]) * rs[i];
        v[i] = (ga[i] * rs[i]) * ((v[i] - m1[i]) - xh * m2[i]);
    }
    *reinterpret_cast<f32x4 *>(p.g + o) = v;
}

// ---- conv_final + sigmoid, and its backward ------------------------------------------------------------------------------------------------
struct TtFinal { const float *a, *w, *b, *dout, *y; float *out, *dt, *da; int C, classes, HW, P; };

__global__ void __launch_bounds__(256) tt_final_fwd_kernel(TtFinal p) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= p.P) return;
    const int img = pix / p.HW, r = pix % p.HW;
    const float *a = p.a + (size_t)pix * p.C;
    for (int k = 0; k < p.classes; ++k) {
        float t = 0.f;
        for (int c = 0; c < p.C; c += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(a + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) t = fmaf(p.w[k * p.C + c + i], v[i], t);
        }
        t += p.b[k];
        p.out[(size_t)(img * p.classes + k) * p.HW + r] = 1.f / (1.f + expf(-t));
    }
}

// dt = dout y (1 - y) [n][classes][HW]; da[px][c] = sum_k w[k][c] dt[k][px]
__global__ void __launch_bounds__(256) tt_final_bwd_kernel(TtFinal p) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= p.P) return;
    const int img = pix / p.HW, r = pix % p.HW;
    float dt[VT_TACTILE_UNET_MAX_CLASSES];
    for (int k = 0; k < VT_TACTILE_UNET_MAX_CLASSES; ++k) {
        dt[k] = 0.f;
        if (k < p.classes) {
            const size_t o = (size_t)(img * p.classes + k) * p.HW + r;
            const float y = p.y[o];
            dt[k] = p.dout[o] * (y * (1.f - y));
            p.dt[o] = dt[k];
        }
    }
    float *da = p.da + (size_t)pix * p.C;
    for (int c = 0; c < p.C; c += 4) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < p.classes; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaf(p.w[k * p.C + c + i], dt[k], v[i]);
        *reinterpret_cast<f32x4 *>(da + c) = v;
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------------------
// D[ca][cb][tap] = sum over the pixels (y, x) of A[img][y][x][ca] * B[img][y'][x'][cb]; MODE 0: 9 taps, (y', x') = (y + ky - 1, x + kx - 1)
// in B's [H][W] image, zero outside; MODE 1: 4 taps, (y', x') = (2 y + dy, 2 x + dx) in B's [2 H][2 W] image.
// part [chunk][CA][CB][ntaps], chunk = img * chunks_per_img + row block.
struct TtWg { const float *A, *B; float *part; int CA, CB, H, W, cpi, nchunks, nBb; };

template <int MODE>
__global__ void __launch_bounds__(256) tt_wgrad_kernel(TtWg p) {
    constexpr int NTAP = MODE == 0 ? 9 : 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5, lp = lane & 31;
    const int chunk = blockIdx.x * 4 + wave;
    if (chunk >= p.nchunks) return;                                    // (wave-uniform; no barrier in this kernel)
    const int ab = blockIdx.y / p.nBb, bb = blockIdx.y % p.nBb;
    const int img = chunk / p.cpi, y0 = (chunk % p.cpi) * TT_ROWS, y1 = y0 + TT_ROWS < p.H ? y0 + TT_ROWS : p.H;
    const int ca = ab * 32 + lp, cb = bb * 32 + lp;
    const bool okA = ca < p.CA, okB = cb < p.CB;
    const int cal = okA ? ca : 0, cbl = okB ? cb : 0;
    const int HB = MODE == 0 ? p.H : 2 * p.H, WB = MODE == 0 ? p.W : 2 * p.W;
    const float *Ai = p.A + (size_t)img * p.H * p.W * p.CA + cal, *Bi = p.B + (size_t)img * HB * WB * p.CB + cbl;
    f32x16 acc[NTAP];
#pragma unroll
    for (int t = 0; t < NTAP; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    for (int y = y0; y < y1; ++y) {
#pragma unroll 2
        for (int x0 = 0; x0 < p.W; x0 += 2) {
            const int x = x0 + h;
            const bool vx = x < p.W;
            const int xc = vx ? x : p.W - 1;
            float av = Ai[(unsigned)((y * p.W + xc) * p.CA)];
            if (!(vx && okA)) av = 0.f;
            float bv[NTAP];
#pragma unroll
            for (int t = 0; t < NTAP; ++t) {
                const int by = MODE == 0 ? y + t / 3 - 1 : 2 * y + (t >> 1), bx = MODE == 0 ? xc + t % 3 - 1 : 2 * xc + (t & 1);
                const bool ok = by >= 0 && by < HB && bx >= 0 && bx < WB;
                const int byc = by < 0 ? 0 : by >= HB ? HB - 1 : by, bxc = bx < 0 ? 0 : bx >= WB ? WB - 1 : bx;
                bv[t] = Bi[(unsigned)((byc * WB + bxc) * p.CB)];
                if (!(ok && vx && okB)) bv[t] = 0.f;
            }
#pragma unroll
            for (int t = 0; t < NTAP; ++t) acc[t] = mfma(av, bv[t], acc[t]);
        }
    }
    float *out = p.part + (size_t)chunk * p.CA * p.CB * NTAP;
#pragma unroll
    for (int t = 0; t < NTAP; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = ab * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
            if (row < p.CA && okB) out[((size_t)row * p.CB + cb) * NTAP + t] = acc[t][r];
        }
}

// out[(row * CBtotal + coloff + col) * ntaps + tap] = the partials of (row, col, tap) added in chunk order (f64), col < CBreal
struct TtWc { const float *part; float *out; int nchunks, CA, CB, ntaps, CBreal, CBtotal, coloff; };

__global__ void __launch_bounds__(256) tt_wcombine_kernel(TtWc p) {
    const int e = blockIdx.x * 256 + threadIdx.x, n = p.CA * p.CB * p.ntaps;
    if (e >= n) return;
    const int tap = e % p.ntaps, col = (e / p.ntaps) % p.CB, row = e / (p.ntaps * p.CB);
    if (col >= p.CBreal) return;
    double s = 0.0;
    for (int k = 0; k < p.nchunks; ++k) s += (double)p.part[(size_t)k * n + e];
    p.out[((size_t)row * p.CBtotal + p.coloff + col) * p.ntaps + tap] = (float)s;
}

// ---- running statistics: per channel, scene after scene, conv1's use then conv2's ---------------------------------------------------------
struct TtRun { float *rm, *rv; const double *st1, *st2; int C, S; double m, unbias; };

__global__ void __launch_bounds__(64) tt_running_kernel(TtRun p) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= p.C) return;
    float mean = p.rm[c], var = p.rv[c];
    for (int s = 0; s < p.S; ++s)
        for (int u = 0; u < 2; ++u) {
            const double *st = u ? p.st2 : p.st1;
            mean = (float)((1.0 - p.m) * (double)mean + p.m * st[s * p.C + c]);
            var = (float)((1.0 - p.m) * (double)var + p.m * (st[(size_t)p.S * p.C + s * p.C + c] * p.unbias));
        }
    p.rm[c] = mean; p.rv[c] = var;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
struct TtCtx {
    TtDims t; TtWs ws; float *base; hipStream_t s;
    float *at(long long off) const { return base + off; }
};

inline unsigned tt_blocks(long long n) { return (unsigned)((n + 255) / 256); }

void tt_pack(const TtCtx &c, const float *w, const float *b, int Cout, int Cin, int CinReal, int ntaps, int so, int sk, int base, int flip, int tapmajor) {
    TtPack p{};
    p.w = w; p.b = b; p.frag = c.at(c.ws.frag); p.bias = c.at(c.ws.bias);
    p.Cout = Cout; p.Cin = Cin; p.CinReal = CinReal; p.ntaps = ntaps; p.so = so; p.sk = sk; p.base = base; p.flip = flip; p.tapmajor = tapmajor;
    hipLaunchKernelGGL(tt_pack_kernel, dim3(128), dim3(256), 0, c.s, p);
}

inline TuConv tt_conv_args(const TtCtx &c, const float *inA, int CA, const float *inB, int CB, int Cout, int H, int W, float *out) {
    TuConvOff o; o.w = c.ws.frag; o.b = c.ws.bias;
    TuConv a = tu_conv_args(inA, CA, inB, CB, c.base, o, Cout, c.t.d.n_img, H, W);
    a.out = out;
    return a;
}

template <int MODE>
void tt_reduce(const TtCtx &c, const float *v, const float *z, const float *mean, const float *rstd, int C, int lvl, int classes) {
    TtRed r{};
    r.v = v; r.z = z; r.mean = mean; r.rstd = rstd; r.part = reinterpret_cast<double *>(c.at(c.ws.red));
    r.C = C; r.HW = (c.t.d.H >> lvl) * (c.t.d.W >> lvl); r.Pg = c.t.G * r.HW; r.nsl = tt_nsl(c.t, lvl); r.groups = c.t.S; r.classes = classes;
    const int CBk = C < 256 ? C : 256;
    hipLaunchKernelGGL(tt_reduce_kernel<MODE>, dim3((unsigned)(r.groups * r.nsl), (unsigned)(C / CBk), (unsigned)classes), dim3(256), 0, c.s, r);
}

inline TtFin tt_fin(const TtCtx &c, int mode, int C, int lvl) {
    TtFin f{};
    f.part = reinterpret_cast<const double *>(c.at(c.ws.red)); f.mode = mode; f.C = C;
    f.Pg = c.t.G * (c.t.d.H >> lvl) * (c.t.d.W >> lvl); f.nsl = tt_nsl(c.t, lvl); f.groups = c.t.S;
    return f;
}
inline void tt_fin_launch(const TtCtx &c, const TtFin &f, int ny) {
    hipLaunchKernelGGL(tt_finalize_kernel, dim3((unsigned)((f.C + 63) / 64), (unsigned)ny), dim3(64), 0, c.s, f);
}

// z = conv(inA | inB) + b, statistics, a = relu(bn(z)) (and the pool)
void tt_conv_bn_fwd(const TtCtx &c, const float *inA, int CA, const float *inB, int CB, const float *w, const float *b, int CinW,
                    const vt_resnet_bn &bn, int Cout, int lvl, long long z, long long a, long long pooled, const TtStat &st) {
    const int H = c.t.d.H >> lvl, W = c.t.d.W >> lvl, S = c.t.S;
    tt_pack(c, w, b, Cout, CA + CB, CinW, 9, CinW * 9, 9, 0, 0, 0);
    tu_launch<TU_RAW>(tt_conv_args(c, inA, CA, inB, CB, Cout, H, W, c.at(z)), c.s);
    tt_reduce<TT_STATS>(c, nullptr, c.at(z), nullptr, nullptr, Cout, lvl, 1);
    TtFin f = tt_fin(c, TT_STATS, Cout, lvl);
    f.eps = bn.eps; f.o0 = c.at(st.f); f.o1 = c.at(st.f) + (size_t)S * Cout; f.od = reinterpret_cast<double *>(c.at(st.d));
    tt_fin_launch(c, f, 1);
    TtBn p{};
    p.z = c.at(z); p.mean = f.o0; p.rstd = f.o1; p.gamma = bn.weight; p.beta = bn.bias; p.a = c.at(a);
    p.C = Cout; p.H = H; p.W = W; p.n_img = c.t.d.n_img; p.G = c.t.G;
    const long long n4 = (long long)c.t.d.n_img * H * W * (Cout / 4);
    if (pooled >= 0) { p.pooled = c.at(pooled); hipLaunchKernelGGL(tt_bn_relu_kernel<true>, dim3(tt_blocks(n4 / 4)), dim3(256), 0, c.s, p); }
    else hipLaunchKernelGGL(tt_bn_relu_kernel<false>, dim3(tt_blocks(n4)), dim3(256), 0, c.s, p);
}

void tt_running(const TtCtx &c, const vt_resnet_bn &bn, const TtStat &s1, const TtStat &s2, int C, int lvl, double momentum) {
    TtRun r{};
    // (the parameter struct is shared with the eval path, whose pointers are const: in train mode the running statistics are outputs)
    r.rm = const_cast<float *>(bn.running_mean); r.rv = const_cast<float *>(bn.running_var);
    r.st1 = reinterpret_cast<const double *>(c.at(s1.d)); r.st2 = reinterpret_cast<const double *>(c.at(s2.d));
    r.C = C; r.S = c.t.S; r.m = momentum;
    const double n = (double)c.t.G * (c.t.d.H >> lvl) * (c.t.d.W >> lvl);
    r.unbias = n / (n - 1.0);
    hipLaunchKernelGGL(tt_running_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, c.s, r);
}

template <int MODE>
void tt_wgrad(const TtCtx &c, const float *A, int CA, const float *B, int CB, int H, int W, float *out, int CBreal, int CBtotal, int coloff) {
    constexpr int NTAP = MODE == 0 ? 9 : 4;
    TtWg g{};
    g.A = A; g.B = B; g.part = c.at(c.ws.wpart); g.CA = CA; g.CB = CB; g.H = H; g.W = W;
    g.cpi = (H + TT_ROWS - 1) / TT_ROWS; g.nchunks = c.t.d.n_img * g.cpi; g.nBb = (CB + 31) / 32;
    hipLaunchKernelGGL(tt_wgrad_kernel<MODE>, dim3((unsigned)((g.nchunks + 3) / 4), (unsigned)(((CA + 31) / 32) * g.nBb)), dim3(256), 0, c.s, g);
    TtWc k{};
    k.part = g.part; k.out = out; k.nchunks = g.nchunks; k.CA = CA; k.CB = CB; k.ntaps = NTAP; k.CBreal = CBreal; k.CBtotal = CBtotal; k.coloff = coloff;
    hipLaunchKernelGGL(tt_wcombine_kernel, dim3(tt_blocks((long long)CA * CB * NTAP)), dim3(256), 0, c.s, k);
}

// the backward of one conv + bn + relu.  g (in place): the gradient of the block's output a, which becomes dz.  dA / dB: where the data
// gradients of the two sources go (null: not needed)
void tt_conv_bn_bwd(const TtCtx &c, float *g, const float *da2, const float *dpool, const float *inA, int CA, const float *inB, int CB,
                    const float *w, int CinW, const vt_resnet_bn &bn, int Cout, int lvl, long long z, long long a, const TtStat &st,
                    float *gw, float *gb, float *ggamma, float *gbeta, int accumulate, float *dA, float *dB) {
    const int H = c.t.d.H >> lvl, W = c.t.d.W >> lvl, S = c.t.S, n_img = c.t.d.n_img;
    const long long n4 = (long long)n_img * H * W * (Cout / 4);
    const float *mean = c.at(st.f), *rstd = c.at(st.f) + (size_t)S * Cout;
    TtG mg{};
    mg.g = g; mg.da2 = da2; mg.a = c.at(a); mg.dpool = dpool; mg.C = Cout; mg.H = H; mg.W = W; mg.n_img = n_img;
    hipLaunchKernelGGL(tt_make_g_kernel, dim3(tt_blocks(n4)), dim3(256), 0, c.s, mg);
    tt_reduce<TT_BNBWD>(c, g, c.at(z), mean, rstd, Cout, lvl, 1);
    TtFin f = tt_fin(c, TT_BNBWD, Cout, lvl);
    f.o0 = c.at(c.ws.m12); f.o1 = c.at(c.ws.m12) + (size_t)S * Cout; f.p0 = gbeta; f.p1 = ggamma; f.accumulate = accumulate;
    tt_fin_launch(c, f, 1);
    TtBnB b{};
    b.g = g; b.z = c.at(z); b.mean = mean; b.rstd = rstd; b.gamma = bn.weight; b.m1 = f.o0; b.m2 = f.o1; b.C = Cout; b.HW = H * W; b.n_img = n_img; b.G = c.t.G;
    hipLaunchKernelGGL(tt_bn_bwd_kernel, dim3(tt_blocks(n4)), dim3(256), 0, c.s, b);
    tt_reduce<TT_SUM>(c, g, nullptr, nullptr, nullptr, Cout, lvl, 1);
    TtFin fb = tt_fin(c, TT_SUM, Cout, lvl);
    fb.p0 = gb;
    tt_fin_launch(c, fb, 1);
    tt_wgrad<0>(c, g, Cout, inA, CA, H, W, gw, CA < CinW ? CA : CinW, CinW, 0);
    if (CB) tt_wgrad<0>(c, g, Cout, inB, CB, H, W, gw, CB, CinW, CA);
    // data gradients: the conv of dz with w[co][ci][8 - tap] as [ci][co][tap], per source
    if (dA) {
        tt_pack(c, w, nullptr, CA, Cout, Cout, 9, 9, CinW * 9, 0, 1, 0);
        tu_launch<TU_RAW>(tt_conv_args(c, g, Cout, nullptr, 0, CA, H, W, dA), c.s);
    }
    if (dB) {
        tt_pack(c, w, nullptr, CB, Cout, Cout, 9, 9, CinW * 9, CA * 9, 1, 0);
        tu_launch<TU_RAW>(tt_conv_args(c, g, Cout, nullptr, 0, CB, H, W, dB), c.s);
    }
}

inline TtDims tt_dims(int depth, int sf, int cin, int classes, int n_img, int group, int H, int W) {
    TtDims t;
    t.d = tu_dims_raw(depth, sf, cin, classes, n_img, H, W); t.G = group; t.S = group > 0 ? n_img / group : 0;
    return t;
}

bool tt_params_ok(const vt_tactile_unet_params *p) {
    for (int i = 0; i < p->depth; ++i) {
        const vt_resnet_bn &bn = p->down_bn[i];
        if (!(p->down_w[i][0] && p->down_b[i][0] && p->down_w[i][1] && p->down_b[i][1] && bn.weight && bn.bias && bn.running_mean && bn.running_var)) return false;
        if (i < p->depth - 1) {
            const vt_resnet_bn &ub = p->up_bn[i];
            if (!(p->up_tw[i] && p->up_tb[i] && p->up_w[i][0] && p->up_b[i][0] && p->up_w[i][1] && p->up_b[i][1] && ub.weight && ub.bias &&
                  ub.running_mean && ub.running_var)) return false;
        }
    }
    return p->final_w && p->final_b;
}

}  // namespace

extern "C" {

int vt_tactile_unet_train_supported(int depth, int start_filts, int in_channels, int num_classes, int n_img, int group, int H, int W) {
    return tt_dims_ok(tt_dims(depth, start_filts, in_channels, num_classes, n_img, group, H, W)) ? 1 : 0;
}

size_t vt_tactile_unet_train_workspace_bytes(int depth, int start_filts, int in_channels, int num_classes, int n_img, int group, int H, int W) {
    const TtDims t = tt_dims(depth, start_filts, in_channels, num_classes, n_img, group, H, W);
    if (!tt_dims_ok(t)) return 0;
    return (size_t)tt_workspace(t).total * sizeof(float);
}

int vt_tactile_unet_train_fwd(const float *x, int n_img, int group, int H, int W, const vt_tactile_unet_params *p, double momentum,
                              void *workspace, size_t workspace_bytes, float *out, void *stream) {
    if (!x || !p || !workspace || !out) return vt_fail(VT_ERR_INVALID, "vt_tactile_unet_train_fwd: null argument");
    TtCtx c;
    c.t = tt_dims(p->depth, p->start_filts, p->in_channels, p->num_classes, n_img, group, H, W);
    if (!tt_dims_ok(c.t)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_tactile_unet_train_fwd: shape not covered (vt_tactile_unet_train_supported)");
    if (!tt_params_ok(p)) return vt_fail(VT_ERR_INVALID, "vt_tactile_unet_train_fwd: null conv or BatchNorm tensor");
    if (momentum > 1.0) return vt_fail(VT_ERR_INVALID, "vt_tactile_unet_train_fwd: momentum above 1");
    c.ws = tt_workspace(c.t);
    if (workspace_bytes < (size_t)c.ws.total * sizeof(float)) return vt_fail(VT_ERR_WORKSPACE, "vt_tactile_unet_train_fwd: workspace too small");
    c.base = reinterpret_cast<float *>(workspace); c.s = (hipStream_t)stream;
    const TuDims &d = c.t.d;
    const TtWs &ws = c.ws;
    const int P = n_img * H * W;
    hipLaunchKernelGGL(tt_to_cl_kernel, dim3(tt_blocks(P)), dim3(256), 0, c.s, x, c.at(ws.xcl), d.cin, H * W, P);
    for (int i = 0; i < d.depth; ++i) {
        const int ch = d.sf << i;
        const bool bottom = i == d.depth - 1;
        if (i == 0) tt_conv_bn_fwd(c, c.at(ws.xcl), 8, nullptr, 0, p->down_w[0][0], p->down_b[0][0], d.cin, p->down_bn[0], ch, 0, ws.dz[0][0], ws.da[0][0], -1, ws.dstat[0][0]);
        else tt_conv_bn_fwd(c, c.at(ws.pooled[i - 1]), ch / 2, nullptr, 0, p->down_w[i][0], p->down_b[i][0], ch / 2, p->down_bn[i], ch, i, ws.dz[i][0], ws.da[i][0], -1, ws.dstat[i][0]);
        tt_conv_bn_fwd(c, c.at(ws.da[i][0]), ch, nullptr, 0, p->down_w[i][1], p->down_b[i][1], ch, p->down_bn[i], ch, i, ws.dz[i][1], ws.da[i][1],
                       bottom ? -1 : ws.pooled[i], ws.dstat[i][1]);
        if (momentum >= 0.0) tt_running(c, p->down_bn[i], ws.dstat[i][0], ws.dstat[i][1], ch, i, momentum);
    }
    const float *cur = c.at(ws.da[d.depth - 1][1]);
    for (int i = d.depth - 2; i >= 0; --i) {
        const int ch = d.sf << i, h = H >> i, w = W >> i;
        tt_pack(c, p->up_tw[i], p->up_tb[i], ch, 2 * ch, 2 * ch, 4, 4, ch * 4, 0, 0, 0);
        tu_launch<TU_UP>(tt_conv_args(c, cur, 2 * ch, nullptr, 0, ch, h / 2, w / 2, c.at(ws.up[i])), c.s);
        tt_conv_bn_fwd(c, c.at(ws.up[i]), ch, c.at(ws.da[i][1]), ch, p->up_w[i][0], p->up_b[i][0], 2 * ch, p->up_bn[i], ch, i, ws.uz[i][0], ws.ua[i][0], -1, ws.ustat[i][0]);
        tt_conv_bn_fwd(c, c.at(ws.ua[i][0]), ch, nullptr, 0, p->up_w[i][1], p->up_b[i][1], ch, p->up_bn[i], ch, i, ws.uz[i][1], ws.ua[i][1], -1, ws.ustat[i][1]);
        if (momentum >= 0.0) tt_running(c, p->up_bn[i], ws.ustat[i][0], ws.ustat[i][1], ch, i, momentum);
        cur = c.at(ws.ua[i][1]);
    }
    TtFinal f{};
    f.a = cur; f.w = p->final_w; f.b = p->final_b; f.out = out; f.C = d.sf; f.classes = d.classes; f.HW = H * W; f.P = P;
    hipLaunchKernelGGL(tt_final_fwd_kernel, dim3(tt_blocks(P)), dim3(256), 0, c.s, f);
    return vt_check(hipGetLastError(), "vt_tactile_unet_train_fwd");
}

int vt_tactile_unet_bwd(const float *dout, const float *out, int n_img, int group, int H, int W, const vt_tactile_unet_params *p,
                        void *workspace, size_t workspace_bytes, const vt_tactile_unet_grads *gr, void *stream) {
    if (!dout || !out || !p || !workspace || !gr) return vt_fail(VT_ERR_INVALID, "vt_tactile_unet_bwd: null argument");
    TtCtx c;
    c.t = tt_dims(p->depth, p->start_filts, p->in_channels, p->num_classes, n_img, group, H, W);
    if (!tt_dims_ok(c.t)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_tactile_unet_bwd: shape not covered (vt_tactile_unet_train_supported)");
    if (!tt_params_ok(p)) return vt_fail(VT_ERR_INVALID, "vt_tactile_unet_bwd: null conv or BatchNorm tensor");
    c.ws = tt_workspace(c.t);
    if (workspace_bytes < (size_t)c.ws.total * sizeof(float)) return vt_fail(VT_ERR_WORKSPACE, "vt_tactile_unet_bwd: workspace too small");
    c.base = reinterpret_cast<float *>(workspace); c.s = (hipStream_t)stream;
    const TuDims &d = c.t.d;
    const TtWs &ws = c.ws;
    for (int i = 0; i < d.depth; ++i) {
        bool ok = gr->down_w[i][0] && gr->down_b[i][0] && gr->down_w[i][1] && gr->down_b[i][1] && gr->down_bn_w[i] && gr->down_bn_b[i];
        if (i < d.depth - 1) ok = ok && gr->up_tw[i] && gr->up_tb[i] && gr->up_w[i][0] && gr->up_b[i][0] && gr->up_w[i][1] && gr->up_b[i][1] && gr->up_bn_w[i] && gr->up_bn_b[i];
        if (!ok) return vt_fail(VT_ERR_INVALID, "vt_tactile_unet_bwd: null gradient tensor");
    }
    if (!gr->final_w || !gr->final_b) return vt_fail(VT_ERR_INVALID, "vt_tactile_unet_bwd: null gradient tensor");
    const int P = n_img * H * W, top = d.depth - 1;
    // conv_final + sigmoid
    const float *last = d.depth > 1 ? c.at(ws.ua[0][1]) : c.at(ws.da[0][1]);
    TtFinal f{};
    f.a = last; f.w = p->final_w; f.b = p->final_b; f.dout = dout; f.y = out; f.dt = c.at(ws.dt); f.da = c.at(ws.gx[0]);
    f.C = d.sf; f.classes = d.classes; f.HW = H * W; f.P = P;
    hipLaunchKernelGGL(tt_final_bwd_kernel, dim3(tt_blocks(P)), dim3(256), 0, c.s, f);
    tt_reduce<TT_FINAL>(c, c.at(ws.dt), last, nullptr, nullptr, d.sf, 0, d.classes);
    TtFin ff = tt_fin(c, TT_FINAL, d.sf, 0);
    ff.p0 = gr->final_w; ff.p1 = gr->final_b;
    tt_fin_launch(c, ff, d.classes);
    // the up path, from level 0 down: the gradient of block i's output is in gx[i]
    for (int i = 0; i < top; ++i) {
        const int ch = d.sf << i, h = H >> i, w = W >> i;
        const float *below = i + 1 == top ? c.at(ws.da[top][1]) : c.at(ws.ua[i + 1][1]);          // the up-conv's input
        tt_conv_bn_bwd(c, c.at(ws.gx[i]), nullptr, nullptr, c.at(ws.ua[i][0]), ch, nullptr, 0, p->up_w[i][1], ch, p->up_bn[i], ch, i, ws.uz[i][1], ws.ua[i][1],
                       ws.ustat[i][1], gr->up_w[i][1], gr->up_b[i][1], gr->up_bn_w[i], gr->up_bn_b[i], 0, c.at(ws.gy[i]), nullptr);
        // (gx[i] is free once conv2's weight and data gradients are out: it takes the up-conv result's gradient; gz[i] the skip's)
        tt_conv_bn_bwd(c, c.at(ws.gy[i]), nullptr, nullptr, c.at(ws.up[i]), ch, c.at(ws.da[i][1]), ch, p->up_w[i][0], 2 * ch, p->up_bn[i], ch, i, ws.uz[i][0],
                       ws.ua[i][0], ws.ustat[i][0], gr->up_w[i][0], gr->up_b[i][0], gr->up_bn_w[i], gr->up_bn_b[i], 1, c.at(ws.gx[i]), c.at(ws.gz[i]));
        // the transposed conv: bias = sum of its output's gradient; weight [2 ch][ch][2][2]; data gradient into the level below
        tt_reduce<TT_SUM>(c, c.at(ws.gx[i]), nullptr, nullptr, nullptr, ch, i, 1);
        TtFin fb = tt_fin(c, TT_SUM, ch, i);
        fb.p0 = gr->up_tb[i];
        tt_fin_launch(c, fb, 1);
        tt_wgrad<1>(c, below, 2 * ch, c.at(ws.gx[i]), ch, h / 2, w / 2, gr->up_tw[i], ch, ch, 0);
        tt_pack(c, p->up_tw[i], nullptr, 2 * ch, ch, ch, 4, ch * 4, 4, 0, 0, 1);
        tu_launch<TU_S2D>(tt_conv_args(c, c.at(ws.gx[i]), ch, nullptr, 0, 2 * ch, h / 2, w / 2, c.at(ws.gx[i + 1])), c.s);
    }
    // the down path, from the bottom up
    for (int i = top; i >= 0; --i) {
        const int ch = d.sf << i;
        const bool bottom = i == top;
        float *g2 = bottom ? c.at(ws.gx[i]) : c.at(ws.gz[i]);
        tt_conv_bn_bwd(c, g2, nullptr, bottom ? nullptr : c.at(ws.gx[i + 1]), c.at(ws.da[i][0]), ch, nullptr, 0, p->down_w[i][1], ch, p->down_bn[i], ch, i,
                       ws.dz[i][1], ws.da[i][1], ws.dstat[i][1], gr->down_w[i][1], gr->down_b[i][1], gr->down_bn_w[i], gr->down_bn_b[i], 0, c.at(ws.gy[i]), nullptr);
        if (i == 0)
            tt_conv_bn_bwd(c, c.at(ws.gy[0]), nullptr, nullptr, c.at(ws.xcl), 8, nullptr, 0, p->down_w[0][0], d.cin, p->down_bn[0], ch, 0, ws.dz[0][0], ws.da[0][0],
                           ws.dstat[0][0], gr->down_w[0][0], gr->down_b[0][0], gr->down_bn_w[0], gr->down_bn_b[0], 1, nullptr, nullptr);
        else
            tt_conv_bn_bwd(c, c.at(ws.gy[i]), nullptr, nullptr, c.at(ws.pooled[i - 1]), ch / 2, nullptr, 0, p->down_w[i][0], ch / 2, p->down_bn[i], ch, i, ws.dz[i][0],
                           ws.da[i][0], ws.dstat[i][0], gr->down_w[i][0], gr->down_b[i][0], gr->down_bn_w[i], gr->down_bn_b[i], 1, c.at(ws.gx[i]), nullptr);
    }
    return vt_check(hipGetLastError(), "vt_tactile_unet_bwd");
}

}  // extern "C"
