// resnet2d_train.hip -- the tactile feature encoder (reference ``ResNet`` with BasicBlocks, src/layers.py:54-207) in TRAIN mode: the forward
// with batch statistics and the backward for every parameter, on hand-written kernels.  vt_resnet_train_fwd, vt_resnet_bwd.
//
// The input is x [F * S][3][H][W], IMAGE-major: image f of scene b is row f * S + b, so the images of scene b (n % S == b) are one
// statistics group (the reference calls the net once per scene on its five images: every BatchNorm sees one scene's images alone).
//
// Forward.  The raw conv weights are packed into MFMA fragment order at every call (no blob).  Every conv writes its raw output z:
//   stem     7x7 stride 2 on the NCHW input (the eval path's K order: 21 (channel, ky) rows of 4 k-steps), 32 pixels per wave
//   conv     resnet2d_conv.h's implicit-GEMM template with the RAW epilogue: 3x3 stride 1, 3x3 stride 2 with the 1x1 stride-2 projection
//            riding in the same launch
//   stats    per (scene, channel) sum and sum of squares of z in f64: slices of RT_SLICE pixels of ONE scene, a slice's four pixel
//            lanes combined in lane order (rt_reduce_kernel), the slices one after the other by one thread per (scene, channel)
//            (rt_finalize_kernel) -> mean, biased variance, 1 / sqrt(var + eps)
//   act      gamma (z - mean) rstd + beta fused with what follows: ReLU and the 3x3/2 max-pool after the stem (which also keeps each
//            window's first maximum, one byte per channel), ReLU after bn1, the residual (the block's input, or the projected and
//            normalised skip) and ReLU after bn2
//   tail     global average pool, linear, fc: one workgroup per image, f64 accumulators (the pooled features and linear's output kept)
//   running  per BatchNorm and channel, scene after scene: running = (1 - m) running + m batch (unbiased variance)
//
// Backward (from dout [F * S][classes]; no gradient for the images), per block in reverse:
//   g = (the sum of the two incoming gradients) * (y > 0); sums of g and g xhat per (scene, channel) by the same slice scheme -> dbeta,
//   dgamma (the scenes added in scene order) and dz = gamma rstd (g - mean(g) - xhat mean(g xhat)); a projected skip's BatchNorm
//   shares the pass.  The max-pool's gradient is a gather over the <= 4 windows that cover a stem pixel.
//   weight gradient (rt_wgrad_kernel): dW[co][ci][tap] = sum over pixels dz[px][co] in[px * stride + tap][ci] on the matrix core,
//   A = 32 output channels, B = 32 input channels, k = pixels.  A workgroup owns 64 x 64 channels, all taps and one (scene, block of
//   output rows); it stages 32 output pixels of dz and the input patch under them in LDS with 16-byte loads and walks the scene's
//   images in order.  The per-(scene, row block) partials are added in f64 in that order (rt_wcombine_kernel).
//   data gradient: 3x3 stride 1 is the conv template with flipped, transposed weights; 3x3 stride 2 runs per parity class of the
//   input pixel (1, 2, 2 or 4 taps), the class of even pixels also taking the 1x1 projection's gradient (rt_dgrad_s2_kernel).
//
// Every sum has a fixed order that is a function of the layer and of one scene's images alone; no atomics.  The results are
// bit-reproducible, a scene's outputs and statistics do not depend on the other scenes of the call, and scenes whose dout is zero add
// exact zeros.
#include "resnet2d_conv.h"

namespace {

constexpr int RT_SLICE = 1024;      // pixels of one scene per partial of a per-channel sum
constexpr int RT_STEM_ROWS = 4;     // stem rows per partial of the stem's weight gradient
constexpr int RT_STEM_COLS = 160;   // the stem's 147 (channel, ky, kx) columns padded to 5 blocks of 32

struct RtDims { RnDims d; int S, G; };

inline RtDims rt_dims_of(const int32_t *blocks, int classes, int n_img, int scenes, int H, int W) {
    RtDims t;
    t.d = rn_dims_of(blocks, classes, n_img, H, W); t.S = scenes; t.G = scenes > 0 ? n_img / scenes : 0;
    return t;
}
inline bool rt_dims_ok(const RtDims &t) {
    if (!rn_dims_ok(t.d)) return false;
    if (t.S < 1 || t.d.n_img % t.S) return false;
    if ((long long)t.d.n_img * rn_half(t.d.H) * rn_half(t.d.W) * 64 >= (1ll << 31)) return false;      // the stem's z
    int h, w;
    rn_stage_hw(t.d, 3, h, w);
    return (long long)t.G * h * w >= 2;
}

// ---- workspace (floats; every offset a multiple of 4) ---------------------------------------------------------------------------------
struct RtStat { long long f, d; };          // floats [2][S][C]: mean, rstd; doubles [2][S][C]: mean, biased variance
struct RtBlock {
    long long w1, w2, wp, z1, a1, z2, y, zk;
    RtStat s1, s2, sk;
    int Cin, Cout, proj, hi, wi, ho, wo;
};
struct RtWs {
    long long wstem, zs, idx, pooled;
    RtStat sstem;
    long long feat, hid, dhid, dfeat, g[4], gstem, m12, sums, red, wpart, wT, wTp, total;
    int nblocks;
    RtBlock blk[4 * VT_RESNET_MAX_BLOCKS];
};
inline long long rt_up4(long long n) { return (n + 3) / 4 * 4; }
inline int rt_nsl(const RtDims &t, int hw) { return (int)(((long long)t.G * hw + RT_SLICE - 1) / RT_SLICE); }
// the weight gradient's tile of 32 output pixels is 2^txl wide, and a partial covers `rows` output rows: by the layer alone
inline int rt_txl(int Wo) { return Wo >= 24 ? 5 : Wo >= 12 ? 4 : 3; }
inline int rt_wg_rows(int Cout) { return 4 * (Cout / 64); }
inline long long rt_wg_chunks(const RtDims &t, int Cout, int Ho) { return (long long)t.S * ((Ho + rt_wg_rows(Cout) - 1) / rt_wg_rows(Cout)); }

inline void rt_workspace(const RtDims &t, RtWs &w) {
    const RnDims &d = t.d;
    long long off = 0;
    auto take = [&](long long n) { const long long o = off; off += rt_up4(n); return o; };
    auto stat = [&](RtStat &s, int C) { s.f = take(2ll * t.S * C); s.d = take(4ll * t.S * C); };
    const int Hs = rn_half(d.H), Ws = rn_half(d.W), Hp = rn_half(Hs), Wp = rn_half(Ws);
    const long long N = d.n_img;
    w.wstem = take(RN_STEM_FRAG);
    w.zs = take(N * Hs * Ws * 64);
    w.idx = take(N * Hp * Wp * 16);
    w.pooled = take(N * Hp * Wp * 64);
    stat(w.sstem, 64);
    long long red = 3ll * t.S * rt_nsl(t, Hs * Ws) * 64;                           // doubles
    long long wpart = (long long)t.S * ((Hs + RT_STEM_ROWS - 1) / RT_STEM_ROWS) * 64 * RT_STEM_COLS, most = 0;
    int cin = 64, h = Hp, wd = Wp, nb = 0;
    for (int s = 0; s < 4; ++s) {
        const int cout = rn_width(s);
        for (int b = 0; b < d.blocks[s]; ++b) {
            RtBlock &k = w.blk[nb++];
            k.Cin = cin; k.Cout = cout; k.proj = (b == 0 && s > 0) ? 1 : 0;
            k.hi = h; k.wi = wd; k.ho = k.proj ? rn_half(h) : h; k.wo = k.proj ? rn_half(wd) : wd;
            const long long n = N * k.ho * k.wo * cout;
            k.w1 = take((long long)cout * cin * 9);
            k.w2 = take((long long)cout * cout * 9);
            k.wp = k.proj ? take((long long)cout * cin) : 0;
            k.z1 = take(n); k.a1 = take(n); k.z2 = take(n); k.y = take(n);
            k.zk = k.proj ? take(n) : 0;
            stat(k.s1, cout); stat(k.s2, cout);
            if (k.proj) stat(k.sk, cout); else k.sk = RtStat{0, 0};
            if (n > most) most = n;
            const long long r = 3ll * t.S * rt_nsl(t, k.ho * k.wo) * cout;
            if (r > red) red = r;
            const long long p = rt_wg_chunks(t, cout, k.ho) * cout * (long long)cout * 9;      // (conv2: the larger of the block's three)
            if (p > wpart) wpart = p;
            cin = cout; h = k.ho; wd = k.wo;
        }
    }
    w.nblocks = nb;
    w.feat = take(N * RN_FEAT); w.hid = take(N * RN_LIN); w.dhid = take(N * RN_LIN); w.dfeat = take(N * RN_FEAT);
    for (int i = 0; i < 4; ++i) w.g[i] = take(most);
    w.gstem = take(N * Hs * Ws * 64);
    w.m12 = take(4ll * t.S * RN_FEAT);
    w.sums = take(8ll * t.S * RN_FEAT);
    w.red = take(2 * red);
    w.wpart = take(wpart);
    w.wT = take((long long)RN_FEAT * RN_FEAT * 9);
    w.wTp = take((long long)RN_FEAT * (RN_FEAT / 2));
    w.total = off;
}

// ---- packing: raw weights -> fragments [M / 32][K / 8][ntaps][64 lanes][4] ---------------------------------------------------------------
// lane l, slot j = w[o * so + k * sk + tap'], o = cb * 32 + l % 32, k = chunk * 8 + 4 (l / 32) + j, tap' = tap or, flipped, ntaps - 1 - tap.
// stem: the eval path's [2][21 rows = (c, ky)][64][4], slot j = w[cb * 32 + l % 32][c][ky][kx = 2 j + l / 32] (kx 7: zero).
struct RtPack { const float *w; float *frag; int M, K, ntaps, so, sk, flip, stem; };

__global__ void __launch_bounds__(256) rt_pack_kernel(RtPack p) {
    const long long nf = p.stem ? RN_STEM_FRAG : (long long)p.M * p.K * p.ntaps;
    const int n_chunks = p.K / 8;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nf; e += (long long)gridDim.x * 256) {
        const int j = (int)(e & 3), l = (int)((e >> 2) & 63);
        long long q = e >> 8;
        float v;
        if (p.stem) {
            const int r = (int)(q % RN_STEM_ROWS), cb = (int)(q / RN_STEM_ROWS);
            const int kx = 2 * j + (l >> 5), c = r / 7, ky = r % 7, co = cb * 32 + (l & 31);
            v = kx < 7 ? p.w[((co * 3 + c) * 7 + ky) * 7 + kx] : 0.f;
        } else {
            const int t = (int)(q % p.ntaps); q /= p.ntaps;
            const int chunk = (int)(q % n_chunks), cb = (int)(q / n_chunks);
            const int k = chunk * 8 + 4 * (l >> 5) + j, o = cb * 32 + (l & 31);
            v = p.w[(size_t)o * p.so + (size_t)k * p.sk + (p.flip ? p.ntaps - 1 - t : t)];
        }
        p.frag[e] = v;
    }
}

// ---- stem: 7x7 stride 2, raw output ------------------------------------------------------------------------------------------------------
struct RtStem { const float *x, *wfrag; float *z; int H, W, Hs, Ws, P; };      // z [n_img][Hs][Ws][64], P = n_img * Hs * Ws

__global__ void __launch_bounds__(256) rt_stem_kernel(RtStem p) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5, lp = lane & 31;
    const int tile = blockIdx.x * 4 + wave;
    if (tile * 32 >= p.P) return;                                      // (wave-uniform; the kernel has no barrier)
    const int pix = tile * 32 + lp;
    const bool valid = pix < p.P;
    const int pc = valid ? pix : p.P - 1;
    const int sx = pc % p.Ws, sy = (pc / p.Ws) % p.Hs, img = pc / (p.Ws * p.Hs);
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
            const bool rowok = valid && iy >= 0 && iy < p.H;
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
    if (!valid) return;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<f32x4 *>(p.z + (size_t)pix * 64 + cb * 32 + 8 * q + 4 * h) = rn_quad(acc[cb], q);
}

// ---- per-(scene, channel) sums ------------------------------------------------------------------------------------------------------------
// pixel j of scene s (0 <= j < G * HW) is pixel j % HW of image (j / HW) * S + s.  part [S][nsl][3][C] doubles.
// RT_STATS: sum z, sum z^2.  RT_BWD: g = (gA + gB) * (y > 0); sum g, sum g xhat, and for a projected skip's BatchNorm sum g xhat_k.
enum { RT_STATS = 0, RT_BWD = 1 };
struct RtRed { const float *z, *mean, *rstd, *zk, *meank, *rstdk, *gA, *gB, *y; double *part; int C, HW, Pg, nsl, S; };

__device__ __forceinline__ float rt_g(const float *gA, const float *gB, const float *y, size_t i) {
    float g = gA[i];
    if (gB) g += gB[i];
    if (y) g = y[i] > 0.f ? g : 0.f;
    return g;
}

template <int MODE>
__global__ void __launch_bounds__(256) rt_reduce_kernel(RtRed p) {
    __shared__ double sh[3][256];
    const int cl = threadIdx.x & 63, pl = threadIdx.x >> 6, c = blockIdx.y * 64 + cl;
    const int s = blockIdx.x / p.nsl, sl = blockIdx.x % p.nsl;
    const int j0 = sl * RT_SLICE, j1 = j0 + RT_SLICE < p.Pg ? j0 + RT_SLICE : p.Pg;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    float mu = 0.f, rs = 0.f, muk = 0.f, rsk = 0.f;
    if (MODE == RT_BWD) {
        mu = p.mean[s * p.C + c]; rs = p.rstd[s * p.C + c];
        if (p.zk) { muk = p.meank[s * p.C + c]; rsk = p.rstdk[s * p.C + c]; }
    }
    for (int j = j0 + pl; j < j1; j += 4) {
        const int img = (j / p.HW) * p.S + s;
        const size_t i = ((size_t)img * p.HW + j % p.HW) * p.C + c;
        if (MODE == RT_STATS) { const double v = p.z[i]; a0 += v; a1 += v * v; }
        else {
            const float g = rt_g(p.gA, p.gB, p.y, i);
            a0 += g; a1 += (double)g * (double)((p.z[i] - mu) * rs);
            if (p.zk) a2 += (double)g * (double)((p.zk[i] - muk) * rsk);
        }
    }
    sh[0][threadIdx.x] = a0; sh[1][threadIdx.x] = a1; sh[2][threadIdx.x] = a2;
    __syncthreads();
    if (pl == 0) {
        for (int q = 1; q < 4; ++q) { a0 += sh[0][q * 64 + cl]; a1 += sh[1][q * 64 + cl]; a2 += sh[2][q * 64 + cl]; }
        double *o = p.part + ((size_t)(s * p.nsl + sl) * 3) * p.C + c;
        o[0] = a0; o[p.C] = a1; o[2 * p.C] = a2;
    }
}

// one thread per (scene, channel): the slices in order
struct RtFin {
    const double *part; int mode, C, Pg, nsl, S; double eps;
    float *o0, *o1, *o2; double *od;      // STATS: mean, rstd [S][C], od [2][S][C] (mean, biased variance); BWD: mean(g), mean(g xhat), mean(g xhat_k)
    double *sums;                         // BWD: [S][3][C] the sums themselves
};

__global__ void __launch_bounds__(256) rt_finalize_kernel(RtFin p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.S * p.C) return;
    const int s = i / p.C, c = i % p.C;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const double *src = p.part + ((size_t)s * p.nsl * 3) * p.C + c;
    for (int k = 0; k < p.nsl; ++k) { a0 += src[(size_t)k * 3 * p.C]; a1 += src[(size_t)k * 3 * p.C + p.C]; a2 += src[(size_t)k * 3 * p.C + 2 * p.C]; }
    if (p.mode == RT_STATS) {
        const double mean = a0 / p.Pg;
        double var = a1 / p.Pg - mean * mean;
        var = var > 0.0 ? var : 0.0;
        p.o0[i] = (float)mean; p.o1[i] = (float)(1.0 / sqrt(var + p.eps));
        p.od[i] = mean; p.od[(size_t)p.S * p.C + i] = var;
    } else {
        p.o0[i] = (float)(a0 / p.Pg); p.o1[i] = (float)(a1 / p.Pg); p.o2[i] = (float)(a2 / p.Pg);
        double *o = p.sums + ((size_t)s * 3) * p.C + c;
        o[0] = a0; o[p.C] = a1; o[2 * p.C] = a2;
    }
}

// dbeta, dgamma (and the projected skip's): the scenes in order
struct RtGb { const double *sums; float *gbeta, *ggamma, *gbetak, *ggammak; int C, S; };

__global__ void __launch_bounds__(256) rt_gamma_beta_kernel(RtGb p) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.C) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int s = 0; s < p.S; ++s) {
        const double *o = p.sums + ((size_t)s * 3) * p.C + c;
        a0 += o[0]; a1 += o[p.C]; a2 += o[2 * p.C];
    }
    p.gbeta[c] = (float)a0; p.ggamma[c] = (float)a1;
    if (p.ggammak) { p.gbetak[c] = (float)a0; p.ggammak[c] = (float)a2; }
}

struct RtRun { float *rm, *rv; const double *st; int C, S; double m, unbias; };

__global__ void __launch_bounds__(256) rt_running_kernel(RtRun p) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.C) return;
    float mean = p.rm[c], var = p.rv[c];
    for (int s = 0; s < p.S; ++s) {
        mean = (float)((1.0 - p.m) * (double)mean + p.m * p.st[s * p.C + c]);
        var = (float)((1.0 - p.m) * (double)var + p.m * (p.st[(size_t)p.S * p.C + s * p.C + c] * p.unbias));
    }
    p.rm[c] = mean; p.rv[c] = var;
}

// ---- BatchNorm fused with what follows -----------------------------------------------------------------------------------------------------
struct RtBnP { const float *z, *mean, *rstd, *gamma, *beta; };

__device__ __forceinline__ f32x4 rt_bn4(const RtBnP &b, size_t o, int st, int c4) {
    const f32x4 z = *reinterpret_cast<const f32x4 *>(b.z + o), mu = *reinterpret_cast<const f32x4 *>(b.mean + st);
    const f32x4 rs = *reinterpret_cast<const f32x4 *>(b.rstd + st), ga = *reinterpret_cast<const f32x4 *>(b.gamma + c4);
    const f32x4 be = *reinterpret_cast<const f32x4 *>(b.beta + c4);
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = fmaf((z[i] - mu[i]) * rs[i], ga[i], be[i]);
    return r;
}

// out = relu(bn(z) + (bn_k(zk) | res | nothing))
struct RtAct { RtBnP b, k; const float *res; float *out; int C, HW, S; long long n4; };

__global__ void __launch_bounds__(256) rt_act_kernel(RtAct p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n4) return;
    const int q4 = p.C >> 2, cq = (int)(i % q4);
    const long long pix = i / q4;
    const int s = (int)((pix / p.HW) % p.S);
    const size_t o = (size_t)pix * p.C + 4 * cq;
    f32x4 v = rt_bn4(p.b, o, s * p.C + 4 * cq, 4 * cq);
    if (p.k.z) v += rt_bn4(p.k, o, s * p.C + 4 * cq, 4 * cq);
    else if (p.res) v += *reinterpret_cast<const f32x4 *>(p.res + o);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    *reinterpret_cast<f32x4 *>(p.out + o) = v;
}

// the stem: pooled = max over the 3x3 stride-2 window (pad 1) of relu(bn(z)); idx: per channel the window position (dy * 3 + dx) of the
// FIRST maximum in row-major order, one byte each
struct RtPool { RtBnP b; float *pooled; unsigned *idx; int Hs, Ws, Hp, Wp, S; long long n; };      // n = n_img * Hp * Wp * 16

__global__ void __launch_bounds__(256) rt_pool_kernel(RtPool p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int cq = (int)(i & 15);
    const long long pp = i >> 4;
    const int px = (int)(pp % p.Wp), py = (int)((pp / p.Wp) % p.Hp), img = (int)(pp / ((long long)p.Wp * p.Hp)), s = img % p.S;
    f32x4 m = {0.f, 0.f, 0.f, 0.f};
    unsigned which = 0;
    bool first = true;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int sy = 2 * py - 1 + dy, sx = 2 * px - 1 + dx;
            if (sy < 0 || sy >= p.Hs || sx < 0 || sx >= p.Ws) continue;
            const f32x4 a = rt_bn4(p.b, ((size_t)(img * p.Hs + sy) * p.Ws + sx) * 64 + 4 * cq, s * 64 + 4 * cq, 4 * cq);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = fmaxf(a[j], 0.f);
                if (first || v > m[j]) { m[j] = v; which = (which & ~(255u << (8 * j))) | ((unsigned)(dy * 3 + dx) << (8 * j)); }
            }
            first = false;
        }
    *reinterpret_cast<f32x4 *>(p.pooled + (size_t)pp * 64 + 4 * cq) = m;
    p.idx[i] = which;
}

// the max-pool's backward as a gather, and the stem's ReLU: g[stem pixel] = (sum over the <= 4 windows that cover it and have their first
// maximum here of gA + gB) * (bn(z) > 0)
struct RtPoolB { RtBnP b; const float *gA, *gB; const unsigned *idx; float *g; int Hs, Ws, Hp, Wp, S; long long n; };   // n = n_img * Hs * Ws * 16

__global__ void __launch_bounds__(256) rt_pool_bwd_kernel(RtPoolB p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int cq = (int)(i & 15);
    const long long sp = i >> 4;
    const int sx = (int)(sp % p.Ws), sy = (int)((sp / p.Ws) % p.Hs), img = (int)(sp / ((long long)p.Ws * p.Hs)), s = img % p.S;
    const f32x4 a = rt_bn4(p.b, (size_t)sp * 64 + 4 * cq, s * 64 + 4 * cq, 4 * cq);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int py = sy >> 1; py <= (sy + 1) >> 1; ++py)
        for (int px = sx >> 1; px <= (sx + 1) >> 1; ++px) {
            if (py >= p.Hp || px >= p.Wp) continue;
            const unsigned me = (unsigned)((sy - (2 * py - 1)) * 3 + (sx - (2 * px - 1)));
            const size_t pp = (size_t)(img * p.Hp + py) * p.Wp + px;
            const unsigned w = p.idx[pp * 16 + cq];
            f32x4 g = *reinterpret_cast<const f32x4 *>(p.gA + pp * 64 + 4 * cq);
            if (p.gB) g += *reinterpret_cast<const f32x4 *>(p.gB + pp * 64 + 4 * cq);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (((w >> (8 * j)) & 255u) == me) acc[j] += g[j];
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = a[j] > 0.f ? acc[j] : 0.f;
    *reinterpret_cast<f32x4 *>(p.g + (size_t)sp * 64 + 4 * cq) = acc;
}

// dz = gamma rstd (g - mean(g) - xhat mean(g xhat)), g = (gA + gB) * (y > 0); gout: g itself (the identity skip's gradient); dzk: the
// same for a projected skip's BatchNorm.  dz, gout and dzk may be gA (every thread reads its own elements before it writes them).
struct RtBnB { const float *gA, *gB, *y; RtBnP b, k; const float *m1, *m2, *m2k; float *dz, *gout, *dzk; int C, HW, S; long long n4; };

__global__ void __launch_bounds__(256) rt_bn_bwd_kernel(RtBnB p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n4) return;
    const int q4 = p.C >> 2, cq = (int)(i % q4);
    const long long pix = i / q4;
    const int st = (int)((pix / p.HW) % p.S) * p.C + 4 * cq;
    const size_t o = (size_t)pix * p.C + 4 * cq;
    f32x4 g = *reinterpret_cast<const f32x4 *>(p.gA + o);
    if (p.gB) g += *reinterpret_cast<const f32x4 *>(p.gB + o);
    if (p.y) {
        const f32x4 y = *reinterpret_cast<const f32x4 *>(p.y + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = y[j] > 0.f ? g[j] : 0.f;
    }
    const f32x4 m1 = *reinterpret_cast<const f32x4 *>(p.m1 + st);
    auto one = [&](const RtBnP &b, const float *m2p) {
        const f32x4 z = *reinterpret_cast<const f32x4 *>(b.z + o), mu = *reinterpret_cast<const f32x4 *>(b.mean + st);
        const f32x4 rs = *reinterpret_cast<const f32x4 *>(b.rstd + st), ga = *reinterpret_cast<const f32x4 *>(b.gamma + 4 * cq);
        const f32x4 m2 = *reinterpret_cast<const f32x4 *>(m2p + st);
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (ga[j] * rs[j]) * ((g[j] - m1[j]) - ((z[j] - mu[j]) * rs[j]) * m2[j]);
        return v;
    };
    const f32x4 dz = one(p.b, p.m2);
    f32x4 dzk = dz;
    if (p.dzk) dzk = one(p.k, p.m2k);
    *reinterpret_cast<f32x4 *>(p.dz + o) = dz;
    if (p.gout) *reinterpret_cast<f32x4 *>(p.gout + o) = g;
    if (p.dzk) *reinterpret_cast<f32x4 *>(p.dzk + o) = dzk;
}

// ---- tail ---------------------------------------------------------------------------------------------------------------------------------
struct RtTail { const float *in, *lw, *lb, *fw, *fb; float *out, *feat, *hid; int HW, classes; };

__global__ void __launch_bounds__(256) rt_tail_kernel(RtTail p) {
    __shared__ double pooled[RN_FEAT];
    __shared__ double hid[RN_LIN];
    const int img = blockIdx.x;
    for (int c = threadIdx.x; c < RN_FEAT; c += 256) {
        double sum = 0.0;
        const float *q = p.in + (size_t)img * p.HW * RN_FEAT + c;
        for (int px = 0; px < p.HW; ++px) sum += (double)q[(size_t)px * RN_FEAT];
        const float f = (float)(sum / (double)p.HW);
        pooled[c] = (double)f;
        p.feat[(size_t)img * RN_FEAT + c] = f;
    }
    __syncthreads();
    if (threadIdx.x < RN_LIN) {
        double a = (double)p.lb[threadIdx.x];
        const float *w = p.lw + threadIdx.x * RN_FEAT;
        for (int k = 0; k < RN_FEAT; ++k) a = fma((double)w[k], pooled[k], a);
        hid[threadIdx.x] = (double)(float)a;
        p.hid[(size_t)img * RN_LIN + threadIdx.x] = (float)a;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < p.classes; o += 256) {
        double a = (double)p.fb[o];
        const float *w = p.fw + (size_t)o * RN_LIN;
        for (int k = 0; k < RN_LIN; ++k) a = fma((double)w[k], hid[k], a);
        p.out[(size_t)img * p.classes + o] = (float)a;
    }
}

// dhid = dout fc.weight, dfeat = dhid linear.weight: one workgroup per image
struct RtTailB { const float *dout, *lw, *fw; float *dhid, *dfeat; int classes; };

__global__ void __launch_bounds__(256) rt_tail_bwd_kernel(RtTailB p) {
    __shared__ double dh[RN_LIN];
    const int img = blockIdx.x;
    if (threadIdx.x < RN_LIN) {
        double a = 0.0;
        for (int o = 0; o < p.classes; ++o) a = fma((double)p.dout[(size_t)img * p.classes + o], (double)p.fw[(size_t)o * RN_LIN + threadIdx.x], a);
        dh[threadIdx.x] = (double)(float)a;
        p.dhid[(size_t)img * RN_LIN + threadIdx.x] = (float)a;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < RN_FEAT; c += 256) {
        double a = 0.0;
        for (int j = 0; j < RN_LIN; ++j) a = fma(dh[j], (double)p.lw[j * RN_FEAT + c], a);
        p.dfeat[(size_t)img * RN_FEAT + c] = (float)a;
    }
}

// the gradients of fc and linear: one thread per element, the images in order
struct RtTailW { const float *dout, *hid, *dhid, *feat; float *gfw, *gfb, *glw, *glb; int N, classes; };

__global__ void __launch_bounds__(256) rt_tail_wgrad_kernel(RtTailW p) {
    const int n0 = p.classes * RN_LIN, n1 = n0 + p.classes, n2 = n1 + RN_LIN * RN_FEAT, n3 = n2 + RN_LIN;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n3) return;
    double a = 0.0;
    if (e < n0) {
        const int o = e / RN_LIN, k = e % RN_LIN;
        for (int n = 0; n < p.N; ++n) a = fma((double)p.dout[(size_t)n * p.classes + o], (double)p.hid[(size_t)n * RN_LIN + k], a);
        p.gfw[e] = (float)a;
    } else if (e < n1) {
        for (int n = 0; n < p.N; ++n) a += (double)p.dout[(size_t)n * p.classes + (e - n0)];
        p.gfb[e - n0] = (float)a;
    } else if (e < n2) {
        const int j = (e - n1) / RN_FEAT, k = (e - n1) % RN_FEAT;
        for (int n = 0; n < p.N; ++n) a = fma((double)p.dhid[(size_t)n * RN_LIN + j], (double)p.feat[(size_t)n * RN_FEAT + k], a);
        p.glw[e - n1] = (float)a;
    } else {
        for (int n = 0; n < p.N; ++n) a += (double)p.dhid[(size_t)n * RN_LIN + (e - n2)];
        p.glb[e - n2] = (float)a;
    }
}

// the average pool's backward: g[img][px][c] = dfeat[img][c] / HW
__global__ void __launch_bounds__(256) rt_avg_bwd_kernel(const float *dfeat, float *g, int HW, long long n4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int cq = (int)(i % (RN_FEAT / 4));
    const long long img = i / (RN_FEAT / 4) / HW;
    f32x4 v = *reinterpret_cast<const f32x4 *>(dfeat + (size_t)img * RN_FEAT + 4 * cq);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] / (float)HW;
    *reinterpret_cast<f32x4 *>(g + (size_t)i * 4) = v;
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------------------
// part [chunk = scene * nrb + row block][Cout][Cin][KSZ * KSZ].  A tile is 32 output pixels, 2^txl wide and 32 >> txl high; As holds their
// dz [32][64], Bs the input patch under them [rows][cols][64], both written with 16-byte loads and stores and read one float per lane
// (32 consecutive channels per half wave: no bank conflict).
struct RtWg { const float *dz, *in; float *part; int Cout, Cin, Hi, Wi, Ho, Wo, S, G, rows, nrb, txl, nci; };

template <int STRIDE, int KSZ>
__global__ void __launch_bounds__(256) rt_wgrad_kernel(RtWg p) {
    constexpr int NT = KSZ * KSZ, PAD = KSZ / 2;
    constexpr int NB = KSZ == 1 ? 105 : STRIDE == 2 ? 195 : 102;      // the largest patch over the three tile shapes
    __shared__ __attribute__((aligned(16))) float As[32 * 64];
    __shared__ __attribute__((aligned(16))) float Bs[NB * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kh = lane >> 5, m = lane & 31;
    const int TX = 1 << p.txl, TY = 32 >> p.txl;
    const int BR = (TY - 1) * STRIDE + KSZ, BC = (TX - 1) * STRIDE + KSZ;
    const int s = blockIdx.x / p.nrb, rb = blockIdx.x % p.nrb, co0 = (blockIdx.y / p.nci) * 64, ci0 = (blockIdx.y % p.nci) * 64;
    const int cob = wave >> 1, cib = wave & 1;
    const int y0 = rb * p.rows, y1 = y0 + p.rows < p.Ho ? y0 + p.rows : p.Ho;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    f32x4 *As4 = reinterpret_cast<f32x4 *>(As), *Bs4 = reinterpret_cast<f32x4 *>(Bs);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int f = 0; f < p.G; ++f) {
        const int img = f * p.S + s;
        const float *dzi = p.dz + (size_t)img * p.Ho * p.Wo * p.Cout + co0, *ini = p.in + (size_t)img * p.Hi * p.Wi * p.Cin + ci0;
        for (int ty0 = y0; ty0 < y1; ty0 += TY)
            for (int tx0 = 0; tx0 < p.Wo; tx0 += TX) {
                for (int e = threadIdx.x; e < 512; e += 256) {
                    const int px = e >> 4, q = e & 15, oy = ty0 + (px >> p.txl), ox = tx0 + (px & (TX - 1));
                    const bool ok = oy < y1 && ox < p.Wo;
                    As4[e] = ok ? *reinterpret_cast<const f32x4 *>(dzi + (size_t)(oy * p.Wo + ox) * p.Cout + 4 * q) : zero;
                }
                for (int e = threadIdx.x; e < BR * BC * 16; e += 256) {
                    const int bp = e >> 4, q = e & 15, iy = ty0 * STRIDE - PAD + bp / BC, ix = tx0 * STRIDE - PAD + bp % BC;
                    const bool ok = iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
                    Bs4[e] = ok ? *reinterpret_cast<const f32x4 *>(ini + (size_t)(iy * p.Wi + ix) * p.Cin + 4 * q) : zero;
                }
                __syncthreads();
#pragma unroll 2
                for (int j = 0; j < 16; ++j) {
                    const int px = 2 * j + kh, pty = px >> p.txl, ptx = px & (TX - 1);
                    const float a = As[px * 64 + cob * 32 + m];
                    const float *brow = Bs + ((pty * STRIDE) * BC + ptx * STRIDE) * 64 + cib * 32 + m;
                    float b[NT];
#pragma unroll
                    for (int ky = 0; ky < KSZ; ++ky)
#pragma unroll
                        for (int kx = 0; kx < KSZ; ++kx) b[ky * KSZ + kx] = brow[(ky * BC + kx) * 64];
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = mfma(a, b[t], acc[t]);
                }
                __syncthreads();
            }
    }
    float *out = p.part + (size_t)blockIdx.x * p.Cout * p.Cin * NT;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = co0 + cob * 32 + 8 * (r >> 2) + 4 * kh + (r & 3), col = ci0 + cib * 32 + m;
            out[((size_t)row * p.Cin + col) * NT + t] = acc[t][r];
        }
}

// out[e] = the partials of element e added in chunk order (f64); a row of the partials is `pitch` long, of the result `width`
struct RtWc { const float *part; float *out; int nchunks, rows, width, pitch; };

__global__ void __launch_bounds__(256) rt_wcombine_kernel(RtWc p) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.rows * p.width) return;
    const int row = e / p.width, col = e % p.width;
    double sum = 0.0;
    for (int k = 0; k < p.nchunks; ++k) sum += (double)p.part[((size_t)k * p.rows + row) * p.pitch + col];
    p.out[e] = (float)sum;
}

// the stem's weight gradient: D[co][(c, ky, kx)] = sum over stem pixels dz[px][co] x[c][2 y - 3 + ky][2 x - 3 + kx]; a wave owns 64 x 32
// of it and one (scene, block of RT_STEM_ROWS stem rows).  part [chunk][64][RT_STEM_COLS]
struct RtWgS { const float *dz, *x; float *part; int H, W, Hs, Ws, S, G, nrb; };

__global__ void __launch_bounds__(64) rt_wgrad_stem_kernel(RtWgS p) {
    const int lane = threadIdx.x, kh = lane >> 5, m = lane & 31;
    const int s = blockIdx.x / p.nrb, rb = blockIdx.x % p.nrb;
    const int col = blockIdx.y * 32 + m;
    const bool colok = col < 147;
    const int cc = colok ? col : 0, c = cc / 49, ky = (cc % 49) / 7, kx = cc % 7;
    const int y0 = rb * RT_STEM_ROWS, y1 = y0 + RT_STEM_ROWS < p.Hs ? y0 + RT_STEM_ROWS : p.Hs;
    f32x16 acc[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
    for (int f = 0; f < p.G; ++f) {
        const int img = f * p.S + s;
        const float *plane = p.x + (size_t)(img * 3 + c) * p.H * p.W;
        for (int sy = y0; sy < y1; ++sy) {
            const int iy = 2 * sy - 3 + ky;
            const bool rowok = colok && iy >= 0 && iy < p.H;
            const int iyc = iy < 0 ? 0 : iy >= p.H ? p.H - 1 : iy;
            const float *dzr = p.dz + ((size_t)(img * p.Hs + sy) * p.Ws) * 64 + m, *xr = plane + (size_t)iyc * p.W;
#pragma unroll 4
            for (int sx0 = 0; sx0 < p.Ws; sx0 += 2) {
                const int sx = sx0 + kh;
                const bool vx = sx < p.Ws;
                const int sxc = vx ? sx : p.Ws - 1, ix = 2 * sxc - 3 + kx;
                float a0 = dzr[(size_t)sxc * 64], a1 = dzr[(size_t)sxc * 64 + 32];
                float b = xr[ix < 0 ? 0 : ix >= p.W ? p.W - 1 : ix];
                if (!vx) { a0 = 0.f; a1 = 0.f; }
                if (!(rowok && vx && ix >= 0 && ix < p.W)) b = 0.f;
                acc[0] = mfma(a0, b, acc[0]);
                acc[1] = mfma(a1, b, acc[1]);
            }
        }
    }
    float *out = p.part + (size_t)blockIdx.x * 64 * RT_STEM_COLS;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(size_t)(cb * 32 + 8 * (r >> 2) + 4 * kh + (r & 3)) * RT_STEM_COLS + col] = acc[cb][r];
}

// ---- data gradient of a 3x3 stride-2 conv (and of the 1x1 stride-2 projection beside it) ---------------------------------------------------
// dx[iy][ix][ci] = sum over the taps (ky, kx) with iy + 1 - ky and ix + 1 - kx even of dz[(iy + 1 - ky) / 2][(ix + 1 - kx) / 2][co] w[co][ci][ky][kx]:
// per parity class (iy % 2, ix % 2) of the input pixel 1, 2, 2 or 4 taps; blockIdx.y is the class, a tile 32 pixels of it.  The even
// class also takes dzk[iy / 2][ix / 2][co] wk[co][ci].  The resnet2d_conv.h template's K split and epilogue: wT [Cin / 32][Cout / 8][9][64][4]
// (not flipped), wTp [Cin / 32][Cout / 8][64][4].
struct RtDg2 { const float *dz, *dzk, *wT, *wTp; float *dx; int Cin, Cout, Hi, Wi, Ho, Wo, N; };

template <int KS>
__global__ void __launch_bounds__(KS * 64) rt_dgrad_s2_kernel(RtDg2 p) {
    __shared__ __attribute__((aligned(16))) float red[KS * 16 * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5, lp = lane & 31;
    const int py = blockIdx.y >> 1, px = blockIdx.y & 1;
    const int Hc = (p.Hi - py + 1) >> 1, Wc = (p.Wi - px + 1) >> 1, Pc = p.N * Hc * Wc;
    const int n_cbp = p.Cin >> 6, cbp = blockIdx.x % n_cbp, tile = blockIdx.x / n_cbp;
    if (tile * 32 >= Pc) return;                                       // (the whole workgroup)
    auto where = [&](int pix, int &img, int &iy, int &ix) {
        img = pix / (Wc * Hc); iy = 2 * ((pix / Wc) % Hc) + py; ix = 2 * (pix % Wc) + px;
    };
    const int pix = tile * 32 + lp;
    const bool valid = pix < Pc;
    int img, iy, ix;
    where(valid ? pix : Pc - 1, img, iy, ix);
    const int n_chunks = p.Cout >> 3, cpw = n_chunks / KS;
    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    const f32x4 *wf0 = reinterpret_cast<const f32x4 *>(p.wT) + (size_t)(2 * cbp) * n_chunks * 9 * 64 + lane;
    const f32x4 *wf1 = wf0 + (size_t)n_chunks * 9 * 64;
    const f32x4 *wp = reinterpret_cast<const f32x4 *>(p.wTp) + lane;
    const unsigned ibase = (unsigned)(img * p.Ho * p.Wo * p.Cout) + 4 * h;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int ck = 0; ck < cpw; ++ck) {
        const int chunk = wave * cpw + ck;
        for (int ky = py ? 0 : 1; ky < 3; ky += 2) {
            const int oy = (iy + 1 - ky) >> 1;
            const bool rowok = valid && oy < p.Ho;
            const int oyc = oy < p.Ho ? oy : p.Ho - 1;
            for (int kx = px ? 0 : 1; kx < 3; kx += 2) {
                const int ox = (ix + 1 - kx) >> 1, oxc = ox < p.Wo ? ox : p.Wo - 1;
                f32x4 b = *reinterpret_cast<const f32x4 *>(p.dz + ibase + chunk * 8 + (unsigned)((oyc * p.Wo + oxc) * p.Cout));
                const f32x4 a0 = wf0[(size_t)(chunk * 9 + ky * 3 + kx) * 64], a1 = wf1[(size_t)(chunk * 9 + ky * 3 + kx) * 64];
                if (!(rowok && ox < p.Wo)) b = zero;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[0] = mfma(a0[j], b[j], acc[0]);
                    acc[1] = mfma(a1[j], b[j], acc[1]);
                }
            }
        }
        if (blockIdx.y == 0 && p.dzk) {
            f32x4 b = *reinterpret_cast<const f32x4 *>(p.dzk + ibase + chunk * 8 + (unsigned)(((iy >> 1) * p.Wo + (ix >> 1)) * p.Cout));
            const f32x4 q0 = wp[(size_t)((2 * cbp) * n_chunks + chunk) * 64], q1 = wp[(size_t)((2 * cbp + 1) * n_chunks + chunk) * 64];
            if (!valid) b = zero;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0] = mfma(q0[j], b[j], acc[0]);
                acc[1] = mfma(q1[j], b[j], acc[1]);
            }
        }
    }
    f32x4 *red4 = reinterpret_cast<f32x4 *>(red);
    const int eq = threadIdx.x >> 6, el = threadIdx.x & 63, epix = tile * 32 + (el & 31);
    int eimg = 0, eiy = 0, eix = 0;
    if (epix < Pc) where(epix, eimg, eiy, eix);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if (a) __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) red4[(wave * 4 + q) * 64 + lane] = rn_quad(acc[a], q);
        __syncthreads();
        if (threadIdx.x < 256 && epix < Pc) {
            f32x4 sum = red4[(0 * 4 + eq) * 64 + el];
#pragma unroll
            for (int w = 1; w < KS; ++w) sum += red4[(w * 4 + eq) * 64 + el];
            const int co = (2 * cbp + a) * 32 + 8 * eq + 4 * (el >> 5);
            *reinterpret_cast<f32x4 *>(p.dx + (size_t)((eimg * p.Hi + eiy) * p.Wi + eix) * p.Cin + co) = sum;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
struct RtCtx {
    RtDims t; RtWs *ws; float *base; hipStream_t s;
    float *at(long long off) const { return base + off; }
};

inline unsigned rt_blocks(long long n) { return (unsigned)((n + 255) / 256); }

void rt_pack(const RtCtx &c, const float *w, float *frag, int M, int K, int ntaps, int so, int sk, int flip, int stem) {
    RtPack p{};
    p.w = w; p.frag = frag; p.M = M; p.K = K; p.ntaps = ntaps; p.so = so; p.sk = sk; p.flip = flip; p.stem = stem;
    const long long nf = stem ? RN_STEM_FRAG : (long long)M * K * ntaps;
    const unsigned nb = rt_blocks(nf);
    hipLaunchKernelGGL(rt_pack_kernel, dim3(nb < 1024 ? nb : 1024), dim3(256), 0, c.s, p);
}

inline RtBnP rt_bnp(const RtCtx &c, long long z, const RtStat &st, const vt_resnet_bn &bn, int C) {
    RtBnP b;
    b.z = c.at(z); b.mean = c.at(st.f); b.rstd = c.at(st.f) + (size_t)c.t.S * C; b.gamma = bn.weight; b.beta = bn.bias;
    return b;
}

// the statistics of z [n_img][hw][C] into st, and the BatchNorm's running statistics
void rt_stats(const RtCtx &c, long long z, const RtStat &st, const vt_resnet_bn &bn, int C, int hw, double momentum) {
    RtRed r{};
    r.z = c.at(z); r.part = reinterpret_cast<double *>(c.at(c.ws->red)); r.C = C; r.HW = hw; r.Pg = c.t.G * hw; r.nsl = rt_nsl(c.t, hw); r.S = c.t.S;
    hipLaunchKernelGGL(rt_reduce_kernel<RT_STATS>, dim3((unsigned)(r.S * r.nsl), (unsigned)(C / 64)), dim3(256), 0, c.s, r);
    RtFin f{};
    f.part = r.part; f.mode = RT_STATS; f.C = C; f.Pg = r.Pg; f.nsl = r.nsl; f.S = r.S; f.eps = bn.eps;
    f.o0 = c.at(st.f); f.o1 = c.at(st.f) + (size_t)r.S * C; f.od = reinterpret_cast<double *>(c.at(st.d));
    hipLaunchKernelGGL(rt_finalize_kernel, dim3(rt_blocks((long long)r.S * C)), dim3(256), 0, c.s, f);
    if (momentum >= 0.0) {
        RtRun u{};
        // (the parameter struct is shared with the eval path, whose pointers are const: in train mode the running statistics are outputs)
        u.rm = const_cast<float *>(bn.running_mean); u.rv = const_cast<float *>(bn.running_var);
        u.st = f.od; u.C = C; u.S = r.S; u.m = momentum; u.unbias = (double)r.Pg / ((double)r.Pg - 1.0);
        hipLaunchKernelGGL(rt_running_kernel, dim3(rt_blocks(C)), dim3(256), 0, c.s, u);
    }
}

// BatchNorm backward of one use (and of the projected skip's beside it): the sums, dgamma / dbeta, then dz
void rt_bn_bwd(const RtCtx &c, const float *gA, const float *gB, const float *y, const RtBnP &b, const RtBnP *k, int C, int hw,
               float *ggamma, float *gbeta, float *ggammak, float *gbetak, float *dz, float *gout, float *dzk) {
    const int S = c.t.S;
    RtRed r{};
    r.z = b.z; r.mean = b.mean; r.rstd = b.rstd; r.gA = gA; r.gB = gB; r.y = y;
    if (k) { r.zk = k->z; r.meank = k->mean; r.rstdk = k->rstd; }
    r.part = reinterpret_cast<double *>(c.at(c.ws->red)); r.C = C; r.HW = hw; r.Pg = c.t.G * hw; r.nsl = rt_nsl(c.t, hw); r.S = S;
    hipLaunchKernelGGL(rt_reduce_kernel<RT_BWD>, dim3((unsigned)(S * r.nsl), (unsigned)(C / 64)), dim3(256), 0, c.s, r);
    RtFin f{};
    f.part = r.part; f.mode = RT_BWD; f.C = C; f.Pg = r.Pg; f.nsl = r.nsl; f.S = S;
    f.o0 = c.at(c.ws->m12); f.o1 = f.o0 + (size_t)S * C; f.o2 = f.o1 + (size_t)S * C; f.sums = reinterpret_cast<double *>(c.at(c.ws->sums));
    hipLaunchKernelGGL(rt_finalize_kernel, dim3(rt_blocks((long long)S * C)), dim3(256), 0, c.s, f);
    RtGb g{};
    g.sums = f.sums; g.gbeta = gbeta; g.ggamma = ggamma; g.gbetak = k ? gbetak : nullptr; g.ggammak = k ? ggammak : nullptr; g.C = C; g.S = S;
    hipLaunchKernelGGL(rt_gamma_beta_kernel, dim3(rt_blocks(C)), dim3(256), 0, c.s, g);
    RtBnB a{};
    a.gA = gA; a.gB = gB; a.y = y; a.b = b; if (k) a.k = *k;
    a.m1 = f.o0; a.m2 = f.o1; a.m2k = f.o2; a.dz = dz; a.gout = gout; a.dzk = k ? dzk : nullptr; a.C = C; a.HW = hw; a.S = S;
    a.n4 = (long long)c.t.d.n_img * hw * (C / 4);
    hipLaunchKernelGGL(rt_bn_bwd_kernel, dim3(rt_blocks(a.n4)), dim3(256), 0, c.s, a);
}

// gw [Cout][Cin][ksz][ksz] from dz [n_img][Ho][Wo][Cout] and the conv's input [n_img][Hi][Wi][Cin]
void rt_wgrad(const RtCtx &c, const float *dz, const float *in, int Cout, int Cin, int Hi, int Wi, int Ho, int Wo, int stride, int ksz, float *gw) {
    RtWg g{};
    g.dz = dz; g.in = in; g.part = c.at(c.ws->wpart); g.Cout = Cout; g.Cin = Cin; g.Hi = Hi; g.Wi = Wi; g.Ho = Ho; g.Wo = Wo;
    g.S = c.t.S; g.G = c.t.G; g.rows = rt_wg_rows(Cout); g.nrb = (Ho + g.rows - 1) / g.rows; g.txl = rt_txl(Wo); g.nci = Cin / 64;
    const dim3 grid((unsigned)(g.S * g.nrb), (unsigned)((Cout / 64) * g.nci));
    if (ksz == 1) hipLaunchKernelGGL((rt_wgrad_kernel<2, 1>), grid, dim3(256), 0, c.s, g);
    else if (stride == 2) hipLaunchKernelGGL((rt_wgrad_kernel<2, 3>), grid, dim3(256), 0, c.s, g);
    else hipLaunchKernelGGL((rt_wgrad_kernel<1, 3>), grid, dim3(256), 0, c.s, g);
    RtWc k{};
    k.part = g.part; k.out = gw; k.nchunks = g.S * g.nrb; k.rows = Cout; k.width = Cin * ksz * ksz; k.pitch = k.width;
    hipLaunchKernelGGL(rt_wcombine_kernel, dim3(rt_blocks((long long)k.rows * k.width)), dim3(256), 0, c.s, k);
}

inline RnConv rt_conv_args(const float *in, const float *wfrag, float *out, int Cin, int Cout, int Hi, int Wi, int Ho, int Wo, int n_img) {
    RnConv a{};
    a.in = in; a.wfrag = wfrag; a.out = out; a.Cin = Cin; a.Cout = Cout; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.P = n_img * Ho * Wo;
    return a;
}

bool rt_params_ok(const vt_resnet_params *p, const RtWs &ws) {
    if (!p->conv1_w || !rn_bn_ok(p->bn1) || !p->linear_w || !p->linear_b || !p->fc_w || !p->fc_b) return false;
    int nb = 0;
    for (int st = 0; st < 4; ++st)
        for (int b = 0; b < p->blocks_num[st]; ++b) {
            const vt_resnet_block &k = p->block[st][b];
            if (!k.conv1_w || !k.conv2_w || !rn_bn_ok(k.bn1) || !rn_bn_ok(k.bn2)) return false;
            if (ws.blk[nb].proj && (!k.down_w || !rn_bn_ok(k.down_bn))) return false;
            ++nb;
        }
    return true;
}

// forward and backward share the argument checks and the layout.  RtWs is large (one entry per block): it lives on the heap
struct RtPlan {
    RtCtx c; RtWs *ws;
    RtPlan() : ws(new RtWs()) {}
    ~RtPlan() { delete ws; }
    RtPlan(const RtPlan &) = delete;
    RtPlan &operator=(const RtPlan &) = delete;
};

int rt_plan(RtPlan &pl, const char *who, int n_img, int scenes, int H, int W, const vt_resnet_params *p, void *workspace, size_t workspace_bytes,
            void *stream) {
    RtCtx &c = pl.c;
    c.t = rt_dims_of(p->blocks_num, p->num_classes, n_img, scenes, H, W);
    if (!rt_dims_ok(c.t)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_resnet_train: shape not covered (vt_resnet_train_supported)");
    rt_workspace(c.t, *pl.ws);
    c.ws = pl.ws;
    if (!rt_params_ok(p, *pl.ws)) return vt_fail(VT_ERR_INVALID, "vt_resnet_train: null conv, BatchNorm, linear or fc tensor");
    if (workspace_bytes < (size_t)pl.ws->total * sizeof(float)) return vt_fail(VT_ERR_WORKSPACE, "vt_resnet_train: workspace too small");
    for (int i = 0; i < pl.ws->nblocks; ++i) {
        const RtBlock &k = pl.ws->blk[i];
        if (!rn_split_ok(k.Cin, rn_waves(k.Cin)) || !rn_split_ok(k.Cout, rn_waves(k.Cout)))
            return vt_fail(VT_ERR_UNSUPPORTED, "vt_resnet_train: a layer's K split would drop input channels");
    }
    c.base = reinterpret_cast<float *>(workspace); c.s = (hipStream_t)stream;
    (void)who;
    return 0;
}

}  // namespace

extern "C" {

int vt_resnet_train_supported(const int32_t *blocks_num, int num_classes, int n_img, int scenes, int H, int W) {
    if (!blocks_num) return 0;
    return rt_dims_ok(rt_dims_of(blocks_num, num_classes, n_img, scenes, H, W)) ? 1 : 0;
}

size_t vt_resnet_train_workspace_bytes(const int32_t *blocks_num, int num_classes, int n_img, int scenes, int H, int W) {
    if (!blocks_num) return 0;
    const RtDims t = rt_dims_of(blocks_num, num_classes, n_img, scenes, H, W);
    if (!rt_dims_ok(t)) return 0;
    RtPlan pl;
    rt_workspace(t, *pl.ws);
    return (size_t)pl.ws->total * sizeof(float);
}

int vt_resnet_train_fwd(const float *x, int n_img, int scenes, int H, int W, const vt_resnet_params *p, double momentum, void *workspace,
                        size_t workspace_bytes, float *out, void *stream) {
    if (!x || !p || !workspace || !out) return vt_fail(VT_ERR_INVALID, "vt_resnet_train_fwd: null argument");
    if (momentum > 1.0) return vt_fail(VT_ERR_INVALID, "vt_resnet_train_fwd: momentum above 1");
    RtPlan pl;
    const int rc = rt_plan(pl, "vt_resnet_train_fwd", n_img, scenes, H, W, p, workspace, workspace_bytes, stream);
    if (rc != 0) return rc;
    const RtCtx &c = pl.c;
    const RtWs &ws = *pl.ws;
    const int Hs = rn_half(H), Ws = rn_half(W), Hp = rn_half(Hs), Wp = rn_half(Ws), S = c.t.S;
    rt_pack(c, p->conv1_w, c.at(ws.wstem), 64, 3, 49, 0, 0, 0, 1);
    {
        RtStem k{};
        k.x = x; k.wfrag = c.at(ws.wstem); k.z = c.at(ws.zs); k.H = H; k.W = W; k.Hs = Hs; k.Ws = Ws; k.P = n_img * Hs * Ws;
        hipLaunchKernelGGL(rt_stem_kernel, dim3((unsigned)((k.P + 127) / 128)), dim3(256), 0, c.s, k);
        rt_stats(c, ws.zs, ws.sstem, p->bn1, 64, Hs * Ws, momentum);
        RtPool q{};
        q.b = rt_bnp(c, ws.zs, ws.sstem, p->bn1, 64); q.pooled = c.at(ws.pooled); q.idx = reinterpret_cast<unsigned *>(c.at(ws.idx));
        q.Hs = Hs; q.Ws = Ws; q.Hp = Hp; q.Wp = Wp; q.S = S; q.n = (long long)n_img * Hp * Wp * 16;
        hipLaunchKernelGGL(rt_pool_kernel, dim3(rt_blocks(q.n)), dim3(256), 0, c.s, q);
    }
    const float *cur = c.at(ws.pooled);
    int nb = 0;
    for (int st = 0; st < 4; ++st)
        for (int b = 0; b < c.t.d.blocks[st]; ++b, ++nb) {
            const RtBlock &k = ws.blk[nb];
            const vt_resnet_block &w = p->block[st][b];
            const int hw = k.ho * k.wo;
            const long long n4 = (long long)n_img * hw * (k.Cout / 4);
            rt_pack(c, w.conv1_w, c.at(k.w1), k.Cout, k.Cin, 9, k.Cin * 9, 9, 0, 0);
            rt_pack(c, w.conv2_w, c.at(k.w2), k.Cout, k.Cout, 9, k.Cout * 9, 9, 0, 0);
            if (k.proj) rt_pack(c, w.down_w, c.at(k.wp), k.Cout, k.Cin, 1, k.Cin, 1, 0, 0);
            RnConv a = rt_conv_args(cur, c.at(k.w1), c.at(k.z1), k.Cin, k.Cout, k.hi, k.wi, k.ho, k.wo, n_img);
            if (k.proj) { a.wproj = c.at(k.wp); a.skip = c.at(k.zk); }
            rn_launch_conv<true>(a, k.proj ? 2 : 1, c.s);
            rt_stats(c, k.z1, k.s1, w.bn1, k.Cout, hw, momentum);
            RtAct f{};
            f.b = rt_bnp(c, k.z1, k.s1, w.bn1, k.Cout); f.out = c.at(k.a1); f.C = k.Cout; f.HW = hw; f.S = S; f.n4 = n4;
            hipLaunchKernelGGL(rt_act_kernel, dim3(rt_blocks(n4)), dim3(256), 0, c.s, f);
            rn_launch_conv<true>(rt_conv_args(c.at(k.a1), c.at(k.w2), c.at(k.z2), k.Cout, k.Cout, k.ho, k.wo, k.ho, k.wo, n_img), 1, c.s);
            rt_stats(c, k.z2, k.s2, w.bn2, k.Cout, hw, momentum);
            RtAct e{};
            e.b = rt_bnp(c, k.z2, k.s2, w.bn2, k.Cout); e.out = c.at(k.y); e.C = k.Cout; e.HW = hw; e.S = S; e.n4 = n4;
            if (k.proj) {
                rt_stats(c, k.zk, k.sk, w.down_bn, k.Cout, hw, momentum);
                e.k = rt_bnp(c, k.zk, k.sk, w.down_bn, k.Cout);
            } else e.res = cur;
            hipLaunchKernelGGL(rt_act_kernel, dim3(rt_blocks(n4)), dim3(256), 0, c.s, e);
            cur = c.at(k.y);
        }
    const RtBlock &last = ws.blk[ws.nblocks - 1];
    RtTail t{};
    t.in = cur; t.lw = p->linear_w; t.lb = p->linear_b; t.fw = p->fc_w; t.fb = p->fc_b; t.out = out; t.feat = c.at(ws.feat); t.hid = c.at(ws.hid);
    t.HW = last.ho * last.wo; t.classes = c.t.d.classes;
    hipLaunchKernelGGL(rt_tail_kernel, dim3((unsigned)n_img), dim3(256), 0, c.s, t);
    return vt_check(hipGetLastError(), "vt_resnet_train_fwd");
}

int vt_resnet_bwd(const float *dout, const float *x, int n_img, int scenes, int H, int W, const vt_resnet_params *p, void *workspace,
                  size_t workspace_bytes, const vt_resnet_grads *gr, void *stream) {
    if (!dout || !x || !p || !workspace || !gr) return vt_fail(VT_ERR_INVALID, "vt_resnet_bwd: null argument");
    RtPlan pl;
    const int rc = rt_plan(pl, "vt_resnet_bwd", n_img, scenes, H, W, p, workspace, workspace_bytes, stream);
    if (rc != 0) return rc;
    const RtCtx &c = pl.c;
    const RtWs &ws = *pl.ws;
    bool ok = gr->conv1_w && gr->bn1_w && gr->bn1_b && gr->linear_w && gr->linear_b && gr->fc_w && gr->fc_b;
    {
        int nb = 0;
        for (int st = 0; st < 4 && ok; ++st)
            for (int b = 0; b < c.t.d.blocks[st]; ++b, ++nb) {
                const vt_resnet_block_grads &g = gr->block[st][b];
                ok = ok && g.conv1_w && g.bn1_w && g.bn1_b && g.conv2_w && g.bn2_w && g.bn2_b;
                if (ws.blk[nb].proj) ok = ok && g.down_w && g.down_bn_w && g.down_bn_b;
            }
    }
    if (!ok) return vt_fail(VT_ERR_INVALID, "vt_resnet_bwd: null gradient tensor");
    const int Hs = rn_half(H), Ws = rn_half(W), Hp = rn_half(Hs), Wp = rn_half(Ws), S = c.t.S, classes = c.t.d.classes;
    // fc, linear, the average pool
    {
        RtTailB t{};
        t.dout = dout; t.lw = p->linear_w; t.fw = p->fc_w; t.dhid = c.at(ws.dhid); t.dfeat = c.at(ws.dfeat); t.classes = classes;
        hipLaunchKernelGGL(rt_tail_bwd_kernel, dim3((unsigned)n_img), dim3(256), 0, c.s, t);
        RtTailW w{};
        w.dout = dout; w.hid = c.at(ws.hid); w.dhid = c.at(ws.dhid); w.feat = c.at(ws.feat);
        w.gfw = gr->fc_w; w.gfb = gr->fc_b; w.glw = gr->linear_w; w.glb = gr->linear_b; w.N = n_img; w.classes = classes;
        hipLaunchKernelGGL(rt_tail_wgrad_kernel, dim3(rt_blocks((long long)classes * RN_LIN + classes + RN_LIN * RN_FEAT + RN_LIN)), dim3(256), 0, c.s, w);
    }
    // the gradient of a block's output is A (+ B when hasB); T1 and T2 are free
    float *A = c.at(ws.g[0]), *B = c.at(ws.g[1]), *T1 = c.at(ws.g[2]), *T2 = c.at(ws.g[3]);
    bool hasB = false;
    {
        const RtBlock &last = ws.blk[ws.nblocks - 1];
        const long long n4 = (long long)n_img * last.ho * last.wo * (RN_FEAT / 4);
        hipLaunchKernelGGL(rt_avg_bwd_kernel, dim3(rt_blocks(n4)), dim3(256), 0, c.s, c.at(ws.dfeat), A, last.ho * last.wo, n4);
    }
    int nb = ws.nblocks - 1;
    for (int st = 3; st >= 0; --st)
        for (int b = c.t.d.blocks[st] - 1; b >= 0; --b, --nb) {
            const RtBlock &k = ws.blk[nb];
            const vt_resnet_block &w = p->block[st][b];
            const vt_resnet_block_grads &g = gr->block[st][b];
            const int hw = k.ho * k.wo, C = k.Cout;
            const float *xin = nb == 0 ? c.at(ws.pooled) : c.at(ws.blk[nb - 1].y);
            // bn2 (and the projected skip's BatchNorm): dz2 -> T1; A becomes the identity skip's gradient, or the projection's dz
            const RtBnP b2 = rt_bnp(c, k.z2, k.s2, w.bn2, C);
            RtBnP bk{};
            if (k.proj) bk = rt_bnp(c, k.zk, k.sk, w.down_bn, C);
            rt_bn_bwd(c, A, hasB ? B : nullptr, c.at(k.y), b2, k.proj ? &bk : nullptr, C, hw, g.bn2_w, g.bn2_b, g.down_bn_w, g.down_bn_b,
                      T1, k.proj ? nullptr : A, A);
            rt_wgrad(c, T1, c.at(k.a1), C, C, k.ho, k.wo, k.ho, k.wo, 1, 3, g.conv2_w);
            rt_pack(c, w.conv2_w, c.at(ws.wT), C, C, 9, 9, C * 9, 1, 0);
            rn_launch_conv<true>(rt_conv_args(T1, c.at(ws.wT), T2, C, C, k.ho, k.wo, k.ho, k.wo, n_img), 1, c.s);
            // bn1: dz1 in place in T2
            rt_bn_bwd(c, T2, nullptr, c.at(k.a1), rt_bnp(c, k.z1, k.s1, w.bn1, C), nullptr, C, hw, g.bn1_w, g.bn1_b, nullptr, nullptr, T2, nullptr, nullptr);
            rt_wgrad(c, T2, xin, C, k.Cin, k.hi, k.wi, k.ho, k.wo, k.proj ? 2 : 1, 3, g.conv1_w);
            if (k.proj) {
                rt_wgrad(c, A, xin, C, k.Cin, k.hi, k.wi, k.ho, k.wo, 2, 1, g.down_w);
                rt_pack(c, w.conv1_w, c.at(ws.wT), k.Cin, C, 9, 9, k.Cin * 9, 0, 0);
                rt_pack(c, w.down_w, c.at(ws.wTp), k.Cin, C, 1, 1, k.Cin, 0, 0);
                RtDg2 d{};
                d.dz = T2; d.dzk = A; d.wT = c.at(ws.wT); d.wTp = c.at(ws.wTp); d.dx = T1;
                d.Cin = k.Cin; d.Cout = C; d.Hi = k.hi; d.Wi = k.wi; d.Ho = k.ho; d.Wo = k.wo; d.N = n_img;
                const int tiles = (n_img * ((k.hi + 1) / 2) * ((k.wi + 1) / 2) + 31) / 32;       // (the even class is the largest)
                hipLaunchKernelGGL((rt_dgrad_s2_kernel<8>), dim3((unsigned)(tiles * (k.Cin / 64)), 4), dim3(512), 0, c.s, d);
                float *t = A; A = T1; T1 = t;
                hasB = false;
            } else {
                rt_pack(c, w.conv1_w, c.at(ws.wT), C, C, 9, 9, C * 9, 1, 0);
                rn_launch_conv<true>(rt_conv_args(T2, c.at(ws.wT), T1, C, C, k.ho, k.wo, k.ho, k.wo, n_img), 1, c.s);
                float *t = B; B = A; A = T1; T1 = t;
                hasB = true;
            }
        }
    // the max-pool, the stem's ReLU and BatchNorm, the stem's weights
    float *gs = c.at(ws.gstem);
    const RtBnP bs = rt_bnp(c, ws.zs, ws.sstem, p->bn1, 64);
    RtPoolB q{};
    q.b = bs; q.gA = A; q.gB = hasB ? B : nullptr; q.idx = reinterpret_cast<const unsigned *>(c.at(ws.idx)); q.g = gs;
    q.Hs = Hs; q.Ws = Ws; q.Hp = Hp; q.Wp = Wp; q.S = S; q.n = (long long)n_img * Hs * Ws * 16;
    hipLaunchKernelGGL(rt_pool_bwd_kernel, dim3(rt_blocks(q.n)), dim3(256), 0, c.s, q);
    rt_bn_bwd(c, gs, nullptr, nullptr, bs, nullptr, 64, Hs * Ws, gr->bn1_w, gr->bn1_b, nullptr, nullptr, gs, nullptr, nullptr);
    RtWgS sw{};
    sw.dz = gs; sw.x = x; sw.part = c.at(ws.wpart); sw.H = H; sw.W = W; sw.Hs = Hs; sw.Ws = Ws; sw.S = S; sw.G = c.t.G;
    sw.nrb = (Hs + RT_STEM_ROWS - 1) / RT_STEM_ROWS;
    hipLaunchKernelGGL(rt_wgrad_stem_kernel, dim3((unsigned)(S * sw.nrb), RT_STEM_COLS / 32), dim3(64), 0, c.s, sw);
    RtWc kc{};
    kc.part = sw.part; kc.out = gr->conv1_w; kc.nchunks = S * sw.nrb; kc.rows = 64; kc.width = 147; kc.pitch = RT_STEM_COLS;
    hipLaunchKernelGGL(rt_wcombine_kernel, dim3(rt_blocks(64 * 147)), dim3(256), 0, c.s, kc);
    return vt_check(hipGetLastError(), "vt_resnet_bwd");
}

}  // extern "C"
