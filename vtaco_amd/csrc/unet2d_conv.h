// unet2d_conv.h -- the tactile U-Net's shared conv template, weight packing and layouts (see unet2d.hip for the description): included by
// unet2d.hip (eval mode) and unet2d_train.hip (train-mode forward and backward, which adds the TU_RAW and TU_S2D epilogues).
#pragma once
#include "vt_common.h"
#include "decode_common.h"

namespace {

constexpr int TU_MAX_HW = 2048, TU_MAX_IMG = 1024;
constexpr int TU_FINAL_FLOATS = VT_TACTILE_UNET_MAX_CLASSES * 64 + 4;      // conv_final: [4 classes][64 channels] zero padded, bias [4]

struct TuDims { int depth, sf, cin, classes, n_img, H, W; };

inline bool tu_net_ok(const TuDims &d) {
    return d.depth >= 1 && d.depth <= VT_TACTILE_UNET_MAX_DEPTH && d.sf >= 8 && d.sf <= 64 && d.sf % 8 == 0 && d.cin >= 1 && d.cin <= 4 &&
           d.classes >= 1 && d.classes <= VT_TACTILE_UNET_MAX_CLASSES;
}
inline bool tu_dims_ok(const TuDims &d) {
    if (!tu_net_ok(d)) return false;
    if (d.n_img <= 0 || d.n_img > TU_MAX_IMG || d.H <= 0 || d.W <= 0 || d.H > TU_MAX_HW || d.W > TU_MAX_HW) return false;
    const int m = 1 << (d.depth - 1);
    if (d.H % m || d.W % m) return false;
    // the largest tensor is a level-0 activation (level i has 4^-i of the pixels and 2^i of the channels): 32-bit element offsets
    return (long long)d.n_img * d.H * d.W * d.sf < (1ll << 31);
}
inline int tu_ncb(int Cout) { return (Cout + 31) / 32; }
inline long long tu_frag_floats(int Cout, int Cin, int ntaps) { return (long long)tu_ncb(Cout) * (Cin / 8) * ntaps * 256; }

// ---- blob layout (floats) ---------------------------------------------------------------------------------------------------------------
// first conv [sf][cin * 9] + bias [sf]; every other conv: fragments + bias [32 ncb]; up-convs: the same with the 4 parities (dy, dx) as taps;
// conv_final padded.  A conv's fragments: [ncb][Cin / 8][ntaps][64 lanes][4]: lane l, slot j =
// W'[cb * 32 + l % 32][chunk * 8 + 4 (l / 32) + j][tap], rows past Cout zero.
struct TuConvOff { long long w, b; };
struct TuLayout {
    long long first_w, first_b;
    TuConvOff down[VT_TACTILE_UNET_MAX_DEPTH][2];      // [0][0] unused (the first conv)
    TuConvOff upt[VT_TACTILE_UNET_MAX_DEPTH];          // indexed by the level the block produces (0 .. depth - 2)
    TuConvOff up[VT_TACTILE_UNET_MAX_DEPTH][2];
    long long final_w, total;
};
inline TuLayout tu_layout(const TuDims &d) {
    TuLayout L{};
    long long off = 0;
    auto conv = [&](TuConvOff &o, int Cout, int Cin, int ntaps) {
        o.w = off; off += tu_frag_floats(Cout, Cin, ntaps);
        o.b = off; off += tu_ncb(Cout) * 32;
    };
    L.first_w = off; off += (d.sf * d.cin * 9 + 3) / 4 * 4;
    L.first_b = off; off += d.sf;
    for (int i = 0; i < d.depth; ++i) {
        const int c = d.sf << i;
        if (i > 0) conv(L.down[i][0], c, c / 2, 9);
        conv(L.down[i][1], c, c, 9);
    }
    for (int i = d.depth - 2; i >= 0; --i) {
        const int c = d.sf << i;
        conv(L.upt[i], c, 2 * c, 4);
        conv(L.up[i][0], c, 2 * c, 9);
        conv(L.up[i][1], c, c, 9);
    }
    L.final_w = off; off += TU_FINAL_FLOATS;
    L.total = off;
    return L;
}

// ---- workspace layout (floats): per level skip, mid, and below the bottom level pooled, up (the up-conv's result), out ----------------
struct TuWs { long long skip[VT_TACTILE_UNET_MAX_DEPTH], mid[VT_TACTILE_UNET_MAX_DEPTH], pooled[VT_TACTILE_UNET_MAX_DEPTH],
              up[VT_TACTILE_UNET_MAX_DEPTH], out[VT_TACTILE_UNET_MAX_DEPTH], total; };
inline TuWs tu_workspace(const TuDims &d) {
    TuWs w{};
    long long off = 0;
    for (int i = 0; i < d.depth; ++i) {
        const long long n = (long long)d.n_img * (d.H >> i) * (d.W >> i) * (d.sf << i);
        w.skip[i] = off; off += n;
        w.mid[i] = off; off += n;
        if (i < d.depth - 1) {
            w.pooled[i] = off; off += n / 4;
            w.up[i] = off; off += n;
            if (i > 0) { w.out[i] = off; off += n; }
        }
    }
    w.total = off;
    return w;
}

// ---- pack -------------------------------------------------------------------------------------------------------------------------------
struct TuPack {
    const float *w, *b;                          // conv weight, conv bias
    const float *gamma, *beta, *mean, *var;      // the BatchNorm behind it, or all null
    double eps;
    float *frag, *bias;
    int Cout, Cin, ntaps, kind;                  // kind 0: conv [Cout][Cin][ntaps] -> fragments; 1: transposed conv [Cin][Cout][4] -> four
};                                               // parities of fragments; 2: the first conv, [Cout][Cin * 9] kept; 3: conv_final, padded

__device__ __forceinline__ double tu_scale(const TuPack &p, int co) {
    return p.gamma ? (double)p.gamma[co] / sqrt((double)p.var[co] + p.eps) : 1.0;
}

__global__ void __launch_bounds__(256) tu_pack_kernel(TuPack p) {
    const int ncb = (p.Cout + 31) / 32, n_chunks = p.Cin / 8;
    long long nf, nb;
    if (p.kind == 0 || p.kind == 1) { nf = (long long)ncb * n_chunks * p.ntaps * 256; nb = ncb * 32; }
    else if (p.kind == 2) { nf = (long long)p.Cout * p.Cin * 9; nb = p.Cout; }
    else { nf = VT_TACTILE_UNET_MAX_CLASSES * 64; nb = 4; }
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nf + nb; e += (long long)gridDim.x * 256) {
        if (e >= nf) {
            const int co = (int)(e - nf);
            double v = 0.0;
            if (co < p.Cout) {
                const double s = tu_scale(p, co);
                v = p.gamma ? ((double)p.b[co] - (double)p.mean[co]) * s + (double)p.beta[co] : (double)p.b[co];
            }
            p.bias[co] = (float)v;
            continue;
        }
        double v = 0.0;
        if (p.kind == 2) {
            const int co = (int)(e / (p.Cin * 9));
            v = (double)p.w[e] * tu_scale(p, co);
        } else if (p.kind == 3) {
            const int k = (int)(e >> 6), c = (int)(e & 63);
            if (k < p.Cout && c < p.Cin) v = (double)p.w[k * p.Cin + c];
        } else {
            const int j = (int)(e & 3), l = (int)((e >> 2) & 63);
            long long q = e >> 8;
            const int t = (int)(q % p.ntaps); q /= p.ntaps;
            const int chunk = (int)(q % n_chunks), cb = (int)(q / n_chunks);
            const int ci = chunk * 8 + 4 * (l >> 5) + j, co = cb * 32 + (l & 31);
            if (co < p.Cout)
                v = p.kind == 0 ? (double)p.w[((size_t)co * p.Cin + ci) * p.ntaps + t] * tu_scale(p, co)
                                : (double)p.w[((size_t)ci * p.Cout + co) * 4 + t];
        }
        p.frag[e] = (float)v;
    }
}

// ---- the first conv -----------------------------------------------------------------------------------------------------------------------
struct TuFirst {
    const float *x;          // [n_img][cin][H][W]
    const float *w, *bias;   // [Cout][cin * 9] folded, [Cout]
    float *out;              // [n_img][H][W][Cout]
    int cin, Cout, H, W, P;  // P = n_img * H * W
};

__global__ void __launch_bounds__(256) tu_first_kernel(TuFirst p) {
    __shared__ float ws[36 * 8 + 8];
    const int g = blockIdx.y, K = p.cin * 9;
    for (int e = threadIdx.x; e < K * 8 + 8; e += 256) {
        if (e < K * 8) { const int k = e >> 3, c = e & 7; ws[e] = p.w[(g * 8 + c) * K + k]; }
        else ws[36 * 8 + (e - K * 8)] = p.bias[g * 8 + (e - K * 8)];
    }
    __syncthreads();
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= p.P) return;
    const int x = pix % p.W, y = (pix / p.W) % p.H, img = pix / (p.W * p.H);
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
    for (int ci = 0; ci < p.cin; ++ci) {
        const float *plane = p.x + (unsigned)((img * p.cin + ci) * p.H * p.W);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = y + ky - 1;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = x + kx - 1;
                const bool ok = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                const float v = ok ? plane[(unsigned)(iy * p.W + ix)] : 0.f;
                const float *wk = ws + ((ci * 3 + ky) * 3 + kx) * 8;
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] = fmaf(wk[c], v, acc[c]);
            }
        }
    }
    f32x4 lo, hi;
#pragma unroll
    for (int c = 0; c < 4; ++c) { lo[c] = fmaxf(acc[c] + ws[36 * 8 + c], 0.f); hi[c] = fmaxf(acc[4 + c] + ws[36 * 8 + 4 + c], 0.f); }
    f32x4 *o = reinterpret_cast<f32x4 *>(p.out + (unsigned)(pix * p.Cout + g * 8));
    o[0] = lo; o[1] = hi;
}

// ---- the conv template ----------------------------------------------------------------------------------------------------------------------
// (train mode, unet2d_train.hip) TU_RAW: a 3x3 conv that stores acc + bias, no ReLU (BatchNorm follows as a pass of its own; with
// flipped, transposed weights it is the conv's data gradient).  TU_S2D: the 2x2 stride-2 conv that is the data gradient of the
// transposed conv: output pixel (y, x) reads input pixels (2 y + dy, 2 x + dx) of a [2 H][2 W][CA] tensor; fragments [ncb][4][CA / 8].
enum { TU_PLAIN = 0, TU_POOL = 1, TU_FINAL = 2, TU_UP = 3, TU_RAW = 4, TU_S2D = 5 };

struct TuConv {
    const float *inA, *inB;  // [n_img][H][W][CA] then [n_img][H][W][CB] along K (CB = 0: one source)
    const float *wfrag, *bias;
    float *out;              // PLAIN, POOL: [n_img][H][W][Cout]; UP: [n_img][2H][2W][Cout]
    float *pooled;           // POOL: [n_img][H/2][W/2][Cout]
    const float *fw;         // FINAL: conv_final [4][64] zero padded, then its bias [4]
    float *fout;             // FINAL: [n_img][classes][H][W]
    int CA, CB, Cout, classes, H, W, tiles_x, tiles_y, n_tiles;
};

// CS: fragments per chunk (9 taps; the up-conv's chunk holds its 4 parities, of which a launch row reads one)
template <int NCB, int NT, int CS>
__device__ __forceinline__ void tu_accumulate(f32x16 (&acc)[NCB], const float *src, int C, int n_chunks, const f32x4 *(&wf)[NCB],
                                              int img, int y, int x, int H, int W, bool valid, int h) {
    const float *inimg = src + (unsigned)(img * H * W * C) + 4 * h;
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const float *inc = inimg + chunk * 8;
#pragma unroll
        for (int ky = 0; ky < NT; ++ky) {
            const int iy = y + (NT == 3 ? ky - 1 : 0);
            const bool rowok = valid && iy >= 0 && iy < H;
            const int iyc = iy < 0 ? 0 : iy >= H ? H - 1 : iy;
            f32x4 b[NT], a[NCB][NT];
            // every load unconditional (coordinates clamped into the image, the value dropped afterwards): they issue back to back
#pragma unroll
            for (int kx = 0; kx < NT; ++kx) {
                const int ix = x + (NT == 3 ? kx - 1 : 0);
                const int ixc = ix < 0 ? 0 : ix >= W ? W - 1 : ix;
                b[kx] = *reinterpret_cast<const f32x4 *>(inc + (unsigned)((iyc * W + ixc) * C));
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) a[cb][kx] = wf[cb][(size_t)(chunk * CS + ky * NT + kx) * 64];
            }
#pragma unroll
            for (int kx = 0; kx < NT; ++kx) {
                const int ix = x + (NT == 3 ? kx - 1 : 0);
                if (!(rowok && ix >= 0 && ix < W)) b[kx] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma(a[cb][kx][j], b[kx][j], acc[cb]);
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) wf[cb] += (size_t)n_chunks * CS * 64;
}

template <int NCB, int EPI>
__global__ void __launch_bounds__(256) tu_conv_kernel(TuConv p) {
    constexpr int NT = EPI == TU_UP || EPI == TU_S2D ? 1 : 3, CS = EPI == TU_UP || EPI == TU_S2D ? 4 : 9;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5, lp = lane & 31;
    const int ncb = (p.Cout + 31) >> 5, n_cbg = (ncb + NCB - 1) / NCB;
    const int cbg = blockIdx.x % n_cbg, tile = (blockIdx.x / n_cbg) * 4 + wave;
    if (tile >= p.n_tiles) return;                                    // (wave-uniform; the kernel has no barrier)
    const int tx = tile % p.tiles_x, ty = (tile / p.tiles_x) % p.tiles_y, img = tile / (p.tiles_x * p.tiles_y);
    const int yr = 2 * ty + (lp >> 4), xr = 16 * tx + (lp & 15);
    const bool valid = yr < p.H && xr < p.W;
    const int y = yr < p.H ? yr : p.H - 1, x = xr < p.W ? xr : p.W - 1;
    const int nA = p.CA >> 3, nB = p.CB >> 3;
    f32x16 acc[NCB];
    const f32x4 *wf[NCB];
    int cbi[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
        const int c = cbg * NCB + cb;
        cbi[cb] = c < ncb ? c : ncb - 1;                              // an odd block count: the spare accumulator repeats the last block
        wf[cb] = reinterpret_cast<const f32x4 *>(p.wfrag) + (size_t)cbi[cb] * (nA + nB) * CS * 64 + (EPI == TU_UP ? blockIdx.y * 64 : 0) + lane;
    }
    if constexpr (EPI == TU_S2D) {
        // parity (dy, dx) of the [2 H][2 W][CA] input seen as an [H][2 W][2 CA] tensor whose pixel (y, x) starts at input pixel (2 y, 2 x)
#pragma unroll
        for (int t = 0; t < 4; ++t)
            tu_accumulate<NCB, 1, 1>(acc, p.inA + (unsigned)(((t >> 1) * 2 * p.W + (t & 1)) * p.CA), 2 * p.CA, nA, wf, img, y, x, p.H, 2 * p.W, valid, h);
    } else {
        tu_accumulate<NCB, NT, CS>(acc, p.inA, p.CA, nA, wf, img, y, x, p.H, p.W, valid, h);
        if (nB) tu_accumulate<NCB, NT, CS>(acc, p.inB, p.CB, nB, wf, img, y, x, p.H, p.W, valid, h);
    }

    if constexpr (EPI == TU_FINAL) {
        // conv_final over this pixel's channels: each half of the wave sums its 16 (32) channels in register order, then the halves meet
        float part[VT_TACTILE_UNET_MAX_CLASSES];
#pragma unroll
        for (int k = 0; k < VT_TACTILE_UNET_MAX_CLASSES; ++k) part[k] = 0.f;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = cb * 32 + 8 * q + 4 * h;
                const f32x4 bias = *reinterpret_cast<const f32x4 *>(p.bias + co);
#pragma unroll
                for (int k = 0; k < VT_TACTILE_UNET_MAX_CLASSES; ++k) {
                    const f32x4 w = *reinterpret_cast<const f32x4 *>(p.fw + k * 64 + co);
#pragma unroll
                    for (int i = 0; i < 4; ++i) part[k] = fmaf(w[i], fmaxf(acc[cb][4 * q + i] + bias[i], 0.f), part[k]);
                }
            }
#pragma unroll
        for (int k = 0; k < VT_TACTILE_UNET_MAX_CLASSES; ++k) {
            const float other = __shfl_xor(part[k], 32);
            const float t = (h == 0 ? part[k] + other : other + part[k]) + p.fw[VT_TACTILE_UNET_MAX_CLASSES * 64 + k];
            if (h == 0 && valid && k < p.classes)
                p.fout[(unsigned)(((img * p.classes + k) * p.H + yr) * p.W + xr)] = 1.f / (1.f + expf(-t));
        }
    } else {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const bool mine = cbg * NCB + cb < ncb;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = cbi[cb] * 32 + 8 * q + 4 * h;
                const f32x4 bias = *reinterpret_cast<const f32x4 *>(p.bias + co);
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    v[i] = EPI == TU_UP || EPI == TU_RAW || EPI == TU_S2D ? acc[cb][4 * q + i] + bias[i] : fmaxf(acc[cb][4 * q + i] + bias[i], 0.f);
                const bool chan = mine && co < p.Cout;
                if constexpr (EPI == TU_UP) {
                    const int oy = 2 * yr + (blockIdx.y >> 1), ox = 2 * xr + (blockIdx.y & 1);
                    if (chan && valid) *reinterpret_cast<f32x4 *>(p.out + (unsigned)(((img * 2 * p.H + oy) * 2 * p.W + ox) * p.Cout + co)) = v;
                } else {
                    if (chan && valid) *reinterpret_cast<f32x4 *>(p.out + (unsigned)(((img * p.H + yr) * p.W + xr) * p.Cout + co)) = v;
                }
                if constexpr (EPI == TU_POOL) {
                    // H and W are even here: a valid pixel at an even (row, column) has its whole window valid and in this patch
                    f32x4 m;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float t = fmaxf(v[i], __shfl_xor(v[i], 1));
                        m[i] = fmaxf(t, __shfl_xor(t, 16));
                    }
                    if (chan && valid && (lp & 17) == 0)
                        *reinterpret_cast<f32x4 *>(p.pooled + (unsigned)(((img * (p.H >> 1) + ty) * (p.W >> 1) + (xr >> 1)) * p.Cout + co)) = m;
                }
            }
        }
    }
}

template <int EPI>
void tu_launch(const TuConv &p, hipStream_t s) {
    const int ncb = tu_ncb(p.Cout), NCB = ncb == 1 ? 1 : 2, n_cbg = (ncb + NCB - 1) / NCB;
    const dim3 grid((unsigned)((p.n_tiles + 3) / 4 * n_cbg), EPI == TU_UP ? 4 : 1);
    if (NCB == 1) hipLaunchKernelGGL((tu_conv_kernel<1, EPI>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((tu_conv_kernel<2, EPI>), grid, dim3(256), 0, s, p);
}

inline TuConv tu_conv_args(const float *inA, int CA, const float *inB, int CB, const float *blob, const TuConvOff &o, int Cout, int n_img, int H, int W) {
    TuConv c{};
    c.inA = inA; c.CA = CA; c.inB = inB ? inB : inA; c.CB = CB; c.wfrag = blob + o.w; c.bias = blob + o.b; c.Cout = Cout;
    c.H = H; c.W = W; c.tiles_x = (W + 15) / 16; c.tiles_y = (H + 1) / 2; c.n_tiles = n_img * c.tiles_x * c.tiles_y;
    return c;
}

inline TuDims tu_dims_of(const vt_tactile_unet_params *p, int n_img, int H, int W) {
    TuDims d;
    d.depth = p->depth; d.sf = p->start_filts; d.cin = p->in_channels; d.classes = p->num_classes; d.n_img = n_img; d.H = H; d.W = W;
    return d;
}
inline TuDims tu_dims_raw(int depth, int sf, int cin, int classes, int n_img, int H, int W) {
    TuDims d;
    d.depth = depth; d.sf = sf; d.cin = cin; d.classes = classes; d.n_img = n_img; d.H = H; d.W = W;
    return d;
}

inline int tu_pack_one(const float *w, const float *b, const vt_resnet_bn *bn, float *frag, float *bias, int Cout, int Cin, int ntaps, int kind,
                hipStream_t s) {
    if (!w || !b || (bn && !(bn->weight && bn->bias && bn->running_mean && bn->running_var)))
        return vt_fail(VT_ERR_INVALID, "vt_tactile_unet_pack: null conv or BatchNorm tensor");
    TuPack p{};
    p.w = w; p.b = b;
    if (bn) { p.gamma = bn->weight; p.beta = bn->bias; p.mean = bn->running_mean; p.var = bn->running_var; p.eps = bn->eps; }
    p.frag = frag; p.bias = bias; p.Cout = Cout; p.Cin = Cin; p.ntaps = ntaps; p.kind = kind;
    hipLaunchKernelGGL(tu_pack_kernel, dim3(64), dim3(256), 0, s, p);
    return 0;
}

}  // namespace
