// resnet2d_conv.h -- the tactile ResNet's shared shapes, blob layout and 3x3 conv template (see resnet2d.hip for the description):
// included by resnet2d.hip (eval mode) and resnet2d_train.hip (train-mode forward and backward, which adds the RAW epilogue).
#pragma once
#include "vt_common.h"
#include "decode_common.h"

namespace {

constexpr int RN_LIN = 100;          // width of `linear` (src/layers.py:147)
constexpr int RN_FEAT = 512;         // channels of layer4
constexpr int RN_STEM_ROWS = 21;     // (input channel, ky) pairs of the stem; 4 k-steps (kx = 2 j + half, kx 7 = zero) each
constexpr int RN_STEM_FRAG = 2 * RN_STEM_ROWS * 256;
constexpr int RN_MAX_HW = 2048, RN_MAX_IMG = 1024;

struct RnDims { int blocks[4]; int classes; int n_img, H, W; };

__host__ __device__ inline int rn_half(int v) { return (v - 1) / 2 + 1; }        // stride-2 output size (7x7 pad 3, 3x3 pad 1, 1x1 pad 0)
inline int rn_width(int stage) { return 64 << stage; }
inline bool rn_net_ok(const int *blocks, int classes) {
    if (classes <= 0 || classes > 65536) return false;
    for (int s = 0; s < 4; ++s)
        if (blocks[s] <= 0 || blocks[s] > VT_RESNET_MAX_BLOCKS) return false;
    return true;
}
// size of stage s's activations, per image
inline void rn_stage_hw(const RnDims &d, int stage, int &h, int &w) {
    h = rn_half(rn_half(d.H)); w = rn_half(rn_half(d.W));
    for (int s = 0; s < stage; ++s) { h = rn_half(h); w = rn_half(w); }
}
// floats of ONE of the four rotating activation buffers: the largest stage's [n_img][h][w][C]
inline long long rn_buf_floats(const RnDims &d) {
    long long most = 0;
    for (int s = 0; s < 4; ++s) {
        int h, w;
        rn_stage_hw(d, s, h, w);
        const long long n = (long long)d.n_img * h * w * rn_width(s);
        if (n > most) most = n;
    }
    return most;
}
inline bool rn_dims_ok(const RnDims &d) {
    if (!rn_net_ok(d.blocks, d.classes)) return false;
    if (d.n_img <= 0 || d.n_img > RN_MAX_IMG || d.H <= 0 || d.W <= 0 || d.H > RN_MAX_HW || d.W > RN_MAX_HW) return false;
    if ((long long)d.n_img * 3 * d.H * d.W >= (1ll << 31)) return false;               // 32-bit element offsets inside a tensor
    if (rn_buf_floats(d) >= (1ll << 31)) return false;
    if ((long long)d.n_img * d.classes >= (1ll << 31)) return false;
    return true;
}

// ---- blob layout (floats): stem fragments + bias; per block conv1 fragments + bias, conv2 fragments + bias, and for a projecting block
// the 1x1 fragments + bias; linear.weight, linear.bias (padded to 4), fc.weight (padded), fc.bias (padded)
struct RnBlockOff { long long w1, b1, w2, b2, wp, bp; int Cin, Cout, proj; };
inline long long rn_pad4(long long n) { return (n + 3) / 4 * 4; }
struct RnLayout {
    long long stem_w, stem_b, lin_w, lin_b, fc_w, fc_b, total;
};
// walks the blob; block (stage, index) -> offsets when `want` matches
inline RnLayout rn_layout(const int *blocks, int classes, int want_stage, int want_block, RnBlockOff *out) {
    RnLayout L;
    long long off = 0;
    L.stem_w = off; off += RN_STEM_FRAG;
    L.stem_b = off; off += 64;
    int cin = 64;
    for (int s = 0; s < 4; ++s) {
        const int cout = rn_width(s);
        for (int b = 0; b < blocks[s]; ++b) {
            RnBlockOff o;
            o.Cin = cin; o.Cout = cout; o.proj = (b == 0 && s > 0) ? 1 : 0;
            o.w1 = off; off += (long long)cout * cin * 9;
            o.b1 = off; off += cout;
            o.w2 = off; off += (long long)cout * cout * 9;
            o.b2 = off; off += cout;
            o.wp = o.bp = 0;
            if (o.proj) { o.wp = off; off += (long long)cout * cin; o.bp = off; off += cout; }
            if (out && s == want_stage && b == want_block) *out = o;
            cin = cout;
        }
    }
    L.lin_w = off; off += (long long)RN_LIN * RN_FEAT;
    L.lin_b = off; off += rn_pad4(RN_LIN);
    L.fc_w = off; off += rn_pad4((long long)classes * RN_LIN);
    L.fc_b = off; off += rn_pad4(classes);
    L.total = off;
    return L;
}

// ---- the 3x3 conv template --------------------------------------------------------------------------------------------------------------
struct RnConv {
    const float *in;         // [n_img][Hi][Wi][Cin]
    const float *wfrag, *bias;
    const float *wproj, *bproj;   // PROJ: the 1x1 stride-2 projection's fragments [Cout / 32][Cin / 8][64][4] and bias
    const float *res;        // residual [P][Cout] added before the ReLU, or null
    float *out;              // [P][Cout]
    float *skip;             // PROJ: the projected skip [P][Cout] (no ReLU)
    int Cin, Cout, Hi, Wi, Ho, Wo, P;      // P = n_img * Ho * Wo output pixels
};

__device__ __forceinline__ f32x4 rn_quad(const f32x16 &a, int q) { return f32x4{a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]}; }

// RAW (train mode, resnet2d_train.hip): the accumulators are stored as they are -- no bias, no residual, no ReLU (BatchNorm follows as a pass
// of its own; with flipped, transposed weights the stride-1 conv is its own data gradient)
template <int KS, int STRIDE, bool PROJ, bool RAW = false>
__global__ void __launch_bounds__(KS * 64) resnet_conv_kernel(RnConv p) {
    __shared__ __attribute__((aligned(16))) float red[KS * 16 * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5, lp = lane & 31;
    const int n_cbp = p.Cout >> 6, cbp = blockIdx.x % n_cbp, tile = blockIdx.x / n_cbp;
    const int pix = tile * 32 + lp;
    const bool valid = pix < p.P;
    const int pc = valid ? pix : p.P - 1;
    const int ox = pc % p.Wo, oy = (pc / p.Wo) % p.Ho, img = pc / (p.Wo * p.Ho);
    const int n_chunks = p.Cin >> 3, cpw = n_chunks / KS;
    constexpr int NA = PROJ ? 4 : 2;                  // accumulators: conv (2 blocks of 32 channels), projection (2)
    f32x16 acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    const f32x4 *wf0 = reinterpret_cast<const f32x4 *>(p.wfrag) + (size_t)(2 * cbp) * n_chunks * 9 * 64 + lane;
    const f32x4 *wf1 = wf0 + (size_t)n_chunks * 9 * 64;
    const float *inimg = p.in + (unsigned)(img * p.Hi * p.Wi * p.Cin) + 4 * h;
    for (int ck = 0; ck < cpw; ++ck) {
        const int chunk = wave * cpw + ck;
        const float *inc = inimg + chunk * 8;
        f32x4 centre = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * STRIDE + ky - 1;
            const bool rowok = valid && iy >= 0 && iy < p.Hi;
            const int iyc = iy < 0 ? 0 : iy >= p.Hi ? p.Hi - 1 : iy;
            f32x4 b[3], a0[3], a1[3];
            // every load unconditional (coordinates clamped into the image, the value dropped afterwards): they issue back to back
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * STRIDE + kx - 1;
                const int ixc = ix < 0 ? 0 : ix >= p.Wi ? p.Wi - 1 : ix;
                b[kx] = *reinterpret_cast<const f32x4 *>(inc + (unsigned)((iyc * p.Wi + ixc) * p.Cin));
                a0[kx] = wf0[(size_t)(chunk * 9 + ky * 3 + kx) * 64];
                a1[kx] = wf1[(size_t)(chunk * 9 + ky * 3 + kx) * 64];
            }
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * STRIDE + kx - 1;
                if (!(rowok && ix >= 0 && ix < p.Wi)) b[kx] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (PROJ && ky == 1 && kx == 1) centre = b[kx];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[0] = mfma(a0[kx][j], b[kx][j], acc[0]);
                    acc[1] = mfma(a1[kx][j], b[kx][j], acc[1]);
                }
            }
        }
        if constexpr (PROJ) {
            const f32x4 *wp = reinterpret_cast<const f32x4 *>(p.wproj) + lane;
            const f32x4 q0 = wp[(size_t)((2 * cbp) * n_chunks + chunk) * 64], q1 = wp[(size_t)((2 * cbp + 1) * n_chunks + chunk) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[2] = mfma(q0[j], centre[j], acc[2]);
                acc[3] = mfma(q1[j], centre[j], acc[3]);
            }
        }
    }
    // ---- the waves' K shares meet in LDS, one accumulator at a time; thread (q, l) of the first four waves sums quad q of lane l over
    // the waves in wave order and finishes 4 channels of one pixel
    f32x4 *red4 = reinterpret_cast<f32x4 *>(red);
    const int eq = threadIdx.x >> 6, el = threadIdx.x & 63;           // (meaningful for threadIdx.x < 256)
    const int epix = tile * 32 + (el & 31);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        if (a) __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) red4[(wave * 4 + q) * 64 + lane] = rn_quad(acc[a], q);
        __syncthreads();
        if (threadIdx.x < 256 && epix < p.P) {
            f32x4 sum = red4[(0 * 4 + eq) * 64 + el];
#pragma unroll
            for (int w = 1; w < KS; ++w) sum += red4[(w * 4 + eq) * 64 + el];
            const int co = (2 * cbp + (a & 1)) * 32 + 8 * eq + 4 * (el >> 5);
            const unsigned o = (unsigned)(epix * p.Cout + co);
            if constexpr (RAW) {
                *reinterpret_cast<f32x4 *>((a < 2 ? p.out : p.skip) + o) = sum;
            } else if (a < 2) {
                sum += *reinterpret_cast<const f32x4 *>(p.bias + co);
                if (p.res) sum += *reinterpret_cast<const f32x4 *>(p.res + o);
                sum = f32x4{fmaxf(sum[0], 0.f), fmaxf(sum[1], 0.f), fmaxf(sum[2], 0.f), fmaxf(sum[3], 0.f)};
                *reinterpret_cast<f32x4 *>(p.out + o) = sum;
            } else {
                sum += *reinterpret_cast<const f32x4 *>(p.bproj + co);
                *reinterpret_cast<f32x4 *>(p.skip + o) = sum;
            }
        }
    }
}

// the K split inside a workgroup: waves per output tile, by the layer's input channels alone (never by the number of images: an
// image's features are the same bits in any batch); each wave takes Cin / (8 KS) chunks of 8 channels
inline int rn_waves(int Cin) { return Cin % 64 == 0 && Cin >= 128 ? 8 : 4; }
inline bool rn_split_ok(int Cin, int KS) { return Cin > 0 && Cin % (8 * KS) == 0; }

template <bool RAW = false>
void rn_launch_conv(const RnConv &p, int stride, hipStream_t s) {
    const int KS = rn_waves(p.Cin);
    const dim3 grid((unsigned)((p.P + 31) / 32 * (p.Cout / 64)));
    if (stride == 2) {
        if (KS == 8) hipLaunchKernelGGL((resnet_conv_kernel<8, 2, true, RAW>), grid, dim3(512), 0, s, p);
        else hipLaunchKernelGGL((resnet_conv_kernel<4, 2, true, RAW>), grid, dim3(256), 0, s, p);
    } else {
        if (KS == 8) hipLaunchKernelGGL((resnet_conv_kernel<8, 1, false, RAW>), grid, dim3(512), 0, s, p);
        else hipLaunchKernelGGL((resnet_conv_kernel<4, 1, false, RAW>), grid, dim3(256), 0, s, p);
    }
}

inline RnDims rn_dims_of(const int32_t *blocks, int classes, int n_img, int H, int W) {
    RnDims d;
    for (int s = 0; s < 4; ++s) d.blocks[s] = blocks ? blocks[s] : 0;
    d.classes = classes; d.n_img = n_img; d.H = H; d.W = W;
    return d;
}

inline bool rn_bn_ok(const vt_resnet_bn &b) { return b.weight && b.bias && b.running_mean && b.running_var; }

}  // namespace
