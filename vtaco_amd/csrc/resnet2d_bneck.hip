// resnet2d_bneck.hip -- the tactile feature encoder with Bottleneck blocks (reference ``ResNet(Bottleneck, ...)``, src/layers.py:86-207:
// ``encoder_img: Resnet50`` of the registry, Resnet101 / Resnet152 beside it) in eval mode: vt_resnet_bneck_pack, vt_resnet_bneck_fwd.
//
// The conventions are resnet2d.hip's: channels-last activations, BatchNorm folded in f64 at pack time into fragment-ordered weights, exact
// f32 on v_mfma_f32_32x32x2f32, no atomics, a K split that depends on the layer's channels alone, layers as launches.  The forward is
// 1 + 3 * (number of blocks) + 1 launches (50 for Resnet50):
//
//   stem    resnet2d_net.h's stem kernel (7x7 stride 2, bias, ReLU, 3x3 stride-2 max-pool).
//   conv1   1x1 stride 1, bias, ReLU: a GEMM over the flat pixel index (bneck_gemm_kernel, one K segment).
//   conv2   3x3 at stride 1 or 2, bias, ReLU: resnet2d_conv.h's template without the projection (bn_launch_conv3x3).
//   conv3   1x1 to 4 C, the skip, ReLU: the same GEMM kernel.  In a projecting block (the first of every stage, layer1.0 included: 64 ->
//           256 at stride 1) conv3 and the 1x1 projection write the same output tile, so they are ONE GEMM whose K runs over two
//           segments in a fixed order -- first the C channels of conv2's output at pixel p, then the Cin channels of the block's input
//           at (stride * oy, stride * ox) -- with the bias b3 + b_proj summed in f64 at pack time: no skip tensor, no extra launch.  In
//           the other blocks the block's input is added in the epilogue.
//   tail    resnet2d_net.h's tail at 2048 features (average pool, Linear(2048, 100), Linear(100, classes), f64 accumulators).
//
// The GEMM kernel: a workgroup owns 32 consecutive pixels (the last tile ragged) x NCB * 32 output channels.  K is cut into chunks of 8
// channels; a lane's B operands of a chunk (4 consecutive channels of its pixel) are one 16-byte load, and so are its A operands of each
// of the NCB channel blocks (fragment order [Cout / 32][K / 8][64][4], the pack kernel's order with ntaps = 1).  So one B load feeds
// 4 NCB MFMAs: NCB = 4 (a 128-channel tile, 64 accumulator registers) where the layer has the tiles to fill the machine, NCB = 2 where
// it has not.  The chunks of both segments, in order, are split evenly over the workgroup's KS = 4 or 8 waves (by the layer's chunk count
// alone); the partial sums meet in LDS in wave order as in resnet2d_conv.h, so a pixel's result is the same bits in any batch and with
// either NCB.
#include "resnet2d_net.h"

namespace {

constexpr int BN_FEAT = 4 * RN_FEAT;     // channels of layer4

// floats of ONE of the four activation buffers: the widest tensor of a stage is its output, [n_img][h][w][4 * width]
inline long long bn_buf_floats(const RnDims &d) {
    long long most = 0;
    for (int s = 0; s < 4; ++s) {
        int h, w;
        rn_stage_hw(d, s, h, w);
        const long long n = (long long)d.n_img * h * w * 4 * rn_width(s);
        if (n > most) most = n;
    }
    return most;
}
inline bool bn_dims_ok(const RnDims &d) {
    if (!rn_dims_ok(d)) return false;
    return bn_buf_floats(d) < (1ll << 31);
}

// ---- blob layout (floats): stem fragments + bias; per block conv1 fragments + bias, conv2 fragments + bias, conv3 fragments, for a
// projecting block the projection's fragments, ONE bias for conv3 (+ projection); linear.weight, linear.bias (padded to 4), fc.weight
// (padded), fc.bias (padded)
struct BnBlockOff { long long w1, b1, w2, b2, w3, wp, b3; int Cin, C, proj, stride; };
struct BnLayout { long long stem_w, stem_b, lin_w, lin_b, fc_w, fc_b, total; };
inline BnLayout bn_layout(const int *blocks, int classes, int want_stage, int want_block, BnBlockOff *out) {
    BnLayout L;
    long long off = 0;
    L.stem_w = off; off += RN_STEM_FRAG;
    L.stem_b = off; off += 64;
    int cin = 64;
    for (int s = 0; s < 4; ++s) {
        const int c = rn_width(s);
        for (int b = 0; b < blocks[s]; ++b) {
            BnBlockOff o;
            o.Cin = cin; o.C = c; o.proj = b == 0 ? 1 : 0; o.stride = (b == 0 && s > 0) ? 2 : 1;
            o.w1 = off; off += (long long)c * cin;
            o.b1 = off; off += c;
            o.w2 = off; off += (long long)c * c * 9;
            o.b2 = off; off += c;
            o.w3 = off; off += (long long)4 * c * c;
            o.wp = 0;
            if (o.proj) { o.wp = off; off += (long long)4 * c * cin; }
            o.b3 = off; off += 4 * c;
            if (out && s == want_stage && b == want_block) *out = o;
            cin = 4 * c;
        }
    }
    L.lin_w = off; off += (long long)RN_LIN * BN_FEAT;
    L.lin_b = off; off += rn_pad4(RN_LIN);
    L.fc_w = off; off += rn_pad4((long long)classes * RN_LIN);
    L.fc_b = off; off += rn_pad4(classes);
    L.total = off;
    return L;
}

// the bias of conv3 + projection: (beta3 - mean3 s3) + (betap - meanp sp) in f64, rounded once
struct BnBias2 {
    const float *g3, *b3, *m3, *v3, *gp, *bp, *mp, *vp;
    double eps3, epsp;
    float *bias;
    int C;
};
__global__ void __launch_bounds__(256) bneck_bias2_kernel(BnBias2 p) {
    const int co = blockIdx.x * 256 + threadIdx.x;
    if (co >= p.C) return;
    const double s3 = (double)p.g3[co] / sqrt((double)p.v3[co] + p.eps3), sp = (double)p.gp[co] / sqrt((double)p.vp[co] + p.epsp);
    p.bias[co] = (float)(((double)p.b3[co] - (double)p.m3[co] * s3) + ((double)p.bp[co] - (double)p.mp[co] * sp));
}

// ---- the 1x1 GEMM over two K segments ------------------------------------------------------------------------------------------------------
struct BnGemm {
    const float *in0;        // segment 0: [P][K0], read at the output pixel
    const float *w0;         // its fragments [Cout / 32][K0 / 8][64][4]
    const float *in1;        // segment 1 (K1 > 0): [n_img][Hi][Wi][K1], read at (stride * oy, stride * ox)
    const float *w1;         // its fragments [Cout / 32][K1 / 8][64][4]
    const float *bias;       // [Cout]
    const float *res;        // residual [P][Cout] added before the ReLU, or null
    float *out;              // [P][Cout]
    int K0, K1, Cout, Hi, Wi, Ho, Wo, stride, P;      // P = n_img * Ho * Wo output pixels
};

template <int KS, int NCB>
__global__ void __launch_bounds__(KS * 64) bneck_gemm_kernel(BnGemm p) {
    __shared__ __attribute__((aligned(16))) float red[KS * 16 * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5, lp = lane & 31;
    const int n_cbg = p.Cout / (32 * NCB), cbg = blockIdx.x % n_cbg, tile = blockIdx.x / n_cbg;
    const int pix = tile * 32 + lp;
    const int pc = pix < p.P ? pix : p.P - 1;                      // (a ragged tile's spare lanes read the last pixel and store nothing)
    const int n0 = p.K0 >> 3, n1 = p.K1 >> 3, cpw = (n0 + n1) / KS;
    const int lo = wave * cpw, hi = lo + cpw;                        // this wave's chunks of the two segments laid end to end
    f32x16 acc[NCB];
#pragma unroll
    for (int a = 0; a < NCB; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    {
        const float *b0 = p.in0 + (unsigned)(pc * p.K0) + 4 * h;
        const f32x4 *a0 = reinterpret_cast<const f32x4 *>(p.w0) + (size_t)(cbg * NCB) * n0 * 64 + lane;
        const int e0 = hi < n0 ? hi : n0;
#pragma unroll 2
        for (int c = lo; c < e0; ++c) {
            const f32x4 b = *reinterpret_cast<const f32x4 *>(b0 + c * 8);
            f32x4 a[NCB];
#pragma unroll
            for (int k = 0; k < NCB; ++k) a[k] = a0[(size_t)(k * n0 + c) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < NCB; ++k) acc[k] = mfma(a[k][j], b[j], acc[k]);
        }
    }
    if (n1 > 0 && hi > n0) {
        const int ox = pc % p.Wo, oy = (pc / p.Wo) % p.Ho, img = pc / (p.Wo * p.Ho);
        const float *b1 = p.in1 + (unsigned)(((img * p.Hi + oy * p.stride) * p.Wi + ox * p.stride) * p.K1) + 4 * h;
        const f32x4 *a1 = reinterpret_cast<const f32x4 *>(p.w1) + (size_t)(cbg * NCB) * n1 * 64 + lane;
        const int s1 = (lo > n0 ? lo : n0) - n0, e1 = hi - n0;
#pragma unroll 2
        for (int c = s1; c < e1; ++c) {
            const f32x4 b = *reinterpret_cast<const f32x4 *>(b1 + c * 8);
            f32x4 a[NCB];
#pragma unroll
            for (int k = 0; k < NCB; ++k) a[k] = a1[(size_t)(k * n1 + c) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < NCB; ++k) acc[k] = mfma(a[k][j], b[j], acc[k]);
        }
    }
    // ---- the waves' K shares meet in LDS, one accumulator at a time, as in resnet2d_conv.h: thread (q, l) of the first four waves sums
    // quad q of lane l over the waves in wave order and finishes 4 channels of one pixel
    f32x4 *red4 = reinterpret_cast<f32x4 *>(red);
    const int eq = threadIdx.x >> 6, el = threadIdx.x & 63;           // (meaningful for threadIdx.x < 256)
    const int epix = tile * 32 + (el & 31);
#pragma unroll
    for (int a = 0; a < NCB; ++a) {
        if (a) __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) red4[(wave * 4 + q) * 64 + lane] = rn_quad(acc[a], q);
        __syncthreads();
        if (threadIdx.x < 256 && epix < p.P) {
            f32x4 sum = red4[(0 * 4 + eq) * 64 + el];
#pragma unroll
            for (int w = 1; w < KS; ++w) sum += red4[(w * 4 + eq) * 64 + el];
            const int co = (cbg * NCB + a) * 32 + 8 * eq + 4 * (el >> 5);
            const unsigned o = (unsigned)(epix * p.Cout + co);
            sum += *reinterpret_cast<const f32x4 *>(p.bias + co);
            if (p.res) sum += *reinterpret_cast<const f32x4 *>(p.res + o);
            sum = f32x4{fmaxf(sum[0], 0.f), fmaxf(sum[1], 0.f), fmaxf(sum[2], 0.f), fmaxf(sum[3], 0.f)};
            *reinterpret_cast<f32x4 *>(p.out + o) = sum;
        }
    }
}

// the K split of the GEMM: waves per tile by the layer's chunk count alone (never by the number of images)
inline int bn_waves(int chunks) { return chunks % 8 == 0 && chunks >= 32 ? 8 : 4; }
// channel blocks per workgroup: 4 where that still leaves two workgroups per compute unit's worth of tiles (the result does not depend on it)
constexpr long long BN_WIDE_TILES = 512;

void bn_launch_gemm(const BnGemm &p, hipStream_t s) {
    const int KS = bn_waves((p.K0 + p.K1) / 8);
    const long long tiles = (p.P + 31) / 32;
    const bool wide = p.Cout % 128 == 0 && tiles * (p.Cout / 128) >= BN_WIDE_TILES;
    const dim3 grid((unsigned)(tiles * (p.Cout / (wide ? 128 : 64))));
    if (KS == 8) {
        if (wide) hipLaunchKernelGGL((bneck_gemm_kernel<8, 4>), grid, dim3(512), 0, s, p);
        else hipLaunchKernelGGL((bneck_gemm_kernel<8, 2>), grid, dim3(512), 0, s, p);
    } else {
        if (wide) hipLaunchKernelGGL((bneck_gemm_kernel<4, 4>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((bneck_gemm_kernel<4, 2>), grid, dim3(256), 0, s, p);
    }
}

// conv2: the 3x3 template at either stride WITHOUT the projection (rn_launch_conv ties stride 2 to it)
void bn_launch_conv3x3(const RnConv &p, int stride, hipStream_t s) {
    const int KS = rn_waves(p.Cin);
    const dim3 grid((unsigned)((p.P + 31) / 32 * (p.Cout / 64)));
    if (stride == 2) {
        if (KS == 8) hipLaunchKernelGGL((resnet_conv_kernel<8, 2, false>), grid, dim3(512), 0, s, p);
        else hipLaunchKernelGGL((resnet_conv_kernel<4, 2, false>), grid, dim3(256), 0, s, p);
    } else {
        if (KS == 8) hipLaunchKernelGGL((resnet_conv_kernel<8, 1, false>), grid, dim3(512), 0, s, p);
        else hipLaunchKernelGGL((resnet_conv_kernel<4, 1, false>), grid, dim3(256), 0, s, p);
    }
}

inline RnDims bn_dims_of(const vt_resnet_bneck_params *p, int n_img, int H, int W) {
    return rn_dims_of(p->blocks_num, p->num_classes, n_img, H, W);
}

}  // namespace

extern "C" {

int vt_resnet_bneck_supported(const int32_t *blocks_num, int num_classes, int n_img, int H, int W) {
    if (!blocks_num) return 0;
    return bn_dims_ok(rn_dims_of(blocks_num, num_classes, n_img, H, W)) ? 1 : 0;
}

size_t vt_resnet_bneck_blob_bytes(const int32_t *blocks_num, int num_classes) {
    if (!blocks_num) return 0;
    const RnDims d = rn_dims_of(blocks_num, num_classes, 1, 64, 64);
    if (!rn_net_ok(d.blocks, d.classes)) return 0;
    return (size_t)bn_layout(d.blocks, d.classes, -1, -1, nullptr).total * sizeof(float);
}

size_t vt_resnet_bneck_workspace_bytes(const int32_t *blocks_num, int num_classes, int n_img, int H, int W) {
    if (!blocks_num) return 0;
    const RnDims d = rn_dims_of(blocks_num, num_classes, n_img, H, W);
    if (!bn_dims_ok(d)) return 0;
    return (size_t)(4 * bn_buf_floats(d)) * sizeof(float);
}

int vt_resnet_bneck_pack(const vt_resnet_bneck_params *p, float *blob, size_t blob_bytes, void *stream) {
    if (!p || !blob) return vt_fail(VT_ERR_INVALID, "vt_resnet_bneck_pack: null argument");
    const size_t need = vt_resnet_bneck_blob_bytes(p->blocks_num, p->num_classes);
    if (!need) return vt_fail(VT_ERR_UNSUPPORTED, "vt_resnet_bneck_pack: blocks_num entries 1..VT_RESNET_MAX_BLOCKS, num_classes >= 1");
    if (blob_bytes < need) return vt_fail(VT_ERR_WORKSPACE, "vt_resnet_bneck_pack: blob too small");
    if (!p->linear_w || !p->linear_b || !p->fc_w || !p->fc_b) return vt_fail(VT_ERR_INVALID, "vt_resnet_bneck_pack: null linear / fc tensor");
    hipStream_t s = (hipStream_t)stream;
    const RnDims d = bn_dims_of(p, 1, 64, 64);
    const BnLayout L = bn_layout(d.blocks, d.classes, -1, -1, nullptr);
    int rc = rn_pack_conv(p->conv1_w, p->bn1, blob + L.stem_w, blob + L.stem_b, 64, 3, 49, 1, s);
    if (rc != 0) return rc;
    for (int st = 0; st < 4; ++st)
        for (int b = 0; b < d.blocks[st]; ++b) {
            BnBlockOff o;
            bn_layout(d.blocks, d.classes, st, b, &o);
            const vt_resnet_bneck_block &k = p->block[st][b];
            if ((rc = rn_pack_conv(k.conv1_w, k.bn1, blob + o.w1, blob + o.b1, o.C, o.Cin, 1, 0, s)) != 0) return rc;
            if ((rc = rn_pack_conv(k.conv2_w, k.bn2, blob + o.w2, blob + o.b2, o.C, o.C, 9, 0, s)) != 0) return rc;
            if ((rc = rn_pack_conv(k.conv3_w, k.bn3, blob + o.w3, blob + o.b3, 4 * o.C, o.C, 1, 0, s)) != 0) return rc;
            if (o.proj) {
                // (the projection's own bias lands in the b3 slot for a moment; the kernel after it writes the f64 sum of the two there)
                if ((rc = rn_pack_conv(k.down_w, k.down_bn, blob + o.wp, blob + o.b3, 4 * o.C, o.Cin, 1, 0, s)) != 0) return rc;
                BnBias2 q;
                q.g3 = k.bn3.weight; q.b3 = k.bn3.bias; q.m3 = k.bn3.running_mean; q.v3 = k.bn3.running_var; q.eps3 = k.bn3.eps;
                q.gp = k.down_bn.weight; q.bp = k.down_bn.bias; q.mp = k.down_bn.running_mean; q.vp = k.down_bn.running_var;
                q.epsp = k.down_bn.eps; q.bias = blob + o.b3; q.C = 4 * o.C;
                hipLaunchKernelGGL(bneck_bias2_kernel, dim3((unsigned)((q.C + 255) / 256)), dim3(256), 0, s, q);
            }
        }
    hipLaunchKernelGGL(resnet_copy_kernel, dim3(64), dim3(256), 0, s, p->linear_w, blob + L.lin_w, (long long)RN_LIN * BN_FEAT);
    hipLaunchKernelGGL(resnet_copy_kernel, dim3(1), dim3(256), 0, s, p->linear_b, blob + L.lin_b, (long long)RN_LIN);
    hipLaunchKernelGGL(resnet_copy_kernel, dim3(16), dim3(256), 0, s, p->fc_w, blob + L.fc_w, (long long)d.classes * RN_LIN);
    hipLaunchKernelGGL(resnet_copy_kernel, dim3(1), dim3(256), 0, s, p->fc_b, blob + L.fc_b, (long long)d.classes);
    return vt_check(hipGetLastError(), "vt_resnet_bneck_pack");
}

int vt_resnet_bneck_fwd(const float *x, int n_img, int H, int W, const vt_resnet_bneck_params *dims, const float *blob, void *workspace,
                        size_t workspace_bytes, float *out, float *const *stage_out, void *stream) {
    if (!x || !dims || !blob || !workspace || !out) return vt_fail(VT_ERR_INVALID, "vt_resnet_bneck_fwd: null argument");
    const RnDims d = bn_dims_of(dims, n_img, H, W);
    if (!bn_dims_ok(d)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_resnet_bneck_fwd: shape not covered (vt_resnet_bneck_supported)");
    if (workspace_bytes < vt_resnet_bneck_workspace_bytes(dims->blocks_num, dims->num_classes, n_img, H, W))
        return vt_fail(VT_ERR_WORKSPACE, "vt_resnet_bneck_fwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const long long buf = bn_buf_floats(d);
    float *ws = reinterpret_cast<float *>(workspace);
    float *cur = ws, *t1 = ws + buf, *t2 = ws + 2 * buf, *nxt = ws + 3 * buf;
    const BnLayout L = bn_layout(d.blocks, d.classes, -1, -1, nullptr);
    int h, w;
    rn_stage_hw(d, 0, h, w);
    {
        RnStem p;
        p.x = x; p.wfrag = blob + L.stem_w; p.bias = blob + L.stem_b; p.out = cur;
        p.H = H; p.W = W; p.Hs = rn_half(H); p.Ws = rn_half(W); p.Hp = h; p.Wp = w;
        p.tiles_x = (w + 3) / 4; p.tiles_y = (h + 3) / 4;
        hipLaunchKernelGGL(resnet_stem_kernel, dim3((unsigned)(n_img * p.tiles_x * p.tiles_y)), dim3(192), 0, s, p);
    }
    for (int st = 0; st < 4; ++st) {
        for (int b = 0; b < d.blocks[st]; ++b) {
            BnBlockOff o;
            bn_layout(d.blocks, d.classes, st, b, &o);
            const int k3 = (o.C + (o.proj ? o.Cin : 0)) / 8;
            if (!rn_split_ok(o.Cin, bn_waves(o.Cin / 8)) || !rn_split_ok(o.C, rn_waves(o.C)) || k3 % bn_waves(k3) != 0)
                return vt_fail(VT_ERR_UNSUPPORTED, "vt_resnet_bneck_fwd: a layer's K split would drop input channels");
            const int ho = o.stride == 2 ? rn_half(h) : h, wo = o.stride == 2 ? rn_half(w) : w;
            BnGemm a{};
            a.in0 = cur; a.w0 = blob + o.w1; a.bias = blob + o.b1; a.out = t1;
            a.K0 = o.Cin; a.K1 = 0; a.Cout = o.C; a.Hi = h; a.Wi = w; a.Ho = h; a.Wo = w; a.stride = 1; a.P = n_img * h * w;
            bn_launch_gemm(a, s);
            RnConv c{};
            c.in = t1; c.wfrag = blob + o.w2; c.bias = blob + o.b2; c.out = t2;
            c.Cin = o.C; c.Cout = o.C; c.Hi = h; c.Wi = w; c.Ho = ho; c.Wo = wo; c.P = n_img * ho * wo;
            bn_launch_conv3x3(c, o.stride, s);
            BnGemm e{};
            e.in0 = t2; e.w0 = blob + o.w3; e.bias = blob + o.b3; e.out = nxt;
            e.K0 = o.C; e.Cout = 4 * o.C; e.Hi = h; e.Wi = w; e.Ho = ho; e.Wo = wo; e.stride = o.stride; e.P = n_img * ho * wo;
            if (o.proj) { e.in1 = cur; e.w1 = blob + o.wp; e.K1 = o.Cin; }
            else e.res = cur;
            bn_launch_gemm(e, s);
            float *t = cur; cur = nxt; nxt = t;
            h = ho; w = wo;
        }
        if (stage_out && stage_out[st])
            hipLaunchKernelGGL(resnet_copy_kernel, dim3(1024), dim3(256), 0, s, cur, stage_out[st], (long long)n_img * h * w * 4 * rn_width(st));
    }
    {
        RnTail p;
        p.in = cur; p.lw = blob + L.lin_w; p.lb = blob + L.lin_b; p.fw = blob + L.fc_w; p.fb = blob + L.fc_b;
        p.out = out; p.HW = h * w; p.classes = d.classes;
        hipLaunchKernelGGL(resnet_tail_kernel<BN_FEAT>, dim3((unsigned)n_img), dim3(256), 0, s, p);
    }
    return vt_check(hipGetLastError(), "vt_resnet_bneck_fwd");
}

}  // extern "C"
