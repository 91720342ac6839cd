// resnet2d.hip -- the tactile feature encoder (reference ``ResNet`` with BasicBlocks, src/layers.py:54-207; ``encoder_img: Resnet18``
// of the shipped VTacO / VTacOH configs, Resnet34 of the registry) in eval mode on hand-written kernels: vt_resnet_pack, vt_resnet_fwd.
//
// Eval-mode BatchNorm is an affine map per channel, so vt_resnet_pack folds it into the conv in front of it (f64: w * gamma /
// sqrt(var + eps), bias beta - mean * gamma / sqrt(var + eps)) and writes the folded weights in MFMA fragment order; no forward kernel
// reads a BatchNorm tensor.  The forward is 1 + 2 * (number of blocks) + 1 launches (18 for Resnet18):
//
//   stem   7x7 stride 2 on the NCHW input, bias, ReLU AND the 3x3 stride-2 max-pool: a workgroup owns 4 x 4 pooled pixels, computes
//          the 9 x 9 stem pixels under them (three waves of 32) into LDS and pools from there (27 % of the stem recomputed at the
//          tile seams, 1.7 % of the net's work, for one launch and one 4x larger tensor less).  K = 3 x 7 x 8 (kx padded to 8).
//   conv   ONE implicit-GEMM template for every 3x3 conv, stride 1 or 2: D[co][px] += W[co][ci][tap] * X[px * stride + tap][ci] on
//          the exact-f32 matrix core (v_mfma_f32_32x32x2f32, A = 32 output channels, B = 32 output pixels).  Pixels are the flat
//          index (image, y, x), so H and W are arbitrary: a tile is 32 consecutive pixels, the last one ragged, zero padding is a
//          predicate on the tap's coordinates.  Activations are channels-last, so a lane's B operands of a tap -- 4 consecutive
//          channels of its pixel, the k-steps pairing channel c with c + 4 -- are ONE 16-byte load straight into registers, and so
//          are its A operands (fragment order): no staging, no barrier inside the K loop.  A workgroup owns 32 pixels x 64 output
//          channels and splits K over its 4 or 8 waves by input channel; the partial sums meet in LDS in wave order (fixed:
//          bit-reproducible, and independent of the number of images).  Epilogue: bias, residual (the block's input or the
//          projected skip), ReLU, 16-byte channels-last stores.
//          The 1x1 stride-2 projection of a stage's first block reads exactly the centre tap of that block's 3x3 stride-2 conv1:
//          it rides in the same launch as a second accumulator pair and leaves the skip tensor for conv2's epilogue.
//   tail   global average pool, Linear(512, 100), Linear(100, num_classes): one workgroup per image, f64 accumulators.
//
// Arithmetic: exact f32 everywhere (no f16 range to leave: folded weights or activations beyond 65504 are as good as any others).
// A device-side barrier between layers was measured and lost (plane_unet.hip): the layers are launches.
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
    const float *in;         // [n_img][HW][512]
    const float *lw, *lb, *fw, *fb;
    float *out;              // [n_img][classes]
    int HW, classes;
};

__global__ void __launch_bounds__(256) resnet_tail_kernel(RnTail p) {
    __shared__ double pooled[RN_FEAT];
    __shared__ double hid[RN_LIN];
    const int img = blockIdx.x;
    for (int c = threadIdx.x; c < RN_FEAT; c += 256) {
        double sum = 0.0;
        const float *q = p.in + (unsigned)(img * p.HW * RN_FEAT + c);
        for (int px = 0; px < p.HW; ++px) sum += (double)q[(unsigned)(px * RN_FEAT)];
        pooled[c] = (double)(float)(sum / (double)p.HW);               // (the reference's pooled tensor is f32)
    }
    __syncthreads();
    if (threadIdx.x < RN_LIN) {
        double a = (double)p.lb[threadIdx.x];
        const float *w = p.lw + threadIdx.x * RN_FEAT;
        for (int k = 0; k < RN_FEAT; ++k) a = fma((double)w[k], pooled[k], a);
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

extern "C" {

int vt_resnet_supported(const int32_t *blocks_num, int num_classes, int n_img, int H, int W) {
    if (!blocks_num) return 0;
    return rn_dims_ok(rn_dims_of(blocks_num, num_classes, n_img, H, W)) ? 1 : 0;
}

size_t vt_resnet_blob_bytes(const int32_t *blocks_num, int num_classes) {
    if (!blocks_num) return 0;
    const RnDims d = rn_dims_of(blocks_num, num_classes, 1, 64, 64);
    if (!rn_net_ok(d.blocks, d.classes)) return 0;
    return (size_t)rn_layout(d.blocks, d.classes, -1, -1, nullptr).total * sizeof(float);
}

size_t vt_resnet_workspace_bytes(const int32_t *blocks_num, int num_classes, int n_img, int H, int W) {
    if (!blocks_num) return 0;
    const RnDims d = rn_dims_of(blocks_num, num_classes, n_img, H, W);
    if (!rn_dims_ok(d)) return 0;
    return (size_t)(4 * rn_buf_floats(d)) * sizeof(float);
}

int vt_resnet_pack(const vt_resnet_params *p, float *blob, size_t blob_bytes, void *stream) {
    if (!p || !blob) return vt_fail(VT_ERR_INVALID, "vt_resnet_pack: null argument");
    const size_t need = vt_resnet_blob_bytes(p->blocks_num, p->num_classes);
    if (!need) return vt_fail(VT_ERR_UNSUPPORTED, "vt_resnet_pack: blocks_num entries 1..VT_RESNET_MAX_BLOCKS, num_classes >= 1");
    if (blob_bytes < need) return vt_fail(VT_ERR_WORKSPACE, "vt_resnet_pack: blob too small");
    if (!p->linear_w || !p->linear_b || !p->fc_w || !p->fc_b) return vt_fail(VT_ERR_INVALID, "vt_resnet_pack: null linear / fc tensor");
    hipStream_t s = (hipStream_t)stream;
    const RnDims d = rn_dims_of(p->blocks_num, p->num_classes, 1, 64, 64);
    const RnLayout L = rn_layout(d.blocks, d.classes, -1, -1, nullptr);
    int rc = rn_pack_conv(p->conv1_w, p->bn1, blob + L.stem_w, blob + L.stem_b, 64, 3, 49, 1, s);
    if (rc != 0) return rc;
    for (int st = 0; st < 4; ++st)
        for (int b = 0; b < d.blocks[st]; ++b) {
            RnBlockOff o;
            rn_layout(d.blocks, d.classes, st, b, &o);
            const vt_resnet_block &k = p->block[st][b];
            if ((rc = rn_pack_conv(k.conv1_w, k.bn1, blob + o.w1, blob + o.b1, o.Cout, o.Cin, 9, 0, s)) != 0) return rc;
            if ((rc = rn_pack_conv(k.conv2_w, k.bn2, blob + o.w2, blob + o.b2, o.Cout, o.Cout, 9, 0, s)) != 0) return rc;
            if (o.proj && (rc = rn_pack_conv(k.down_w, k.down_bn, blob + o.wp, blob + o.bp, o.Cout, o.Cin, 1, 0, s)) != 0) return rc;
        }
    hipLaunchKernelGGL(resnet_copy_kernel, dim3(64), dim3(256), 0, s, p->linear_w, blob + L.lin_w, (long long)RN_LIN * RN_FEAT);
    hipLaunchKernelGGL(resnet_copy_kernel, dim3(1), dim3(256), 0, s, p->linear_b, blob + L.lin_b, (long long)RN_LIN);
    hipLaunchKernelGGL(resnet_copy_kernel, dim3(16), dim3(256), 0, s, p->fc_w, blob + L.fc_w, (long long)d.classes * RN_LIN);
    hipLaunchKernelGGL(resnet_copy_kernel, dim3(1), dim3(256), 0, s, p->fc_b, blob + L.fc_b, (long long)d.classes);
    return vt_check(hipGetLastError(), "vt_resnet_pack");
}

int vt_resnet_fwd(const float *x, int n_img, int H, int W, const vt_resnet_params *dims, const float *blob, void *workspace,
                  size_t workspace_bytes, float *out, void *stream) {
    if (!x || !dims || !blob || !workspace || !out) return vt_fail(VT_ERR_INVALID, "vt_resnet_fwd: null argument");
    const RnDims d = rn_dims_of(dims->blocks_num, dims->num_classes, n_img, H, W);
    if (!rn_dims_ok(d)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_resnet_fwd: shape not covered (vt_resnet_supported)");
    if (workspace_bytes < vt_resnet_workspace_bytes(dims->blocks_num, dims->num_classes, n_img, H, W))
        return vt_fail(VT_ERR_WORKSPACE, "vt_resnet_fwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const long long buf = rn_buf_floats(d);
    float *ws = reinterpret_cast<float *>(workspace);
    float *cur = ws, *mid = ws + buf, *skip = ws + 2 * buf, *nxt = ws + 3 * buf;
    const RnLayout L = rn_layout(d.blocks, d.classes, -1, -1, nullptr);
    int h, w;
    rn_stage_hw(d, 0, h, w);
    {
        RnStem p;
        p.x = x; p.wfrag = blob + L.stem_w; p.bias = blob + L.stem_b; p.out = cur;
        p.H = H; p.W = W; p.Hs = rn_half(H); p.Ws = rn_half(W); p.Hp = h; p.Wp = w;
        p.tiles_x = (w + 3) / 4; p.tiles_y = (h + 3) / 4;
        hipLaunchKernelGGL(resnet_stem_kernel, dim3((unsigned)(n_img * p.tiles_x * p.tiles_y)), dim3(192), 0, s, p);
    }
    for (int st = 0; st < 4; ++st)
        for (int b = 0; b < d.blocks[st]; ++b) {
            RnBlockOff o;
            rn_layout(d.blocks, d.classes, st, b, &o);
            if (!rn_split_ok(o.Cin, rn_waves(o.Cin)) || !rn_split_ok(o.Cout, rn_waves(o.Cout)))
                return vt_fail(VT_ERR_UNSUPPORTED, "vt_resnet_fwd: a layer's K split would drop input channels");
            const int stride = o.proj ? 2 : 1;
            const int ho = stride == 2 ? rn_half(h) : h, wo = stride == 2 ? rn_half(w) : w;
            RnConv c{};
            c.in = cur; c.wfrag = blob + o.w1; c.bias = blob + o.b1; c.res = nullptr; c.out = mid;
            c.wproj = o.proj ? blob + o.wp : nullptr; c.bproj = o.proj ? blob + o.bp : nullptr; c.skip = o.proj ? skip : nullptr;
            c.Cin = o.Cin; c.Cout = o.Cout; c.Hi = h; c.Wi = w; c.Ho = ho; c.Wo = wo; c.P = n_img * ho * wo;
            rn_launch_conv(c, stride, s);
            RnConv e{};
            e.in = mid; e.wfrag = blob + o.w2; e.bias = blob + o.b2; e.res = o.proj ? skip : cur; e.out = nxt;
            e.Cin = o.Cout; e.Cout = o.Cout; e.Hi = ho; e.Wi = wo; e.Ho = ho; e.Wo = wo; e.P = n_img * ho * wo;
            rn_launch_conv(e, 1, s);
            float *t = cur; cur = nxt; nxt = t;
            h = ho; w = wo;
        }
    {
        RnTail p;
        p.in = cur; p.lw = blob + L.lin_w; p.lb = blob + L.lin_b; p.fw = blob + L.fc_w; p.fb = blob + L.fc_b;
        p.out = out; p.HW = h * w; p.classes = d.classes;
        hipLaunchKernelGGL(resnet_tail_kernel, dim3((unsigned)n_img), dim3(256), 0, s, p);
    }
    return vt_check(hipGetLastError(), "vt_resnet_fwd");
}

}  // extern "C"
