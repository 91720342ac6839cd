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
#include "resnet2d_net.h"

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
        hipLaunchKernelGGL(resnet_tail_kernel<RN_FEAT>, dim3((unsigned)n_img), dim3(256), 0, s, p);
    }
    return vt_check(hipGetLastError(), "vt_resnet_fwd");
}

}  // extern "C"
