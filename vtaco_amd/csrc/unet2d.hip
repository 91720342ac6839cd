// unet2d.hip -- the tactile depth estimator (reference ``UNet``, src/layers.py:322-450; ``encoder_img: UNet`` of the tactile and t2d
// configs: up_mode 'transpose', merge_mode 'concat') in eval mode on hand-written kernels: vt_tactile_unet_pack, vt_tactile_unet_fwd.
//
// Eval-mode BatchNorm is an affine map per channel, so vt_tactile_unet_pack folds it into the conv in front of it (f64:
// w * gamma / sqrt(var + eps), bias (b - mean) * gamma / sqrt(var + eps) + beta; a block's ONE bn module follows both of its convs, so
// the same statistics go into both) and writes the folded weights in MFMA fragment order; no forward kernel reads a BatchNorm tensor.
// The forward is 2 * depth + 3 * (depth - 1) launches (12 for depth 3), no pool, concat, activation or sigmoid kernel among them:
//
//   first  the network's first conv (1..4 input channels, K = 9..36) on the NCHW input: one thread per pixel and 8 output channels,
//          weights in LDS, bias + ReLU, channels-last store.  1 % of the net's work: not worth a matrix-core layout of its own.
//   conv   ONE implicit-GEMM template for every other 3x3 conv: D[co][px] += W[co][ci][tap] * X[px + tap][ci] on the exact-f32 matrix
//          core (v_mfma_f32_32x32x2f32, A = 32 output channels, B = 32 pixels).  A wave owns a 2 x 16 patch of pixels of one image and
//          32 or 64 output channels over the WHOLE of K: no K split, no LDS, no barrier, so the order of every sum is fixed and an
//          image's result does not depend on the batch it is in.  Activations are channels-last: a lane's B operands of a tap -- 4
//          consecutive channels of its pixel, the k-steps pairing channel c with c + 4 -- are one 16-byte load, and so are its A
//          operands (fragment order).  H and W are arbitrary (ragged patches: coordinates clamped for the loads, stores predicated).
//          The up block's first conv reads its K from TWO tensors, the up-conv's result then the skip: the concat is never written.
//          Epilogues: bias + ReLU always; POOL also writes the 2x2 max (the patch holds whole windows: two lane exchanges); FINAL
//          does not store the conv's result at all but conv_final (1x1) + sigmoid of it, NCHW.
//   up     the 2x2 stride-2 transposed conv as four 1x1 GEMMs, one per output parity (blockIdx.y), in one launch of the same template
//          with one tap; the store goes to pixel (2 y + dy, 2 x + dx).
//
// Arithmetic: exact f32 everywhere, like resnet2d.hip (no f16 range to leave).
#include "unet2d_conv.h"

extern "C" {

int vt_tactile_unet_supported(int depth, int start_filts, int in_channels, int num_classes, int n_img, int H, int W) {
    return tu_dims_ok(tu_dims_raw(depth, start_filts, in_channels, num_classes, n_img, H, W)) ? 1 : 0;
}

size_t vt_tactile_unet_blob_bytes(int depth, int start_filts, int in_channels, int num_classes) {
    const TuDims d = tu_dims_raw(depth, start_filts, in_channels, num_classes, 1, 16, 16);
    if (!tu_net_ok(d)) return 0;
    return (size_t)tu_layout(d).total * sizeof(float);
}

size_t vt_tactile_unet_workspace_bytes(int depth, int start_filts, int in_channels, int num_classes, int n_img, int H, int W) {
    const TuDims d = tu_dims_raw(depth, start_filts, in_channels, num_classes, n_img, H, W);
    if (!tu_dims_ok(d)) return 0;
    return (size_t)tu_workspace(d).total * sizeof(float);
}

int vt_tactile_unet_pack(const vt_tactile_unet_params *p, float *blob, size_t blob_bytes, void *stream) {
    if (!p || !blob) return vt_fail(VT_ERR_INVALID, "vt_tactile_unet_pack: null argument");
    const size_t need = vt_tactile_unet_blob_bytes(p->depth, p->start_filts, p->in_channels, p->num_classes);
    if (!need) return vt_fail(VT_ERR_UNSUPPORTED, "vt_tactile_unet_pack: depth 1..5, start_filts 8..64 (multiple of 8), in_channels 1..4, num_classes 1..4");
    if (blob_bytes < need) return vt_fail(VT_ERR_WORKSPACE, "vt_tactile_unet_pack: blob too small");
    hipStream_t s = (hipStream_t)stream;
    const TuDims d = tu_dims_of(p, 1, 16, 16);
    const TuLayout L = tu_layout(d);
    int rc = tu_pack_one(p->down_w[0][0], p->down_b[0][0], &p->down_bn[0], blob + L.first_w, blob + L.first_b, d.sf, d.cin, 9, 2, s);
    if (rc != 0) return rc;
    for (int i = 0; i < d.depth; ++i) {
        const int c = d.sf << i;
        if (i > 0 && (rc = tu_pack_one(p->down_w[i][0], p->down_b[i][0], &p->down_bn[i], blob + L.down[i][0].w, blob + L.down[i][0].b, c, c / 2, 9, 0, s)) != 0) return rc;
        if ((rc = tu_pack_one(p->down_w[i][1], p->down_b[i][1], &p->down_bn[i], blob + L.down[i][1].w, blob + L.down[i][1].b, c, c, 9, 0, s)) != 0) return rc;
    }
    for (int i = d.depth - 2; i >= 0; --i) {
        const int c = d.sf << i;
        if ((rc = tu_pack_one(p->up_tw[i], p->up_tb[i], nullptr, blob + L.upt[i].w, blob + L.upt[i].b, c, 2 * c, 4, 1, s)) != 0) return rc;
        if ((rc = tu_pack_one(p->up_w[i][0], p->up_b[i][0], &p->up_bn[i], blob + L.up[i][0].w, blob + L.up[i][0].b, c, 2 * c, 9, 0, s)) != 0) return rc;
        if ((rc = tu_pack_one(p->up_w[i][1], p->up_b[i][1], &p->up_bn[i], blob + L.up[i][1].w, blob + L.up[i][1].b, c, c, 9, 0, s)) != 0) return rc;
    }
    if ((rc = tu_pack_one(p->final_w, p->final_b, nullptr, blob + L.final_w, blob + L.final_w + VT_TACTILE_UNET_MAX_CLASSES * 64, d.classes, d.sf, 1, 3, s)) != 0)
        return rc;
    return vt_check(hipGetLastError(), "vt_tactile_unet_pack");
}

int vt_tactile_unet_fwd(const float *x, int n_img, int H, int W, const vt_tactile_unet_params *dims, const float *blob, void *workspace,
                        size_t workspace_bytes, float *out, void *stream) {
    if (!x || !dims || !blob || !workspace || !out) return vt_fail(VT_ERR_INVALID, "vt_tactile_unet_fwd: null argument");
    const TuDims d = tu_dims_of(dims, n_img, H, W);
    if (!tu_dims_ok(d)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_tactile_unet_fwd: shape not covered (vt_tactile_unet_supported)");
    const TuWs ws = tu_workspace(d);
    if (workspace_bytes < (size_t)ws.total * sizeof(float)) return vt_fail(VT_ERR_WORKSPACE, "vt_tactile_unet_fwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float *base = reinterpret_cast<float *>(workspace);
    const TuLayout L = tu_layout(d);
    const float *fw = blob + L.final_w;
    auto second = [&](TuConv c, float *dst, float *pooled, bool last) {
        if (last) { c.fw = fw; c.fout = out; c.classes = d.classes; tu_launch<TU_FINAL>(c, s); }
        else if (pooled) { c.out = dst; c.pooled = pooled; tu_launch<TU_POOL>(c, s); }
        else { c.out = dst; tu_launch<TU_PLAIN>(c, s); }
    };
    {
        TuFirst f;
        f.x = x; f.w = blob + L.first_w; f.bias = blob + L.first_b; f.out = base + ws.mid[0];
        f.cin = d.cin; f.Cout = d.sf; f.H = H; f.W = W; f.P = n_img * H * W;
        hipLaunchKernelGGL(tu_first_kernel, dim3((unsigned)((f.P + 255) / 256), (unsigned)(d.sf / 8)), dim3(256), 0, s, f);
    }
    for (int i = 0; i < d.depth; ++i) {
        const int c = d.sf << i, h = H >> i, w = W >> i;
        if (i > 0) {
            TuConv a = tu_conv_args(base + ws.pooled[i - 1], c / 2, nullptr, 0, blob, L.down[i][0], c, n_img, h, w);
            a.out = base + ws.mid[i];
            tu_launch<TU_PLAIN>(a, s);
        }
        const bool bottom = i == d.depth - 1;
        second(tu_conv_args(base + ws.mid[i], c, nullptr, 0, blob, L.down[i][1], c, n_img, h, w), base + ws.skip[i],
               bottom ? nullptr : base + ws.pooled[i], bottom && i == 0);
    }
    const float *cur = base + ws.skip[d.depth - 1];
    for (int i = d.depth - 2; i >= 0; --i) {
        const int c = d.sf << i, h = H >> i, w = W >> i;
        TuConv u = tu_conv_args(cur, 2 * c, nullptr, 0, blob, L.upt[i], c, n_img, h / 2, w / 2);
        u.out = base + ws.up[i];
        tu_launch<TU_UP>(u, s);
        TuConv a = tu_conv_args(base + ws.up[i], c, base + ws.skip[i], c, blob, L.up[i][0], c, n_img, h, w);
        a.out = base + ws.mid[i];
        tu_launch<TU_PLAIN>(a, s);
        second(tu_conv_args(base + ws.mid[i], c, nullptr, 0, blob, L.up[i][1], c, n_img, h, w), base + ws.out[i], nullptr, i == 0);
        cur = base + ws.out[i];
    }
    return vt_check(hipGetLastError(), "vt_tactile_unet_fwd");
}

}  // extern "C"
