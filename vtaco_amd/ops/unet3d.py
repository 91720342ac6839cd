"""The 3-D U-Net's channels-last building blocks: convolutions, GroupNorm, pooling and the fused forward."""
import ctypes
import os

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, _c, keep_for_graph
from .decode import PRECISIONS, SPLIT_PRECISIONS


def conv3d_pack(weight, precision="f32"):
    """Fragment-ordered copy of a [Cout,Cin,3,3,3] conv weight: f32 (vt_conv3d_pack), split-bf16 hi/lo fragments
    (vt_conv3d_pack_bf16x3; same size) or split-f16 tap-pair fragments (vt_conv3d_pack_f16x3; its own size)."""
    lib = _lib.load()
    Cout, Cin = weight.shape[0], weight.shape[1]
    n = lib.vt_conv3d_packed_floats_f16x3(Cout, Cin) if precision == "f16x3" else lib.vt_conv3d_packed_floats(Cout, Cin)
    if n == 0 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise VtError(f"conv3d_pack: unsupported weight shape {tuple(weight.shape)}")
    w = _c(weight)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    if precision == "f16x3_thin":      # the thin-tile / K-split kernels' fragments (vt_conv3d_pack_bf16x3's layout) with IEEE-half pairs
        check(lib.vt_conv3d_pack_f16x3_thin(dev_ptr(w, "w"), Cout, Cin, dev_ptr(out, "packed"), stream_ptr()), "vt_conv3d_pack_f16x3_thin")
        return out
    if precision not in PRECISIONS:
        raise VtError(f"precision must be one of {PRECISIONS} (got {precision!r})")
    if precision in SPLIT_PRECISIONS:
        name = "vt_conv3d_pack_" + precision
        check(getattr(lib, name)(dev_ptr(w, "w"), Cout, Cin, dev_ptr(out, "packed"), stream_ptr()), name)
    else:
        check(lib.vt_conv3d_pack(dev_ptr(w, "w"), Cout, Cin, dev_ptr(out, "packed"), stream_ptr()), "vt_conv3d_pack")
    return out


def conv3d_pack_t(weight):
    """vt_conv3d_pack_f16x3_t: the split-f16 fragments of the data-gradient conv of a [Cout,Cin,3,3,3] weight (channels swapped, taps
    flipped) without materialising weight.flip(2, 3, 4).transpose(0, 1)."""
    lib = _lib.load()
    Cout, Cin = weight.shape[0], weight.shape[1]
    n = lib.vt_conv3d_packed_floats_f16x3(Cin, Cout)
    if n == 0 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise VtError(f"conv3d_pack_t: unsupported weight shape {tuple(weight.shape)}")
    w = _c(weight)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    check(lib.vt_conv3d_pack_f16x3_t(dev_ptr(w, "w"), Cout, Cin, dev_ptr(out, "packed"), stream_ptr()), "vt_conv3d_pack_f16x3_t")
    return out


def conv3d_pack_up(weight, c_skip):
    """The merged class weights of a decoder-entry conv's upsampled channels (vt_conv3d_pack_f16x3_up): ``weight``
    [Cout, c_skip + C2, 3, 3, 3] of the layer that reads [skip | upsample(low)]; None where the per-parity kernel does not
    take the channel counts."""
    lib = _lib.load()
    Cout, Cin = weight.shape[0], weight.shape[1]
    n = lib.vt_conv3d_up_packed_floats(Cout, Cin - c_skip) if 0 < c_skip < Cin else 0
    if n == 0 or tuple(weight.shape[2:]) != (3, 3, 3):
        return None
    w = _c(weight)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    check(lib.vt_conv3d_pack_f16x3_up(dev_ptr(w, "w"), Cout, Cin, c_skip, dev_ptr(out, "packed"), stream_ptr()), "vt_conv3d_pack_f16x3_up")
    return out


def conv3d_up_covers(C1, C2, B, D, H, W, Cout):
    """Does the per-parity kernel take this decoder-entry layer (vt_conv3d_up_covers)?"""
    return bool(_lib.load().vt_conv3d_up_covers(int(C1), int(C2), int(B), int(D), int(H), int(W), int(Cout)))


def conv3d_gcr_final(x, ss, packed_w_f16x3, final_packed, final_bias):
    """relu(conv3x3x3(x * scale + shift)) followed by the final 1x1x1 conv (32 -> 32) in the same launch
    (vt_conv3d_gcr_f16x3_final); check ``final_fusable`` first."""
    B, D, H, W, C1 = x.shape
    out = torch.empty((B, D, H, W, 32), dtype=torch.float32, device=x.device)
    check(_lib.load().vt_conv3d_gcr_f16x3_final(dev_ptr(x, "x"), C1, None, 0, B, D, H, W, dev_ptr(ss, "scale_shift"),
                                                dev_ptr(packed_w_f16x3, "packed_w"), 32, dev_ptr(final_packed, "final_packed"),
                                                dev_ptr(final_bias, "final_bias"), dev_ptr(out, "out"), stream_ptr()),
          "vt_conv3d_gcr_f16x3_final")
    return out


def conv3d_gcr_final_keep(x, ss, packed_w_f16x3, final_packed, final_bias):
    """As conv3d_gcr_final, returning (y, out): y = relu(conv3x3x3(x * scale + shift)) is stored too
    (vt_conv3d_gcr_f16x3_final_keep: the training forward of the last layer + final conv)."""
    B, D, H, W, C1 = x.shape
    y = torch.empty((B, D, H, W, 32), dtype=torch.float32, device=x.device)
    out = torch.empty((B, D, H, W, 32), dtype=torch.float32, device=x.device)
    check(_lib.load().vt_conv3d_gcr_f16x3_final_keep(dev_ptr(x, "x"), C1, None, 0, B, D, H, W, dev_ptr(ss, "scale_shift"),
                                                     dev_ptr(packed_w_f16x3, "packed_w"), 32, dev_ptr(final_packed, "final_packed"),
                                                     dev_ptr(_c(final_bias), "final_bias"), dev_ptr(out, "out"), dev_ptr(y, "y_keep"),
                                                     stream_ptr()), "vt_conv3d_gcr_f16x3_final_keep")
    return y, out


def conv3d_skip_covers(x, Cout):
    """Does the persistent split-f16 kernel (the one that takes block flags) run a plain layer of this shape?"""
    B, D, H, W, C = x.shape
    return bool(_lib.load().vt_conv3d_stat_blocks_f16x3(B, D, H, W, C, Cout))


def conv3d_gcr_skip(x, ss, packed_w_f16x3, Cout, tile_flags, relu=True):
    """relu?(conv3x3x3(x * scale + shift)) with the taps of the flagged 8^3 blocks skipped (vt_conv3d_gcr_f16x3_skip; plain layers on
    the persistent split-f16 kernel): returns (out, (part, nblk)).  ``tile_flags`` [B, (D/8)(H/8)(W/8)] uint8, 1 = x is zero over the
    block's halo."""
    lib = _lib.load()
    B, D, H, W, C = x.shape
    nblk = lib.vt_conv3d_stat_blocks_f16x3(B, D, H, W, C, Cout)
    if not nblk:
        raise VtError("conv3d_gcr_skip: shape not covered by the split-f16 kernel")
    out = torch.empty((B, D, H, W, Cout), dtype=torch.float32, device=x.device)
    part = torch.empty((B, nblk, Cout, 2), dtype=torch.float32, device=x.device)
    check(lib.vt_conv3d_gcr_f16x3_skip(dev_ptr(x, "x"), C, B, D, H, W, dev_ptr(ss, "scale_shift"), dev_ptr(packed_w_f16x3, "packed_w"), Cout,
                                       int(relu), dev_ptr(tile_flags, "tile_flags", torch.uint8), dev_ptr(out, "out"), dev_ptr(part, "part"),
                                       stream_ptr()), "vt_conv3d_gcr_f16x3_skip")
    return out, (part, nblk)


def final_fusable(x, Cout):
    B, D, H, W, C1 = x.shape
    return bool(_lib.load().vt_conv3d_final_fusable(B, D, H, W, C1, Cout))


def conv1x1_pack_f16x3(weight):
    """Split-half A-operand fragments of a [32,32(,1,1,1)] final conv weight (vt_conv1x1_pack_f16x3), for the fused epilogue of
    vt_conv3d_gcr_f16x3_final."""
    w = _c(weight).reshape(weight.shape[0], -1)
    out = torch.empty(1024, dtype=torch.float32, device=w.device)
    check(_lib.load().vt_conv1x1_pack_f16x3(dev_ptr(w, "w"), w.shape[0], w.shape[1], dev_ptr(out, "packed"), stream_ptr()),
          "vt_conv1x1_pack_f16x3")
    return out


def stat_blocks(V):
    """Blocks of a GroupNorm statistics pass over V voxels: vt_unet3d_fwd's rule (unet3d.hip::stat_blocks), so that the per-layer path
    sums the same blocks in the same order."""
    return max(1, min(1024, V // (16 if V >= 16384 else 8)))


def channel_stats(x):
    """Per-block partial (sum, sumsq) of a channels-last tensor: (part, nblk)."""
    B, D, H, W, C = x.shape
    V = D * H * W
    nblk = stat_blocks(V)
    part = torch.empty((B, nblk, C, 2), dtype=torch.float32, device=x.device)
    check(_lib.load().vt_channel_stats(dev_ptr(x, "x"), B, V, C, nblk, dev_ptr(part, "part"), stream_ptr()), "vt_channel_stats")
    return part, nblk


def gn_scale_shift(x_stats, low_stats, C1, C2, B, voxels, gamma, beta, groups, eps, device):
    """GroupNorm statistics of [x | upsample(low)] from the producers' partial sums -> scale_shift [B,C,2]."""
    ss = torch.empty((B, C1 + C2, 2), dtype=torch.float32, device=device)
    p2, n2 = low_stats if low_stats is not None else (None, 0)
    check(_lib.load().vt_gn_scale_shift(dev_ptr(x_stats[0], "part1"), x_stats[1], C1, dev_ptr(p2, "part2"), n2, C2, B, voxels,
                                        groups, dev_ptr(_c(gamma), "gamma"), dev_ptr(_c(beta), "beta"), float(eps),
                                        dev_ptr(ss, "scale_shift"), stream_ptr()), "vt_gn_scale_shift")
    return ss


def conv3d_gcr(x, low, ss, packed_w, Cout, relu=True, packed_w_bf16x3=None, want_stats=True, packed_w_f16x3=None,
               in_absmax=None, thin_half=False, packed_w_up=None):
    """relu?(conv3x3x3(x_cat * scale + shift)) on channels-last tensors (``ss`` None: no normalisation);
    returns (out, (part, nblk) or None).  With ``packed_w_f16x3`` / ``packed_w_bf16x3`` the convolution runs on the
    16-bit matrix core with split operands where that kernel covers the shape (f16x3 first).  ``thin_half``: ``packed_w_bf16x3``
    holds conv3d_pack(..., "f16x3_thin") fragments and the thin-tile / K-split kernels run on IEEE-half pairs."""
    lib = _lib.load()
    B, D, H, W, C1 = x.shape
    C2 = low.shape[-1] if low is not None else 0
    dev = x.device
    st = stream_ptr()
    out = torch.empty((B, D, H, W, Cout), dtype=torch.float32, device=dev)
    if callable(packed_w) and packed_w_f16x3 is None and packed_w_bf16x3 is None:
        packed_w = packed_w()
    fn, name, pw = lib.vt_conv3d_gcr, "vt_conv3d_gcr", packed_w      # (a callable: packed on demand, only if the f32 kernel runs)
    nblk = lib.vt_conv3d_stat_blocks_f16x3(B, D, H, W, C1 + C2, Cout) if packed_w_f16x3 is not None else 0
    if nblk:
        fn, name, pw = lib.vt_conv3d_gcr_f16x3, "vt_conv3d_gcr_f16x3", packed_w_f16x3
    else:
        ksbytes = lib.vt_conv3d_ksplit_workspace_bytes(B, D, H, W, C1 + C2, Cout) if packed_w_bf16x3 is not None else 0
        if ksbytes:
            # thin level (16^3 / 8^3 of one scene): the input channels dealt over several workgroups per output tile
            nblk = lib.vt_conv3d_stat_blocks_ksplit(B, D, H, W, C1 + C2, Cout)
            part = torch.empty((B, nblk, Cout, 2), dtype=torch.float32, device=dev) if want_stats else None
            ws = torch.empty(ksbytes // 4, dtype=torch.float32, device=dev)
            kfn = lib.vt_conv3d_gcr_f16x3_thin_ksplit if thin_half else lib.vt_conv3d_gcr_bf16x3_ksplit
            check(kfn(dev_ptr(x, "x"), C1, dev_ptr(low, "low"), C2, B, D, H, W, dev_ptr(ss, "scale_shift"),
                      dev_ptr(packed_w_bf16x3, "packed_w"), Cout, int(relu), dev_ptr(out, "out"),
                      dev_ptr(part, "part"), ctypes.c_void_p(ws.data_ptr()), ksbytes, st),
                  "vt_conv3d_gcr_f16x3_thin_ksplit" if thin_half else "vt_conv3d_gcr_bf16x3_ksplit")
            return out, ((part, nblk) if want_stats else None)
        nblk = lib.vt_conv3d_stat_blocks_bf16x3(B, D, H, W, C1 + C2, Cout) if packed_w_bf16x3 is not None else 0
        if nblk:
            fn, name, pw = lib.vt_conv3d_gcr_bf16x3, "vt_conv3d_gcr_bf16x3", packed_w_bf16x3
            if thin_half:
                fn, name = lib.vt_conv3d_gcr_f16x3_thin, "vt_conv3d_gcr_f16x3_thin"
        else:
            nblk = lib.vt_conv3d_stat_blocks(B, D, H, W, C1 + C2, Cout)
            if callable(pw):
                pw = pw()
    part = torch.empty((B, nblk, Cout, 2), dtype=torch.float32, device=dev) if want_stats else None
    if (packed_w_up is not None and low is not None and in_absmax is None and name == "vt_conv3d_gcr_f16x3"
            and lib.vt_conv3d_up_covers(C1, C2, B, D, H, W, Cout)):
        # decoder entry [skip | upsample(low)]: the low channels as a 2x2x2 conv per output parity class (conv3d_pack_up)
        check(lib.vt_conv3d_gcr_f16x3_up(dev_ptr(x, "x"), C1, dev_ptr(low, "low"), C2, B, D, H, W, dev_ptr(ss, "scale_shift"),
                                         dev_ptr(pw, "packed_w"), dev_ptr(packed_w_up, "packed_up"), Cout, int(relu),
                                         dev_ptr(out, "out"), dev_ptr(part, "part"), st), "vt_conv3d_gcr_f16x3_up")
        return out, ((part, nblk) if want_stats else None)
    if in_absmax is not None and name == "vt_conv3d_gcr_f16x3":
        # input far below the half range (output gradients): the kernel rescales it by a power of two around the split
        check(lib.vt_conv3d_gcr_f16x3_scaled(dev_ptr(x, "x"), C1, dev_ptr(low, "low"), C2, B, D, H, W, dev_ptr(ss, "scale_shift"),
                                             dev_ptr(pw, "packed_w"), Cout, int(relu), dev_ptr(out, "out"), dev_ptr(part, "part"),
                                             dev_ptr(in_absmax, "in_absmax"), st), "vt_conv3d_gcr_f16x3_scaled")
        return out, ((part, nblk) if want_stats else None)
    check(fn(dev_ptr(x, "x"), C1, dev_ptr(low, "low"), C2, B, D, H, W, dev_ptr(ss, "scale_shift"),
             dev_ptr(pw, "packed_w"), Cout, int(relu), dev_ptr(out, "out"), dev_ptr(part, "part"), st), name)
    return out, ((part, nblk) if want_stats else None)


def gn_conv3d_relu(x, x_stats, low, low_stats, gamma, beta, groups, packed_w, Cout, eps=1e-5, relu=True,
                   packed_w_bf16x3=None, packed_w_f16x3=None, thin_half=False, packed_w_up=None):
    """relu(conv3x3x3(GroupNorm([x | upsample(low)]))) on channels-last tensors; the statistics
    come from the producers' partial sums.  Returns (out, out_stats)."""
    B, D, H, W, C1 = x.shape
    C2 = low.shape[-1] if low is not None else 0
    ss = gn_scale_shift(x_stats, low_stats if low is not None else None, C1, C2, B, D * H * W, gamma, beta, groups, eps, x.device)
    return conv3d_gcr(x, low, ss, packed_w, Cout, relu, packed_w_bf16x3, packed_w_f16x3=packed_w_f16x3, thin_half=thin_half,
                      packed_w_up=packed_w_up)


def relu_mask(dy, y, want_absmax=False):
    """g = dy where y > 0 else 0 (vt_relu_mask); with ``want_absmax`` also max |g| as a device scalar [1] from the same pass
    (vt_relu_mask_absmax): returns (g, absmax)."""
    dy = _c(dy)
    g = torch.empty_like(dy)
    if want_absmax:
        m = torch.empty(1, dtype=torch.float32, device=dy.device)
        check(_lib.load().vt_relu_mask_absmax(dev_ptr(dy, "dy"), dev_ptr(y, "y"), dev_ptr(g, "g"), dy.numel(), dev_ptr(m, "absmax"),
                                              stream_ptr()), "vt_relu_mask_absmax")
        return g, m
    check(_lib.load().vt_relu_mask(dev_ptr(dy, "dy"), dev_ptr(y, "y"), dev_ptr(g, "g"), dy.numel(), stream_ptr()), "vt_relu_mask")
    return g


def conv1x1_bwd_masked(dout, y, w, want_dw=True, want_db=True):
    """Backward of a 32 -> 32 pointwise conv out = y W^T + b whose input y is the ReLU output of the layer in front of it
    (vt_conv1x1_bwd_masked): returns (g, gmax, dw, db) with g = (y > 0) * (dout W) -- that layer's masked output gradient -- its
    max |g| as a device scalar, dw [32,32] and db [32] (None where not wanted)."""
    lib = _lib.load()
    if w.shape != (32, 32) or y.shape[-1] != 32 or dout.shape != y.shape:
        raise VtError(f"conv1x1_bwd_masked: built for 32 -> 32 channels over equal-shaped dout / y, got {tuple(w.shape)}, {tuple(dout.shape)}, {tuple(y.shape)}")
    dout, y, w = _c(dout), _c(y), _c(w)
    n = y.numel() // 32
    g = torch.empty_like(y)
    gmax = torch.empty(1, dtype=torch.float32, device=y.device)
    dw = torch.empty((32, 32), dtype=torch.float32, device=y.device) if want_dw else None
    db = torch.empty(32, dtype=torch.float32, device=y.device) if want_db else None
    nbytes = lib.vt_conv1x1_bwd_workspace_bytes()
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=y.device)
    check(lib.vt_conv1x1_bwd_masked(dev_ptr(dout, "dout"), dev_ptr(y, "y"), dev_ptr(w, "w"), n, dev_ptr(g, "g"), dev_ptr(gmax, "absmax"),
                                    dev_ptr(dw, "dw"), dev_ptr(db, "db"), ctypes.c_void_p(ws.data_ptr()), nbytes, stream_ptr()),
          "vt_conv1x1_bwd_masked")
    return g, gmax, dw, db


_WGRAD_UP = os.environ.get("VTACO_UNET_WGRAD_UP", "1") != "0"       # A/B knob: decoder-entry weight gradients per parity class


def conv3d_wgrad(x, low, ss, g, precision="f32", g_absmax=None):
    """dW [Cout,Cin,3,3,3] of the 3x3x3 conv over xn = [x | upsample(low)] * scale + shift (vt_conv3d_wgrad).
    ``precision="f16x3"``: vt_conv3d_wgrad_f16x3 where it covers the shape (split-half operands on the f16 matrix core;
    ``g_absmax`` = device scalar max |g| for its power-of-two rescale of g), the f32 kernel elsewhere."""
    lib = _lib.load()
    B, D, H, W, C1 = x.shape
    C2 = low.shape[-1] if low is not None else 0
    Cout = g.shape[-1]
    ubytes = (lib.vt_conv3d_wgrad_f16x3_up_workspace_bytes(B, D, H, W, C1, C2, Cout)
              if precision == "f16x3" and low is not None and _WGRAD_UP else 0)
    if ubytes:
        # a decoder entry: the upsampled channels per output parity class (2 x 2 x 2 taps over the low-resolution grid)
        ws = torch.empty(ubytes // 4, dtype=torch.float32, device=x.device)
        dw = torch.empty((Cout, C1 + C2, 3, 3, 3), dtype=torch.float32, device=x.device)
        check(lib.vt_conv3d_wgrad_f16x3_up(dev_ptr(x, "x"), C1, dev_ptr(low, "low"), C2, B, D, H, W, dev_ptr(ss, "scale_shift"),
                                           dev_ptr(g, "g"), Cout, dev_ptr(g_absmax, "g_absmax"), ctypes.c_void_p(ws.data_ptr()), ubytes,
                                           dev_ptr(dw, "dw"), stream_ptr()), "vt_conv3d_wgrad_f16x3_up")
        return dw
    hbytes = lib.vt_conv3d_wgrad_f16x3_workspace_bytes(B, D, H, W, C1 + C2, Cout) if precision == "f16x3" else 0
    if hbytes:
        ws = torch.empty(hbytes // 4, dtype=torch.float32, device=x.device)
        dw = torch.empty((Cout, C1 + C2, 3, 3, 3), dtype=torch.float32, device=x.device)
        check(lib.vt_conv3d_wgrad_f16x3(dev_ptr(x, "x"), C1, dev_ptr(low, "low"), C2, B, D, H, W, dev_ptr(ss, "scale_shift"),
                                        dev_ptr(g, "g"), Cout, dev_ptr(g_absmax, "g_absmax"), ctypes.c_void_p(ws.data_ptr()), hbytes,
                                        dev_ptr(dw, "dw"), stream_ptr()), "vt_conv3d_wgrad_f16x3")
        return dw
    nbytes = lib.vt_conv3d_wgrad_workspace_bytes(B, D, H, W, C1 + C2, Cout)
    if nbytes == 0:
        raise VtError("conv3d_wgrad: unsupported shape")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    dw = torch.empty((Cout, C1 + C2, 3, 3, 3), dtype=torch.float32, device=x.device)
    check(lib.vt_conv3d_wgrad(dev_ptr(x, "x"), C1, dev_ptr(low, "low"), C2, B, D, H, W, dev_ptr(ss, "scale_shift"),
                              dev_ptr(g, "g"), Cout, ctypes.c_void_p(ws.data_ptr()), nbytes, dev_ptr(dw, "dw"), stream_ptr()),
          "vt_conv3d_wgrad")
    return dw


def conv3d_wgrad_sparse(x, ss, g, tile_flags, g_absmax=None):
    """dW of a layer whose input is exactly zero over the blocks ``tile_flags`` marks (vt_conv3d_wgrad_f16x3_sparse: the taps over the
    other blocks' tiles + the GroupNorm shift's rank-one share); None where the shape is not on that kernel."""
    lib = _lib.load()
    B, D, H, W, C = x.shape
    Cout = g.shape[-1]
    nbytes = lib.vt_conv3d_wgrad_f16x3_sparse_workspace_bytes(B, D, H, W, C, Cout)
    if not nbytes or tile_flags is None or tile_flags.numel() != B * (D // 8) * (H // 8) * (W // 8):
        return None
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    dw = torch.empty((Cout, C, 3, 3, 3), dtype=torch.float32, device=x.device)
    check(lib.vt_conv3d_wgrad_f16x3_sparse(dev_ptr(x, "x"), C, B, D, H, W, dev_ptr(ss, "scale_shift"),
                                           dev_ptr(tile_flags, "tile_flags", torch.uint8), dev_ptr(g, "g"), Cout, dev_ptr(g_absmax, "g_absmax"), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                           dev_ptr(dw, "dw"), stream_ptr()), "vt_conv3d_wgrad_f16x3_sparse")
    return dw


def conv3d_dgrad_xstats(g, packed_t, Cin, g_absmax, x):
    """The data gradient of a plain 'gcr' layer with the GroupNorm backward's sums from its epilogue (vt_conv3d_gcr_f16x3_xstats):
    ``g`` [B,D,H,W,Cout] the masked output gradient, ``packed_t`` = conv3d_pack_t(weight), ``x`` [B,D,H,W,Cin] the layer's input.
    Returns (dxn, (bpart, nblk)) or None where the shape is not on that kernel."""
    lib = _lib.load()
    B, D, H, W, C = g.shape
    nblk = lib.vt_conv3d_xstats_blocks(B, D, H, W, C, int(Cin)) if g_absmax is not None else 0
    if not nblk or tuple(x.shape) != (B, D, H, W, Cin):
        return None
    dxn = torch.empty((B, D, H, W, Cin), dtype=torch.float32, device=g.device)
    part = torch.empty((B, nblk, Cin, 2), dtype=torch.float32, device=g.device)
    check(lib.vt_conv3d_gcr_f16x3_xstats(dev_ptr(_c(g), "g"), C, B, D, H, W, dev_ptr(packed_t, "packed_w"), int(Cin), dev_ptr(g_absmax, "in_absmax"),
                                         dev_ptr(_c(x), "x"), dev_ptr(dxn, "out"), dev_ptr(part, "part"), stream_ptr()), "vt_conv3d_gcr_f16x3_xstats")
    return dxn, (part, nblk)


def gn_bwd(x, x_stats, low, low_stats, dxn, gamma, groups, eps, want_skip=True, want_low=True, mask_skip=False, mask_low=False, bpart=None):
    """GroupNorm backward of xn = GN([x | upsample(low)]) given dxn (vt_gn_bwd): returns
    (dskip or None, dlow or None, dgamma [C], dbeta [C]).  ``mask_skip`` / ``mask_low`` (vt_gn_bwd_masked): x / low is the ReLU
    output of the layer in front and this is its only gradient -- the gradient comes out masked by (x > 0) and the call returns
    (dskip, dlow, dgamma, dbeta, absmax_skip, absmax_low) with the device scalars max |gradient| (None where not asked): what that
    layer's relu_mask(..., want_absmax=True) would compute in a pass of its own.  ``bpart`` = (part, nblk) from conv3d_dgrad_xstats:
    the statistics pass over dxn and x is not launched (vt_gn_bwd_from_part)."""
    B, D, H, W, C1 = x.shape
    C2 = low.shape[-1] if low is not None else 0
    C = C1 + C2
    dev = x.device
    V = D * H * W
    have_part = bpart is not None
    if have_part:
        bpart, nblkb = bpart
    else:
        nblkb = max(1, min(1024, V // 64))
        bpart = torch.empty((B, nblkb, C, 2), dtype=torch.float32, device=dev)
    coef = torch.empty((B, C, 3), dtype=torch.float32, device=dev)
    dgb = torch.empty((B, C, 2), dtype=torch.float32, device=dev)
    dskip = torch.empty_like(x) if want_skip else None
    dlow = torch.empty_like(low) if (low is not None and want_low) else None
    p2, n2 = low_stats if low is not None else (None, 0)
    mask_skip = bool(mask_skip and dskip is not None)
    mask_low = bool(mask_low and dlow is not None)
    am_s = torch.empty(1, dtype=torch.float32, device=dev) if mask_skip else None
    am_l = torch.empty(1, dtype=torch.float32, device=dev) if mask_low else None
    # (dgamma, dbeta) summed over the scenes by the pass that writes the gradients, where there is one
    gsum = torch.empty((2, C), dtype=torch.float32, device=dev) if (dskip is not None or dlow is not None) else None
    fn = _lib.load().vt_gn_bwd_from_part if have_part else _lib.load().vt_gn_bwd_masked
    check(fn(dev_ptr(x, "x"), C1, dev_ptr(low, "low"), C2, B, D, H, W,
             dev_ptr(x_stats[0], "part1"), x_stats[1], dev_ptr(p2, "part2"), n2,
             dev_ptr(_c(dxn), "dxn"), groups, dev_ptr(_c(gamma), "gamma"), float(eps),
             dev_ptr(bpart, "bpart"), nblkb, dev_ptr(coef, "coef"), dev_ptr(dgb, "dgb"),
             dev_ptr(dskip, "dskip"), dev_ptr(dlow, "dlow"), (1 if mask_skip else 0) | (2 if mask_low else 0),
             dev_ptr(am_s, "absmax_skip"), dev_ptr(am_l, "absmax_low"), dev_ptr(gsum, "dgb_sum"), stream_ptr()),
          "vt_gn_bwd_from_part" if have_part else "vt_gn_bwd_masked")
    g = gsum if gsum is not None else dgb.sum(0).t().contiguous()              # [2, C]: dgamma, dbeta as rows
    if mask_skip or mask_low:
        return dskip, dlow, g[0], g[1], am_s, am_l
    return dskip, dlow, g[0], g[1]


def maxpool3d_cl_bwd(x, dy):
    B, D, H, W, C = x.shape
    dx = torch.empty_like(x)
    check(_lib.load().vt_maxpool3d_cl_bwd(dev_ptr(x, "x"), dev_ptr(_c(dy), "dy"), B, D, H, W, C, dev_ptr(dx, "dx"), stream_ptr()),
          "vt_maxpool3d_cl_bwd")
    return dx


def maxpool3d_cl_bwd_fork(y, dskip, dpooled, want_absmax=True):
    """g = (y > 0 ? dskip + maxpool_backward(dpooled) : 0) for a tensor y that feeds a 2x2x2 max-pool and a skip connection
    (vt_maxpool3d_cl_bwd_fork); with ``want_absmax`` also the device scalar max |g|: returns (g, absmax or None)."""
    B, D, H, W, C = y.shape
    dskip, dpooled = _c(dskip), _c(dpooled)
    g = torch.empty_like(y)
    m = torch.empty(1, dtype=torch.float32, device=y.device) if want_absmax else None
    check(_lib.load().vt_maxpool3d_cl_bwd_fork(dev_ptr(y, "y"), dev_ptr(dskip, "dskip"), dev_ptr(dpooled, "dpooled"), B, D, H, W, C,
                                               dev_ptr(g, "g"), dev_ptr(m, "absmax"), stream_ptr()), "vt_maxpool3d_cl_bwd_fork")
    return g, m


def maxpool3d_cl(x):
    B, D, H, W, C = x.shape
    out = torch.empty((B, D // 2, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    check(_lib.load().vt_maxpool3d_cl(dev_ptr(x, "x"), B, D, H, W, C, dev_ptr(out, "out"), stream_ptr()), "vt_maxpool3d_cl")
    return out


def maxpool3d_cl_stats(x):
    """2x2x2 max-pool and the pooled tensor's GroupNorm partial sums from one pass: (out, (part, nblk)) -- what maxpool3d_cl followed by
    channel_stats returns, bit for bit (vt_maxpool3d_cl_stats)."""
    B, D, H, W, C = x.shape
    out = torch.empty((B, D // 2, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    V = (D // 2) * (H // 2) * (W // 2)
    nblk = stat_blocks(V)
    part = torch.empty((B, nblk, C, 2), dtype=torch.float32, device=x.device)
    check(_lib.load().vt_maxpool3d_cl_stats(dev_ptr(x, "x"), B, D, H, W, C, dev_ptr(out, "out"), nblk, dev_ptr(part, "part"), stream_ptr()),
          "vt_maxpool3d_cl_stats")
    return out, (part, nblk)


def conv1x1_cl(x, weight, bias):
    B, D, H, W, Cin = x.shape
    Cout = weight.shape[0]
    out = torch.empty((B, D, H, W, Cout), dtype=torch.float32, device=x.device)
    w = _c(weight).reshape(Cout, Cin)
    check(_lib.load().vt_conv1x1_cl(dev_ptr(x, "x"), B * D * H * W, Cin, dev_ptr(w, "w"),
                                    dev_ptr(_c(bias) if bias is not None else None, "bias"), Cout,
                                    dev_ptr(out, "out"), stream_ptr()), "vt_conv1x1_cl")
    return out


_unet_ws = {}


def unet3d_skip_layers(B, R, params):
    """How many layers of this UNet3D take the block flags at this batch and resolution (vt_unet3d_skip_layers): 0, 1 (the first layer)
    or 2 (the first DoubleConv: the second layer over the blocks whose 12^3 halo is empty)."""
    return int(_lib.load().vt_unet3d_skip_layers(int(B), int(R), ctypes.byref(params)))


def unet3d_fwd(x_cl, params, keep, in_stats=None, tile_flags=None):
    """Whole UNet3D forward (vt_unet3d_fwd).  ``params``: a filled _lib.UnetParams; ``keep``: the
    tensors its pointers refer to (kept alive by the caller).  ``in_stats`` = (part, nblk): GroupNorm partial sums of the
    input that its producer already has (vt_unet3d_fwd_stats: no statistics pass over the input).  ``tile_flags``
    (voxel_tile_flags): the 8^3 blocks over whose halo x is zero -- the first layer skips their taps (vt_unet3d_fwd_skip)."""
    lib = _lib.load()
    B, R = x_cl.shape[0], x_cl.shape[1]
    need = lib.vt_unet3d_workspace_bytes(B, R, ctypes.byref(params))
    if need == 0:
        raise VtError("unet3d_fwd: unsupported configuration: " + lib.vt_last_error().decode())
    key = (x_cl.device, need)
    ws = _unet_ws.get(key)
    if ws is None:
        _unet_ws.clear()
        ws = _unet_ws[key] = torch.empty(need, dtype=torch.uint8, device=x_cl.device)
    keep_for_graph(ws, *keep)
    out = torch.empty((B, R, R, R, params.out_channels), dtype=torch.float32, device=x_cl.device)
    if tile_flags is not None:
        keep_for_graph(tile_flags, *([in_stats[0]] if in_stats is not None else []))
        check(lib.vt_unet3d_fwd_skip(dev_ptr(x_cl, "x"), dev_ptr(in_stats[0], "in_part") if in_stats is not None else None,
                                     int(in_stats[1]) if in_stats is not None else 0, dev_ptr(tile_flags, "tile_flags", torch.uint8), B, R,
                                     ctypes.byref(params), ctypes.c_void_p(ws.data_ptr()), need, dev_ptr(out, "out"), stream_ptr()),
              "vt_unet3d_fwd_skip")
        return out
    if in_stats is not None:
        keep_for_graph(in_stats[0])
        check(lib.vt_unet3d_fwd_stats(dev_ptr(x_cl, "x"), dev_ptr(in_stats[0], "in_part"), int(in_stats[1]), B, R, ctypes.byref(params),
                                      ctypes.c_void_p(ws.data_ptr()), need, dev_ptr(out, "out"), stream_ptr()), "vt_unet3d_fwd_stats")
        return out
    check(lib.vt_unet3d_fwd(dev_ptr(x_cl, "x"), B, R, ctypes.byref(params), ctypes.c_void_p(ws.data_ptr()), need,
                            dev_ptr(out, "out"), stream_ptr()), "vt_unet3d_fwd")
    return out
