"""PointNet dense layers: row-wise linear, ResnetBlockFC forward / backward / weight gradients, the fused MLP."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, _c, keep_for_graph


def linear_rows(x, weight, bias=None):
    """nn.Linear over the rows of x [..., Cin] -> [..., Cout]."""
    x = _c(x)
    Cout, Cin = weight.shape
    out = torch.empty(x.shape[:-1] + (Cout,), dtype=torch.float32, device=x.device)
    check(_lib.load().vt_linear_rows(dev_ptr(x, "x"), dev_ptr(_c(weight), "weight"),
                                     dev_ptr(_c(bias) if bias is not None else None, "bias"),
                                     x.numel() // Cin, Cin, Cout, dev_ptr(out, "out"), stream_ptr()), "vt_linear_rows")
    return out


def resblock_fc(x1, x2, fc_0, fc_1, shortcut):
    """ResnetBlockFC (layers.py:8-50) on the rows of cat([x1, x2], -1) (x2 may be None); the arguments after x2 are
    the block's nn.Linear modules (shortcut None = identity)."""
    x1 = _c(x1)
    x2 = _c(x2) if x2 is not None else None
    C1, C2 = x1.shape[-1], (x2.shape[-1] if x2 is not None else 0)
    H, O = fc_0.weight.shape[0], fc_1.weight.shape[0]
    out = torch.empty(x1.shape[:-1] + (O,), dtype=torch.float32, device=x1.device)
    check(_lib.load().vt_resblock_fc(dev_ptr(x1, "x1"), C1, dev_ptr(x2, "x2"), C2, x1.numel() // C1,
                                     dev_ptr(_c(fc_0.weight), "fc_0.weight"), dev_ptr(_c(fc_0.bias), "fc_0.bias"),
                                     dev_ptr(_c(fc_1.weight), "fc_1.weight"), dev_ptr(_c(fc_1.bias), "fc_1.bias"),
                                     dev_ptr(_c(shortcut.weight) if shortcut is not None else None, "shortcut.weight"),
                                     H, O, dev_ptr(out, "out"), stream_ptr()), "vt_resblock_fc")
    return out


def resblock_fc_bwd(x1, x2, fc_0_w, fc_0_b, fc_1_w, shortcut_w, dout, want_dx2=True):
    """vt_resblock_fc_bwd: (dx1, dx2 or None, act = relu(h) [.., H], dh [.., H])."""
    x1, dout = _c(x1), _c(dout)
    x2 = _c(x2) if x2 is not None else None
    C1, C2 = x1.shape[-1], (x2.shape[-1] if x2 is not None else 0)
    H, O = fc_0_w.shape[0], fc_1_w.shape[0]
    N = x1.numel() // C1
    dev = x1.device
    dx1 = torch.empty_like(x1)
    dx2 = torch.empty_like(x2) if (x2 is not None and want_dx2) else None
    act = torch.empty(x1.shape[:-1] + (H,), dtype=torch.float32, device=dev)
    dh = torch.empty_like(act)
    check(_lib.load().vt_resblock_fc_bwd(dev_ptr(x1, "x1"), C1, dev_ptr(x2, "x2"), C2, N, dev_ptr(_c(fc_0_w), "fc_0.weight"),
                                         dev_ptr(_c(fc_0_b), "fc_0.bias"), dev_ptr(_c(fc_1_w), "fc_1.weight"),
                                         dev_ptr(_c(shortcut_w) if shortcut_w is not None else None, "shortcut.weight"), H, O,
                                         dev_ptr(dout, "dout"), dev_ptr(dx1, "dx1"), dev_ptr(dx2, "dx2"), dev_ptr(act, "act"),
                                         dev_ptr(dh, "dh"), stream_ptr()), "vt_resblock_fc_bwd")
    return dx1, dx2, act, dh


def rows_wgrad(g, x1, x2=None, relu_x=False, want_bias=True):
    """vt_rows_wgrad: dW [M, K] = g^T [x1 | x2] over the rows (x relu'd when ``relu_x``), db [M] = column sums of g."""
    g, x1 = _c(g), _c(x1)
    x2 = _c(x2) if x2 is not None else None
    M, C1, C2 = g.shape[-1], x1.shape[-1], (x2.shape[-1] if x2 is not None else 0)
    N = g.numel() // M
    lib = _lib.load()
    dev = g.device
    wsb = lib.vt_rows_wgrad_workspace_bytes(N, M, C1 + C2)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    dW = torch.empty((M, C1 + C2), dtype=torch.float32, device=dev)
    db = torch.empty((M,), dtype=torch.float32, device=dev) if want_bias else None
    check(lib.vt_rows_wgrad(dev_ptr(g, "g"), M, dev_ptr(x1, "x1"), C1, dev_ptr(x2, "x2"), C2, int(relu_x), N,
                            ctypes.c_void_p(ws.data_ptr()), wsb, dev_ptr(dW, "dW"), dev_ptr(db, "db"), stream_ptr()), "vt_rows_wgrad")
    return dW, db


def resblock_wgrad(x1, x2, act, dh, dout, has_shortcut):
    """The three weight gradients of a ResnetBlockFC in one pair of launches (vt_resblock_wgrad): returns (dw0, db0, dw1, db1, dws or
    None), or None where the block is too wide for it (use rows_wgrad per product)."""
    x1, act, dh, dout = _c(x1), _c(act), _c(dh), _c(dout)
    x2 = _c(x2) if x2 is not None else None
    C1, C2 = x1.shape[-1], (x2.shape[-1] if x2 is not None else 0)
    H, O = act.shape[-1], dout.shape[-1]
    N = x1.numel() // C1
    lib = _lib.load()
    wsb = lib.vt_resblock_wgrad_workspace_bytes(N, C1 + C2, H, O, 1 if has_shortcut else 0)
    if not wsb:
        return None
    dev = x1.device
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    dw0 = torch.empty((H, C1 + C2), dtype=torch.float32, device=dev)
    db0 = torch.empty((H,), dtype=torch.float32, device=dev)
    dw1 = torch.empty((O, H), dtype=torch.float32, device=dev)
    db1 = torch.empty((O,), dtype=torch.float32, device=dev)
    dws = torch.empty((O, C1 + C2), dtype=torch.float32, device=dev) if has_shortcut else None
    check(lib.vt_resblock_wgrad(dev_ptr(x1, "x1"), C1, dev_ptr(x2, "x2"), C2, N, dev_ptr(act, "act"), dev_ptr(dh, "dh"), dev_ptr(dout, "dout"),
                                H, O, ctypes.c_void_p(ws.data_ptr()), wsb, dev_ptr(dw0, "dw0"), dev_ptr(db0, "db0"), dev_ptr(dw1, "dw1"),
                                dev_ptr(db1, "db1"), dev_ptr(dws, "dws"), stream_ptr()), "vt_resblock_wgrad")
    return dw0, db0, dw1, db1, dws


def pointnet_mlp_weights(fc_pos, blocks, fc_c):
    """The weight pointers vt_pointnet_mlp_fused takes, gathered once: (ctypes pointer array of the 25 block tensors, those tensors,
    [fc_pos.weight, fc_pos.bias, fc_c.weight, fc_c.bias]); valid while the parameters keep their storage."""
    ws = []
    for blk in blocks:
        ws += [_c(blk.fc_0.weight), _c(blk.fc_0.bias), _c(blk.fc_1.weight), _c(blk.fc_1.bias), _c(blk.shortcut.weight)]
    ptrs = (ctypes.c_void_p * len(ws))(*[t.data_ptr() for t in ws])
    return ptrs, ws, [_c(fc_pos.weight), _c(fc_pos.bias), _c(fc_c.weight), _c(fc_c.bias)]


def pointnet_mlp_fused(p, vi, fc_pos, blocks, fc_c, want_grid=False, weights=None, zeroed_grid=None):
    """fc_pos -> block 0 -> 4 x (pool over the point's cell, concat, block) -> fc_c for one voxel index in ONE launch
    (vt_pointnet_mlp_fused; inference): [B,T,c_dim], bit-identical to the launch-per-layer path.  ``want_grid``: instead of the
    point features, the voxeliser's channels-last mean grid [B,R,R,R,c_dim] and its GroupNorm partial sums (part, nblk) from
    the same kernel (scatter_mean + channel_stats without their launches and the pass over the grid); ``zeroed_grid``: that grid,
    already cleared (VoxelIndex(clear=...))."""
    p = _c(p.float())
    B, T, _ = p.shape
    c_dim = fc_c.weight.shape[0]
    ptrs, ws, keep = weights if weights is not None else pointnet_mlp_weights(fc_pos, blocks, fc_c)
    lib = _lib.load()
    scratch = torch.empty((B, T, 32), dtype=torch.float32, device=p.device)
    out = grid = part = None
    nblk = 0
    if want_grid:
        R = vi.R
        if zeroed_grid is not None and tuple(zeroed_grid.shape) != (B, R, R, R, c_dim):
            raise VtError(f"pointnet_mlp_fused: zeroed_grid must be {(B, R, R, R, c_dim)}, got {tuple(zeroed_grid.shape)}")
        grid = zeroed_grid if zeroed_grid is not None else torch.zeros((B, R, R, R, c_dim), dtype=torch.float32, device=p.device)
        nblk = lib.vt_pointnet_mlp_stat_blocks(B, T)
        part = torch.empty((B, nblk, c_dim, 2), dtype=torch.float32, device=p.device)
    else:
        out = torch.empty((B, T, c_dim), dtype=torch.float32, device=p.device)
    check(lib.vt_pointnet_mlp_fused(dev_ptr(p, "p"), B, T, dev_ptr(vi.order, "order", I32), dev_ptr(vi.seg_lo, "seg_lo", I32),
                                    dev_ptr(vi.seg_hi, "seg_hi", I32), dev_ptr(keep[0], "fc_pos.weight"), dev_ptr(keep[1], "fc_pos.bias"),
                                    ptrs, 32, dev_ptr(keep[2], "fc_c.weight"), dev_ptr(keep[3], "fc_c.bias"), c_dim,
                                    dev_ptr(scratch, "scratch"), dev_ptr(out, "out"), dev_ptr(vi.idx, "idx", I32) if want_grid else None,
                                    vi.R if want_grid else 0, dev_ptr(grid, "grid"), dev_ptr(part, "part"), stream_ptr()), "vt_pointnet_mlp_fused")
    keep_for_graph(scratch, *ws, *keep)
    return (grid, (part, nblk)) if want_grid else out
