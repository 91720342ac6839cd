"""The 32/32 decoder under autograd: saved activations, backward, weight gradients and the grid scatter."""
import ctypes
import os

import torch

from ._base import _lib, check, dev_ptr, stream_ptr, I32, _c
from .voxel import VoxelIndex


def decode_save_buffer(total_points, device):
    n = _lib.load().vt_decode_save_bytes(total_points) // 4
    return torch.empty(n, dtype=torch.float32, device=device)


def decode_bwd(grid_shape, blob_t, grad_out, save, pts=None, lattice=None, with_c_img=False, c_img=None,
               padding=0.1, want_grid_grad=True, grad_out2=None):
    """vt_decode_bwd + vt_decode_wgrad (with ``grad_out2``, the contact head's logit gradient: the _contact forms).
    Returns (grad_grid [B,C,R,R,R] channels-last strided or None, grad_c_img [B,N,C] or None, flat parameter gradients)."""
    lib = _lib.load()
    B, C, R = grid_shape[0], grid_shape[1], grid_shape[2]
    grad_out = _c(grad_out.float())
    dev = grad_out.device
    if pts is not None:
        pts = _c(pts.float())
        N = pts.shape[1]
        nx, box, first = 0, 0.0, 0
    else:
        nx, box, first, N = lattice
    total = B * N
    ggrid = torch.zeros((B, R, R, R, C), dtype=torch.float32, device=dev) if want_grid_grad else None
    gimg = torch.empty((B, N, C), dtype=torch.float32, device=dev) if with_c_img else None
    g2 = _c(grad_out2.float()) if grad_out2 is not None else None
    if total == 0:                                                  # an empty query set: every gradient is zero, no launch
        p_in = 3 + C if with_c_img else 3
        nflat = lib.vt_decode_wgrad_floats_contact(p_in) if g2 is not None else lib.vt_decode_wgrad_floats(p_in)
        return ((ggrid.permute(0, 4, 1, 2, 3) if ggrid is not None else None), gimg,
                torch.zeros(nflat, dtype=torch.float32, device=dev))
    gws = torch.empty(lib.vt_decode_gws_bytes(total) // 4, dtype=torch.float32, device=dev)
    st = stream_ptr()
    if ggrid is not None and pts is not None and GRID_SCATTER_SORTED and R >= 3:
        # grid gradient by cell (vt_sample_grid_bwd_sorted): the data pass leaves d c, the points are binned by trilinear cell
        # (vt_voxel_build at R - 1) and every cell scatters once -- training points cluster (contact clouds), and per-point f32
        # atomics that collide were 0.8 of the 0.9 ms this call took in a training step
        dc = torch.empty((total, C), dtype=torch.float32, device=dev)
        check(lib.vt_decode_bwd_dc(B, R, C, dev_ptr(pts, "pts"), N, float(padding), dev_ptr(blob_t, "blob_t"),
                                   dev_ptr(grad_out, "grad_out"), dev_ptr(g2, "grad_out2"), dev_ptr(save, "save"), dev_ptr(gws, "gws"),
                                   dev_ptr(dc, "grad_c"), dev_ptr(gimg, "grad_c_img"), st), "vt_decode_bwd_dc")
        sample_grid_bwd_sorted_into(ggrid, pts, dc, padding)
    else:
        check(lib.vt_decode_bwd_contact(B, R, C, dev_ptr(pts, "pts"), N, nx, box, first, float(padding),
                                        dev_ptr(blob_t, "blob_t"), dev_ptr(grad_out, "grad_out"), dev_ptr(g2, "grad_out2"),
                                        dev_ptr(save, "save"), dev_ptr(gws, "gws"), dev_ptr(ggrid, "grad_grid"),
                                        dev_ptr(gimg, "grad_c_img"), st), "vt_decode_bwd")
    wsb = lib.vt_decode_wgrad_workspace_bytes(total)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    p_in = 3 + C if with_c_img else 3
    nflat = lib.vt_decode_wgrad_floats_contact(p_in) if g2 is not None else lib.vt_decode_wgrad_floats(p_in)
    flat = torch.empty(nflat, dtype=torch.float32, device=dev)
    ci = _c(c_img) if with_c_img else None
    check(lib.vt_decode_wgrad_contact(B, dev_ptr(pts, "pts"), N, nx, box, first, dev_ptr(ci, "c_img"),
                                      dev_ptr(grad_out, "grad_out"), dev_ptr(g2, "grad_out2"), dev_ptr(save, "save"),
                                      dev_ptr(gws, "gws"), ctypes.c_void_p(ws.data_ptr()), wsb, dev_ptr(flat, "grads"), st),
          "vt_decode_wgrad")
    return (ggrid.permute(0, 4, 1, 2, 3) if ggrid is not None else None), gimg, flat


def split_decoder_grads(flat, p_in, hidden=32, c_dim=32, nb=5):
    """Views of the flat gradient buffer in the order documented in vtaco_hip.h."""
    o = 0

    def take(n, shape):
        nonlocal o
        v = flat[o:o + n].view(shape)
        o += n
        return v
    g = {"fc_p.weight": take(hidden * p_in, (hidden, p_in)), "fc_p.bias": take(hidden, (hidden,))}
    g["fc_c.weight"] = take(nb * hidden * c_dim, (nb, hidden, c_dim))
    g["fc_c.bias"] = take(nb * hidden, (nb, hidden))
    g["fc_0.weight"] = take(nb * hidden * hidden, (nb, hidden, hidden))
    g["fc_0.bias"] = take(nb * hidden, (nb, hidden))
    g["fc_1.weight"] = take(nb * hidden * hidden, (nb, hidden, hidden))
    g["fc_1.bias"] = take(nb * hidden, (nb, hidden))
    g["fc_out.weight"] = take(hidden, (1, hidden))
    g["fc_out.bias"] = take(1, (1,))
    if flat.numel() - o >= hidden + 1:                  # the _contact layout
        g["fc_out_contact.weight"] = take(hidden, (1, hidden))
        g["fc_out_contact.bias"] = take(1, (1,))
    return g


GRID_SCATTER_SORTED = os.environ.get("VTACO_GRID_SCATTER", "sorted") != "points"     # "points": one set of atomics per point (round 1-3)


def sample_grid_bwd_sorted_into(ggrid_cl, pts, grad_feat, padding=0.1):
    """Scatter d feat [B,N,C] of query points pts [B,N,3] into the zeroed channels-last grid gradient [B,R,R,R,C], the points grouped
    by trilinear cell (vt_voxel_build at resolution R - 1 + vt_sample_grid_bwd_sorted: the cell sums that meet at a node are added in
    a fixed order, so the result is reproducible bit for bit)."""
    B, R, C = ggrid_cl.shape[0], ggrid_cl.shape[1], ggrid_cl.shape[4]
    N = pts.shape[1]
    if B * N == 0:                                                  # no points: the zeroed gradient is the answer
        return
    vi = VoxelIndex(pts, R - 1, padding)
    check(_lib.load().vt_sample_grid_bwd_sorted(B, R, C, dev_ptr(pts, "pts"), N, float(padding), dev_ptr(grad_feat, "grad_feat"),
                                                dev_ptr(vi.order, "order", I32), dev_ptr(vi.seg_lo, "seg_lo", I32),
                                                dev_ptr(vi.seg_hi, "seg_hi", I32), dev_ptr(ggrid_cl, "grad_grid"), stream_ptr()),
          "vt_sample_grid_bwd_sorted")


def sample_grid_bwd(grid_shape, pts, grad_feat, padding=0.1):
    """Backward of :func:`sample_grid` w.r.t. the grid (vt_sample_grid_bwd): [B,C,R,R,R] with channels-last strides."""
    B, C, R = grid_shape[0], grid_shape[1], grid_shape[2]
    pts = _c(pts.float())
    grad_feat = _c(grad_feat.float())
    ggrid = torch.zeros((B, R, R, R, C), dtype=torch.float32, device=grad_feat.device)
    if GRID_SCATTER_SORTED and R >= 3:
        sample_grid_bwd_sorted_into(ggrid, pts, grad_feat, padding)
        return ggrid.permute(0, 4, 1, 2, 3)
    check(_lib.load().vt_sample_grid_bwd(B, R, C, dev_ptr(pts, "pts"), pts.shape[1], 0, 0.0, 0, float(padding),
                                         dev_ptr(grad_feat, "grad_feat"), dev_ptr(ggrid, "grad_grid"), stream_ptr()),
          "vt_sample_grid_bwd")
    return ggrid.permute(0, 4, 1, 2, 3)


def decode_mlp_fwd_train(c, blob, pts):
    """:func:`decode_mlp_fwd` that also returns the activations its backward needs (vt_decode_mlp_fwd_train)."""
    lib = _lib.load()
    c = _c(c)
    pts = _c(pts.float())
    B, N, C = c.shape
    out = torch.empty((B, N), dtype=torch.float32, device=c.device)
    save = torch.empty(lib.vt_decode_save_bytes(B * N) // 4, dtype=torch.float32, device=c.device)
    check(lib.vt_decode_mlp_fwd_train(dev_ptr(c, "c"), B, C, dev_ptr(pts, "pts"), N, 0, 0.0, 0,
                                      dev_ptr(blob, "blob"), dev_ptr(out, "out"), dev_ptr(save, "save"), stream_ptr()),
          "vt_decode_mlp_fwd_train")
    return out, save


def decode_mlp_bwd(blob_t, grad_out, save, pts, C=32):
    """vt_decode_mlp_bwd + vt_decode_wgrad: (grad_c [B,N,C], flat parameter gradients with p_in = 3)."""
    lib = _lib.load()
    pts = _c(pts.float())
    grad_out = _c(grad_out.float())
    B, N = grad_out.shape
    dev = grad_out.device
    total = B * N
    gws = torch.empty(lib.vt_decode_gws_bytes(total) // 4, dtype=torch.float32, device=dev)
    grad_c = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    st = stream_ptr()
    check(lib.vt_decode_mlp_bwd(B, C, dev_ptr(pts, "pts"), N, 0, 0.0, 0, dev_ptr(blob_t, "blob_t"), dev_ptr(grad_out, "grad_out"),
                                dev_ptr(save, "save"), dev_ptr(gws, "gws"), dev_ptr(grad_c, "grad_c"), st), "vt_decode_mlp_bwd")
    wsb = lib.vt_decode_wgrad_workspace_bytes(total)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    flat = torch.empty(lib.vt_decode_wgrad_floats(3), dtype=torch.float32, device=dev)
    check(lib.vt_decode_wgrad(B, dev_ptr(pts, "pts"), N, 0, 0.0, 0, None, dev_ptr(grad_out, "grad_out"), dev_ptr(save, "save"),
                              dev_ptr(gws, "gws"), ctypes.c_void_p(ws.data_ptr()), wsb, dev_ptr(flat, "grads"), st), "vt_decode_wgrad")
    return grad_c, flat
