"""The wide decoder (hidden_size / c_dim beyond 32 / 32) under autograd."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, _c
from .decode import _cl_storage
from .pointnet import rows_wgrad


def _wide_flags(leaky, nearest):
    return (1 if leaky else 0) | (2 if nearest else 0)          # VT_WIDE_LEAKY | VT_WIDE_NEAREST


WIDE_KINDS = ("f32", "bwd", "f16x3")        # VT_WIDE_KIND_*


def decode_wide_form(hidden, c_dim, nb, kind="f32", tactile=False, total=0, workspace=False):
    """Which kernel a wide decode takes and its launch shape (vt_decode_wide_form: the launchers' own rule, asked without launching
    anything): ``kind`` "f32" (the exact forward, inference or training), "bwd" or "f16x3"; ``tactile``: the call gives c_img or finger
    ids; ``workspace``: a split-f16 call with what the 64 / 32 pipeline reads (what decode_fwd and decode_mlp_fwd give it).  Returns
    {"waves", "groups", "pairs", "heads_on_c", "tile_points", "grid_cap", "pipeline"}; raises VtError where the launcher would refuse."""
    if kind not in WIDE_KINDS:
        raise VtError(f"decode_wide_form: kind must be one of {WIDE_KINDS} (got {kind!r})")
    keys = ("waves", "groups", "pairs", "heads_on_c", "tile_points", "grid_cap", "pipeline")
    out = [ctypes.c_int(0) for _ in keys]
    rc = _lib.load().vt_decode_wide_form(int(hidden), int(c_dim), int(nb), int(bool(tactile)), WIDE_KINDS.index(kind), int(total),
                                         int(bool(workspace)), *[ctypes.byref(v) for v in out])
    if rc < 0:
        raise VtError(f"decode_wide_form: no {kind!r} wide decode of hidden={hidden}, c_dim={c_dim}, n_blocks={nb} (code {rc})")
    return {k: int(v.value) for k, v in zip(keys, out)}


def decode_fwd_wide_train(grid, blob, pts, c_img, hidden, nb, leaky, nearest, padding=0.1, want_contact=False):
    """vt_decode_fwd_wide_train: logits [B,N] (and the contact logits) plus the saved layer inputs (opaque f32 tensor)."""
    lib = _lib.load()
    B, C, D, H, W = grid.shape
    keep, gptr = _cl_storage(grid)
    pts = _c(pts.detach().float())
    N = pts.shape[1]
    ci = _c(c_img.detach().float()) if c_img is not None else None
    dev = grid.device
    out = torch.empty((B, N), dtype=torch.float32, device=dev)
    out2 = torch.empty((B, N), dtype=torch.float32, device=dev) if want_contact else None
    # (an empty query set is not 'shape not built': the shape is judged on one point, the save of no points is empty)
    if lib.vt_decode_wide_save_floats(1, int(hidden), C, int(nb)) == 0:
        raise VtError(f"decoder shape hidden={hidden}, c_dim={C}, n_blocks={nb} is not built (multiples of 32 up to 256)")
    nsave = lib.vt_decode_wide_save_floats(B * N, int(hidden), C, int(nb)) if B * N else 0
    save = torch.empty(nsave, dtype=torch.float32, device=dev)
    if N:
        check(lib.vt_decode_fwd_wide_train(gptr, B, D, C, dev_ptr(pts, "pts"), N, dev_ptr(ci, "c_img"), dev_ptr(blob, "blob"),
                                           int(hidden), int(nb), _wide_flags(leaky, nearest), float(padding), dev_ptr(out, "out"),
                                           dev_ptr(out2, "out2"), dev_ptr(save, "save"), stream_ptr()), "vt_decode_fwd_wide_train")
    return out, out2, save


def pack_decoder_wide_t(fc_p_w, fc_c, blocks, fc_out_w, fc_out2_w=None):
    """vt_decoder_pack_wide_t: the transposed weight fragments vt_decode_bwd_wide streams."""
    lib = _lib.load()
    hidden, p_in = fc_p_w.shape
    c_dim, nb = fc_c[0].shape[1], len(blocks)
    keep = []

    def ptr(t, name):
        t = _c(t)
        keep.append(t)
        return dev_ptr(t, name)
    prm = _lib.DecoderParams()
    prm.hidden, prm.c_dim, prm.n_blocks, prm.p_in = hidden, c_dim, nb, p_in
    prm.fc_p_w = ptr(fc_p_w, "fc_p.weight")
    for i, w in enumerate(fc_c):
        prm.fc_c_w[i] = ptr(w, f"fc_c.{i}.weight").value
    for i, (w0, w1) in enumerate(blocks):
        prm.fc0_w[i], prm.fc1_w[i] = ptr(w0, "fc_0.weight").value, ptr(w1, "fc_1.weight").value
    prm.fc_out_w = ptr(fc_out_w, "fc_out.weight")
    if fc_out2_w is not None:
        prm.fc_out2_w = ptr(fc_out2_w, "fc_out_contact.weight")
    n = lib.vt_decoder_wide_blob_t_bytes(hidden, c_dim, nb)
    if n == 0:
        raise VtError(f"decoder shape hidden={hidden}, c_dim={c_dim}, n_blocks={nb} is not built (multiples of 32 up to 256)")
    out = torch.empty(n // 4, dtype=torch.float32, device=fc_p_w.device)
    check(lib.vt_decoder_pack_wide_t(ctypes.byref(prm), dev_ptr(out, "blob_t"), n, stream_ptr()), "vt_decoder_pack_wide_t")
    return out


def _wide_zero_grads(H, C, nb, p_in, dev, contact):
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    g = {"fc_p.weight": z(H, p_in), "fc_p.bias": z(H), "fc_c.weight": [z(H, C) for _ in range(nb)], "fc_c.bias": [z(H) for _ in range(nb)],
         "fc_0.weight": [z(H, H) for _ in range(nb)], "fc_0.bias": [z(H) for _ in range(nb)],
         "fc_1.weight": [z(H, H) for _ in range(nb)], "fc_1.bias": [z(H) for _ in range(nb)],
         "fc_out.weight": z(1, H), "fc_out.bias": z(1)}
    if contact:
        g["fc_out_contact.weight"], g["fc_out_contact.bias"] = z(1, H), z(1)
    return g


def _wide_wgrads(save, gws, P, H, C, nb, pts, c_rows, c_img, grad_out, g2):
    """The decoder's parameter gradients from the rows the data pass leaves (vt_rows_wgrad per layer; layouts: decode_wide.hip
    wide_save_layout / wide_gws_layout).  ``c_rows`` [P, C]: the conditioning features (the save's c slot, or the caller's)."""
    sv_blk = save[P * C:P * C + 2 * nb * P * H].view(nb, 2, P, H)
    sv_af = save[P * C + 2 * nb * P * H:].view(P, H)
    dn = gws[:(nb + 1) * P * H].view(nb + 1, P, H)
    dh = gws[(nb + 1) * P * H:].view(nb, P, H)
    g = {}
    x2 = _c(c_img.float()).view(P, C) if c_img is not None else None
    g["fc_p.weight"], g["fc_p.bias"] = rows_wgrad(dn[0], pts.view(P, 3), x2)
    wc, bc, w0, b0, w1, b1 = [], [], [], [], [], []
    for i in range(nb):
        a, b = rows_wgrad(dn[i], c_rows); wc.append(a); bc.append(b)
        a, b = rows_wgrad(dh[i], sv_blk[i, 0]); w0.append(a); b0.append(b)
        a, b = rows_wgrad(dn[i + 1], sv_blk[i, 1]); w1.append(a); b1.append(b)
    g["fc_c.weight"], g["fc_c.bias"] = wc, bc
    g["fc_0.weight"], g["fc_0.bias"], g["fc_1.weight"], g["fc_1.bias"] = w0, b0, w1, b1
    g["fc_out.weight"], g["fc_out.bias"] = rows_wgrad(grad_out.view(P, 1), sv_af)
    if g2 is not None:
        g["fc_out_contact.weight"], g["fc_out_contact.bias"] = rows_wgrad(g2.view(P, 1), sv_af)
    return g


def _wide_rows(gws, P, H, nb):
    return {"rows.dN": gws[:(nb + 1) * P * H].view(nb + 1, P, H), "rows.dH": gws[(nb + 1) * P * H:].view(nb, P, H)}


def decode_bwd_wide(grid_shape, blob_t, grad_out, save, pts, hidden, nb, leaky, nearest, padding=0.1, c_img=None,
                    want_grid_grad=True, grad_out2=None, want_rows=False):
    """vt_decode_bwd_wide + the weight gradients (vt_rows_wgrad over the saved layer inputs and the output gradients the data pass
    leaves).  Returns (grad_grid channels-last strided [B,C,R,R,R] or None, grad_c_img [B,N,C] or None, dict of parameter gradients
    keyed like split_decoder_grads); with ``want_rows`` the dict also holds "rows.dN" [nb + 1, P, H] and "rows.dH" [nb, P, H], the
    output gradients the data pass leaves (wide_gws_layout)."""
    lib = _lib.load()
    B, C, R = grid_shape[0], grid_shape[1], grid_shape[2]
    H = int(hidden)
    grad_out = _c(grad_out.float())
    dev = grad_out.device
    pts = _c(pts.float())
    N = pts.shape[1]
    P = B * N
    g2 = _c(grad_out2.float()) if grad_out2 is not None else None
    ggrid = torch.zeros((B, R, R, R, C), dtype=torch.float32, device=dev) if want_grid_grad else None
    gimg = torch.empty((B, N, C), dtype=torch.float32, device=dev) if c_img is not None else None
    if P == 0:                                                      # an empty query set: every gradient is zero, no launch
        g = _wide_zero_grads(H, C, nb, 3 + C if c_img is not None else 3, dev, g2 is not None)
        return (ggrid.permute(0, 4, 1, 2, 3) if ggrid is not None else None), gimg, g
    gws = torch.empty(lib.vt_decode_wide_gws_floats(P, H, C, int(nb)), dtype=torch.float32, device=dev)
    check(lib.vt_decode_bwd_wide(B, R, C, dev_ptr(pts, "pts"), N, dev_ptr(blob_t, "blob_t"), H, int(nb), _wide_flags(leaky, nearest),
                                 float(padding), dev_ptr(grad_out, "grad_out"), dev_ptr(g2, "grad_out2"), dev_ptr(save, "save"),
                                 dev_ptr(gws, "gws"), dev_ptr(ggrid, "grad_grid"), dev_ptr(gimg, "grad_c_img"), stream_ptr()),
          "vt_decode_bwd_wide")
    g = _wide_wgrads(save, gws, P, H, C, int(nb), pts, save[:P * C].view(P, C), c_img, grad_out, g2)
    if want_rows:
        g.update(_wide_rows(gws, P, H, int(nb)))
    return (ggrid.permute(0, 4, 1, 2, 3) if ggrid is not None else None), gimg, g


def decode_mlp_fwd_wide_train(c, blob, pts, hidden, nb, leaky):
    """vt_decode_mlp_fwd_wide_train: the conditioned MLP on given features c [B,N,C] at the wide shapes, keeping every layer's input."""
    lib = _lib.load()
    c = _c(c.detach().float())
    pts = _c(pts.detach().float())
    B, N, C = c.shape
    if lib.vt_decode_wide_save_floats(1, int(hidden), C, int(nb)) == 0:
        raise VtError(f"decoder shape hidden={hidden}, c_dim={C}, n_blocks={nb} is not built (multiples of 32 up to 256)")
    out = torch.empty((B, N), dtype=torch.float32, device=c.device)
    save = torch.empty(lib.vt_decode_wide_save_floats(B * N, int(hidden), C, int(nb)) if B * N else 0, dtype=torch.float32, device=c.device)
    if B * N:
        check(lib.vt_decode_mlp_fwd_wide_train(dev_ptr(c, "c"), B, C, dev_ptr(pts, "pts"), N, dev_ptr(blob, "blob"), int(hidden), int(nb),
                                               _wide_flags(leaky, False), dev_ptr(out, "out"), None, dev_ptr(save, "save"), stream_ptr()),
              "vt_decode_mlp_fwd_wide_train")
    return out, save


def decode_mlp_bwd_wide(blob_t, grad_out, save, pts, c, hidden, nb, leaky, want_rows=False):
    """vt_decode_mlp_bwd_wide + the weight gradients: (grad_c [B,N,C], dict of parameter gradients keyed like split_decoder_grads;
    with ``want_rows`` also "rows.dN" / "rows.dH" as decode_bwd_wide's)."""
    lib = _lib.load()
    grad_out = _c(grad_out.float())
    pts = _c(pts.float())
    c = _c(c.float())
    B, N, C = c.shape
    H, P, dev = int(hidden), B * N, grad_out.device
    grad_c = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    if P == 0:
        return grad_c, _wide_zero_grads(H, C, nb, 3, dev, False)
    gws = torch.empty(lib.vt_decode_wide_gws_floats(P, H, C, int(nb)), dtype=torch.float32, device=dev)
    check(lib.vt_decode_mlp_bwd_wide(B, C, dev_ptr(pts, "pts"), N, dev_ptr(blob_t, "blob_t"), H, int(nb), _wide_flags(leaky, False),
                                     dev_ptr(grad_out, "grad_out"), None, dev_ptr(save, "save"), dev_ptr(gws, "gws"),
                                     dev_ptr(grad_c, "grad_c"), stream_ptr()), "vt_decode_mlp_bwd_wide")
    g = _wide_wgrads(save, gws, P, H, C, int(nb), pts, c.view(P, C), None, grad_out, None)
    if want_rows:
        g.update(_wide_rows(gws, P, H, int(nb)))
    return grad_c, g
