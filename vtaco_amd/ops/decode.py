"""The occupancy decoder's forward paths: packing, range guard, channels-last grids, decode / sample / MLP launches."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, U8, _c, keep_for_graph


def blob_floats(hidden=32, c_dim=32, n_blocks=5):
    n = _lib.load().vt_decoder_blob_bytes(hidden, c_dim, n_blocks)
    if n == 0:
        raise VtError(f"decoder shape hidden={hidden}, c_dim={c_dim}, n_blocks={n_blocks} is not built "
                      "(gfx950 kernels cover the shipped VTacO shape 32/32/5)")
    return n // 4


PRECISIONS = ("f32", "bf16x3", "f16x3", "f16f8")
SPLIT_PRECISIONS = ("bf16x3", "f16x3", "f16f8")   # dense layers on the 16-bit matrix core with hi + lo operands
# "f16f8": f16 hi products + ONE fp8 MFMA for both correction products of a layer (vt_decode_fwd_f16f8: ~4e-5 on the golden logits,
# the fastest form); it exists for lattice slabs only -- see f16f8_covers -- and LocalDecoder falls back to "f16x3" elsewhere


def f16f8_covers(grid, lattice, padding=0.1):
    """True if vt_decode_fwd_f16f8 covers this lattice slab (whole x-plane pairs, nx % 8 == 0, < 0.55 voxels per step)."""
    if lattice is None:
        return False
    nx, box, first, count = lattice
    B, C, D, H, W = grid.shape
    return bool(_lib.load().vt_decode_f16f8_covers(D, C, int(nx), float(box), int(first), int(count), float(padding)))


LATTICE_FORMS = ("linear", "brick", "staged", "staged2", "staged3")   # VT_LATTICE_*: the kernel forms of a lattice decode


def decode_lattice_form(R, lattice, padding=0.1, precision="f32", want_contact=False, c_direct=False, C=32):
    """The kernel form a lattice decode of this shape takes (vt_decode_lattice_form: the launchers' own dispatch rule, asked
    without launching anything): one of LATTICE_FORMS for a grid of side ``R`` with ``C`` channels, ``lattice=(nx, box, first,
    count)`` and a precision of PRECISIONS; ``c_direct``: the features are given (decode_mlp_fwd).  Raises VtError where the
    launcher would refuse the call."""
    if precision not in PRECISIONS:
        raise VtError(f"precision must be one of {PRECISIONS} (got {precision!r})")
    nx, box, first, count = lattice
    rc = _lib.load().vt_decode_lattice_form(int(R), int(C), int(nx), float(box), int(first), int(count), float(padding),
                                            PRECISIONS.index(precision), int(bool(want_contact)), int(bool(c_direct)))
    if rc < 0:
        raise VtError(f"decode_lattice_form: no {precision!r} lattice decode of R={R}, C={C}, lattice={tuple(lattice)} (code {rc})")
    return LATTICE_FORMS[rc]


def pack_decoder(fc_p_w, fc_p_b, fc_c, blocks, fc_out, fc_out2=None, out=None, transposed=False, precision="f32"):
    """Repack decoder parameters into the MFMA-fragment blob (vt_decoder_pack; with
    ``precision="bf16x3"`` / ``"f16x3"`` the split blob of vt_decoder_pack_bf16x3 / _f16x3), or with
    ``transposed=True`` into the transposed-weight blob of the backward (vt_decoder_pack_t).

    fc_c: list of (weight, bias); blocks: list of (fc0_w, fc0_b, fc1_w, fc1_b);
    fc_out / fc_out2: (weight, bias).  ``fc_p_w`` is fc_p.weight [H,3] or
    fc_p_img.weight [H,3+C].
    """
    lib = _lib.load()
    hidden, p_in = fc_p_w.shape
    c_dim = fc_c[0][0].shape[1]
    nb = len(blocks)
    if nb > _lib.VT_MAX_BLOCKS:
        raise VtError(f"n_blocks={nb} exceeds VT_MAX_BLOCKS")
    keep = []

    def ptr(t, name):
        t = _c(t)
        keep.append(t)
        return dev_ptr(t, name)

    prm = _lib.DecoderParams()
    prm.hidden, prm.c_dim, prm.n_blocks, prm.p_in = hidden, c_dim, nb, p_in
    prm.fc_p_w, prm.fc_p_b = ptr(fc_p_w, "fc_p.weight"), ptr(fc_p_b, "fc_p.bias")
    for i, (w, b) in enumerate(fc_c):
        prm.fc_c_w[i], prm.fc_c_b[i] = ptr(w, f"fc_c.{i}.weight").value, ptr(b, f"fc_c.{i}.bias").value
    for i, (w0, b0, w1, b1) in enumerate(blocks):
        prm.fc0_w[i], prm.fc0_b[i] = ptr(w0, "fc_0.weight").value, ptr(b0, "fc_0.bias").value
        prm.fc1_w[i], prm.fc1_b[i] = ptr(w1, "fc_1.weight").value, ptr(b1, "fc_1.bias").value
    prm.fc_out_w, prm.fc_out_b = ptr(fc_out[0], "fc_out.weight"), ptr(fc_out[1], "fc_out.bias")
    if fc_out2 is not None:
        prm.fc_out2_w, prm.fc_out2_b = ptr(fc_out2[0], "fc_out_contact.weight"), ptr(fc_out2[1], "fc_out_contact.bias")
    if transposed:
        n = lib.vt_decoder_blob_t_bytes(hidden, c_dim, nb) // 4
        if n == 0:
            raise VtError("decoder shape not built (32/32/5 only)")
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=fc_p_w.device)
        check(lib.vt_decoder_pack_t(ctypes.byref(prm), dev_ptr(out, "blob_t"), n * 4, stream_ptr()), "vt_decoder_pack_t")
        return out
    if precision in ("wide", "wide_f16x3"):
        # the general-shape kernel (vt_decode_fwd_wide): hidden / c_dim multiples of 32 up to 256, weights streamed in fragment order; or
        # the same shapes on the f16 matrix core with split operands (vt_decode_fwd_wide_f16x3): its own fragment format
        f16 = "_f16x3" if precision == "wide_f16x3" else ""
        n = getattr(lib, f"vt_decoder_wide_blob{f16}_bytes")(hidden, c_dim, nb, p_in) // 4
        if n == 0:
            raise VtError(f"decoder shape hidden={hidden}, c_dim={c_dim}, n_blocks={nb} is not built: hidden_size and c_dim must be "
                          f"multiples of 32 up to 256, n_blocks <= {_lib.VT_MAX_BLOCKS}")
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=fc_p_w.device)
        check(getattr(lib, "vt_decoder_pack_wide" + f16)(ctypes.byref(prm), dev_ptr(out, "blob"), n * 4, stream_ptr()), "vt_decoder_pack_wide" + f16)
        return out
    if precision not in PRECISIONS:
        raise VtError(f"precision must be one of {PRECISIONS} (got {precision!r})")
    n = blob_floats(hidden, c_dim, nb)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=fc_p_w.device)
    if precision in SPLIT_PRECISIONS:
        name = "vt_decoder_pack_" + precision
        check(getattr(lib, name)(ctypes.byref(prm), dev_ptr(out, "blob"), n * 4, stream_ptr()), name)
    else:
        check(lib.vt_decoder_pack(ctypes.byref(prm), dev_ptr(out, "blob"), n * 4, stream_ptr()), "vt_decoder_pack")
    return out


RANGE_HALF, RANGE_FP8, RANGE_LOGIT = 1, 2, 4


def decode_range_status(reset=True):
    """The current device's range-guard word (vt_decode_range_status).  Bit 0 (RANGE_HALF): a half-precision lattice decode
    ("f16x3" / "f16f8") since the last reset met activations at the edge of the half range (its hi operand saturated at 65504:
    the logits of those launches are not to be trusted).  Bit 1 (RANGE_FP8): an "f16f8" decode met activations >= 1024, where
    the fp8 copies of its correction products begin to clip, bit 2 (RANGE_LOGIT): an "f16f8" decode wrote a logit beyond 2.5 in
    magnitude (its error is relative, ~3e-5 |logit|) -- in both cases its 1e-4 contract ends and "f16x3" is the form to use.
    Synchronises the stream."""
    word = ctypes.c_uint32(0)
    check(_lib.load().vt_decode_range_status(ctypes.byref(word), int(bool(reset)), stream_ptr()), "vt_decode_range_status")
    return int(word.value)


def decode_range_clear():
    """Clear the current device's range-guard word without reading it (an asynchronous 4-byte fill on the current stream: what
    the generator does when a scene begins, so that bits left by earlier launches are not attributed to it)."""
    check(_lib.load().vt_decode_range_status(None, 1, stream_ptr()), "vt_decode_range_status")


def decode_last_clock(workgroups=False):
    """Clock evidence of the last lattice decode launch on the current device (vt_decode_last_clock): workgroup 0's lifetime in
    shader cycles and in ticks of the constant-rate counter -> {"shader_mhz", "wg0_us", "shader_cycles"}; with
    ``workgroups=True`` also the launch's shape in time from every workgroup's (start, end) stamps: "span_us" (first start to
    last end: the kernel's duration as the chip saw it), "start_spread_us" (the dispatch ramp), "wg_us_min/median/max" and
    the raw stamps as "wg_ticks" ([n, 2] list, ticks of "ref_khz").  Synchronises."""
    cyc, ref, khz, n = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_int(0)
    cap = 512 if workgroups else 0
    buf = (ctypes.c_uint64 * (2 * cap))() if cap else None
    check(_lib.load().vt_decode_last_clock(ctypes.byref(cyc), ctypes.byref(ref), ctypes.byref(khz), buf, cap, ctypes.byref(n),
                                           stream_ptr()), "vt_decode_last_clock")
    if ref.value == 0 or khz.value <= 0:
        return None
    tick_us = 1e3 / khz.value
    us = ref.value * tick_us
    res = {"shader_mhz": cyc.value / us, "wg0_us": us, "shader_cycles": int(cyc.value), "ref_khz": int(khz.value)}
    if workgroups and n.value > 0:
        st = [(buf[2 * i], buf[2 * i + 1]) for i in range(n.value)]
        t0 = min(a for a, _ in st)
        dur = sorted((b - a) * tick_us for a, b in st)
        res.update({"workgroups": n.value, "span_us": (max(b for _, b in st) - t0) * tick_us,
                    "start_spread_us": (max(a for a, _ in st) - t0) * tick_us,
                    "wg_us_min": dur[0], "wg_us_median": dur[len(dur) // 2], "wg_us_max": dur[-1],
                    "wg_ticks": [[int(a - t0), int(b - t0)] for a, b in st]})
    return res


def is_channels_last_grid(grid):
    """True if ``grid`` [B,C,D,H,W] is laid out b,z,y,x,c in memory."""
    B, C, D, H, W = grid.shape
    return grid.stride() == (D * H * W * C, 1, H * W * C, W * C, C)


def grid_to_channels_last(grid):
    """[B,C,D,H,W] contiguous -> tensor of the SAME shape whose memory is
    [B,D,H,W,C] (torch.channels_last_3d), via vt_grid_to_channels_last."""
    if is_channels_last_grid(grid):
        return grid
    g = _c(grid)
    B, C, D, H, W = g.shape
    out = torch.empty((B, D, H, W, C), dtype=torch.float32, device=g.device)
    check(_lib.load().vt_grid_to_channels_last(dev_ptr(g, "grid"), dev_ptr(out, "grid_cl"), B, C, D, H, W, stream_ptr()),
          "vt_grid_to_channels_last")
    return out.permute(0, 4, 1, 2, 3)


def grid_from_channels_last(grid_cl):
    """Inverse of :func:`grid_to_channels_last`: returns a contiguous NCDHW tensor."""
    B, C, D, H, W = grid_cl.shape
    if not is_channels_last_grid(grid_cl):
        raise VtError("grid_from_channels_last: input is not channels-last")
    out = torch.empty((B, C, D, H, W), dtype=torch.float32, device=grid_cl.device)
    src = grid_cl.permute(0, 2, 3, 4, 1)
    check(_lib.load().vt_grid_from_channels_last(dev_ptr(src, "grid_cl"), dev_ptr(out, "grid"), B, C, D, H, W, stream_ptr()),
          "vt_grid_from_channels_last")
    return out


def _cl_storage(grid):
    """Device pointer of the channels-last storage of a [B,C,R,R,R] grid."""
    g = grid_to_channels_last(grid)
    return g, dev_ptr(g.permute(0, 2, 3, 4, 1), "grid")


_wide_ws = {}          # per (device, stream): the sampling workspace of the 64 / 32 pipeline (vt_decode_fwd_wide_f16x3_ws)
WIDE_SLICE = 1 << 19   # points per launch pair of that pipeline


def decode_fwd(grid, blob, pts=None, c_img=None, padding=0.1, lattice=None, want_contact=False, out=None, save=None,
               precision="f32", wide=None, finger_ids=None, finger_feats=None):
    """Fused trilinear gather + conditioned MLP (vt_decode_fwd; ``precision="bf16x3"`` / ``"f16x3"``:
    vt_decode_fwd_bf16x3 / vt_decode_fwd_f16x3 with a blob packed for it; ``precision="wide"`` /
    ``"wide_f16x3"`` with ``wide=(hidden_size, n_blocks, leaky[, nearest])``: vt_decode_fwd_wide[_f16x3], the exact-f32 / split-f16
    kernels of the shapes beyond 32/32).

    grid  [B,C,R,R,R] (any layout; converted to channels-last if needed)
    pts   [B,N,3] or None with lattice=(nx, box, first, count)
    c_img [B,N,C] or None.  Returns logits [B,N] (and contact logits).
    """
    lib = _lib.load()
    B, C, D, H, W = grid.shape
    if not (D == H == W):
        raise VtError("feature grid must be cubic")
    keep, gptr = _cl_storage(grid)
    if pts is not None:
        pts = _c(pts.float())
        if pts.shape[0] != B or pts.shape[-1] != 3:
            raise VtError(f"pts must be [B,N,3] with B={B} (got {tuple(pts.shape)})")
        N = pts.shape[1]
        nx, box, first = 0, 0.0, 0
    else:
        nx, box, first, N = lattice
    if c_img is not None:
        c_img = _c(c_img)
        if tuple(c_img.shape) != (B, N, C):
            raise VtError(f"c_img must be [B,N,C]=({B},{N},{C}) (got {tuple(c_img.shape)})")
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=grid.device)
    out2 = torch.empty((B, N), dtype=torch.float32, device=grid.device) if want_contact else None
    if N == 0:                                   # empty query set: nothing to launch
        return (out, out2) if want_contact else out
    keep_for_graph(blob, keep)
    if precision in ("wide", "wide_f16x3"):
        if save is not None or wide is None:
            raise VtError("decode_fwd: precision 'wide' is inference only and needs wide=(hidden_size, n_blocks, leaky)")
        hidden, nb, leaky = wide[:3]
        flags = (1 if leaky else 0) | (2 if len(wide) > 3 and wide[3] else 0)          # VT_WIDE_LEAKY | VT_WIDE_NEAREST
        name = "vt_decode_fwd_wide" if precision == "wide" else "vt_decode_fwd_wide_f16x3"
        if finger_ids is not None:
            # the tactile feature by finger id (uint8 [B,N], 255 = none) and the [F,C] table: no dense [B,N,C] tensor
            ids, feats = _c(finger_ids), _c(finger_feats.detach().float())
            if c_img is not None or ids.dtype != torch.uint8 or ids.numel() != B * N or feats.dim() != 2 or feats.shape[1] != C:
                raise VtError(f"decode_fwd: finger ids must be uint8 [B,N] with a [F,{C}] feature table (and no c_img)")
            keep_for_graph(ids, feats)
            check(getattr(lib, name + "_ids")(gptr, B, D, C, dev_ptr(pts, "pts"), N, nx, box, first, dev_ptr(ids, "finger_ids", torch.uint8),
                                              dev_ptr(feats, "finger_feats"), int(feats.shape[0]), dev_ptr(blob, "blob"), int(hidden),
                                              int(nb), flags, float(padding), dev_ptr(out, "out"), dev_ptr(out2, "out2"), stream_ptr()),
                  name + "_ids")
            return (out, out2) if want_contact else out
        wsb = lib.vt_decode_wide_f16x3_workspace_bytes(B * N, int(hidden), C, int(nb), 0 if c_img is None else 1) if precision == "wide_f16x3" else 0
        if wsb:
            # 64 / 32 / <= 5: the register-resident pipeline on the grid's samples, which a pre-pass leaves in a workspace.  The call
            # runs scene by scene in slices of WIDE_SLICE points (the workspace is 128 bytes per point: 67 MB per slice instead of 268 MB
            # for a 128^3 lattice and 2.1 GB for 256^3; a slice's samples are still in the Infinity Cache when the pipeline reads them),
            # one workspace per (device, stream) -- two streams decoding at once do not share it -- released when a smaller call comes
            step = min(N, WIDE_SLICE)
            wsb = lib.vt_decode_wide_f16x3_workspace_bytes(step, int(hidden), C, int(nb), 0 if c_img is None else 1)
            key = (grid.device, stream_ptr().value)
            ws = _wide_ws.get(key)
            if ws is None or ws.numel() < wsb or ws.numel() > 4 * wsb:
                ws = _wide_ws[key] = torch.empty(wsb, dtype=torch.uint8, device=grid.device)
            keep_for_graph(ws)
            cl = keep.permute(0, 2, 3, 4, 1)                           # [B, R, R, R, C] contiguous: scene b starts at cl[b]
            for b in range(B):
                for lo in range(0, N, step):
                    n = min(step, N - lo)
                    sl = (slice(b, b + 1), slice(lo, lo + n))
                    check(lib.vt_decode_fwd_wide_f16x3_ws(dev_ptr(cl[b], "grid"), 1, D, C, dev_ptr(pts[sl] if pts is not None else None, "pts"), n,
                                                          nx, box, first + lo if pts is None else 0,
                                                          dev_ptr(c_img[sl] if c_img is not None else None, "c_img"), dev_ptr(blob, "blob"),
                                                          int(hidden), int(nb), flags, float(padding), dev_ptr(out[sl], "out"),
                                                          dev_ptr(out2[sl] if out2 is not None else None, "out2"),
                                                          ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream_ptr()),
                          "vt_decode_fwd_wide_f16x3_ws")
            return (out, out2) if want_contact else out
        check(getattr(lib, name)(gptr, B, D, C, dev_ptr(pts, "pts"), N, nx, box, first, dev_ptr(c_img, "c_img"),
                                 dev_ptr(blob, "blob"), int(hidden), int(nb), flags, float(padding),
                                 dev_ptr(out, "out"), dev_ptr(out2, "out2"), stream_ptr()), name)
    elif precision == "f16f8":
        if pts is not None or want_contact or save is not None:
            raise VtError("decode_fwd: precision 'f16f8' covers lattice slabs only (ops.f16f8_covers); use 'f16x3'")
        check(lib.vt_decode_fwd_f16f8(gptr, B, D, C, N, nx, box, first, dev_ptr(c_img, "c_img"), None, None, 0,
                                      dev_ptr(blob, "blob"), float(padding), dev_ptr(out, "out"), stream_ptr()), "vt_decode_fwd_f16f8")
    elif precision in SPLIT_PRECISIONS:
        if save is not None:
            raise VtError("decode_fwd: the training forward (save) is exact-f32 only")
        name = "vt_decode_fwd_" + precision
        check(getattr(lib, name)(gptr, B, D, C, dev_ptr(pts, "pts"), N, nx, box, first,
                                 dev_ptr(c_img, "c_img"), None, None, 0, dev_ptr(blob, "blob"), float(padding),
                                 dev_ptr(out, "out"), dev_ptr(out2, "out2"), stream_ptr()), name)
    elif precision == "f32":
        check(lib.vt_decode_fwd(gptr, B, D, C, dev_ptr(pts, "pts"), N, nx, box, first,
                                dev_ptr(c_img, "c_img"), dev_ptr(blob, "blob"), float(padding),
                                dev_ptr(out, "out"), dev_ptr(out2, "out2"), dev_ptr(save, "save"), stream_ptr()), "vt_decode_fwd")
    else:
        raise VtError(f"precision must be one of {PRECISIONS} (got {precision!r})")
    return (out, out2) if want_contact else out


def sample_grid(grid, pts=None, padding=0.1, lattice=None):
    """Trilinear features [B,N,C] of ``grid`` at ``pts`` [B,N,3], or with ``lattice=(nx, box, first, count)`` at the points
    ``box * make_3d_grid(...)[first:first+count]`` generated in the kernel (vt_sample_grid; slabs of whole x-plane pairs with
    nx % 8 == 0 and < 0.55 voxels per step run the LDS-staged gather: the same bits, ~2.5x the rate)."""
    B, C, D, H, W = grid.shape
    keep, gptr = _cl_storage(grid)
    if pts is not None:
        pts = _c(pts.float())
        N, nx, box, first = pts.shape[1], 0, 0.0, 0
    else:
        nx, box, first, N = lattice
    feat = torch.empty((B, N, C), dtype=torch.float32, device=grid.device)
    if N:
        check(_lib.load().vt_sample_grid(gptr, B, D, C, dev_ptr(pts, "pts"), N, int(nx), float(box), int(first), float(padding),
                                         dev_ptr(feat, "feat"), stream_ptr()), "vt_sample_grid")
    return feat


def decode_mlp_fwd(c, blob, pts, precision="f32", wide=None):
    """The conditioned MLP on given features c [B,N,C] (vt_decode_mlp_fwd; ``precision="f16x3"`` with a blob packed for it:
    vt_decode_mlp_fwd_f16x3).  ``precision="wide"`` / ``"wide_f16x3"`` with ``wide=(hidden_size, n_blocks, leaky)``: the shapes
    beyond 32 / 32 (vt_decode_mlp_fwd_wide[_f16x3], blob from pack_decoder(..., precision="wide" / "wide_f16x3"))."""
    if precision not in ("f32", "f16x3", "wide", "wide_f16x3"):
        raise VtError(f"decode_mlp_fwd: precision must be 'f32', 'f16x3', 'wide' or 'wide_f16x3' (got {precision!r})")
    c = _c(c.float())
    pts = _c(pts.float())
    B, N, C = c.shape
    out = torch.empty((B, N), dtype=torch.float32, device=c.device)
    if N and precision in ("wide", "wide_f16x3"):
        if wide is None:
            raise VtError("decode_mlp_fwd: precision 'wide' needs wide=(hidden_size, n_blocks, leaky)")
        hidden, nb, leaky = wide[:3]
        name = "vt_decode_mlp_fwd_wide" if precision == "wide" else "vt_decode_mlp_fwd_wide_f16x3"
        check(getattr(_lib.load(), name)(dev_ptr(c, "c"), B, C, dev_ptr(pts, "pts"), N, 0, 0.0, 0, dev_ptr(blob, "blob"),
                                         int(hidden), int(nb), 1 if leaky else 0, dev_ptr(out, "out"), None, stream_ptr()), name)
        return out
    if N:
        name = "vt_decode_mlp_fwd" if precision == "f32" else "vt_decode_mlp_fwd_f16x3"
        check(getattr(_lib.load(), name)(dev_ptr(c, "c"), B, C, dev_ptr(pts, "pts"), N, 0, 0.0, 0,
                                         dev_ptr(blob, "blob"), dev_ptr(out, "out"), stream_ptr()), name)
    return out


def tactile_assign(anchors, success, mode, radius, pts=None, lattice=None, count=None, B=1):
    """Finger id per query point (uint8, 255 = none).  anchors [F,K,3] f32; success [F];
    mode 'nearest' (K=1, generation.py:186-200) or 'within' (generation.py:245-255)."""
    anchors = _c(anchors.float())
    F, K = anchors.shape[0], anchors.shape[1]
    dev = anchors.device
    if count is None:
        count = torch.full((F,), K, dtype=I32, device=dev)
    count = _c(count.to(I32))
    success = _c(success.to(U8))
    if pts is not None:
        pts = _c(pts.float())
        B, N = pts.shape[0], pts.shape[1]
        nx, box, first = 0, 0.0, 0
    else:
        nx, box, first, N = lattice
    ids = torch.empty((B, N), dtype=U8, device=dev)
    check(_lib.load().vt_tactile_assign(dev_ptr(pts, "pts"), B, N, nx, box, first, dev_ptr(anchors, "anchors"),
                                        dev_ptr(count, "count", I32), dev_ptr(success, "success", U8), F, K,
                                        {"nearest": 0, "within": 1}[mode], float(radius), dev_ptr(ids, "ids", U8), stream_ptr()),
          "vt_tactile_assign")
    return ids


def decode_fwd_ids(grid, blob, ids, feats, pts=None, lattice=None, padding=0.1, out=None, precision="f32"):
    """vt_decode_fwd_ids: forward_img with c_img[b,n] = feats[ids[b,n]] (zeros where ids == 255)."""
    B, C, D, H, W = grid.shape
    keep, gptr = _cl_storage(grid)
    feats = _c(feats.float())
    if pts is not None:
        pts = _c(pts.float())
        N = pts.shape[1]
        nx, box, first = 0, 0.0, 0
    else:
        nx, box, first, N = lattice
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=grid.device)
    if precision == "f16f8":
        if pts is not None:
            raise VtError("decode_fwd_ids: precision 'f16f8' covers lattice slabs only (ops.f16f8_covers); use 'f16x3'")
        check(_lib.load().vt_decode_fwd_f16f8(gptr, B, D, C, N, nx, box, first, None, dev_ptr(_c(ids), "ids", U8), dev_ptr(feats, "feats"),
                                              feats.shape[0], dev_ptr(blob, "blob"), float(padding), dev_ptr(out, "out"), stream_ptr()),
              "vt_decode_fwd_f16f8")
        return out
    if precision in SPLIT_PRECISIONS:
        name = "vt_decode_fwd_" + precision
        check(getattr(_lib.load(), name)(gptr, B, D, C, dev_ptr(pts, "pts"), N, nx, box, first, None,
                                         dev_ptr(_c(ids), "ids", U8), dev_ptr(feats, "feats"), feats.shape[0],
                                         dev_ptr(blob, "blob"), float(padding), dev_ptr(out, "out"), None, stream_ptr()), name)
        return out
    check(_lib.load().vt_decode_fwd_ids(gptr, B, D, C, dev_ptr(pts, "pts"), N, nx, box, first, dev_ptr(_c(ids), "ids", U8),
                                        dev_ptr(feats, "feats"), feats.shape[0], dev_ptr(blob, "blob"), float(padding),
                                        dev_ptr(out, "out"), stream_ptr()), "vt_decode_fwd_ids")
    return out
