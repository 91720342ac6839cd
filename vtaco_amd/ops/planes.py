"""The canonical feature planes at the decoder's query points (vt_sample_planes, vt_sample_planes_bwd) and the conditioned MLP on
lattice slabs of given features.  Reached as ``ops.planes.name``: the module adds no name to ``vtaco_amd.ops`` itself."""
import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, _c

ORDER = ("xz", "xy", "yz")              # the order the reference sums the planes in, whatever order the caller's dict has
NEAREST, LATTICE_POINTS, PREPARED = 1, 2, 4          # VT_PLANES_NEAREST, VT_PLANES_LATTICE_POINTS, VT_PLANES_PREPARED
# how a lattice slab is sampled: "table" = per plane the nx^2 distinct samples once, then three coalesced rows per lattice point;
# "points" = the point kernel on coordinates generated in the kernel.  The same bits; the faster one ships
# (profiles/plane_decode_bench.json).
LATTICE_FORM = "table"


def _three(planes, what):
    """[xz, xy, yz] contiguous float tensors or None, and their common (B, C, R)."""
    keys = set(planes)
    if not keys or not keys <= set(ORDER):
        raise VtError(f"{what}: planes must be a non-empty subset of {ORDER} (got {sorted(keys)})")
    out, shape = [], None
    for k in ORDER:
        t = planes.get(k)
        if t is not None:
            t = _c(t.float())
            if t.dim() != 4 or t.shape[2] != t.shape[3]:
                raise VtError(f"{what}: plane {k!r} must be [B,C,R,R] (got {tuple(t.shape)})")
            if shape is not None and tuple(t.shape) != shape:
                raise VtError(f"{what}: all planes of a call share one shape (got {tuple(t.shape)} next to {shape})")
            shape = tuple(t.shape)
        out.append(t)
    return out, (shape[0], shape[1], shape[2])


class Prepared:
    """What sample_planes keeps between calls on the same planes: the workspace with their channels-last copies and, for a lattice in
    table form, the per-plane tables.  Hand one object to every call of a run over one scene (the slabs of a lattice, the levels of
    a MISE extraction): calls after the first skip the preparation (VT_PLANES_PREPARED) while the planes' storage and version, the
    mode and the lattice's nx / box are what they were; anything else prepares again."""

    def __init__(self):
        self.ws, self.key = None, None


def sample_planes(planes, pts=None, padding=0.1, base=None, lattice=None, nearest=False, lattice_form=None, prepared=None):
    """feat [B,N,C] = base? + xz? + xy? + yz? (vt_sample_planes): the bilinear ('nearest': rounded) sample of every plane of the dict
    ``planes`` ([B,C,R,R] each) at ``pts`` [B,N,3], or with ``lattice=(nx, box, first, count)`` at the points
    ``box * make_3d_grid(...)[first:first+count]`` generated in the kernel -- bit for bit the point form's result on those points.
    ``base`` [B,N,C]: what to add the planes onto (the grid's ops.sample_grid), overwritten with the result.  ``prepared``: a
    :class:`Prepared` kept by the caller across calls on the same planes."""
    if (pts is None) == (lattice is None):
        raise VtError("sample_planes: give the query points as pts [B,N,3] or as lattice=(nx, box, first, count), one of the two")
    ts, (B, C, R) = _three(planes, "sample_planes")
    dev = next(t for t in ts if t is not None).device
    if pts is not None:
        pts = _c(pts.float())
        if pts.dim() != 3 or pts.shape[0] != B or pts.shape[2] != 3:
            raise VtError(f"sample_planes: pts must be [B,N,3] with B={B} (got {tuple(pts.shape)})")
        N, nx, box, first = pts.shape[1], 0, 0.0, 0
    else:
        nx, box, first, N = lattice
        if nx < 2 or first < 0 or N < 0 or first + N > nx ** 3:
            raise VtError(f"sample_planes: slab [{first}, {first + N}) outside the {nx}^3 lattice")
    flags = NEAREST if nearest else 0
    if pts is None and (lattice_form or LATTICE_FORM) == "points":
        flags |= LATTICE_POINTS
    if base is not None:
        if tuple(base.shape) != (B, N, C) or not base.is_contiguous() or base.dtype != torch.float32:
            raise VtError(f"sample_planes: base must be a contiguous float32 [B,N,C]=({B},{N},{C}) (got {tuple(base.shape)})")
        feat = base.detach()
    else:
        feat = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    lib = _lib.load()
    n_planes = sum(t is not None for t in ts)
    wsb = lib.vt_sample_planes_workspace_bytes(B, R, C, n_planes, int(nx) if not flags & LATTICE_POINTS else 0)
    key = (tuple((t.data_ptr(), t._version) if t is not None else None for t in (planes.get(k) for k in ORDER)), B, C, R, flags,
           int(nx), float(box), float(padding), stream_ptr().value)
    if prepared is not None and prepared.key == key and prepared.ws is not None and prepared.ws.numel() >= wsb:
        ws, flags = prepared.ws, flags | PREPARED
    else:
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        if prepared is not None:
            prepared.ws, prepared.key = ws, key
    check(lib.vt_sample_planes(dev_ptr(ts[0], "xz"), dev_ptr(ts[1], "xy"), dev_ptr(ts[2], "yz"), B, R, C, dev_ptr(pts, "pts"), N,
                               int(nx), float(box), int(first), float(padding), flags, dev_ptr(feat, "base") if base is not None else None,
                               dev_ptr(feat, "feat"), dev_ptr(ws, "workspace", torch.uint8), ws.numel(), stream_ptr()), "vt_sample_planes")
    return feat


def sample_planes_bwd(keys, shape, pts, grad_feat, padding=0.1, nearest=False, out=None):
    """The planes' gradients of sample_planes (vt_sample_planes_bwd): {key: [B,C,R,R]} for ``keys`` (a subset of 'xz','xy','yz') of
    planes of ``shape`` (B, C, R, R), from ``grad_feat`` [B,N,C] at ``pts`` [B,N,3].  Every element of every returned tensor is
    written (no pre-zeroing); ``out``: buffers to write into by key -- those of keys not asked for are left alone."""
    keys = set(keys)
    if not keys or not keys <= set(ORDER):
        raise VtError(f"sample_planes_bwd: keys must be a non-empty subset of {ORDER} (got {sorted(keys)})")
    B, C, R = int(shape[0]), int(shape[1]), int(shape[2])
    pts = _c(pts.float())
    grad_feat = _c(grad_feat.float())
    N = pts.shape[1]
    if tuple(pts.shape) != (B, N, 3) or tuple(grad_feat.shape) != (B, N, C):
        raise VtError(f"sample_planes_bwd: pts [B,N,3] and grad_feat [B,N,C] with B={B}, C={C} (got {tuple(pts.shape)}, {tuple(grad_feat.shape)})")
    dev = grad_feat.device
    grads = {}
    for k in ORDER:
        if k in keys:
            g = out[k] if out is not None and k in out else torch.empty((B, C, R, R), dtype=torch.float32, device=dev)
            if tuple(g.shape) != (B, C, R, R):
                raise VtError(f"sample_planes_bwd: out[{k!r}] must be [B,C,R,R]=({B},{C},{R},{R}) (got {tuple(g.shape)})")
            grads[k] = g
    lib = _lib.load()
    wsb = lib.vt_sample_planes_bwd_workspace_bytes(B, N, R, C, len(grads))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    check(lib.vt_sample_planes_bwd(B, R, C, dev_ptr(pts, "pts"), N, float(padding), NEAREST if nearest else 0, dev_ptr(grad_feat, "grad_feat"),
                                   dev_ptr(grads.get("xz"), "grad_xz"), dev_ptr(grads.get("xy"), "grad_xy"), dev_ptr(grads.get("yz"), "grad_yz"),
                                   dev_ptr(ws, "workspace", torch.uint8), ws.numel(), stream_ptr()), "vt_sample_planes_bwd")
    return grads


def decode_mlp_lattice(c, blob, lattice, precision="f32", wide=None, out=None):
    """ops.decode_mlp_fwd for a lattice slab: the conditioned MLP on given features c [B,count,C] at the points
    ``box * make_3d_grid(...)[first:first+count]`` of ``lattice=(nx, box, first, count)``, generated in the kernel (the C entries'
    lattice arguments, which ops.decode_mlp_fwd pins to 0): a dense decode needs no point tensor.  ``out``: a contiguous [B,count]
    tensor to write the logits into."""
    if precision not in ("f32", "f16x3", "wide", "wide_f16x3"):
        raise VtError(f"decode_mlp_lattice: precision must be 'f32', 'f16x3', 'wide' or 'wide_f16x3' (got {precision!r})")
    c = _c(c.float())
    B, N, C = c.shape
    nx, box, first, count = lattice
    if count != N:
        raise VtError(f"decode_mlp_lattice: c holds {N} points per scene, the slab {count}")
    if nx < 2 or first < 0 or first + count > nx ** 3:
        raise VtError(f"decode_mlp_lattice: slab [{first}, {first + count}) outside the {nx}^3 lattice")
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=c.device)
    elif tuple(out.shape) != (B, N):
        raise VtError(f"decode_mlp_lattice: out must be [B,count]=({B},{N}) (got {tuple(out.shape)})")
    if not N:
        return out
    lib = _lib.load()
    if precision in ("wide", "wide_f16x3"):
        if wide is None:
            raise VtError("decode_mlp_lattice: precision 'wide' needs wide=(hidden_size, n_blocks, leaky)")
        hidden, nb, leaky = wide[:3]
        name = "vt_decode_mlp_fwd_wide" if precision == "wide" else "vt_decode_mlp_fwd_wide_f16x3"
        check(getattr(lib, name)(dev_ptr(c, "c"), B, C, None, N, int(nx), float(box), int(first), dev_ptr(blob, "blob"),
                                 int(hidden), int(nb), 1 if leaky else 0, dev_ptr(out, "out"), None, stream_ptr()), name)
        return out
    name = "vt_decode_mlp_fwd" if precision == "f32" else "vt_decode_mlp_fwd_f16x3"
    check(getattr(lib, name)(dev_ptr(c, "c"), B, C, None, N, int(nx), float(box), int(first), dev_ptr(blob, "blob"), dev_ptr(out, "out"),
                             stream_ptr()), name)
    return out
