"""The voxel-input encoder's front end (vt_voxel_encode_grid / _planes / _bwd): conv_in, ReLU and the scatter-mean of the voxel features
onto the grid or the canonical planes in one launch, and the conv's weight / bias gradient.  Reached as ``ops.voxel_encoder.name``: the
module adds no name to ``vtaco_amd.ops`` itself.

A voxel's cell follows from the volume's shape alone, per axis: ``tables`` evaluates the reference's own f32 expressions
(src/encoder/voxels.py:94-96, src/common.py:268-309, 333-348) on the CPU once per (dims, reso, padding, device, kind) and keeps the
result on the device."""
from collections import OrderedDict

import torch

from ._base import _lib, VtError, check, dev_ptr, keep_for_graph, stream_ptr, _c

ORDER = ("xz", "xy", "yz")              # the order the encoder stacks its planes in, whatever order the caller names them
_BIT = {"xz": 1, "xy": 2, "yz": 4}
MAX_TABLES = 64
_tables = OrderedDict()                 # (dims, reso, padding, device, kind) -> Tables


def axis_index(D, reso, padding, kind):
    """int64 [D]: the cell index along one axis of the D voxels at linspace(-0.5, 0.5, D), in the reference's f32 arithmetic on the
    CPU.  kind 'grid': normalize_3d_coordinate (divisor 1 + padding + 10e-4, clamp 1 - 10e-4); 'plane': normalize_coordinate (10e-6)."""
    eps = 10e-4 if kind == "grid" else 10e-6
    q = torch.linspace(-0.5, 0.5, D) / (1 + padding + eps)
    q = q + 0.5
    q = torch.where(q >= 1, torch.full_like(q, 1 - eps), q)
    q = torch.where(q < 0, torch.zeros_like(q), q)
    return (q * reso).long()


class Tables:
    """One device tensor: index a1 | a2 | a3 (int32 [D1 + D2 + D3]) followed by ranges [3][R][2]."""

    def __init__(self, dims, reso, padding, device, kind):
        idx, rng = [], []
        for D in dims:
            a = axis_index(D, reso, padding, kind)
            if int(a.min()) < 0 or int(a.max()) >= reso or bool((a[1:] < a[:-1]).any()):
                raise VtError(f"voxel_encoder: the cell index of {D} voxels at resolution {reso}, padding {padding} leaves [0, {reso}) or decreases")
            r = torch.arange(reso)
            rng.append(torch.stack((torch.searchsorted(a, r, right=False), torch.searchsorted(a, r, right=True)), dim=1))
            idx.append(a)
        self.n_index = sum(dims)
        self.buf = torch.cat([torch.cat(idx), torch.stack(rng).reshape(-1)]).to(torch.int32).to(device)
        self.index, self.ranges = self.buf[:self.n_index], self.buf[self.n_index:]


def tables(dims, reso, padding, device, kind="grid"):
    """The cached Tables of a volume shape: a second call with the same arguments copies nothing to the device."""
    if kind not in ("grid", "plane"):
        raise VtError(f"voxel_encoder.tables: kind must be 'grid' or 'plane' (got {kind!r})")
    key = (tuple(int(d) for d in dims), int(reso), float(padding), torch.device(device), kind)
    t = _tables.get(key)
    if t is None:
        t = _tables[key] = Tables(key[0], key[1], key[2], key[3], kind)
        while len(_tables) > MAX_TABLES:
            _tables.popitem(last=False)
    else:
        _tables.move_to_end(key)
    keep_for_graph(t.buf)
    return t


def _conv_args(x, weight, bias, what):
    if not x.is_cuda:
        raise VtError(f"{what}: inputs must live on a HIP device (got {x.device})")
    x, weight, bias = _c(x.float()), _c(weight.float()), _c(bias.float())
    if x.dim() != 4 or min(x.shape[1:]) < 2:
        raise VtError(f"{what}: x must be [B,D1,D2,D3] with every D >= 2 (got {tuple(x.shape)})")
    C, k = weight.shape[0], weight.shape[-1]
    if weight.dim() != 5 or tuple(weight.shape) != (C, 1, k, k, k) or k not in (1, 3) or tuple(bias.shape) != (C,):
        raise VtError(f"{what}: weight must be [C,1,k,k,k] with k 1 or 3 and bias [C] (got {tuple(weight.shape)}, {tuple(bias.shape)})")
    if C % 32 or not 32 <= C <= 128:
        raise VtError(f"{what}: C must be a multiple of 32 up to 128 (got {C})")
    return x, weight, bias, C, k


def _mask(planes, what):
    keys = [planes] if isinstance(planes, str) else list(planes)
    if not keys or not set(keys) <= set(ORDER) or len(set(keys)) != len(keys):
        raise VtError(f"{what}: planes must be a non-empty subset of {ORDER} (got {keys})")
    return sum(_BIT[k] for k in keys), len(keys)


def encode_grid(x, weight, bias, reso, padding=0.1):
    """[B,R,R,R,C] channels-last: the mean of relu(conv(x)) over the voxels of every grid cell, empty cells 0 (vt_voxel_encode_grid)."""
    x, weight, bias, C, k = _conv_args(x, weight, bias, "voxel_encoder.encode_grid")
    B, R = x.shape[0], int(reso)
    t = tables(x.shape[1:], R, padding, x.device, "grid")
    out = torch.empty((B, R, R, R, C), dtype=torch.float32, device=x.device)
    check(_lib.load().vt_voxel_encode_grid(dev_ptr(x, "x"), B, x.shape[1], x.shape[2], x.shape[3], dev_ptr(weight, "weight"), dev_ptr(bias, "bias"),
                                           C, k, dev_ptr(t.ranges, "ranges", torch.int32), R, dev_ptr(out, "grid"), stream_ptr()),
          "vt_voxel_encode_grid")
    return out


def encode_planes(x, weight, bias, reso, padding=0.1, planes=ORDER):
    """[P B,C,R,R]: the requested planes in ORDER one after the other (what LocalPoolPointnet.forward_planes stacks), each cell the mean of
    relu(conv(x)) over its two ranges times the dropped axis (vt_voxel_encode_planes)."""
    x, weight, bias, C, k = _conv_args(x, weight, bias, "voxel_encoder.encode_planes")
    mask, P = _mask(planes, "voxel_encoder.encode_planes")
    B, R = x.shape[0], int(reso)
    t = tables(x.shape[1:], R, padding, x.device, "plane")
    out = torch.empty((P * B, C, R, R), dtype=torch.float32, device=x.device)
    check(_lib.load().vt_voxel_encode_planes(dev_ptr(x, "x"), B, x.shape[1], x.shape[2], x.shape[3], dev_ptr(weight, "weight"), dev_ptr(bias, "bias"),
                                             C, k, dev_ptr(t.ranges, "ranges", torch.int32), R, mask, dev_ptr(out, "planes"), stream_ptr()),
          "vt_voxel_encode_planes")
    return out


def encode_bwd(x, weight, bias, padding=0.1, grad_grid=None, grad_planes=None, planes=ORDER):
    """(grad_weight [C,1,k,k,k], grad_bias [C]) from the upstream gradient of encode_grid's output (``grad_grid`` [B,R,R,R,C]) and / or
    of encode_planes' (``grad_planes`` [P B,C,R,R] for ``planes``) (vt_voxel_encode_bwd); the resolutions are read off the gradients."""
    what = "voxel_encoder.encode_bwd"
    x, weight, bias, C, k = _conv_args(x, weight, bias, what)
    if grad_grid is None and grad_planes is None:
        raise VtError(f"{what}: give grad_grid, grad_planes or both")
    B, dims = x.shape[0], tuple(x.shape[1:])
    tg = tp = None
    Rg = Rp = mask = 0
    if grad_grid is not None:
        grad_grid = _c(grad_grid.float())
        Rg = grad_grid.shape[1] if grad_grid.dim() == 5 else 0
        if tuple(grad_grid.shape) != (B, Rg, Rg, Rg, C):
            raise VtError(f"{what}: grad_grid must be [B,R,R,R,C] with B={B}, C={C} (got {tuple(grad_grid.shape)})")
        tg = tables(dims, Rg, padding, x.device, "grid")
    if grad_planes is not None:
        mask, P = _mask(planes, what)
        grad_planes = _c(grad_planes.float())
        Rp = grad_planes.shape[-1] if grad_planes.dim() == 4 else 0
        if tuple(grad_planes.shape) != (P * B, C, Rp, Rp):
            raise VtError(f"{what}: grad_planes must be [P B,C,R,R] with P={P}, B={B}, C={C} (got {tuple(grad_planes.shape)})")
        tp = tables(dims, Rp, padding, x.device, "plane")
    lib = _lib.load()
    ws = torch.empty(max(lib.vt_voxel_encode_bwd_workspace_bytes(B, *dims, C), 16), dtype=torch.uint8, device=x.device)
    dw, db = torch.empty_like(weight), torch.empty_like(bias)
    i32 = torch.int32
    check(lib.vt_voxel_encode_bwd(dev_ptr(x, "x"), B, *dims, dev_ptr(weight, "weight"), dev_ptr(bias, "bias"), C, k,
                                  dev_ptr(grad_grid, "grad_grid"), dev_ptr(tg.index if tg else None, "index", i32),
                                  dev_ptr(tg.ranges if tg else None, "ranges", i32), Rg,
                                  dev_ptr(grad_planes, "grad_planes"), dev_ptr(tp.index if tp else None, "index", i32),
                                  dev_ptr(tp.ranges if tp else None, "ranges", i32), Rp, mask,
                                  dev_ptr(dw, "grad_weight"), dev_ptr(db, "grad_bias"), dev_ptr(ws, "workspace", torch.uint8), ws.numel(), stream_ptr()),
          "vt_voxel_encode_bwd")
    return dw, db
