"""Float64 numpy statement of the voxel encoder's front end (reference src/encoder/voxels.py:88-119 without the U-Nets): the 1 -> C
Conv3d (kernel 3 with zero padding 1, or kernel 1), ReLU, the scatter-mean of the voxel features onto the grid / the planes, and the
conv's weight and bias gradient under an upstream gradient on any of the outputs.  The cell of a voxel comes from the oracle's
restatement of normalize_3d_coordinate / normalize_coordinate / coordinate2index on the voxel coordinates, not from the package.

``host32`` is the same composition in float32 through torch on the CPU (F.conv3d, index_add_, autograd): the host path whose own
error against float64 the GPU tests' gate is measured in.  Every function returns arrays in the layouts the encoder returns:
'grid' [B,C,R,R,R], a plane [B,C,R,R]."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vtaco_oracle as orc  # noqa: E402

PLANES = ("xz", "xy", "yz")


def voxel_coordinates(dims):
    """[1, D1 D2 D3, 3] f32: linspace(-0.5, 0.5, D) per axis, the first axis slowest (voxels.py:94-102)."""
    axes = [torch.linspace(-0.5, 0.5, d) for d in dims]
    mesh = torch.meshgrid(*axes, indexing="ij")
    return torch.stack([m.reshape(-1) for m in mesh], dim=1).unsqueeze(0)


def cell_ids(dims, reso, padding, name):
    """(ids int64 [D1 D2 D3], number of cells) of output ``name`` in 'grid', 'xz', 'xy', 'yz'."""
    p = voxel_coordinates(dims)
    if name == "grid":
        return orc.voxel_index(p, reso, padding)[0].numpy(), reso ** 3
    return orc.plane_index(p, reso, padding, plane=name)[0].numpy(), reso ** 2


def _shape(name, B, C, reso):
    return (B, C) + (reso,) * (3 if name == "grid" else 2)


def preact(x, w, b, dtype=np.float64):
    """(pre, mag, taps): pre[b,c,v] = bias + sum W x, mag the same sum over magnitudes, taps [k^3][B, V] the shifted volumes."""
    x, w, b = np.asarray(x, dtype), np.asarray(w, dtype), np.asarray(b, dtype)
    B, (D1, D2, D3) = x.shape[0], x.shape[1:]
    k = w.shape[-1]
    pad = k // 2
    xp = np.pad(x, ((0, 0),) + ((pad, pad),) * 3)
    pre = np.broadcast_to(b[None, :, None], (B, w.shape[0], D1 * D2 * D3)).copy()
    mag = np.abs(pre)
    taps = []
    for t1 in range(k):
        for t2 in range(k):
            for t3 in range(k):
                xs = xp[:, t1:t1 + D1, t2:t2 + D2, t3:t3 + D3].reshape(B, 1, -1)
                wt = w[:, 0, t1, t2, t3][None, :, None]
                pre += wt * xs
                mag += np.abs(wt) * np.abs(xs)
                taps.append(xs[:, 0])
    return pre, mag, taps


def _mean(f, ids, cells):
    out = np.zeros(f.shape[:2] + (cells,), f.dtype)
    np.add.at(out, (slice(None), slice(None), ids), f)
    cnt = np.bincount(ids, minlength=cells)
    return out / np.maximum(cnt, 1).astype(f.dtype), cnt


def forward(x, w, b, reso, padding, names, dtype=np.float64):
    """({name: output}, {name: bound}, pre): the outputs, the same means over the magnitude sums, the pre-activation [B,C,V]."""
    pre, mag, _ = preact(x, w, b, dtype)
    f = np.maximum(pre, 0)
    B, C = pre.shape[:2]
    out, bound = {}, {}
    for name in names:
        ids, cells = cell_ids(x.shape[1:], reso, padding, name)
        out[name] = _mean(f, ids, cells)[0].reshape(_shape(name, B, C, reso))
        bound[name] = _mean(mag, ids, cells)[0].reshape(_shape(name, B, C, reso))
    return out, bound, pre


def backward(x, w, b, reso, padding, up, dtype=np.float64):
    """(dW [C,1,k,k,k], dbias [C], bound dW, bound dbias) under the upstream gradients ``up`` {name: array shaped like the output}; a
    voxel takes up[cell] / n from every output it fed, masked pre > 0."""
    pre, _, taps = preact(x, w, b, dtype)
    B, C, V = pre.shape
    G = np.zeros_like(pre)
    for name, u in up.items():
        ids, cells = cell_ids(x.shape[1:], reso, padding, name)
        cnt = np.bincount(ids, minlength=cells)
        G += np.asarray(u, dtype).reshape(B, C, cells)[:, :, ids] / cnt[ids].astype(dtype)
    G = G * (pre > 0)
    k = w.shape[-1]
    dw = np.stack([(G * t[:, None, :]).sum(axis=(0, 2)) for t in taps], axis=1).reshape(C, 1, k, k, k)
    dw_bound = np.stack([np.abs(G * t[:, None, :]).sum(axis=(0, 2)) for t in taps], axis=1).reshape(C, 1, k, k, k)
    return dw, G.sum(axis=(0, 2)), dw_bound, np.abs(G).sum(axis=(0, 2))


def host32(x, w, b, reso, padding, names, up=None):
    """The host composition in float32 on the CPU: ({name: output}, dW, dbias) (the gradients None without ``up``)."""
    x = torch.as_tensor(np.asarray(x, np.float32))
    w = torch.as_tensor(np.asarray(w, np.float32)).clone().requires_grad_(up is not None)
    b = torch.as_tensor(np.asarray(b, np.float32)).clone().requires_grad_(up is not None)
    B, C, k = x.shape[0], w.shape[0], w.shape[-1]
    f = F.relu(F.conv3d(x.unsqueeze(1), w, b, padding=k // 2)).reshape(B, C, -1)
    out = {}
    for name in names:
        ids, cells = cell_ids(x.shape[1:], reso, padding, name)
        ids = torch.from_numpy(ids)
        cnt = torch.bincount(ids, minlength=cells).clamp(min=1).float()
        out[name] = (torch.zeros(B, C, cells).index_add(2, ids, f) / cnt).reshape(_shape(name, B, C, reso))
    if up is None:
        return {n: v.detach().numpy() for n, v in out.items()}, None, None
    sum((out[n] * torch.as_tensor(np.asarray(up[n], np.float32))).sum() for n in up).backward()
    return {n: v.detach().numpy() for n, v in out.items()}, w.grad.numpy(), b.grad.numpy()


def fixture(dims, C, k, seed, B=2):
    """A seeded case (x [B,D1,D2,D3] about 30 % occupied with a few non-binary values, weight [C,1,k,k,k], bias [C]) as float32 arrays.
    Unit-variance weights: the pre-activations spread over a few units, so that a seed with min |pre| >= 1e-5 is easy to find."""
    g = torch.Generator().manual_seed(seed)
    shape = (B,) + tuple(dims)
    x = (torch.rand(shape, generator=g) < 0.3).float()
    soft = torch.rand(shape, generator=g) < 0.05
    x = torch.where(soft, torch.rand(shape, generator=g), x)
    w = torch.randn(C, 1, k, k, k, generator=g)
    b = 0.5 * torch.randn(C, generator=g)
    return x.numpy(), w.numpy(), b.numpy()
