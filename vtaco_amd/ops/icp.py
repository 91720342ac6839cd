"""Rigid registration of point sets (vt_nn_points, vt_icp_fit, vt_icp: csrc/icp.hip).  A submodule only: callers write ``ops.icp.icp``,
``ops.icp.icp_fit``, ``ops.icp.nn_points``.  Point sets are device tensors [B,N,3] or [N,3], float64 (float32 is converted exactly); a
[N,3] call returns unbatched results.  Transforms are row-major 4x4 float64."""
from collections import namedtuple
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, _c


F64 = torch.float64
IcpResult = namedtuple("IcpResult", ["T", "distances", "idx", "iterations"])


def _points(what, **sets):
    """The sets as contiguous float64 [B,n,3] on one HIP device, and whether the call was unbatched."""
    names = list(sets)
    ts = list(sets.values())
    if not all(torch.is_tensor(t) for t in ts):
        raise VtError(f"{what}: {', '.join(names)} must be tensors")
    if not all(t.is_cuda for t in ts) or any(t.device != ts[0].device for t in ts):
        raise VtError(f"{what}: {', '.join(names)} must live on one HIP device (got {', '.join(str(t.device) for t in ts)}); "
                      "vtaco_amd has no CPU path")
    dims = {t.dim() for t in ts}
    if dims not in ({2}, {3}) or any(t.shape[-1] != 3 for t in ts) or len({t.shape[0] for t in ts if t.dim() == 3}) > 1:
        raise VtError(f"{what}: expected point sets [B,N,3] with one B, or [N,3] (got {', '.join(str(tuple(t.shape)) for t in ts)})")
    if any(t.dtype not in (torch.float32, F64) for t in ts):
        raise VtError(f"{what}: point sets must be float64 or float32 (got {', '.join(str(t.dtype) for t in ts)})")
    single = dims == {2}
    out = [_c((t[None] if single else t).to(F64)) for t in ts]
    if any(t.shape[0] == 0 or t.shape[1] == 0 for t in out):
        raise VtError(f"{what}: empty point set ({', '.join(str(tuple(t.shape)) for t in ts)})")
    return out, single


def _pose(what, T, B, dev, name):
    """A [4,4] or [B,4,4] transform as contiguous float64 [B,4,4] on ``dev``, or None."""
    if T is None:
        return None
    if not torch.is_tensor(T) or not T.is_cuda or T.device != dev:
        raise VtError(f"{what}: {name} must be a tensor on the points' HIP device")
    if T.dtype not in (torch.float32, F64) or T.shape[-2:] != (4, 4) or T.dim() not in (2, 3) or (T.dim() == 3 and T.shape[0] != B):
        raise VtError(f"{what}: {name} must be a float64 [4,4] or [B,4,4] transform (got {T.dtype} {tuple(T.shape)})")
    T = T.to(F64)
    return _c(T[None].expand(B, 4, 4) if T.dim() == 2 else T)


def _ws(nbytes, dev):
    return torch.empty((max(int(nbytes), 8) + 7) // 8, dtype=torch.int64, device=dev)


def nn_slab_points(N, M, B=1):
    """The targets per slab vt_nn_points uses for N queries and M targets (times B problems): a multiple of 256."""
    return int(_lib.load().vt_nn_points_slab_points(int(N), int(M), int(B)))


def nn_points(src, dst, T=None):
    """(d2 [B,N] f64, idx [B,N] i32): the squared distance from every point of src [B,N,3] (moved by T [B,4,4] or [4,4] first, when given)
    to the nearest point of dst [B,M,3] and its index, the lowest among equal minima (vt_nn_points; nearest_neighbor, icp.py:50-66)."""
    what = "nn_points"
    (src, dst), single = _points(what, src=src, dst=dst)
    B, N, M = src.shape[0], src.shape[1], dst.shape[1]
    dev = src.device
    T = _pose(what, T, B, dev, "T")
    d2 = torch.empty((B, N), dtype=F64, device=dev)
    idx = torch.empty((B, N), dtype=I32, device=dev)
    lib = _lib.load()
    ws = _ws(lib.vt_nn_points_workspace_bytes(N, M, B), dev)
    check(lib.vt_nn_points(dev_ptr(src, "src", F64), N, dev_ptr(dst, "dst", F64), M, B, dev_ptr(T, "T", F64), dev_ptr(d2, "d2", F64),
                           dev_ptr(idx, "idx", I32), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_nn_points")
    return (d2[0], idx[0]) if single else (d2, idx)


def icp_fit(a, b, idx=None):
    """T [B,4,4] f64: the least-squares rigid transform of the points a [B,N,3] onto b[idx] (idx [B,N] integer, every entry in [0, M)), or
    onto b itself (same shape) without idx (vt_icp_fit; best_fit_transform, icp.py:5-47)."""
    what = "icp_fit"
    (a, b), single = _points(what, a=a, b=b)
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    dev = a.device
    if idx is None:
        if M != N:
            raise VtError(f"{what}: without idx the sets correspond row by row and must have one shape (got {N} and {M} points)")
    else:
        if not torch.is_tensor(idx) or idx.device != dev or idx.dtype not in (torch.int32, torch.int64):
            raise VtError(f"{what}: idx must be an int32 or int64 tensor on the points' HIP device")
        idx = idx[None] if single and idx.dim() == 1 else idx
        if tuple(idx.shape) != (B, N):
            raise VtError(f"{what}: idx must have one entry per point of a (got {tuple(idx.shape)} for {(B, N)})")
        if int(idx.min()) < 0 or int(idx.max()) >= M:
            raise VtError(f"{what}: idx has entries outside [0, {M})")
        idx = _c(idx.to(I32))
    T = torch.empty((B, 4, 4), dtype=F64, device=dev)
    lib = _lib.load()
    ws = _ws(lib.vt_icp_fit_workspace_bytes(N, B), dev)
    check(lib.vt_icp_fit(dev_ptr(a, "a", F64), dev_ptr(b, "b", F64), N, M, dev_ptr(idx, "idx", I32), B, dev_ptr(T, "T", F64),
                         ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_icp_fit")
    return T[0] if single else T


def icp(A, B, init_pose=None, max_iterations=20, tolerance=0.001):
    """IcpResult(T [B,4,4] f64, distances [B,N] f64, idx [B,N] i32, iterations [B] i32) of the iterative closest point loop that maps the
    points A [B,N,3] onto B [B,M,3] (vt_icp; icp, icp.py:69-121), enqueued in full on the current stream: nothing here waits for the
    device.  distances and idx are the last executed iteration's; iterations is its 0-based index (the reference's ``i``)."""
    what = "icp"
    (a, b), single = _points(what, A=A, B=B)
    nb, N, M = a.shape[0], a.shape[1], b.shape[1]
    dev = a.device
    if int(max_iterations) != max_iterations or int(max_iterations) < 1:
        raise VtError(f"{what}: max_iterations must be an integer >= 1 (got {max_iterations})")
    if not float(tolerance) >= 0.0:
        raise VtError(f"{what}: tolerance must be >= 0 (got {tolerance})")
    pose = _pose(what, init_pose, nb, dev, "init_pose")
    T = torch.empty((nb, 4, 4), dtype=F64, device=dev)
    dist = torch.empty((nb, N), dtype=F64, device=dev)
    idx = torch.empty((nb, N), dtype=I32, device=dev)
    its = torch.empty((nb,), dtype=I32, device=dev)
    lib = _lib.load()
    ws = _ws(lib.vt_icp_workspace_bytes(N, M, nb), dev)
    check(lib.vt_icp(dev_ptr(a, "A", F64), N, dev_ptr(b, "B", F64), M, nb, dev_ptr(pose, "init_pose", F64), int(max_iterations), float(tolerance),
                     dev_ptr(T, "T", F64), dev_ptr(dist, "distances", F64), dev_ptr(idx, "idx", I32), dev_ptr(its, "iterations", I32),
                     ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_icp")
    return IcpResult(T[0], dist[0], idx[0], its[0]) if single else IcpResult(T, dist, idx, its)
