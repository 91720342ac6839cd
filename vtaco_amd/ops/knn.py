"""The k nearest points of a point set and normals from them (vt_knn_points, vt_point_tree_knn, vt_knn_normals: csrc/knn.hip).  A
submodule only: callers write ``ops.knn.knn_points``, ``ops.knn.knn_slab_points``, ``ops.knn.normals``.  Point sets are device tensors
[B,N,3] or [N,3], float64 (float32 is converted exactly); a [N,3] call returns unbatched results.  There is no CPU path."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, _c
from ._octree import _ws
from .icp import F64, PointTree, _lanes, _method, _points, _pose, _tree_for


MAX_K = 32      # VT_KNN_MAX_K


def _k(what, k):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
        raise VtError(f"{what}: k must be an integer in [1, {MAX_K}] (got {k!r}); larger neighbourhoods are not built")
    return int(k)


def knn_slab_points(N, M, B=1):
    """The targets per slab vt_knn_points uses by itself for N queries and M targets (times B problems): a multiple of 256."""
    return int(_lib.load().vt_knn_points_slab_points(int(N), int(M), int(B)))


def knn_points(src, dst, k, T=None, method="brute", tree=None, lanes=None, stats=False, slab=None):
    """(d2 [B,N,k] f64, idx [B,N,k] i32): per point of src [B,N,3] (moved by T [B,4,4] or [4,4] first, when given) the k points of dst
    [B,M,3] smallest in the order (squared distance, index), ascending.  With M < k the tail is (+inf, -1); a query with a coordinate
    that is not finite returns all (+inf, -1).  ``k = 1`` is ``ops.icp.nn_points`` bit for bit.
    ``method='brute'`` tests every target (vt_knn_points); ``slab`` (a multiple of 256, default: the library's choice) is the number of
    targets per workgroup and changes no result.  ``method='tree'`` walks a PointTree of dst (vt_point_tree_knn): the same bits;
    ``tree=`` (``ops.icp.point_tree_build(dst)``) reuses a built one, ``lanes`` is ``ops.icp.point_tree_query``'s, and ``stats=True``
    also returns int32 [B,N,2], the boxes and the points tested per query."""
    what = "knn_points"
    k = _k(what, k)
    if _method(what, method) == "brute":
        if tree is not None:
            raise VtError(f"{what}: tree= is for method='tree'")
        if stats or lanes is not None:
            raise VtError(f"{what}: stats and lanes are for method='tree'")
    elif slab is not None:
        raise VtError(f"{what}: slab= is for method='brute'")
    if tree is not None and not isinstance(tree, PointTree):
        raise VtError(f"{what}: expected a PointTree (ops.icp.point_tree_build)")
    (src, dst), single = _points(what, src=src, dst=dst)
    B, N, M = src.shape[0], src.shape[1], dst.shape[1]
    dev = src.device
    T = _pose(what, T, B, dev, "T")
    d2 = torch.empty((B, N, k), dtype=F64, device=dev)
    idx = torch.empty((B, N, k), dtype=I32, device=dev)
    st = None
    lib = _lib.load()
    if method == "brute":
        slab = 0 if slab is None else slab
        if isinstance(slab, bool) or int(slab) != slab or int(slab) < 0 or int(slab) % 256:
            raise VtError(f"{what}: slab must be a multiple of 256 (got {slab!r})")
        slab = int(slab)
        ws = _ws(lib.vt_knn_points_workspace_bytes(N, M, B, k, slab), dev)
        check(lib.vt_knn_points(dev_ptr(src, "src", F64), N, dev_ptr(dst, "dst", F64), M, B, dev_ptr(T, "T", F64), k, slab, dev_ptr(d2, "d2", F64),
                                dev_ptr(idx, "idx", I32), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_knn_points")
    else:
        lanes = _lanes(what, lanes)
        given = tree is not None
        tree = _tree_for(what, tree, dst, B, M, dev)
        if given and tree.single != single:
            raise VtError(f"{what}: src and the tree's targets must both be batched or both unbatched")
        if stats:
            st = torch.empty((B, N, 2), dtype=I32, device=dev)
        tp, tb = ctypes.c_void_p(tree.buf.data_ptr()), tree.buf.numel() * 8
        perm = None
        if lanes == "morton":
            perm = torch.empty((B, N), dtype=I32, device=dev)
            ws = _ws(lib.vt_point_tree_lanes_workspace_bytes(N, B, tree.depth), dev)
            check(lib.vt_point_tree_lanes(tp, tb, M, tree.depth, B, tree._state, dev_ptr(src, "src", F64), N, dev_ptr(T, "T", F64),
                                          dev_ptr(perm, "perm", I32), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()),
                  "vt_point_tree_lanes")
        check(lib.vt_point_tree_knn(tp, tb, M, tree.depth, B, tree._state, dev_ptr(src, "src", F64), N, dev_ptr(T, "T", F64), k,
                                    dev_ptr(d2, "d2", F64), dev_ptr(idx, "idx", I32), dev_ptr(st, "stats", I32), dev_ptr(perm, "perm", I32),
                                    stream_ptr()), "vt_point_tree_knn")
    out = (d2[0], idx[0]) if single else (d2, idx)
    return out + ((st[0] if single else st),) if stats else out


def normals(pts, idx, view=None):
    """(normal [B,N,3] f64, eig [B,N,3] f64) of the neighbourhoods idx [B,N,k] (int32 or int64; entries outside [0, M) are left out) of
    the points pts [B,M,3] (vt_knn_normals): the unit eigenvector of the smallest eigenvalue of the neighbours' covariance and the
    eigenvalues, ascending.  ``view`` [3], [B,3] or [B,N,3] turns every normal towards that point (seen from the neighbourhood's first
    point); without it the component of largest magnitude is positive.  Fewer than 3 neighbours, or coincident ones, give zeros."""
    what = "normals"
    (pts,), single = _points(what, pts=pts)
    B, M = pts.shape[0], pts.shape[1]
    dev = pts.device
    if not torch.is_tensor(idx) or idx.device != dev or idx.dtype not in (torch.int32, torch.int64):
        raise VtError(f"{what}: idx must be an int32 or int64 tensor on the points' HIP device")
    if idx.dim() != (2 if single else 3) or (not single and idx.shape[0] != B) or not 1 <= idx.shape[-1] <= MAX_K or idx.shape[-2] == 0:
        raise VtError(f"{what}: idx must be [N,k] for points [M,3] or [B,N,k] for [B,M,3], 1 <= k <= {MAX_K} (got {tuple(idx.shape)})")
    idx = _c((idx[None] if single else idx).to(I32))
    N, k = idx.shape[1], idx.shape[2]
    per_point = 0
    if view is not None:
        if not torch.is_tensor(view) or view.device != dev or view.dtype not in (torch.float32, F64) or view.shape[-1] != 3:
            raise VtError(f"{what}: view must be a float64 tensor [3], [B,3] or [B,N,3] on the points' HIP device")
        view = view.to(F64)
        if view.dim() == 1:
            view = view[None].expand(B, 3)
        elif single and view.dim() == 2 and tuple(view.shape) == (N, 3) and N != 1:
            view = view[None]
        if view.dim() == 3 and tuple(view.shape) == (B, N, 3):
            per_point = 1
        elif view.dim() != 2 or tuple(view.shape) != (B, 3):
            raise VtError(f"{what}: view must be [3], [B,3] or [B,N,3] (got {tuple(view.shape)} for B = {B}, N = {N})")
        view = _c(view)
    nrm = torch.empty((B, N, 3), dtype=F64, device=dev)
    eig = torch.empty((B, N, 3), dtype=F64, device=dev)
    check(_lib.load().vt_knn_normals(dev_ptr(pts, "pts", F64), M, dev_ptr(idx, "idx", I32), N, k, B, dev_ptr(view, "view", F64), per_point,
                                     dev_ptr(nrm, "normal", F64), dev_ptr(eig, "eig", F64), stream_ptr()), "vt_knn_normals")
    return (nrm[0], eig[0]) if single else (nrm, eig)
