"""Rigid registration of point sets (vt_nn_points, vt_icp_fit, vt_icp, vt_icp_tree: csrc/icp.hip) and the octree over a point set that
answers the same neighbour queries without testing every target (vt_point_tree_*: csrc/point_tree.hip).  A submodule only: callers write
``ops.icp.icp``, ``ops.icp.icp_fit``, ``ops.icp.nn_points``, ``ops.icp.point_tree_build``, ``ops.icp.point_tree_query``.  Point sets are device tensors [B,N,3] or [N,3], float64 (float32 is converted exactly); a
[N,3] call returns unbatched results.  Transforms are row-major 4x4 float64."""
from collections import namedtuple
import ctypes
import os

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, _c
from ._octree import _Octree, _ws


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


def nn_slab_points(N, M, B=1):
    """The targets per slab vt_nn_points uses for N queries and M targets (times B problems): a multiple of 256."""
    return int(_lib.load().vt_nn_points_slab_points(int(N), int(M), int(B)))


class PointTree(_Octree):
    """The octrees of B target sets with one M (vt_point_tree_build): ``buf`` (the device buffer of all B trees), ``dst`` (the targets,
    float64 [B,M,3]), ``depth``, ``counts`` (occupied cells per level, root first; one list per problem when the build was batched) and
    ``status`` (the builds' status words or-ed: 0 for a built tree).  The accessors alias ``buf``; ``b`` picks the problem."""

    def __init__(self, buf, dst, depth, state, offsets, single):
        self.buf, self.dst, self.depth, self.single = buf, dst, int(depth), single
        self.n_problems, self.n_points, self.device = dst.shape[0], dst.shape[1], dst.device
        self._state, self._offsets = state, offsets
        per = [[int(state[16 * b + 1 + l]) for l in range(self.depth + 1)] for b in range(self.n_problems)]
        self._counts = per
        self.counts = per[0] if single else per
        self.status = 0
        for b in range(self.n_problems):
            self.status |= int(state[16 * b])
        self._base = [0]
        for l in range(self.depth + 1):
            self._base.append(self._base[-1] + max(c[l] for c in per))
        self._stride, self._items, self._leaves = offsets[5], self.n_points, [c[self.depth] for c in per]

    frame, pyramid, list_offsets, lists = _Octree._frame, _Octree._pyramid, _Octree._list_offsets, _Octree._lists

    def boxes(self, level, b=0):
        """float64 [counts[level], 6]: lo[3], hi[3] of the level's occupied cells, in rank order."""
        return self._view(self._offsets[1] + 48 * self._base[level], F64, 6 * self._counts[b][level], b).view(-1, 6)

    def points(self, b=0):
        """float64 [M, 3]: the targets in list order."""
        return self._view(self._offsets[4], F64, 3 * self.n_points, b).view(-1, 3)


def point_tree_default_depth(M):
    """The smallest depth in [1, 7] with 8^depth * 8 >= M."""
    return int(_lib.load().vt_point_tree_default_depth(int(M)))


def point_tree_build(dst, depth=None):
    """The PointTree of the targets dst [B,M,3] or [M,3] (float64; float32 is converted exactly): one octree per problem, all built by
    the same launches, with one host read (64 bytes per problem) between the count and the build.  ``depth`` in [1, 7]; by default the
    smallest with 8^depth * 8 >= M.  A target coordinate that is not finite raises VtError."""
    what = "point_tree_build"
    (dst,), single = _points(what, dst=dst)
    B, M = dst.shape[0], dst.shape[1]
    dev = dst.device
    lib = _lib.load()
    if depth is None:
        depth = lib.vt_point_tree_default_depth(M)
    elif int(depth) != depth or not 1 <= int(depth) <= 7:
        raise VtError(f"{what}: depth must be an integer in [1, 7] (got {depth})")
    depth = int(depth)
    ws = _ws(lib.vt_point_tree_workspace_bytes(M, B, depth), dev)
    ws_p = ctypes.c_void_p(ws.data_ptr())
    dp = dev_ptr(dst, "dst", F64)
    check(lib.vt_point_tree_count(dp, M, B, depth, ws_p, ws.numel() * 8, stream_ptr()), "vt_point_tree_count")
    state = (ctypes.c_int32 * (16 * B))(*ws[:8 * B].view(I32).tolist())
    if any(state[16 * b] for b in range(B)):
        raise VtError(f"{what}: a target coordinate is not finite (found on the device by the count; no tree was built)")
    offsets = (ctypes.c_size_t * 7)()
    check(lib.vt_point_tree_layout(M, depth, B, state, offsets), "vt_point_tree_layout")
    buf = _ws(offsets[6], dev)
    check(lib.vt_point_tree_build(dp, M, B, depth, state, ws_p, ws.numel() * 8, ctypes.c_void_p(buf.data_ptr()), buf.numel() * 8, stream_ptr()),
          "vt_point_tree_build")
    return PointTree(buf, dst, depth, state, list(offsets), single)


def _tree_for(what, tree, dst, B, M, dev):
    """``tree`` checked against the targets it is used with, or a fresh one of ``dst``."""
    if tree is None:
        return point_tree_build(dst)
    if not isinstance(tree, PointTree):
        raise VtError(f"{what}: expected a PointTree (ops.icp.point_tree_build)")
    if tree.n_problems != B or tree.n_points != M or tree.device != dev:
        raise VtError(f"{what}: the tree given was built for {tree.n_problems} x {tree.n_points} targets on {tree.device}, "
                      f"not for {B} x {M} on {dev}")
    return tree


LANES = "morton"    # the default lane order of point_tree_query; VTACO_POINT_TREE_LANES = query | morton overrides it


def _lanes(what, lanes):
    lanes = lanes or os.environ.get("VTACO_POINT_TREE_LANES") or LANES
    if lanes not in ("query", "morton"):
        raise VtError(f"{what}: lanes must be 'query' or 'morton' (got {lanes!r})")
    return lanes


def point_tree_query(tree, src, T=None, stats=False, lanes=None):
    """``nn_points(src, tree.dst, T)``'s (d2 f64, idx i32) bit for bit, from a walk of the tree that skips every cell whose box is farther
    than the best point so far (vt_point_tree_query; reads nothing back, may be captured).  With ``stats`` also int32 [B,N,2]: the boxes
    and the points tested per query.  ``lanes='morton'`` hands the queries to lanes in Morton order of the tree's leaves
    (vt_point_tree_lanes: a permutation per call, three more small launches), so that a wave's lanes walk neighbouring cells; outputs stay
    in query order and no result depends on it.  ``None``: VTACO_POINT_TREE_LANES, else ``LANES``."""
    what = "point_tree_query"
    lanes = _lanes(what, lanes)
    if not isinstance(tree, PointTree):
        raise VtError(f"{what}: expected a PointTree (ops.icp.point_tree_build)")
    (src,), single = _points(what, src=src)
    B, N = src.shape[0], src.shape[1]
    dev = src.device
    if single != tree.single:
        raise VtError(f"{what}: src and the tree's targets must both be batched or both unbatched")
    _tree_for(what, tree, None, B, tree.n_points, dev)
    T = _pose(what, T, B, dev, "T")
    d2 = torch.empty((B, N), dtype=F64, device=dev)
    idx = torch.empty((B, N), dtype=I32, device=dev)
    st = torch.empty((B, N, 2), dtype=I32, device=dev) if stats else None
    lib = _lib.load()
    perm = None
    if lanes == "morton":
        perm = torch.empty((B, N), dtype=I32, device=dev)
        ws = _ws(lib.vt_point_tree_lanes_workspace_bytes(N, B, tree.depth), dev)
        check(lib.vt_point_tree_lanes(ctypes.c_void_p(tree.buf.data_ptr()), tree.buf.numel() * 8, tree.n_points, tree.depth, B, tree._state,
                                      dev_ptr(src, "src", F64), N, dev_ptr(T, "T", F64), dev_ptr(perm, "perm", I32),
                                      ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_point_tree_lanes")
    check(lib.vt_point_tree_query(ctypes.c_void_p(tree.buf.data_ptr()), tree.buf.numel() * 8, tree.n_points, tree.depth, B, tree._state,
                                  dev_ptr(src, "src", F64), N, dev_ptr(T, "T", F64), dev_ptr(d2, "d2", F64), dev_ptr(idx, "idx", I32),
                                  dev_ptr(st, "stats", I32), dev_ptr(perm, "perm", I32), stream_ptr()), "vt_point_tree_query")
    out = (d2[0], idx[0]) if single else (d2, idx)
    return out + ((st[0] if single else st),) if stats else out


def _method(what, method):
    if method not in ("brute", "tree"):
        raise VtError(f"{what}: method must be 'brute' or 'tree' (got {method!r})")
    return method


def nn_points(src, dst, T=None, method="brute"):
    """(d2 [B,N] f64, idx [B,N] i32): the squared distance from every point of src [B,N,3] (moved by T [B,4,4] or [4,4] first, when given)
    to the nearest point of dst [B,M,3] and its index, the lowest among equal minima (vt_nn_points; nearest_neighbor, icp.py:50-66).
    ``method='tree'`` builds a PointTree of dst and walks it (``point_tree_build``, ``point_tree_query``): the same bits from far fewer
    targets per query on a large set."""
    what = "nn_points"
    if _method(what, method) == "tree":
        (s, d), single = _points(what, src=src, dst=dst)
        d2, idx = point_tree_query(point_tree_build(d), s, T=T)
        return (d2[0], idx[0]) if single else (d2, idx)
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


def icp(A, B, init_pose=None, max_iterations=20, tolerance=0.001, method="brute", tree=None, lanes=None):
    """IcpResult(T [B,4,4] f64, distances [B,N] f64, idx [B,N] i32, iterations [B] i32) of the iterative closest point loop that maps the
    points A [B,N,3] onto B [B,M,3] (vt_icp; icp, icp.py:69-121), enqueued in full on the current stream: nothing here waits for the
    device.  distances and idx are the last executed iteration's; iterations is its 0-based index (the reference's ``i``).
    ``method='tree'`` searches the neighbours of every iteration in a PointTree of B (vt_icp_tree): equal bits in every output; the one
    host read is the build's, before the loop, and ``tree=`` (``point_tree_build(B)``) reuses a built one; ``lanes`` is
    ``point_tree_query``'s, the order being taken once from the cloud the loop starts with."""
    what = "icp"
    (a, b), single = _points(what, A=A, B=B)
    nb, N, M = a.shape[0], a.shape[1], b.shape[1]
    dev = a.device
    if int(max_iterations) != max_iterations or int(max_iterations) < 1:
        raise VtError(f"{what}: max_iterations must be an integer >= 1 (got {max_iterations})")
    if not float(tolerance) >= 0.0:
        raise VtError(f"{what}: tolerance must be >= 0 (got {tolerance})")
    if _method(what, method) == "brute" and tree is not None:
        raise VtError(f"{what}: tree= is for method='tree'")
    pose = _pose(what, init_pose, nb, dev, "init_pose")
    if method == "tree":
        tree = _tree_for(what, tree, b, nb, M, dev)
    T = torch.empty((nb, 4, 4), dtype=F64, device=dev)
    dist = torch.empty((nb, N), dtype=F64, device=dev)
    idx = torch.empty((nb, N), dtype=I32, device=dev)
    its = torch.empty((nb,), dtype=I32, device=dev)
    lib = _lib.load()
    if method == "tree":
        ws = _ws(lib.vt_icp_tree_workspace_bytes(N, nb, tree.depth), dev)
        check(lib.vt_icp_tree(dev_ptr(a, "A", F64), N, dev_ptr(b, "B", F64), M, nb, ctypes.c_void_p(tree.buf.data_ptr()), tree.buf.numel() * 8,
                              tree.depth, tree._state, 1 if _lanes(what, lanes) == "morton" else 0, dev_ptr(pose, "init_pose", F64),
                              int(max_iterations), float(tolerance),
                              dev_ptr(T, "T", F64), dev_ptr(dist, "distances", F64), dev_ptr(idx, "idx", I32), dev_ptr(its, "iterations", I32),
                              ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_icp_tree")
    else:
        ws = _ws(lib.vt_icp_workspace_bytes(N, M, nb), dev)
        check(lib.vt_icp(dev_ptr(a, "A", F64), N, dev_ptr(b, "B", F64), M, nb, dev_ptr(pose, "init_pose", F64), int(max_iterations),
                         float(tolerance), dev_ptr(T, "T", F64), dev_ptr(dist, "distances", F64), dev_ptr(idx, "idx", I32),
                         dev_ptr(its, "iterations", I32), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_icp")
    return IcpResult(T[0], dist[0], idx[0], its[0]) if single else IcpResult(T, dist, idx, its)
