"""Fast winding number (vt_winding_tree_*: csrc/winding_fast.hip).  A submodule only: callers write ``ops.winding.build``,
``ops.winding.query``, ``ops.winding.fast``, ``ops.winding.query_scenes``.  The exact sum stays ``ops.winding_number``.

An octree over the faces' centroids whose cells carry the dipole expansion of their faces (Barill et al. 2018): what the reference's
igl.fast_winding_number_for_meshes(V, F, Q) computes.  A tree is built once per mesh (two launches with one small host read between
them, which sizes the records) and queried any number of times; a query reads nothing back and may be captured."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, _c
from ._octree import _Octree, _ws

MAX_DEPTH = 7
REC = 36            # float64 per cell record: p[3], r, N0[3], M1[3][3], M2[6][3], area, faces


class Tree(_Octree):
    """A built tree: ``buf`` (the device buffer), ``depth``, ``counts`` (records per level, root first) and ``n_faces``.  The views
    below alias ``buf``."""

    def __init__(self, buf, depth, state, n_faces, offsets, device):
        self.buf, self.depth, self.n_faces, self.device = buf, int(depth), int(n_faces), device
        self._state = state
        self._offsets = offsets
        self.counts = [int(state[1 + l]) for l in range(self.depth + 1)]
        self._stride, self._items, self._leaves = 0, self.n_faces, [self.counts[self.depth]]

    def pyramid(self, level):
        return self._pyramid(level)

    list_offsets = property(_Octree._list_offsets)
    lists = property(_Octree._lists)
    frame = property(_Octree._frame)

    def records(self, level):
        """float64 [counts[level], 36]."""
        base = sum(self.counts[:level])
        return self._view(self._offsets[1] + 8 * REC * base, torch.float64, REC * self.counts[level]).view(-1, REC)


def default_depth(n_faces):
    """The smallest depth with 8^depth >= n_faces / 8, in [1, 7]."""
    return int(_lib.load().vt_winding_tree_default_depth(int(n_faces)))


def build(verts, faces, depth=None):
    """The tree of the mesh (verts [V,3] f32, faces [F,3] int, device tensors).  ``depth`` in [1, 7]; by default the smallest with
    8^depth >= F / 8.  One host read (64 bytes) between the two launches."""
    if not torch.is_tensor(verts) or not torch.is_tensor(faces) or not verts.is_cuda or faces.device != verts.device:
        raise VtError("winding.build: verts and faces must be tensors on one HIP device; vtaco_amd has no CPU path")
    if verts.dim() != 2 or verts.shape[-1] != 3 or faces.dim() != 2 or faces.shape[-1] != 3:
        raise VtError(f"winding.build: expected verts [V,3] and faces [F,3] (got {tuple(verts.shape)} and {tuple(faces.shape)})")
    verts, faces = _c(verts.float()), _c(faces.to(I32))
    V, F = verts.shape[0], faces.shape[0]
    dev = verts.device
    lib = _lib.load()
    depth = default_depth(F) if depth is None else int(depth)
    nbytes = lib.vt_winding_tree_workspace_bytes(V, F, depth)
    ws = _ws(nbytes, dev)
    ws_p = ctypes.c_void_p(ws.data_ptr())
    vp = dev_ptr(verts, "verts") if V else None
    fp = dev_ptr(faces, "faces", I32) if F else None
    check(lib.vt_winding_tree_count(vp, V, fp, F, depth, ws_p, ws.numel() * 8, stream_ptr()), "vt_winding_tree_count")
    state = (ctypes.c_int32 * 16)(*ws[:8].view(I32).tolist())
    offsets = (ctypes.c_size_t * 6)()
    check(lib.vt_winding_tree_layout(F, depth, state, offsets), "vt_winding_tree_layout")
    buf = _ws(offsets[5], dev)
    check(lib.vt_winding_tree_build(vp, V, fp, F, depth, state, ws_p, ws.numel() * 8, ctypes.c_void_p(buf.data_ptr()), buf.numel() * 8,
                                    stream_ptr()), "vt_winding_tree_build")
    return Tree(buf, depth, state, F, list(offsets), dev)


def query(tree, pts, accuracy=2.0, order=2, dtype=torch.float32, stats=False):
    """w(q) of pts [..., 3] -> [...] in ``dtype`` (float32 or float64).  A cell stands for its faces when the query is farther than
    ``accuracy`` radii from its centre (2.0: libigl's default); ``order`` 0, 1 or 2 is the expansion's.  With ``stats`` also int32
    [..., 2]: the cells accepted and the faces summed exactly, per query."""
    if dtype not in (torch.float32, torch.float64):
        raise VtError("winding.query: dtype must be float32 or float64")
    if not torch.is_tensor(pts) or pts.shape[-1] != 3 or pts.device != tree.device:
        raise VtError("winding.query: pts must be a [..., 3] tensor on the tree's device")
    pts = _c(pts.float())
    N = pts.numel() // 3
    out = torch.empty(pts.shape[:-1], dtype=dtype, device=pts.device)
    st = torch.empty(pts.shape[:-1] + (2,), dtype=I32, device=pts.device) if stats else None
    check(_lib.load().vt_winding_tree_query(ctypes.c_void_p(tree.buf.data_ptr()), tree.buf.numel() * 8, tree.n_faces, tree.depth, tree._state,
                                            dev_ptr(pts, "pts") if N else None, N, float(accuracy), int(order),
                                            ctypes.c_void_p(out.data_ptr()) if N else None, 1 if dtype == torch.float64 else 0,
                                            dev_ptr(st, "stats", I32) if stats and N else None, stream_ptr()), "vt_winding_tree_query")
    return (out, st) if stats else out


def fast(verts, faces, pts, depth=None, **kw):
    """``query(build(verts, faces, depth), pts, **kw)``."""
    return query(build(verts, faces, depth), pts, **kw)


def query_scenes(trees, pts, **kw):
    """pts [B, N, 3] against one tree per scene -> [B, N] (and [B, N, 2] with ``stats``): one launch per scene."""
    if pts.dim() != 3 or len(trees) != pts.shape[0]:
        raise VtError(f"winding.query_scenes: {len(trees)} trees for points {tuple(pts.shape)}")
    res = [query(t, pts[b], **kw) for b, t in enumerate(trees)]
    if kw.get("stats"):
        return torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res])
    return torch.stack(res) if res else torch.empty(pts.shape[:2], dtype=kw.get("dtype", torch.float32), device=pts.device)
