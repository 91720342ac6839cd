"""Evaluation metrics (vt_chamfer_nn, vt_emd_auction, vt_closest_point_mesh, vt_closest_tree_*).  ``from .metrics import *`` hands the
package the names of ``__all__``; the closest-point launchers are reached through the submodule: ``ops.metrics.closest_point_mesh``,
``ops.metrics.closest_point_tree_build`` / ``closest_point_tree_query``."""
from collections import namedtuple
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, _c


EMD_EPS_FINAL = 1e-6          # the auction's last epsilon at a cost range in [1, 2), ~4 f32 ulps of a price near 2; the kernel ends at
                              # eps = EMD_EPS_FINAL * 2^floor(log2(cost range)): cost <= optimum + max(N, M) * eps / N
EMD_MAX_ROUNDS = 500_000      # Jacobi rounds over all phases before the kernel gives up (status 1 -> VtError)
EMD_MAX_POINTS = 4096         # per side: the padded problem lives in the workgroup's LDS (30 bytes per point)

EmdResult = namedtuple("EmdResult", ["emd", "assign", "prices", "rounds", "bids", "phases", "eps"])
ClosestPoint = namedtuple("ClosestPoint", ["d2", "face", "closest"])

__all__ = ["EMD_EPS_FINAL", "EMD_MAX_ROUNDS", "EMD_MAX_POINTS", "EmdResult", "chamfer_nn", "emd_assignment"]


def _point_sets(a, b, what):
    if not (torch.is_tensor(a) and torch.is_tensor(b)):
        raise VtError(f"{what}: point sets must be tensors")
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3 or a.shape[0] != b.shape[0]:
        raise VtError(f"{what}: expected a [B,N,3] and b [B,M,3] (got {tuple(a.shape)} and {tuple(b.shape)})")
    if a.shape[1] == 0 or b.shape[1] == 0:
        raise VtError(f"{what}: empty point set ({tuple(a.shape)}, {tuple(b.shape)})")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise VtError(f"{what}: point sets must be float32 (got {a.dtype}, {b.dtype})")
    if not (a.is_cuda and b.is_cuda) or a.device != b.device:
        raise VtError(f"{what}: both point sets must live on one HIP device (got {a.device}, {b.device})")
    return _c(a), _c(b)


def chamfer_nn(a, b):
    """Nearest neighbours both ways (vt_chamfer_nn): a [B,N,3], b [B,M,3] f32 on the device -> (d_ab [B,N] f32, i_ab [B,N] i32,
    d_ba [B,M] f32, i_ba [B,M] i32): squared distance from every point to the nearest point of the other set and its index
    (the smallest among equal minima).  The naive Chamfer distance of common.py:69-91 is d_ba.mean(1) + d_ab.mean(1)."""
    a, b = _point_sets(a, b, "chamfer_nn")
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    d_ab = torch.empty((B, N), dtype=torch.float32, device=a.device)
    d_ba = torch.empty((B, M), dtype=torch.float32, device=a.device)
    i_ab = torch.empty((B, N), dtype=I32, device=a.device)
    i_ba = torch.empty((B, M), dtype=I32, device=a.device)
    check(_lib.load().vt_chamfer_nn(dev_ptr(a, "a"), dev_ptr(b, "b"), B, N, M, dev_ptr(d_ab, "d_ab"), dev_ptr(i_ab, "i_ab", I32),
                                    dev_ptr(d_ba, "d_ba"), dev_ptr(i_ba, "i_ba", I32), stream_ptr()), "vt_chamfer_nn")
    return d_ab, i_ab, d_ba, i_ba


def emd_assignment(a, b, eps_final=None, max_rounds=None):
    """Minimum-cost assignment of the rows of a [B,N,3] to the rows of b [B,M,3] under Euclidean cost (scipy's cdist +
    linear_sum_assignment, common.py:45-51) by the epsilon-scaling auction of vt_emd_auction, one workgroup per problem.
    Returns EmdResult(emd [B] f64 on the host: the assignment's cost in float64 / N, assign [B,n] i32 and prices [B,n] f32 on
    the device (n = max(N, M): person i -> object assign[i] of the problem padded with zero-cost dummies), the per-problem
    rounds / bids / phases the auction took, and eps [B] f64: the last epsilon, in the inputs' units).  The cost is within
    max(N, M) * eps / N of the optimum, with eps = eps_final * 2^floor(log2(cost range)) (``eps_final`` defaults to EMD_EPS_FINAL;
    the cost range is the f32 diagonal of the two clouds' common bounding box; eps = eps_final when it is 0): the epsilon follows
    the scale of the clouds, so clouds scaled by a power of two give the same assignment.  max(N, M) > EMD_MAX_POINTS, an auction
    that spends ``max_rounds`` rounds without finishing, or a NaN or infinite coordinate (found on the device before the first
    round; "non-finite") raises VtError."""
    a, b = _point_sets(a, b, "emd_assignment")
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    eps = EMD_EPS_FINAL if eps_final is None else float(eps_final)
    rounds = EMD_MAX_ROUNDS if max_rounds is None else int(max_rounds)
    if not eps > 0 or rounds < 0:
        raise VtError(f"emd_assignment: eps_final must be > 0 and max_rounds >= 0 (got {eps}, {rounds})")
    lib = _lib.load()
    per = lib.vt_emd_workspace_bytes(N, M)
    if per == 0:
        raise VtError(f"emd_assignment: {N} x {M} points: at most {EMD_MAX_POINTS} on a side (the problem is held in LDS)")
    n = max(N, M)
    dev = a.device
    assign = torch.empty((B, n), dtype=I32, device=dev)
    prices = torch.empty((B, n), dtype=torch.float32, device=dev)
    cost = torch.empty((B,), dtype=torch.float64, device=dev)
    status = torch.empty((B,), dtype=I32, device=dev)
    ws = torch.empty((B, per // 8), dtype=torch.int64, device=dev)
    check(lib.vt_emd_auction(dev_ptr(a, "a"), N, dev_ptr(b, "b"), M, B, eps, rounds, dev_ptr(assign, "assign", I32),
                             dev_ptr(prices, "prices"), dev_ptr(cost, "cost", torch.float64), dev_ptr(status, "status", I32),
                             ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), "vt_emd_auction")
    st, counters = status.cpu(), ws.cpu()
    bad = torch.nonzero(st == 2).flatten().tolist()
    if bad:
        raise VtError(f"emd_assignment: non-finite coordinates, or a coordinate range beyond float32 (problems {bad[:8]}); "
                      "no auction was run for them")
    bad = torch.nonzero(st).flatten().tolist()
    if bad:
        raise VtError(f"emd_assignment: the auction did not finish within {rounds} rounds (problems {bad[:8]}, "
                      f"eps_final {eps:g}); raise max_rounds or eps_final")
    eps_last = counters.numpy().view("<f4")[:, 5].astype("float64")          # the record's f32 behind the i32 phases
    return EmdResult(cost.cpu().numpy(), assign, prices, counters[:, 0].numpy(), counters[:, 1].numpy(),
                     (counters[:, 2] & 0xffffffff).numpy(), eps_last)


def _cp_status(ws, what):
    st = int(ws[0].item())
    if st & 1:
        raise VtError(f"{what}: a face index lies outside [0, V) (found on the device by the prepare pass; that face was not read)")
    if st & 2:
        raise VtError(f"{what}: a scene's mesh has no vertices, no faces or more faces than max_F")


def closest_point_slab_faces(F, N, B=1):
    """The faces per slab vt_closest_point_mesh uses for F faces and N queries (times B scenes): a multiple of 256."""
    return int(_lib.load().vt_closest_point_mesh_slab_faces(int(F), int(N), int(B)))


def _cp_tensors(what, verts, faces, pts):
    """The three arguments of a closest-point call, checked and contiguous (faces as int32)."""
    if not (torch.is_tensor(verts) and torch.is_tensor(faces) and torch.is_tensor(pts)):
        raise VtError(f"{what}: verts, faces and pts must be tensors")
    if not (verts.is_cuda and faces.is_cuda and pts.is_cuda) or verts.device != faces.device or verts.device != pts.device:
        raise VtError(f"{what}: verts, faces and pts must live on one HIP device (got {verts.device}, {faces.device}, {pts.device}); "
                      "vtaco_amd has no CPU path")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or pts.dim() != 2 or pts.shape[1] != 3:
        raise VtError(f"{what}: expected verts [V,3], faces [F,3] and pts [N,3] (got {tuple(verts.shape)}, {tuple(faces.shape)}, {tuple(pts.shape)})")
    if verts.dtype != torch.float32 or pts.dtype != torch.float32 or faces.dtype not in (torch.int32, torch.int64):
        raise VtError(f"{what}: verts and pts must be float32 and faces int32 or int64 (got {verts.dtype}, {pts.dtype}, {faces.dtype})")
    return _c(verts), _c(faces.to(I32)), _c(pts)


def closest_point_mesh(verts, faces, pts, want_point=True, method='brute'):
    """ClosestPoint(d2 [N] f64, face [N] i32, closest [N,3] f64 or None) of the query points pts [N,3] f32 against the mesh (verts [V,3]
    f32, faces [F,3] i32 / i64) on the device (vt_closest_point_mesh): the smallest squared distance to a closed triangle in float64, the
    face that attains it (the lowest index among equals) and the point on it -- trimesh.proximity.closest_point (training.py:415).  A mesh
    without vertices or faces, or a face index outside [0, V), raises VtError.  ``method='tree'`` builds the face octree and walks it
    (``closest_point_tree_build``, ``closest_point_tree_query``): the same bits from far fewer faces per query on a large mesh."""
    what = "closest_point_mesh"
    if method == 'tree':
        _cp_tensors(what, verts, faces, pts)
        return closest_point_tree_query(closest_point_tree_build(verts, faces), pts, want_point=want_point)
    if method != 'brute':
        raise VtError(f"{what}: method must be 'brute' or 'tree' (got {method!r})")
    verts, faces, pts = _cp_tensors(what, verts, faces, pts)
    V, F, N = verts.shape[0], faces.shape[0], pts.shape[0]
    dev = pts.device
    d2 = torch.empty((N,), dtype=torch.float64, device=dev)
    face = torch.empty((N,), dtype=I32, device=dev)
    closest = torch.empty((N, 3), dtype=torch.float64, device=dev) if want_point else None
    lib = _lib.load()
    ws = torch.empty((max(lib.vt_closest_point_mesh_workspace_bytes(F, N), 8) // 4,), dtype=I32, device=dev)
    check(lib.vt_closest_point_mesh(dev_ptr(verts, "verts") if V else None, V, dev_ptr(faces, "faces", I32) if F else None, F, dev_ptr(pts, "pts"), N,
                                    dev_ptr(d2, "d2", torch.float64), dev_ptr(face, "face", I32),
                                    dev_ptr(closest, "closest", torch.float64), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4, stream_ptr()),
          "vt_closest_point_mesh")
    if N:
        _cp_status(ws, what)
    return ClosestPoint(d2, face, closest)


def closest_point_mesh_scenes(meshes, pts, want_point=True):
    """The same for a batch of scenes in one launch sequence (vt_closest_point_mesh_scenes): ``meshes`` = [(verts [V,3] f32, faces [F,3] i32)]
    device tensors per scene (the records of ``winding_number_scenes``), pts [B,N,3] f32 -> ClosestPoint(d2 [B,N], face [B,N], closest
    [B,N,3]).  Each scene equals its single call bit for bit."""
    import struct
    what = "closest_point_mesh_scenes"
    if not torch.is_tensor(pts) or pts.dim() != 3 or pts.shape[2] != 3 or pts.dtype != torch.float32 or not pts.is_cuda:
        raise VtError(f"{what}: pts must be a float32 [B,N,3] device tensor")
    pts = _c(pts)
    B, N = pts.shape[:2]
    if len(meshes) != B:
        raise VtError(f"{what}: {len(meshes)} meshes for {B} scenes")
    rec = bytearray()
    max_f = 0
    for v, f in meshes:
        if v.dtype != torch.float32 or f.dtype != I32 or not v.is_contiguous() or not f.is_contiguous() or v.device != pts.device or f.device != pts.device:
            raise VtError(f"{what}: meshes must be contiguous tensors on the points' device (verts f32 [V,3], faces i32 [F,3])")
        if v.shape[0] == 0 or f.shape[0] == 0:
            raise VtError(f"{what}: a mesh without vertices or faces has no closest point")
        rec += struct.pack("<QQii", v.data_ptr(), f.data_ptr(), v.shape[0], f.shape[0])
        max_f = max(max_f, f.shape[0])
    dev = pts.device
    d2 = torch.empty((B, N), dtype=torch.float64, device=dev)
    face = torch.empty((B, N), dtype=I32, device=dev)
    closest = torch.empty((B, N, 3), dtype=torch.float64, device=dev) if want_point else None
    if B == 0 or N == 0:
        return ClosestPoint(d2, face, closest)
    table = torch.frombuffer(rec, dtype=torch.uint8).to(dev, non_blocking=True)
    lib = _lib.load()
    ws = torch.empty((B * lib.vt_closest_point_mesh_workspace_bytes(max_f, N) // 4,), dtype=I32, device=dev)
    check(lib.vt_closest_point_mesh_scenes(ctypes.c_void_p(table.data_ptr()), B, max_f, dev_ptr(pts, "pts"), N, dev_ptr(d2, "d2", torch.float64),
                                           dev_ptr(face, "face", I32), dev_ptr(closest, "closest", torch.float64),
                                           ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4, stream_ptr()), "vt_closest_point_mesh_scenes")
    _cp_status(ws, what)
    return ClosestPoint(d2, face, closest)


class ClosestTree:
    """The face octree of a mesh with what a closest-point walk reads (vt_closest_tree_build): ``tree`` (the ``ops.winding.Tree``, shared
    with the fast winding number), ``side`` (the device buffer of boxes and face records), ``status`` (the build's status word: bit 0,
    a face index outside [0, V)).  The views below alias ``side``."""

    def __init__(self, tree, side, offsets, status):
        self.tree, self.side, self._offsets, self.status = tree, side, offsets, int(status)

    def boxes(self, level):
        """float64 [counts[level], 6]: lo[3], hi[3] of the level's occupied cells, in the order of the tree's records."""
        base, n = sum(self.tree.counts[:level]), self.tree.counts[level]
        at = self._offsets[0] + 48 * base
        return self.side.view(torch.uint8)[at:at + 48 * n].view(torch.float64).view(-1, 6)

    @property
    def records(self):
        """float64 [F, 14]: the face records in list order (slot t is face ``tree.lists[t]``)."""
        at = self._offsets[1]
        return self.side.view(torch.uint8)[at:at + 112 * self.tree.n_faces].view(torch.float64).view(-1, 14)


def closest_point_tree_build(verts, faces, depth=None, tree=None):
    """The ClosestTree of the mesh (verts [V,3] f32, faces [F,3] i32 / i64 on the device): ``ops.winding.build``'s octree (``depth`` as
    there), or the caller's ``tree`` of the same mesh -- sign and distance then share one build -- with one bounding box per occupied
    cell and the faces' records in list order.  One host read (the status word) at the end.  A mesh without vertices or faces raises
    VtError, as ``closest_point_mesh`` does; a face index outside [0, V) is kept in ``status`` and raised by the query."""
    from . import winding
    what = "closest_point_tree_build"
    if not (torch.is_tensor(verts) and torch.is_tensor(faces)) or not (verts.is_cuda and faces.is_cuda) or verts.device != faces.device:
        raise VtError(f"{what}: verts and faces must be tensors on one HIP device; vtaco_amd has no CPU path")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise VtError(f"{what}: expected verts [V,3] and faces [F,3] (got {tuple(verts.shape)} and {tuple(faces.shape)})")
    if verts.dtype != torch.float32 or faces.dtype not in (torch.int32, torch.int64):
        raise VtError(f"{what}: verts must be float32 and faces int32 or int64 (got {verts.dtype}, {faces.dtype})")
    verts, faces = _c(verts), _c(faces.to(I32))
    V, F = verts.shape[0], faces.shape[0]
    if V == 0 or F == 0:
        raise VtError(f"{what}: a mesh without vertices or faces has no closest point")
    if tree is None:
        tree = winding.build(verts, faces, depth)
    elif tree.n_faces != F or tree.device != verts.device or (depth is not None and int(depth) != tree.depth):
        raise VtError(f"{what}: the tree given is not one of this mesh ({tree.n_faces} faces at depth {tree.depth} on {tree.device})")
    lib = _lib.load()
    offsets = (ctypes.c_size_t * 3)()
    check(lib.vt_closest_tree_layout(F, tree.depth, tree._state, offsets), "vt_closest_tree_layout")
    side = torch.empty((offsets[2] + 7) // 8, dtype=torch.int64, device=verts.device)
    check(lib.vt_closest_tree_build(dev_ptr(verts, "verts"), V, dev_ptr(faces, "faces", I32), F, tree.depth, tree._state,
                                    ctypes.c_void_p(tree.buf.data_ptr()), tree.buf.numel() * 8, ctypes.c_void_p(side.data_ptr()), side.numel() * 8,
                                    stream_ptr()), "vt_closest_tree_build")
    return ClosestTree(tree, side, list(offsets), side[:1].view(I32)[0].item())


def closest_point_tree_query(ctree, pts, want_point=True, stats=False, strict=True):
    """``closest_point_mesh``'s ClosestPoint of pts [N,3] f32 against a ClosestTree, bit for bit (vt_closest_tree_query: a walk of the octree
    that skips every cell whose box is farther than the best face so far; reads nothing back).  With ``stats`` also int32 [N,2]: the boxes
    and the faces tested per query.  A tree whose mesh has a face index outside [0, V) raises VtError as the brute-force call does;
    ``strict=False`` answers from the other faces instead."""
    what = "closest_point_tree_query"
    if not isinstance(ctree, ClosestTree):
        raise VtError(f"{what}: expected a ClosestTree (closest_point_tree_build)")
    if not torch.is_tensor(pts) or pts.dim() != 2 or pts.shape[1] != 3 or pts.dtype != torch.float32 or pts.device != ctree.tree.device:
        raise VtError(f"{what}: pts must be a float32 [N,3] tensor on the tree's device")
    if strict and ctree.status & 1:
        raise VtError(f"{what}: a face index lies outside [0, V) (found on the device by the build; that face was not read)")
    pts = _c(pts)
    N, dev, t = pts.shape[0], pts.device, ctree.tree
    d2 = torch.empty((N,), dtype=torch.float64, device=dev)
    face = torch.empty((N,), dtype=I32, device=dev)
    closest = torch.empty((N, 3), dtype=torch.float64, device=dev) if want_point else None
    st = torch.empty((N, 2), dtype=I32, device=dev) if stats else None
    check(_lib.load().vt_closest_tree_query(ctypes.c_void_p(t.buf.data_ptr()), t.buf.numel() * 8, ctypes.c_void_p(ctree.side.data_ptr()),
                                            ctree.side.numel() * 8, t.n_faces, t.depth, t._state, dev_ptr(pts, "pts") if N else None, N,
                                            dev_ptr(d2, "d2", torch.float64) if N else None, dev_ptr(face, "face", I32) if N else None,
                                            dev_ptr(closest, "closest", torch.float64) if want_point and N else None,
                                            dev_ptr(st, "stats", I32) if stats and N else None, stream_ptr()), "vt_closest_tree_query")
    out = ClosestPoint(d2, face, closest)
    return (out, st) if stats else out


def closest_point_tree_query_scenes(ctrees, pts, want_point=True, stats=False, strict=True):
    """pts [B,N,3] against one ClosestTree per scene -> ClosestPoint(d2 [B,N], face [B,N], closest [B,N,3]) (and stats [B,N,2]): one launch
    per scene, each equal to its single call."""
    what = "closest_point_tree_query_scenes"
    if not torch.is_tensor(pts) or pts.dim() != 3 or pts.shape[2] != 3 or len(ctrees) != pts.shape[0]:
        raise VtError(f"{what}: {len(ctrees)} trees for points {tuple(pts.shape) if torch.is_tensor(pts) else pts}")
    res = [closest_point_tree_query(t, pts[b], want_point=want_point, stats=stats, strict=strict) for b, t in enumerate(ctrees)]
    cps = [r[0] for r in res] if stats else res
    B, N = pts.shape[:2]
    if B == 0:
        empty = ClosestPoint(torch.empty((0, N), dtype=torch.float64, device=pts.device), torch.empty((0, N), dtype=I32, device=pts.device),
                             torch.empty((0, N, 3), dtype=torch.float64, device=pts.device) if want_point else None)
        return (empty, torch.empty((0, N, 2), dtype=I32, device=pts.device)) if stats else empty
    out = ClosestPoint(torch.stack([c.d2 for c in cps]), torch.stack([c.face for c in cps]),
                       torch.stack([c.closest for c in cps]) if want_point else None)
    return (out, torch.stack([r[1] for r in res])) if stats else out
