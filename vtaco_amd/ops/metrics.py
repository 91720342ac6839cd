"""Evaluation metrics (vt_chamfer_nn, vt_emd_auction, vt_closest_point_mesh).  ``from .metrics import *`` hands the package the names of
``__all__``; the closest-point launchers are reached through the submodule: ``ops.metrics.closest_point_mesh``."""
from collections import namedtuple
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, _c


EMD_EPS_FINAL = 1e-6          # the auction's last epsilon: cost <= optimum + max(N, M) * eps / N, ~4 f32 ulps of a price near 2
EMD_MAX_ROUNDS = 500_000      # Jacobi rounds over all phases before the kernel gives up (status 1 -> VtError)
EMD_MAX_POINTS = 4096         # per side: the padded problem lives in the workgroup's LDS (30 bytes per point)

EmdResult = namedtuple("EmdResult", ["emd", "assign", "prices", "rounds", "bids", "phases"])
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
    the device (n = max(N, M): person i -> object assign[i] of the problem padded with zero-cost dummies), and the per-problem
    rounds / bids / phases the auction took).  max(N, M) > EMD_MAX_POINTS, or an auction that spends ``max_rounds`` rounds
    without finishing, raises VtError."""
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
    bad = torch.nonzero(st).flatten().tolist()
    if bad:
        raise VtError(f"emd_assignment: the auction did not finish within {rounds} rounds (problems {bad[:8]}, "
                      f"eps_final {eps:g}); raise max_rounds or eps_final")
    return EmdResult(cost.cpu().numpy(), assign, prices, counters[:, 0].numpy(), counters[:, 1].numpy(),
                     (counters[:, 2] & 0xffffffff).numpy())


def _cp_status(ws, what):
    st = int(ws[0].item())
    if st & 1:
        raise VtError(f"{what}: a face index lies outside [0, V) (found on the device by the prepare pass; that face was not read)")
    if st & 2:
        raise VtError(f"{what}: a scene's mesh has no vertices, no faces or more faces than max_F")


def closest_point_slab_faces(F, N, B=1):
    """The faces per slab vt_closest_point_mesh uses for F faces and N queries (times B scenes): a multiple of 256."""
    return int(_lib.load().vt_closest_point_mesh_slab_faces(int(F), int(N), int(B)))


def closest_point_mesh(verts, faces, pts, want_point=True):
    """ClosestPoint(d2 [N] f64, face [N] i32, closest [N,3] f64 or None) of the query points pts [N,3] f32 against the mesh (verts [V,3]
    f32, faces [F,3] i32 / i64) on the device (vt_closest_point_mesh): the smallest squared distance to a closed triangle in float64, the
    face that attains it (the lowest index among equals) and the point on it -- trimesh.proximity.closest_point (training.py:415).  A mesh
    without vertices or faces, or a face index outside [0, V), raises VtError."""
    what = "closest_point_mesh"
    if not (torch.is_tensor(verts) and torch.is_tensor(faces) and torch.is_tensor(pts)):
        raise VtError(f"{what}: verts, faces and pts must be tensors")
    if not (verts.is_cuda and faces.is_cuda and pts.is_cuda) or verts.device != faces.device or verts.device != pts.device:
        raise VtError(f"{what}: verts, faces and pts must live on one HIP device (got {verts.device}, {faces.device}, {pts.device}); "
                      "vtaco_amd has no CPU path")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or pts.dim() != 2 or pts.shape[1] != 3:
        raise VtError(f"{what}: expected verts [V,3], faces [F,3] and pts [N,3] (got {tuple(verts.shape)}, {tuple(faces.shape)}, {tuple(pts.shape)})")
    if verts.dtype != torch.float32 or pts.dtype != torch.float32 or faces.dtype not in (torch.int32, torch.int64):
        raise VtError(f"{what}: verts and pts must be float32 and faces int32 or int64 (got {verts.dtype}, {pts.dtype}, {faces.dtype})")
    verts, faces, pts = _c(verts), _c(faces.to(I32)), _c(pts)
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
