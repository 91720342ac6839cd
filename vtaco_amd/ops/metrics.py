"""Evaluation metrics (vt_chamfer_nn, vt_emd_auction)."""
from collections import namedtuple
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, _c


EMD_EPS_FINAL = 1e-6          # the auction's last epsilon: cost <= optimum + max(N, M) * eps / N, ~4 f32 ulps of a price near 2
EMD_MAX_ROUNDS = 500_000      # Jacobi rounds over all phases before the kernel gives up (status 1 -> VtError)
EMD_MAX_POINTS = 4096         # per side: the padded problem lives in the workgroup's LDS (30 bytes per point)

EmdResult = namedtuple("EmdResult", ["emd", "assign", "prices", "rounds", "bids", "phases"])


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
