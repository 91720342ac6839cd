"""Evaluation metrics of the reference (src/common.py:11-91): the host functions as the reference writes them, and the
device forms of the two the visualise block calls (chamfer_distance_device, earth_mover_distance_device: HIP kernels)."""
from __future__ import annotations

import numpy as np
import torch


def compute_iou(occ1, occ2, threshold=None):
    """IoU of two occupancy sets (common.py:11-43).  As in the reference the ``threshold`` argument is
    IGNORED: both sets are binarised at mean(occ2)."""
    occ1, occ2 = np.asarray(occ1), np.asarray(occ2)
    if occ1.ndim >= 2:
        occ1 = occ1.reshape(occ1.shape[0], -1)
    if occ2.ndim >= 2:
        occ2 = occ2.reshape(occ2.shape[0], -1)
    thr = np.mean(occ2)
    a, b = occ1 >= thr, occ2 >= thr
    union = (a | b).astype(np.float32).sum(axis=-1)
    inter = (a & b).astype(np.float32).sum(axis=-1)
    return inter / union


def chamfer_distance_naive(points1, points2):
    """Squared-distance Chamfer of two [B,T,3] tensors (common.py:62-83); runs on whatever device they live on."""
    if points2.size(1) < 2048:
        points1 = points1[:, :points2.size(1), :]
    assert points1.size() == points2.size()
    d = (points1.unsqueeze(2) - points2.unsqueeze(1)).pow(2).sum(-1)
    return d.min(dim=1)[0].mean(dim=1) + d.min(dim=2)[0].mean(dim=1)


def earth_mover_distance(points1, points2):
    """EMD by optimal assignment (common.py:45-51)."""
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial import distance
    d = distance.cdist(points1, points2)
    rows, cols = linear_sum_assignment(d)
    return d[rows, cols].sum() / len(d)


def chamfer_distance_device(points1, points2, give_id=False):
    """``chamfer_distance(points1, points2, use_kdtree=False)`` (common.py:69-91) on the device: [B,T,3] f32 HIP tensors -> [B]
    (f32, on the device): mean over points2 of the squared distance to the nearest point of points1, plus the same the other way
    (vt_chamfer_nn: the minima are numpy's f32 restatement bit for bit).  The reference's truncation rule holds: when points2 has
    fewer than 2048 points, points1 is cut to that many, and the two sizes must then agree (VtError otherwise).  ``give_id``:
    also the nearest indices, (chamfer, idx_12 [B,T] of points2 for each point1, idx_21 [B,T] of points1 for each point2) as
    int64, like the kd-tree variant returns them."""
    from . import ops
    from ._lib import VtError
    if points1.dim() != 3 or points2.dim() != 3:
        raise VtError(f"chamfer_distance_device: expected [B,T,3] point sets (got {tuple(points1.shape)}, {tuple(points2.shape)})")
    if points2.size(1) < 2048:
        points1 = points1[:, :points2.size(1), :]
    if points1.size() != points2.size():
        raise VtError(f"chamfer_distance_device: point sets of different sizes {tuple(points1.size())} and {tuple(points2.size())}")
    d_12, i_12, d_21, i_21 = ops.chamfer_nn(points1, points2)
    chamfer = d_21.mean(dim=1) + d_12.mean(dim=1)
    if give_id:
        return chamfer, i_12.long(), i_21.long()
    return chamfer


def earth_mover_distance_device(points1, points2, return_assignment=False):
    """``EarthMoverDistance(points1, points2)`` (common.py:45-51: cdist, linear_sum_assignment, sum / len(d)) on the device:
    points1 [N,3], points2 [M,3] (or batches [B,N,3], [B,M,3]) -> the mean matched distance as a float (a float64 array [B] for
    batches).  The assignment is the epsilon-scaling auction of ops.emd_assignment (exact for N != M: the smaller side is padded
    with zero-cost dummies; cost within max(N, M) * ops.EMD_EPS_FINAL / N of the optimum), its cost is evaluated in float64 as cdist
    does.  Inputs are taken as float32 and moved to the current HIP device when they are elsewhere.  ``return_assignment``: also
    the ops.EmdResult (assign [.., max(N, M)] i32: row i of points1 -> row assign[i] of points2, >= M = left unmatched)."""
    from . import ops
    from ._lib import VtError
    dev = torch.device("cuda", torch.cuda.current_device())

    def dev_f32(p):
        t = p if torch.is_tensor(p) else torch.from_numpy(np.asarray(p))
        return t.to(dev if not t.is_cuda else t.device, torch.float32)
    a, b = dev_f32(points1), dev_f32(points2)
    single = a.dim() == 2
    if single:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    if a.dim() != 3 or b.dim() != 3:
        raise VtError(f"earth_mover_distance_device: expected [N,3] / [B,N,3] point sets (got {tuple(a.shape)}, {tuple(b.shape)})")
    res = ops.emd_assignment(a, b)
    emd = float(res.emd[0]) if single else res.emd
    return (emd, res) if return_assignment else emd
