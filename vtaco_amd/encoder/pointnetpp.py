"""PointNet++ encoder of the PointConv baseline (drop-in for reference src/encoder/pointnetpp.py): per-point features of the input
cloud, ``(xyz [B,N,3], features [B,N,c_dim])``, for ``LocalPointDecoder``.

Same classes, constructor arguments and ``state_dict`` keys as the reference.  The geometry -- farthest-point sampling, the ball
query and the 3-nearest-neighbour weights -- runs on the HIP kernels of pointnetpp.hip (ops.points; ``VTACO_POINTCONV=host``: on
their torch restatement, pointconv_host).  Those stages give indices and weights only, so autograd sees plain gathers; the shared
MLPs (1x1 convolutions, BatchNorm, ReLU, the max over a group) are ``nn`` modules on the device in both modes.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops, pointconv_host as host
from .._lib import VtError


def _on_device(t, what):
    if not t.is_cuda:
        raise VtError(f"{what}: inputs must live on a HIP device (got {t.device})")


def fps(xyz, npoint, start):
    return (ops.points.fps if host.form("fps") == "hip" else host.fps)(xyz, npoint, start)


def ball_query(xyz, centres, radius, nsample):
    return (ops.points.ball_query if host.form("ball_query") == "hip" else host.ball_query)(xyz, centres, radius, nsample)


def three_nn(tgt, src):
    return (ops.points.three_nn if host.form("three_nn") == "hip" else host.three_nn)(tgt, src)


def index_points(points, idx):
    """points [B,N,C] at idx [B,...] -> [B,...,C] (pointnetpp.py:168-185)."""
    B = points.shape[0]
    batch = torch.arange(B, dtype=torch.long, device=points.device).view(B, *([1] * (idx.dim() - 1)))
    return points[batch, idx, :]


class PointNetSetAbstraction(nn.Module):
    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, group_all
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last = out_channel

    def _group(self, xyz, points):
        """sample_and_group (pointnetpp.py:235-268): (centres [B,S,3], grouped [B,S,nsample,3+D])."""
        B, N, _ = xyz.shape
        # the reference draws the start indices inside farthest_point_sample: one CPU draw per set abstraction, in call order
        start = torch.randint(0, N, (B,), dtype=torch.long)
        with torch.no_grad():
            centres_idx = fps(xyz, self.npoint, start)
            new_xyz = index_points(xyz, centres_idx)
            idx = ball_query(xyz, new_xyz, self.radius, self.nsample)
        grouped = index_points(xyz, idx) - new_xyz.view(B, self.npoint, 1, 3)
        if points is not None:
            grouped = torch.cat([grouped, index_points(points, idx)], dim=-1)
        return new_xyz, grouped

    def forward(self, xyz, points):
        """xyz [B,3,N], points [B,D,N] or None -> (new_xyz [B,3,S], new_points [B,D',S])."""
        xyz = xyz.permute(0, 2, 1)
        if points is not None:
            points = points.permute(0, 2, 1)
        if self.group_all:
            B, N, C = xyz.shape
            new_xyz = torch.zeros(B, 1, C, device=xyz.device, dtype=xyz.dtype)
            grouped = xyz.view(B, 1, N, C)
            if points is not None:
                grouped = torch.cat([grouped, points.view(B, 1, N, -1)], dim=-1)
        else:
            if xyz.shape[1] < self.npoint:
                raise VtError(f"PointNetSetAbstraction: the cloud has {xyz.shape[1]} points, fewer than npoint = {self.npoint}")
            new_xyz, grouped = self._group(xyz.contiguous(), points)
        x = grouped.permute(0, 3, 2, 1)                      # [B, C+D, nsample, npoint]
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            x = F.relu(bn(conv(x)))
        return new_xyz.permute(0, 2, 1), torch.max(x, 2)[0]


class PointNetFeaturePropagation(nn.Module):
    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv1d(last, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out_channel))
            last = out_channel

    def forward(self, xyz1, xyz2, points1, points2):
        """xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D,N] or None, points2 [B,D,S] -> [B,D',N]."""
        xyz1, xyz2, points2 = xyz1.permute(0, 2, 1), xyz2.permute(0, 2, 1), points2.permute(0, 2, 1)
        B, N, _ = xyz1.shape
        with torch.no_grad():
            idx, weight = three_nn(xyz1.contiguous(), xyz2.contiguous())        # S == 1: index 0, weight 1 -- the reference's repeat
        interpolated = torch.sum(index_points(points2, idx) * weight.unsqueeze(-1), dim=2)
        if points1 is not None:
            interpolated = torch.cat([points1.permute(0, 2, 1), interpolated], dim=-1)
        x = interpolated.permute(0, 2, 1)
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            x = F.relu(bn(conv(x)))
        return x


class PointNetPlusPlus(nn.Module):
    """``encoder: pointnet_plus_plus`` (pointnetpp.py:105-129).  ``dim`` and ``padding`` are accepted and unused, as in the reference."""

    def __init__(self, dim=None, c_dim=128, padding=0.1):
        super().__init__()
        self.c_dim = c_dim
        self.sa1 = PointNetSetAbstraction(npoint=512, radius=0.2, nsample=32, in_channel=6, mlp=[64, 64, 128], group_all=False)
        self.sa2 = PointNetSetAbstraction(npoint=128, radius=0.4, nsample=64, in_channel=128 + 3, mlp=[128, 128, 256], group_all=False)
        self.sa3 = PointNetSetAbstraction(npoint=None, radius=None, nsample=None, in_channel=256 + 3, mlp=[256, 512, 1024], group_all=True)
        self.fp3 = PointNetFeaturePropagation(in_channel=1280, mlp=[256, 256])
        self.fp2 = PointNetFeaturePropagation(in_channel=384, mlp=[256, 128])
        self.fp1 = PointNetFeaturePropagation(in_channel=128, mlp=[128, 128, c_dim])

    def forward(self, xyz):
        """xyz [B,N,3] -> (xyz [B,N,3], features [B,N,c_dim])."""
        _on_device(xyz, "PointNetPlusPlus")
        if xyz.dim() != 3 or xyz.shape[2] != 3:
            raise VtError(f"PointNetPlusPlus: the input cloud must be [B,N,3] (got {tuple(xyz.shape)})")
        xyz = xyz.float().permute(0, 2, 1)
        l0_points, l0_xyz = xyz, xyz[:, :3, :]
        l1_xyz, l1_points = self.sa1(l0_xyz, l0_points)
        l2_xyz, l2_points = self.sa2(l1_xyz, l1_points)
        l3_xyz, l3_points = self.sa3(l2_xyz, l2_points)
        l2_points = self.fp3(l2_xyz, l3_xyz, l2_points, l3_points)
        l1_points = self.fp2(l1_xyz, l2_xyz, l1_points, l2_points)
        l0_points = self.fp1(l0_xyz, l1_xyz, None, l1_points)
        return xyz.permute(0, 2, 1), l0_points.permute(0, 2, 1)
