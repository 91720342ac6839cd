"""The PointConv baseline's five operations restated in torch ops on the device, and the knob that picks between them and the HIP
kernels (ops.points).

``VTACO_POINTCONV=hip|host`` (read once): ``host`` runs the encoder's geometry and the decoder's sampler on the functions below --
the reference's own formulation (a Python loop for the farthest points, sorts for the ball query and the 3 nearest neighbours, the
[M,N] weight matrix for the sampler).  It is the fall-back and what tools/bench_pointconv.py times the kernels against.  Unset,
every stage takes DEFAULT_FORM: "hip" where the committed run of that benchmark (profiles/pointconv_bench.json) shows the kernel
faster than the host form by more than the spread between rounds, "host" elsewhere.  The sampler is two stages, because the two
forms win at different sizes: "sample" is the point form (training's 2 048 queries, MISE levels), "sample_lattice" the dense slabs.
"""
import os

import torch

from ._lib import VtError
from .common import make_3d_grid

STAGES = ("fps", "ball_query", "three_nn", "sample", "sample_lattice")
# per stage, from profiles/pointconv_bench.json (README): at 2 048 point queries the kernel's 16 workgroups lose
# to the host matrix product (0.41 against 0.20 ms); on the 128^3 lattice it wins 17-fold
DEFAULT_FORM = {"fps": "hip", "ball_query": "hip", "three_nn": "hip", "sample": "host", "sample_lattice": "hip"}

_env = os.environ.get("VTACO_POINTCONV")
if _env not in (None, "", "hip", "host"):
    raise VtError(f"VTACO_POINTCONV must be 'hip' or 'host' (got {_env!r})")
FORM = {s: (_env or DEFAULT_FORM[s]) for s in STAGES}

SAMPLE_CHUNK = 4096          # queries per [chunk, N] weight matrix of the host sampler


def form(stage):
    return FORM[stage]


def _d2(a, b):
    """((dx dx + dy dy) + dz dz) of a [..., 3] - b [..., 3], broadcast."""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def fps(xyz, npoint, start):
    """pointnetpp.py:188-209 with the start indices given: int64 [B,npoint]."""
    B, N, _ = xyz.shape
    if N < npoint:
        raise VtError(f"fps: the cloud has {N} points, fewer than npoint = {npoint}")
    centroids = torch.zeros(B, npoint, dtype=torch.long, device=xyz.device)
    distance = torch.full((B, N), 1e10, dtype=xyz.dtype, device=xyz.device)
    farthest = start.to(xyz.device, torch.long)
    batch = torch.arange(B, dtype=torch.long, device=xyz.device)
    for i in range(npoint):
        centroids[:, i] = farthest
        dist = _d2(xyz, xyz[batch, farthest, :].view(B, 1, 3))
        distance = torch.minimum(distance, dist)
        farthest = torch.max(distance, -1)[1]
    return centroids


def ball_query(xyz, centres, radius, nsample):
    """pointnetpp.py:212-232: int64 [B,S,nsample]; a row with nothing in range reads 0."""
    B, N, _ = xyz.shape
    S = centres.shape[1]
    group = torch.arange(N, dtype=torch.long, device=xyz.device).view(1, 1, N).repeat(B, S, 1)
    sq = _d2(xyz[:, None, :, :], centres[:, :, None, :])
    r2 = torch.tensor(float(radius) ** 2, dtype=torch.float64).to(sq.dtype).item()
    group[sq > r2] = N
    group = group.sort(dim=-1)[0][:, :, :nsample]
    if group.shape[2] < nsample:
        group = torch.cat([group, group.new_full((B, S, nsample - group.shape[2]), N)], dim=2)
    first = group[:, :, :1].expand(-1, -1, nsample)
    group = torch.where(group == N, first, group)
    return torch.where(group == N, torch.zeros_like(group), group)


def three_nn(tgt, src):
    """pointnetpp.py:84-90: (idx int64 [B,N,k], weight [B,N,k]), k = min(3, S)."""
    k = min(3, src.shape[1])
    d, idx = _d2(tgt[:, :, None, :], src[:, None, :, :]).sort(dim=-1)
    d, idx = d[:, :, :k], idx[:, :, :k]
    recip = 1.0 / (d + 1e-8)
    return idx, recip / recip.sum(dim=2, keepdim=True)


def point_sample(cloud, fea, pts=None, lattice=None, sample_mode='gaussian', gaussian_val=None):
    """decoder.py:468-485 in the shifted form, chunked over the queries; differentiable in ``fea`` by autograd."""
    if pts is None:
        nx, box, first, count = lattice
        grid = box * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (nx,) * 3)
        pts = grid[first:first + count].to(cloud.device).unsqueeze(0).expand(cloud.shape[0], -1, -1)
    if sample_mode == 'gaussian':
        if gaussian_val is None:
            raise VtError("point_sample: sample_mode 'gaussian' needs gaussian_val")
        var = float(gaussian_val) ** 2
    out = []
    for q in torch.split(pts.float(), SAMPLE_CHUNK, dim=1):
        d = torch.sqrt(_d2(cloud[:, None, :, :], q[:, :, None, :])) + 10e-6
        if sample_mode == 'gaussian':
            e = -(d ** 2) / var
            w = (e - e.max(dim=2, keepdim=True)[0]).exp()
        else:
            w = 1.0 / d
        out.append((w / w.sum(dim=2, keepdim=True)) @ fea)
    return torch.cat(out, dim=1) if out else fea.new_zeros((fea.shape[0], 0, fea.shape[2]))
