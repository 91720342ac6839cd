"""What one does with a dense point cloud, on the device: k nearest neighbours, PCA normals, statistical outlier removal -- the three
things Open3D or scipy are usually asked for after ``Generator3D.generate_tactile_pc``, all on ``ops.knn`` (csrc/knn.hip).  Every function
takes a device tensor [N,3] or [B,N,3] (float64; float32 is converted exactly) and returns tensors of the same batching; nothing is read
back to the host."""
import torch

from .. import ops
from .._lib import VtError

# ``method=None`` searches with the tree from this many targets on and with brute force below: what tools/bench_knn.py measured
# (profiles/knn_bench.json; README, "knn.hip").  For k >= 2 the tree, its build included, won at every size measured, 2 048 points and
# up; for k = 1 brute force won at 2 048 and 16 384 and lost at 100 000.  Below 2 048 nothing was measured: brute force.
TREE_FROM = 2048
TREE_FROM_K1 = 100000


def _pick(method, M, k):
    if method is not None:
        return method
    return "tree" if M >= (TREE_FROM_K1 if k == 1 else TREE_FROM) else "brute"


def _count(what, points):
    if not torch.is_tensor(points) or points.dim() not in (2, 3):
        raise VtError(f"{what}: points must be a tensor [N,3] or [B,N,3]")
    return points.shape[-2]


def knn(points, k, queries=None, method=None):
    """(distances f64 [..,N,k], idx i32 [..,N,k]): the k nearest points of ``points`` to every query, ascending by (distance, index);
    distances are Euclidean (the float64 square root of the kernel's squared distance).  Without ``queries`` the cloud is searched for
    its own points, and every point is its own neighbour 0 (distance 0) unless an equal point with a lower index comes first, as with
    scipy's and Open3D's trees.  ``method``: 'brute', 'tree' or None (by the size of ``points`` and k, see ``TREE_FROM``)."""
    src = points if queries is None else queries
    d2, idx = ops.knn.knn_points(src, points, k, method=_pick(method, _count("knn", points), k))
    return torch.sqrt(d2), idx


def estimate_normals(points, k=16, view=None, method=None):
    """(normals f64 [..,N,3], eig f64 [..,N,3]): per point the unit normal of the plane through its k nearest neighbours (itself
    included) by PCA, and the covariance's eigenvalues, ascending (``ops.knn.normals``).  ``view`` ([3], [B,3] or [B,N,3]) turns every
    normal towards that point; without it the sign makes the largest component positive."""
    _, idx = ops.knn.knn_points(points, points, k, method=_pick(method, _count("estimate_normals", points), k))
    return ops.knn.normals(points, idx, view=view)


def surface_variation(eig):
    """lambda_0 / (lambda_0 + lambda_1 + lambda_2) of ``estimate_normals``' eigenvalues (Pauly et al. 2002): 0 on a plane, 1/3 for an
    isotropic neighbourhood; 0 where the sum is not positive."""
    total = (eig[..., 0] + eig[..., 1]) + eig[..., 2]
    return torch.where(total > 0, eig[..., 0] / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(total))


def statistical_outlier_mask(points, k=20, std_ratio=2.0, method=None):
    """bool [..,N]: Open3D's remove_statistical_outlier rule.  Per point the mean Euclidean distance to its k nearest neighbours, itself
    included; a point is kept when that mean is <= mean + std_ratio * std of the means over its cloud (std with N - 1 in the
    denominator, as Open3D has it).  A cloud of fewer than k points uses all of them.  The reductions are float64 torch on the
    device; nothing is read back."""
    N = _count("statistical_outlier_mask", points)
    if not float(std_ratio) >= 0.0:
        raise VtError(f"statistical_outlier_mask: std_ratio must be >= 0 (got {std_ratio})")
    dist, _ = knn(points, min(int(k), N) if int(k) == k and k >= 1 else k, method=method)
    stat = dist.mean(dim=-1)
    mean = stat.mean(dim=-1, keepdim=True)
    std = torch.sqrt(((stat - mean) ** 2).sum(dim=-1, keepdim=True) / max(N - 1, 1))
    return stat <= mean + float(std_ratio) * std


def remove_statistical_outliers(points, k=20, std_ratio=2.0, method=None):
    """(kept points, mask): ``points[mask]`` for a cloud [N,3]; for a batch [B,N,3] a list of B tensors (the clouds keep different
    numbers of points) and the mask [B,N].  Selecting by the mask reads its count back."""
    mask = statistical_outlier_mask(points, k, std_ratio, method)
    if points.dim() == 2:
        return points[mask], mask
    return [p[m] for p, m in zip(points, mask)], mask
